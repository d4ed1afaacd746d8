"""Reference and helpers of the vector-leaf tests: the rule of tahoe_vector_forest_create in numpy (one sequential float32 sum per
(row, k)), the K-fold expansion of a vector-leaf forest into sparse trees with scalar leaves (what tahoe_sparse_forest_create_ex
takes with num_classes = K), and the named small forests both test files use.

A forest is a dict(nodes [SPARSE_NODE_DTYPE], trees int32 [T], leaves float32 [L, K], k, cols).  A tree is written as a nested
spec -- a leaf is the index of its vector, an internal node (fid, thr, def_left, left, right) -- and laid out breadth-first with
the two children of a node adjacent, so that right = left + 1."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oblivious_ref import GRID, MISSING, bitreverse, make_data  # noqa: E402,F401

SPARSE_NODE_DTYPE = np.dtype([("val", "<f4"), ("bits", "<i4"), ("left_idx", "<i4")])
IS_LEAF, DEF_LEFT, FID_MASK = 1 << 31, 1 << 30, (1 << 30) - 1


def _bits(v):
    return np.int64(v).astype(np.int32) if v < (1 << 31) else np.int32(v - (1 << 32))


def layout_tree(spec):
    """Nested spec -> nodes of one tree: the root at 0, the children of a node in two adjacent slots after it"""
    out = [None]
    todo = [(0, spec)]
    while todo:
        i, s = todo.pop(0)
        if isinstance(s, (int, np.integer)):
            out[i] = (0.0, _bits(IS_LEAF), int(s))
        else:
            fid, thr, def_left, left, right = s
            li = len(out)
            out += [None, None]
            out[i] = (thr, _bits(int(fid) | (DEF_LEFT if def_left else 0)), li)
            todo += [(li, left), (li + 1, right)]
    return np.array(out, SPARSE_NODE_DTYPE)


def make(specs, leaves, k, cols):
    parts = [layout_tree(s) for s in specs]
    trees = np.cumsum([0] + [p.size for p in parts[:-1]]).astype(np.int32) if parts else np.empty(0, np.int32)
    nodes = np.concatenate(parts) if parts else np.empty(0, SPARSE_NODE_DTYPE)
    leaves = np.ascontiguousarray(np.asarray(leaves, np.float32).reshape(-1, k))
    return dict(nodes=nodes, trees=trees, leaves=leaves, k=k, cols=cols)


def vector_ref(forest, data, missing=MISSING):
    """-> (margins float32 [rows, K], leaf indices uint32 [rows, T], steps int [rows, T]).  At a node |x - missing| <= 1e-6 takes
    the default branch (right iff not def_left), NaN goes left, else right iff x >= val; the margins are float32 sums from +0.0
    over the trees in order of the row's leaf vector; a leaf index is the leaf node's index relative to its root; steps counts
    the internal nodes on the row's path."""
    nodes, trees, leaves, k = forest["nodes"], forest["trees"], forest["leaves"], forest["k"]
    data = np.asarray(data, np.float32)
    rows = data.shape[0]
    sums = np.zeros((rows, k), np.float32)
    leaf = np.zeros((rows, trees.size), np.uint32)
    steps = np.zeros((rows, trees.size), np.int64)
    r = np.arange(rows)
    with np.errstate(invalid="ignore"):
        for t, root in enumerate(trees):
            curr = np.zeros(rows, np.int64)
            while True:
                n = nodes[int(root) + curr]
                bits = n["bits"].astype(np.int64) & 0xFFFFFFFF
                live = (bits & IS_LEAF) == 0
                if not live.any():
                    break
                x = data[r, np.where(live, bits & FID_MASK, 0)] if data.shape[1] else np.zeros(rows, np.float32)
                miss = np.abs(x - np.float32(missing)) <= np.float32(1e-6)
                right = np.where(miss, (bits & DEF_LEFT) == 0, x >= n["val"])
                curr = np.where(live, n["left_idx"].astype(np.int64) + right, curr)
                steps[:, t] += live
            leaf[:, t] = curr
            sums = sums + leaves[nodes["left_idx"][int(root) + curr]]  # float32 + float32, tree order
    return sums, leaf, steps


def expand(forest):
    """The T x K-tree expansion: tree t * K + k is tree t with val = leaves[left_idx][k] at its leaves.  -> (nodes, trees)"""
    nodes, trees, leaves, k = forest["nodes"], forest["trees"], forest["leaves"], forest["k"]
    bounds = list(trees) + [nodes.size]
    parts, roots, at = [], [], 0
    for t in range(trees.size):
        tree = nodes[bounds[t]:bounds[t + 1]]
        is_leaf = tree["bits"] < 0
        for c in range(k):
            copy = tree.copy()
            copy["val"][is_leaf] = leaves[tree["left_idx"][is_leaf], c]
            copy["left_idx"][is_leaf] = 0
            parts.append(copy)
            roots.append(at)
            at += copy.size
    return (np.concatenate(parts) if parts else np.empty(0, SPARSE_NODE_DTYPE)), np.array(roots, np.int32)


# ---- the tests' forests ----
def random_tree(rng, cols, num_vectors, max_depth, leaf_prob, depth=0):
    if depth >= max_depth or (depth > 0 and rng.random() < leaf_prob):
        return int(rng.integers(0, num_vectors))
    return (int(rng.integers(0, cols)), float(rng.choice(GRID)), bool(rng.integers(0, 2)),
            random_tree(rng, cols, num_vectors, max_depth, leaf_prob, depth + 1),
            random_tree(rng, cols, num_vectors, max_depth, leaf_prob, depth + 1))


def chain(rng, cols, num_vectors, depth=24):
    """A one-sided chain: every internal node has a leaf on the left and the chain on the right.  Most thresholds are the grid's
    smallest value, so that rows leave the chain at every step and a few reach its end."""
    spec = int(rng.integers(0, num_vectors))
    for _ in range(depth):
        thr = float(GRID[0]) if rng.random() < 0.8 else float(rng.choice(GRID))
        spec = (int(rng.integers(0, cols)), thr, bool(rng.integers(0, 2)), int(rng.integers(0, num_vectors)), spec)
    return spec


def stump(rng, cols, num_vectors):
    return (int(rng.integers(0, cols)), float(rng.choice(GRID)), bool(rng.integers(0, 2)), int(rng.integers(0, num_vectors)),
            int(rng.integers(0, num_vectors)))


def mixed_leaves(rng, num_vectors, k):
    """Leaf values of mixed magnitude, so that a float32 sum depends on its order"""
    return (rng.standard_normal((num_vectors, k)) * 10.0 ** rng.integers(-3, 4, (num_vectors, k))).astype(np.float32)


def make_named(kinds, cols, k, seed, num_vectors=11):
    """kinds: per tree "leaf" (a single leaf), "stump", "chain" (depth 24) or an int (a random tree of at most that depth).  The
    leaves draw their vector from a table of num_vectors rows at random: vectors are shared, and their order is unrelated to the
    node order."""
    rng = np.random.default_rng(seed)
    specs = []
    for kind in kinds:
        if kind == "leaf":
            specs.append(int(rng.integers(0, num_vectors)))
        elif kind == "stump":
            specs.append(stump(rng, cols, num_vectors))
        elif kind == "chain":
            specs.append(chain(rng, cols, num_vectors))
        else:
            specs.append(random_tree(rng, cols, num_vectors, int(kind), 0.3))
    return make(specs, mixed_leaves(rng, num_vectors, k), k, cols)


# name -> (kinds, num_cols, K): T in {0, 1, 3, 4, 5, 9} (the 4-tree window and its remainder), K in {1, 3, 8, 9, 17} (the 8-class
# block), num_cols in {1, 5, 8} (the scalar and the 16-byte staging loops)
FORESTS = {
    "empty_k3": ([], 5, 3),
    "single_leaf_k1": (["leaf"], 1, 1),
    "stump_k3": (["stump"], 1, 3),
    "three_k1": (["stump", "chain", "leaf"], 5, 1),
    "four_k8": ([5, "stump", 3, 7], 8, 8),
    "five_k9": ([4, "chain", "leaf", "stump", 6], 8, 9),
    "nine_k1": ([6, 2, "leaf", "chain", 1, 5, "stump", 3, 6], 8, 1),
    "nine_k17": ([3, "stump", 6, "leaf", 2, "chain", 5, 1, 4], 5, 17),
    "five_k3_one_col": ([3, "chain", 2, "stump", 4], 1, 3),
}
ROWS = 257
_cache = {}


def case(name):
    """(forest, data [ROWS, cols], reference sums [ROWS, K], reference leaves [ROWS, T], steps), computed once and read-only"""
    if name not in _cache:
        kinds, cols, k = FORESTS[name]
        forest = make_named(kinds, cols, k, seed=2000 + sum(map(ord, name)))
        data = make_data(ROWS, cols, seed=17 + cols)
        sums, leaf, steps = vector_ref(forest, data)
        for a in (forest["nodes"], forest["trees"], forest["leaves"], data, sums, leaf, steps):
            a.setflags(write=False)
        _cache[name] = (forest, data, sums, leaf, steps)
    return _cache[name]


def from_oblivious(ob):
    """An oblivious forest (tests/oblivious_ref.make_forest) written as vector-leaf trees: tree t as a complete heap of depth
    d_t whose level l carries split l; the leaf at heap position p names vector lo_t + bitreverse(p - (2^d - 1))."""
    depths, k = np.asarray(ob["depths"], np.int64), ob["k"]
    parts, roots, s, lo, at = [], [], 0, 0, 0
    for d in depths:
        d = int(d)
        tree = np.zeros((2 << d) - 1, SPARSE_NODE_DTYPE)
        for l in range(d):
            level = tree[(1 << l) - 1:(2 << l) - 1]
            level["val"] = ob["thr"][s]
            level["bits"] = np.int32(int(ob["fids"][s]) | (DEF_LEFT if ob["def_left"][s] else 0))
            level["left_idx"] = 2 * np.arange((1 << l) - 1, (2 << l) - 1) + 1
            s += 1
        bottom = tree[(1 << d) - 1:]
        bottom["bits"] = _bits(IS_LEAF)
        bottom["left_idx"] = lo + bitreverse(np.arange(1 << d), d)
        lo += 1 << d
        parts.append(tree)
        roots.append(at)
        at += tree.size
    nodes = np.concatenate(parts) if parts else np.empty(0, SPARSE_NODE_DTYPE)
    return dict(nodes=nodes, trees=np.array(roots, np.int32), leaves=np.asarray(ob["leaves"], np.float32).reshape(-1, k), k=k,
                cols=ob["cols"])
