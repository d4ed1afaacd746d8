"""Helpers of the vector-leaf TreeSHAP tests (tahoe_vector_forest_create_ex with TAHOE_CREATE_CONTRIBS): node covers for the forests
of tests/vector_ref.py, a few more named forests, the covers tiled over the K-fold expansion, a float64 brute force evaluated
directly on the vector forest (all K outputs of a leaf at once), and the library's bin packing restated, so that the CPU tests
can check that the named forests have the shapes the GPU tests rely on.

A forest is tests/vector_ref.py's dict.  cover_sets(name) -> {label: covers float32 [num_nodes]}: "consistent" (random positive
leaf covers, a parent's the sum of its children's: what training produces) and "unrelated" (independent positive covers per
node); the forests that carry hand-written covers have the single label "fixed"."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_shap_ref as ssr  # noqa: E402
import vector_ref as vr  # noqa: E402

MISSING = vr.MISSING
ROWS = vr.ROWS
LEAF = vr._bits(vr.IS_LEAF)


def _node(fid, thr, def_left, left):
    return (thr, vr._bits(int(fid) | (vr.DEF_LEFT if def_left else 0)), left)


def _wide_k9():
    """3 trees of depth <= 4 on 700 columns: a row of the tile and its slabs takes kilobytes of LDS, so the rows of a tile and the
    class block both shrink"""
    return vr.make_named([4, 3, 4], 700, 9, seed=4100), None


def _repeat_k3():
    """One depth-24 chain on 5 features: repeated features merge into one element, paths are short and many share a bin, and
    several lanes of a bin carry the same feature (rounds > 1)"""
    return vr.make_named(["chain"], 5, 3, seed=4200), None


def _zero_side_k3():
    """A stump whose left child has cover 0"""
    rng = np.random.default_rng(4300)
    nodes = np.array([_node(1, 0.25, True, 1), (0.0, LEAF, 0), (0.0, LEAF, 1)], vr.SPARSE_NODE_DTYPE)
    forest = dict(nodes=nodes, trees=np.array([0], np.int32), leaves=vr.mixed_leaves(rng, 2, 3), k=3, cols=3)
    return forest, np.array([1.0, 0.0, 1.0], np.float32)


def _tiny_ratio_k3():
    """Covers (1e-39, 1) below the root and (1e-20, 1e20) below its right child: zero fractions under the 2^-121 cut"""
    rng = np.random.default_rng(4400)
    nodes = np.array([_node(0, 0.0, False, 1), (0.0, LEAF, 2), _node(2, 0.5, True, 3), (0.0, LEAF, 0), (0.0, LEAF, 1)],
                     vr.SPARSE_NODE_DTYPE)
    forest = dict(nodes=nodes, trees=np.array([0], np.int32), leaves=vr.mixed_leaves(rng, 3, 3), k=3, cols=3)
    return forest, np.array([1.0, 1e-39, 1.0, 1e-20, 1e20], np.float32)


EXTRA = {"wide_k9": _wide_k9, "repeat_k3": _repeat_k3, "zero_side_k3": _zero_side_k3, "tiny_ratio_k3": _tiny_ratio_k3}
NAMES = list(vr.FORESTS) + list(EXTRA)
SMALL = [n for n in NAMES if n != "wide_k9"]  # num_cols <= 8: the brute force can play every feature
_cache = {}


def consistent_covers(forest, seed):
    """Random positive leaf covers; an internal node's cover is the sum of its children's (float64, rounded once)"""
    nodes, trees = forest["nodes"], forest["trees"]
    rng = np.random.default_rng(seed)
    cv = rng.uniform(0.5, 20.0, nodes.size)
    bounds = list(trees) + [nodes.size]
    for t in range(trees.size):
        lo, hi = int(bounds[t]), int(bounds[t + 1])
        for i in range(hi - 1, lo - 1, -1):  # children come after their parent
            if nodes["bits"][i] >= 0:
                li = lo + int(nodes["left_idx"][i])
                cv[i] = cv[li] + cv[li + 1]
    return cv.astype(np.float32)


def unrelated_covers(forest, seed):
    return np.random.default_rng(seed).uniform(0.05, 1.0, forest["nodes"].size).astype(np.float32)


def case(name):
    """(forest, data [ROWS, cols], {label: covers}), computed once and read-only"""
    if name not in _cache:
        if name in EXTRA:
            forest, fixed = EXTRA[name]()
            data = vr.make_data(ROWS, forest["cols"], seed=31 + forest["cols"])
        else:
            forest, data = vr.case(name)[:2]
            fixed = None
        seed = 5000 + sum(map(ord, name))
        covers = {"fixed": fixed} if fixed is not None else {"consistent": consistent_covers(forest, seed),
                                                              "unrelated": unrelated_covers(forest, seed + 1)}
        for a in (forest["nodes"], forest["trees"], forest["leaves"], data, *covers.values()):
            a.setflags(write=False)
        _cache[name] = (forest, data, covers)
    return _cache[name]


def cover_cases():
    """[(forest name, cover label)] of every forest"""
    return [(n, label) for n in NAMES for label in (("fixed",) if n in ("zero_side_k3", "tiny_ratio_k3") else ("consistent", "unrelated"))]


def tile_covers(forest, covers):
    """The covers of tests/vector_ref.expand(forest): every copy of tree t carries tree t's covers"""
    trees, k = forest["trees"], forest["k"]
    bounds = list(trees) + [forest["nodes"].size]
    parts = [covers[int(bounds[t]):int(bounds[t + 1])] for t in range(trees.size) for _ in range(k)]
    return np.concatenate(parts).astype(np.float32) if parts else np.empty(0, np.float32)


# ---- float64 brute force, directly on the vector forest ----
def _cond_exp(tree, cov, leaves, x, S, missing):
    """v(S) of one tree for every row and output: float64 [rows, K]; sparse_shap_ref._cond_exp with a vector at the leaves"""
    bits = tree["bits"].view(np.uint32)

    def rec(i):
        if bits[i] >> 31:
            return np.broadcast_to(leaves[int(tree["left_idx"][i])].astype(np.float64), (x.shape[0], leaves.shape[1]))
        fid, dl = int(bits[i] & 0x3FFFFFFF), bool((bits[i] >> 30) & 1)
        li = int(tree["left_idx"][i])
        if fid in S:
            r = ssr._go_right(x[:, fid], tree["val"][i], dl, missing)
            return np.where(r[:, None], rec(li + 1), rec(li))
        wl, wr = float(cov[li]), float(cov[li + 1])
        return (wl * rec(li) + wr * rec(li + 1)) / (wl + wr)

    return rec(0)


def contribs(forest, covers, x, missing=MISSING, avg=False, global_bias=0.0):
    """Shapley values of v(S) = E[f_k(x) | x_S] for every output k: float64 [rows, K, cols + 1], bias last; every feature of
    [0, cols) is a player (cols must stay small)"""
    nodes, trees, leaves, K, F = forest["nodes"], forest["trees"], forest["leaves"], forest["k"], forest["cols"]
    x = np.ascontiguousarray(x, np.float32)
    bounds = list(trees) + [nodes.size]
    v = np.zeros((1 << F, x.shape[0], K))
    for t in range(trees.size):
        lo, hi = int(bounds[t]), int(bounds[t + 1])
        for mask in range(1 << F):
            v[mask] += _cond_exp(nodes[lo:hi], covers[lo:hi], leaves, x, {i for i in range(F) if mask >> i & 1}, missing)
    phi = np.zeros((x.shape[0], K, F + 1))
    for i in range(F):
        for mask in range(1 << F):
            if mask >> i & 1:
                continue
            s = bin(mask).count("1")
            w = math.factorial(s) * math.factorial(F - s - 1) / math.factorial(F)
            phi[:, :, i] += w * (v[mask | 1 << i] - v[mask])
    phi[:, :, F] = v[0]
    if avg and trees.size:
        phi /= trees.size
    phi[:, :, F] += global_bias
    return phi


def bias_column(forest, covers, avg=False, global_bias=0.0):
    """[K] float32: the bias column of tahoe_forest_predict_contribs on the vector-leaf handle, in the library's order of
    operations: per k the float64 sum over the trees in order of E_t[k] (sparse_shap_ref.expectation with element k at the
    leaves), / T with AVG, + global_bias, rounded once"""
    nodes, trees, leaves, K = forest["nodes"], forest["trees"], forest["leaves"], forest["k"]
    bounds = list(trees) + [nodes.size]
    out = np.empty(K, np.float32)
    for k in range(K):
        e = 0.0
        for t in range(trees.size):
            tree = nodes[int(bounds[t]):int(bounds[t + 1])].copy()
            leaf = tree["bits"] < 0
            tree["val"][leaf] = leaves[tree["left_idx"][leaf], k]
            e += ssr.expectation(tree, covers[int(bounds[t]):int(bounds[t + 1])])
        out[k] = np.float32((e / trees.size if avg and trees.size else e) + float(global_bias))
    return out


# ---- the library's path bins, restated: what shares a bin, and in how many rounds a bin adds ----
def paths(forest):
    """[[features of the leaf's path, repeated ones merged, in order of first appearance]] per reachable leaf with at least one
    feature, trees in order, leaves in pre-order (left first): the library's paths, one element more (the root element) each"""
    nodes, trees = forest["nodes"], forest["trees"]
    out = []
    for root in trees:
        stack = [(0, ())]
        while stack:
            i, feats = stack.pop()
            n = nodes[int(root) + i]
            if n["bits"] < 0:
                if feats:
                    out.append(list(feats))
                continue
            fid = int(n["bits"]) & vr.FID_MASK
            f2 = feats if fid in feats else feats + (fid,)
            stack += [(int(n["left_idx"]) + 1, f2), (int(n["left_idx"]), f2)]
    return out


def bins(forest):
    """Next-fit packing of the paths (root element included) into 64 lanes -> [(paths of the bin, rounds)]: rounds = the most
    lanes of the bin that carry one feature"""
    out, cur, fill = [], [], 0
    for p in paths(forest) + [None]:
        if p is None or fill + len(p) + 1 > 64:
            if cur:
                feats = [f for q in cur for f in q]
                out.append((cur, max(feats.count(f) for f in set(feats))))
            cur, fill = [], 0
        if p is not None:
            cur.append(p)
            fill += len(p) + 1
    return out
