"""Reference and helpers of the tests of category-set splits on oblivious forests (tahoe_oblivious_forest_create_cat): test
infrastructure, not product.

A forest is oblivious_ref.make_forest's dict with two more keys: "cats" = {split index: category ids}, the index running over the
flattened (tree, level) records, and "ml" = the split indices whose members go left.  At such a level thr is ignored and, with x
the row's value of the level's feature:
  missing (|x - missing| <= 1e-6 in float32): right iff not def_left;
  member = 0 <= x < 32 * nwords and bit trunc(x) of the set is on (nwords = largest id // 32 + 1, 0 for an empty set);
  right = member != (split in ml).
- split_right / cat_ref: that rule and the walk of oblivious_ref.oblivious_ref with it.
- expand_to_sparse: the forest as complete trees of sparse nodes in heap order (left_idx = 2 i + 1), tree t * K + k carrying output
  k, with the categories / members_left dicts a SparseForest takes and the subtree covers of its nodes.
- seam: the float32 restatements of oblivious_shap_ref, oblivious_inter_ref and oblivious_iv_ref read the row at two places only,
  oblivious_shap_ref._bits and oblivious_ref.ref_of; inside `with seam():` both follow the rule above on forests that have "cats".
- members_right / members_left_of: the two identities of DESIGN.md section 31, which turn a numeric forest with integer
  thresholds into a categorical forest with the same bits on suitable data."""
from __future__ import annotations

import contextlib

import numpy as np

import oblivious_ref as obr
import oblivious_shap_ref as osr

SPARSE_NODE_DTYPE = np.dtype([("val", "<f4"), ("bits", "<i4"), ("left_idx", "<i4")])
MISSING = obr.MISSING


def nwords_of(cats):
    cats = list(cats)
    return max(cats) // 32 + 1 if cats else 0


def split_right(forest, s, x, missing):
    """right [rows] (bool) of the split record s for the values x of its feature"""
    x = np.asarray(x, np.float32)
    cats = forest.get("cats", {})
    with np.errstate(invalid="ignore"):
        miss = np.abs(x - np.float32(missing)) <= np.float32(1e-6)
        if s not in cats:
            return np.where(miss, not bool(forest["def_left"][s]), x >= np.float32(forest["thr"][s]))
        nw = nwords_of(cats[s])
        inside = (x >= np.float32(0.0)) & (x < np.float32(32 * nw))
    c = np.where(inside, x, np.float32(0.0)).astype(np.int64)  # truncation of a value >= 0
    member = inside & np.isin(c, np.fromiter(cats[s], np.int64, len(cats[s])))
    return np.where(miss, not bool(forest["def_left"][s]), member != (s in forest.get("ml", ())))


def cat_ref(forest, data, missing=MISSING, init=None):
    """oblivious_ref.oblivious_ref with split_right -> (margins float32 [rows, k], leaf indices uint32 [rows, trees])"""
    depths = np.asarray(forest["depths"], np.int64)
    k = forest["k"]
    leaves = np.asarray(forest["leaves"], np.float32).reshape(-1, k)
    data = np.asarray(data, np.float32)
    rows = data.shape[0]
    sums = np.zeros((rows, k), np.float32)
    if init is not None:
        sums[:, 0] = init
    leaf = np.zeros((rows, depths.size), np.uint32)
    s = lo = 0
    for t, d in enumerate(depths):
        idx = np.zeros(rows, np.int64)
        for l in range(d):
            idx |= split_right(forest, s, data[:, int(forest["fids"][s])], missing).astype(np.int64) << l
            s += 1
        leaf[:, t] = idx
        sums = sums + leaves[lo + idx]  # float32 + float32, tree order
        lo += 1 << d
    return sums, leaf


def cat_bits(forest, sl, data, missing):
    """oblivious_shap_ref._bits with split_right: right[l, rows] of the levels sl of a tree"""
    out = [split_right(forest, s, data[:, int(forest["fids"][s])], missing) for s in range(sl.start, sl.stop)]
    return np.array(out, bool).reshape(len(out), data.shape[0])


@contextlib.contextmanager
def seam():
    """Inside, oblivious_shap_ref._bits and oblivious_ref.ref_of follow the category sets of a forest that has them"""
    old_bits, old_ref = osr._bits, obr.ref_of
    osr._bits = lambda forest, sl, data, missing: (cat_bits if "cats" in forest else old_bits)(forest, sl, data, missing)
    obr.ref_of = lambda forest, data, missing=MISSING, init=None: (cat_ref if "cats" in forest else old_ref)(forest, data, missing,
                                                                                                           init)
    try:
        yield
    finally:
        osr._bits, obr.ref_of = old_bits, old_ref


def expand_to_sparse(forest, covers=None):
    """-> (nodes, trees, categories, members_left, node covers or None).  Tree t * K + k is tree t for output k: a complete tree of
    depth d in heap order, node i of level l carrying split l, its children at 2 i + 1 and 2 i + 2; the leaf at heap position p of
    level d -- its bits in root-first order -- takes leaves[bitreverse_d(p)][k].  A SparseForest(num_classes=K) adds tree t * K + k
    to class k in tree order: the sums of the oblivious handle.  covers [leaves]: every node's cover = the float32 of the float64
    sum of the leaf covers below it."""
    depths = np.asarray(forest["depths"], np.int64)
    k = forest["k"]
    leaves = np.asarray(forest["leaves"], np.float32).reshape(-1, k)
    cats, ml = forest.get("cats", {}), forest.get("ml", ())
    nodes, trees, categories, members_left, cov = [], [], {}, [], []
    s0 = lo = 0
    for t, d in enumerate(depths):
        d = int(d)
        heap_cover = osr.heap(d, covers[lo:lo + (1 << d)])[0] if covers is not None else None
        for c in range(k):
            root = sum(len(n) for n in nodes)
            trees.append(root)
            tree = np.zeros((2 << d) - 1, SPARSE_NODE_DTYPE)
            for l in range(d):
                i = np.arange((1 << l) - 1, (2 << l) - 1)
                tree["val"][i] = forest["thr"][s0 + l]
                tree["bits"][i] = np.int32(int(forest["fids"][s0 + l]) | (int(bool(forest["def_left"][s0 + l])) << 30))
                tree["left_idx"][i] = 2 * i + 1
                if s0 + l in cats:
                    for j in i:
                        categories[root + int(j)] = list(cats[s0 + l])
                        if s0 + l in ml:
                            members_left.append(root + int(j))
            p = np.arange(1 << d)
            tree["val"][(1 << d) - 1 + p] = leaves[lo + obr.bitreverse(p, d), c]
            tree["bits"][(1 << d) - 1 + p] = np.int32(-(1 << 31))
            nodes.append(tree)
            if covers is not None:
                cv = np.zeros(tree.size, np.float32)
                for l in range(d + 1):
                    cv[(1 << l) - 1:(2 << l) - 1] = heap_cover[l][obr.bitreverse(np.arange(1 << l), l)].astype(np.float32)
                cov.append(cv)
        s0 += d
        lo += 1 << d
    cat = np.concatenate(nodes) if nodes else np.zeros(0, SPARSE_NODE_DTYPE)
    return cat, np.array(trees, np.int32), categories, members_left, (np.concatenate(cov) if cov else None) if covers is not None else None


def sparse_leaf_to_oblivious(sparse_leaf, forest):
    """Leaf indices of the expansion (relative to the root, heap numbering; K trees per oblivious tree) -> the oblivious numbering
    of output 0's trees, [rows, T]"""
    depths = np.asarray(forest["depths"], np.int64)
    return obr.heap_leaf_to_oblivious(np.ascontiguousarray(sparse_leaf[:, ::forest["k"]]), depths)


# ---- forests with sets ----
def with_sets(forest, sets, ml=()):
    """A copy of the forest whose splits `sets` = {split index: ids} are category sets; their thr becomes NaN (ignored)"""
    out = dict(forest, thr=np.array(forest["thr"], np.float32), cats={int(s): sorted(int(c) for c in v) for s, v in sets.items()},
               ml=frozenset(int(s) for s in ml))
    for s in out["cats"]:
        out["thr"][s] = np.nan
    return out


def numeric_part(forest):
    return {k: v for k, v in forest.items() if k not in ("cats", "ml")}


def integer_thresholds(forest, W, seed):
    """The forest with every thr an integer in [1, 32 W)"""
    rng = np.random.default_rng(seed)
    return dict(forest, thr=rng.integers(1, 32 * W, len(forest["thr"])).astype(np.float32))


def members_right(forest, W, every=1):
    """Identity 1: split s of threshold k (an integer in [1, 32 W)) -> the set {c : k <= c < 32 W}, members right.  For every x below
    32 W -- negatives, +-0.0, non-integers, -inf, NaN, the sentinel -- x >= k <=> member."""
    return with_sets(forest, {s: range(int(forest["thr"][s]), 32 * W) for s in range(0, len(forest["thr"]), every)})


def members_left_of(forest, W, every=1):
    """Identity 2: split s of threshold k -> the set {c : c < k} with members_left.  For every x >= 0 (+-0.0, values past the words,
    >= 2^24, +inf) and the sentinel, x >= k <=> not member."""
    idx = range(0, len(forest["thr"]), every)
    return with_sets(forest, {s: range(0, int(forest["thr"][s])) for s in idx}, ml=idx)


def identity_data(rows, cols, W, seed, left, missing=MISSING):
    """Rows for an identity: ids around every threshold, non-integers, and what the identity allows of the IEEE values"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 32 * W, (rows, cols)).astype(np.float32)
    frac = rng.random((rows, cols)) < 0.2
    x[frac] += np.float32(0.7)
    x[x >= 32 * W] = np.float32(32 * W - 1)
    if left:  # x >= 0, past the words, >= 2^24, +inf, the sentinel
        special = np.array([missing, 0.0, -0.0, 32.0 * W, 32.0 * W + 5, 2.0 ** 24, 2.0 ** 24 + 2, 3e38, np.inf], np.float32)
    else:  # everything below 32 W
        special = np.array([missing, 0.0, -0.0, -1.0, -2.7, 2.7, -np.inf, np.nan, np.nextafter(np.float32(missing), np.float32(0)),
                            32.0 * W - 0.5], np.float32)
    pick = rng.random((rows, cols)) < 0.3
    x[pick] = rng.choice(special, int(pick.sum()))
    return np.ascontiguousarray(x)


# ---- the GPU tests' forest with genuine sets, and its data ----
def set_kinds():
    """name -> (ids, members_left): empty, one bit, 31 and 32 categories (either side of inline / pooled), three words, one crossing a
    word boundary"""
    return {"empty": ([], False), "one": ([5], False), "one_left": ([0], True), "c31": (list(range(0, 31, 2)) + [30], False),
            "c32": ([1, 4, 31], True), "c33": ([0, 7, 32], False), "three": ([3, 40, 70, 95], False),
            "cross": (list(range(28, 37)), True), "wide_left": ([2, 33, 64, 65], True)}


def sets_forest(depths, cols, k, seed, share=0.5):
    """make_forest with about `share` of the records turned into sets of every kind of set_kinds in turn; the first and the last
    record of the forest, and every level of the deepest tree, are among them; the last set is empty when pooled sets precede it"""
    forest = obr.make_forest(depths, cols, k, seed)
    n = len(forest["thr"])
    rng = np.random.default_rng(seed + 1)
    pick = set(np.flatnonzero(rng.random(n) < share).tolist())
    d = np.asarray(forest["depths"], np.int64)
    off = np.concatenate([[0], np.cumsum(d)])
    if n:
        deepest = int(np.argmax(d))
        pick |= {0, n - 1} | set(range(int(off[deepest]), int(off[deepest + 1])))
        for t in range(d.size):  # a set at level 0 and at the last level of every other tree that has two levels
            if d[t] >= 2 and t % 2 == 0:
                pick |= {int(off[t]), int(off[t + 1]) - 1}
    kinds = list(set_kinds().values())
    sets, ml = {}, []
    for i, s in enumerate(sorted(pick)):
        ids, left = kinds[i % len(kinds)]
        sets[s] = ids
        if left:
            ml.append(s)
    return with_sets(forest, sets, ml)


def sets_data(rows, cols, seed, missing=MISSING):
    """Ids in and around the sets, 2.7, -0.0, negatives, NaN, +-inf, 32 nwords exactly, 2^24, the sentinel and its neighbour"""
    rng = np.random.default_rng(seed)
    ids = np.array([0, 1, 2, 3, 4, 5, 6, 7, 27, 28, 29, 30, 31, 32, 33, 36, 37, 40, 63, 64, 65, 70, 95, 96, 97], np.float32)
    special = np.array([missing, np.nextafter(np.float32(missing), np.float32(0)), 2.7, 5.999, -0.0, -1.0, -0.5, np.nan, np.inf,
                        -np.inf, 32.0, 64.0, 96.0, 2.0 ** 24, 2.0 ** 24 + 2, 4294967296.0 + 5, 0.25, 0.5], np.float32)
    x = rng.choice(ids, (rows, cols)).astype(np.float32)
    pick = rng.random((rows, cols)) < 0.35
    x[pick] = rng.choice(special, int(pick.sum()))
    return np.ascontiguousarray(x)


def pool_bytes(forest):
    """What the sets add to device_bytes: 4 (1 + nwords) per set of two words or more (the header's formula)"""
    return sum(4 * (1 + nwords_of(c)) for c in forest.get("cats", {}).values() if nwords_of(c) >= 2)


def handle_args(forest):
    """The categories / members_left arguments of ObliviousForest"""
    return dict(categories=forest["cats"], members_left=sorted(forest["ml"]))
