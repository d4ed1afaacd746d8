"""The forests and rows of the TAHOE_CREATE_CAT_CONTRIBS tests, shared by the CPU and the GPU file: test infrastructure.

twin(): sparse trees whose every internal node tests an integer k in [1, 63], as a numeric threshold (x >= k), as the set
{c : c >= k} of two words with members going right, and as the set {c : c < k} with members going left.  On integers of [0, 64)
the three rules agree; NaN and negatives go left under the first two only.
mixed(): random irregular trees whose internal nodes are numeric or categorical at random (sets of 0, 1, 2 or 5 words, members
left or right at random), plus one tree written by hand that holds what a random draw may miss."""
import numpy as np

import cat_shap_ref as cref

MISSING = -999.0
LEAF = np.int32(-(1 << 31))


def _inner(sn):
    return np.nonzero((sn["bits"].view(np.uint32) >> 31) == 0)[0]


def twin(ta, T=12, F=6, seed=11):
    """(numeric nodes, roots, B = {node: ids >= k}, C = {node: ids < k} with every node in members_left)."""
    sn, tr = ta.capi.synth_sparse_forest(T, F, 3, 8, 0.3, 200, seed)
    rng = np.random.default_rng(seed)
    sn = sn.copy()
    ge, lt = {}, {}
    for i in _inner(sn):
        k = int(rng.integers(1, 64))
        sn["val"][i] = np.float32(k)
        ge[int(i)] = range(k, 64)
        lt[int(i)] = range(0, k)
    return sn, tr, ge, lt


def twin_rows(rows, F, seed, odd=True):
    """Integers of [0, 64), 10 % missing, and (odd) a few NaN and -1."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 64, (rows, F)).astype(np.float32)
    x[rng.random((rows, F)) < 0.1] = MISSING
    if odd:
        x[rng.random((rows, F)) < 0.04] = np.nan
        x[rng.random((rows, F)) < 0.04] = -1.0
    return x


def _random_set(rng, nwords):
    if nwords == 0:
        return []
    ids = set(int(c) for c in np.nonzero(rng.random(32 * nwords) < 0.5)[0])
    ids.add(32 * (nwords - 1) + int(rng.integers(32)))  # the top word is not empty: the split keeps nwords words
    return sorted(ids)


def _hand_tree(F):
    """One path (right, right, left, ...) crosses two need = 1 edges on feature 0 with disjoint sets of 1 and 2 words (its
    element never follows) and a numeric edge on the same feature; node 6 is an empty set (no words) whose members go left."""
    sn = np.zeros(9, dtype=[("val", "<f4"), ("bits", "<i4"), ("left_idx", "<i4")])
    sn[0] = (0.0, 0, 1)
    sn[1] = (0.75, LEAF, 0)
    sn[2] = (0.0, 0 | 1 << 30, 3)
    sn[3] = (-0.5, LEAF, 0)
    sn[4] = (2.5, 0, 5)
    sn[5] = (0.25, LEAF, 0)
    sn[6] = (0.0, 1 % F, 7)
    sn[7] = (-1.0, LEAF, 0)
    sn[8] = (0.625, LEAF, 0)
    return sn, {0: [1, 2, 3], 2: [40, 41], 6: []}, {6}


def mixed(ta, F, seed):
    """(CatForest, covers): five random trees of depth <= 10 and <= 300 nodes and the hand tree; covers in [0.05, 1]."""
    sn, tr = ta.capi.synth_sparse_forest(5, F, 3, 10, 0.45, 300, seed)
    rng = np.random.default_rng(seed)
    sn = sn.copy()
    cats, left = {}, set()
    for i in _inner(sn):
        if rng.random() < 0.6:
            cats[int(i)] = _random_set(rng, int(rng.choice([0, 1, 2, 5])))
            if rng.random() < 0.5:
                left.add(int(i))
        else:
            sn["val"][i] = np.float32(rng.integers(0, 170) + 0.5)
    hand, hcats, hleft = _hand_tree(F)
    off = sn.size
    cats.update({k + off: v for k, v in hcats.items()})
    left |= {k + off for k in hleft}
    sn = np.concatenate([sn, hand.astype(sn.dtype)])
    tr = np.append(tr, off).astype(np.int32)
    covers = rng.uniform(0.05, 1.0, sn.size).astype(np.float32)
    return cref.CatForest(sn, tr, cats, left), covers


def mixed_rows(rows, F, seed):
    """Ids inside and beyond every set's words, 2.7, -0.0, -3, NaN, 2^24 and the sentinel."""
    rng = np.random.default_rng(seed)
    pool = np.array([0, 1, 2, 3, 31, 32, 40, 41, 63, 64, 100, 159, 160, 200, 2.7, -0.0, -3.0, np.nan, 2.0 ** 24, MISSING], np.float32)
    x = rng.choice(pool, (rows, F)).astype(np.float32)
    some = rng.random((rows, F)) < 0.4
    x[some] = rng.integers(0, 170, int(some.sum())).astype(np.float32)
    return x
