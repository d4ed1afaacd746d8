"""Reference and helpers of the oblivious-forest tests: the rule of tahoe_oblivious_forest_create in numpy, the expansion of an
oblivious forest into complete heap trees (what a dense handle or the CPU oracle takes), and the tests' forests and data."""
import numpy as np

NODE_DTYPE = np.dtype([("weight", "<f4"), ("val", "<f4"), ("bits", "<i4")])
MISSING = -999.0


def oblivious_ref(depths, fids, thr, def_left, leaves, k, data, missing, init=None):
    """-> (margins float32 [rows, k], leaf indices uint32 [rows, trees]).  Level l of a tree: |x - missing| <= 1e-6 takes the
    default branch (right iff not def_left), NaN goes left, else right iff x >= thr; leaf index = sum_l bit_l << l; the margins
    are float32 sums from +0.0 (or init [rows]) over the trees in order.  leaves: flat, (tree, leaf, k)."""
    depths = np.asarray(depths, np.int64)
    fids, thr, def_left = np.asarray(fids, np.int64), np.asarray(thr, np.float32), np.asarray(def_left).astype(bool)
    leaves = np.asarray(leaves, np.float32).reshape(-1, k)
    data = np.asarray(data, np.float32)
    rows = data.shape[0]
    sums = np.zeros((rows, k), np.float32)
    if init is not None:
        sums[:, 0] = init
    leaf = np.zeros((rows, depths.size), np.uint32)
    s = lo = 0
    with np.errstate(invalid="ignore"):
        for t, d in enumerate(depths):
            idx = np.zeros(rows, np.int64)
            for l in range(d):
                x = data[:, fids[s]]
                miss = np.abs(x - np.float32(missing)) <= np.float32(1e-6)
                right = np.where(miss, not def_left[s], x >= thr[s])
                idx |= right.astype(np.int64) << l
                s += 1
            leaf[:, t] = idx
            sums = sums + leaves[lo + idx]  # float32 + float32, tree order
            lo += 1 << d
    return sums, leaf


def bitreverse(p, d):
    p = np.asarray(p, np.int64)
    r = np.zeros_like(p)
    for b in range(d):
        r |= ((p >> b) & 1) << (d - 1 - b)
    return r


def expand_to_dense(depths, fids, thr, def_left, leaves, k, cls=0):
    """Heap trees of depth D = max(depths) (2^(D+1) - 1 nodes each, tree-major) for output `cls` of the k: level l of every tree
    carries split l, a tree of depth d < D has its leaves at level d, and the leaf at heap position p of level d -- its bits are in
    root-first order -- takes leaves[bitreverse_d(p)][cls].  -> (nodes, D)"""
    depths = np.asarray(depths, np.int64)
    leaves = np.asarray(leaves, np.float32).reshape(-1, k)
    D = int(depths.max()) if depths.size else 0
    per = (1 << (D + 1)) - 1
    nodes = np.zeros(depths.size * per, NODE_DTYPE)
    nodes["bits"] = np.int32(-(1 << 31))  # below the leaves: never reached
    s = lo = 0
    for t, d in enumerate(depths):
        tree = nodes[t * per:(t + 1) * per]
        for l in range(d):
            level = tree[(1 << l) - 1:(1 << (l + 1)) - 1]
            level["val"] = thr[s]
            level["bits"] = np.int32(int(fids[s]) | (int(bool(def_left[s])) << 30))
            s += 1
        tree["val"][(1 << d) - 1:(1 << (d + 1)) - 1] = leaves[lo + bitreverse(np.arange(1 << d), d), cls]
        lo += 1 << d
    return nodes, D


def heap_leaf_to_oblivious(heap_leaf, depths):
    """Leaf indices in heap numbering (a dense handle's, the oracle's) -> the oblivious numbering"""
    out = np.empty_like(heap_leaf)
    for t, d in enumerate(np.asarray(depths, np.int64)):
        out[:, t] = bitreverse(heap_leaf[:, t].astype(np.int64) - ((1 << d) - 1), d)
    return out


GRID = np.array([-2.0, -1.0, -0.5, -0.0, 0.0, 0.25, 0.5, 1.0, 2.0], np.float32)  # thresholds and most data values: ties abound


def make_forest(depths, cols, k, seed):
    """-> dict(depths, fids, thr, def_left, leaves [flat], k, cols): thresholds from GRID, leaves of mixed magnitude so that the
    float32 sum depends on its order"""
    rng = np.random.default_rng(seed)
    depths = np.asarray(depths, np.int32)
    n = int(depths.sum())
    fids = rng.integers(0, max(cols, 1), n)
    thr = rng.choice(GRID, n).astype(np.float32)
    def_left = rng.integers(0, 2, n).astype(bool)
    nleaf = int((1 << depths.astype(np.int64)).sum())
    leaves = (rng.standard_normal(nleaf * k) * 10.0 ** rng.integers(-3, 4, nleaf * k)).astype(np.float32)
    return dict(depths=depths, fids=fids, thr=thr, def_left=def_left, leaves=leaves, k=k, cols=cols)


def make_data(rows, cols, seed, missing=MISSING):
    """Rows over GRID (ties on the thresholds, +-0.0) with the sentinel, a value within 1e-6 of it, NaN and +-inf mixed in"""
    rng = np.random.default_rng(seed)
    special = np.array([missing, np.nextafter(np.float32(missing), np.float32(0)), np.nan, np.inf, -np.inf, -0.0, 0.0,
                        np.float32(3.4028235e38), np.float32(1e-45)], np.float32)
    x = rng.choice(GRID, (rows, cols)).astype(np.float32)
    pick = rng.random((rows, cols)) < 0.35
    x[pick] = rng.choice(special, int(pick.sum()))
    return np.ascontiguousarray(x)


def ref_of(forest, data, missing=MISSING, init=None):
    return oblivious_ref(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], forest["k"], data,
                         missing, init)


def dense_of(forest, cls=0):
    return expand_to_dense(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], forest["k"], cls)
