"""Partial dependence at the edges (numpy only): the forests, grids and expectations of tests/test_pd_edges_ref.py and
tests/test_pd_edges_gpu.py, on the node layout and the references of tests/pd_cases.py and tests/pd_ref.py.

order_forest / ORDER_CASES: many tiny trees whose leaves carry one power-of-ten scale per tree over six decades, so that the
float32 sum over a class's trees depends on the order of its adds; the tree counts put class_trees on both sides of 16, 32 and
48 (pd_sum_kernel adds blocks of 16, then a tail) and leave 0, 1, 2 and 3 trees to the walk's last workgroup of four.
IEEE_CASES: subnormal fractions and sums, a weight that underflows to 0 above an infinite leaf, -0.0 leaves, infinities that meet
in the sum over trees, a mix.  STRUCTURE_CASES: root leaves, stumps beside them, no trees, nodes before the first root, an
internal node no path reaches, a feature id with bit 29 set.

A case is a forest dict as pd_cases builds them with three more keys: `targets` (the listed target columns), `grid`
([G, len(targets)] float32) and `expect` ({run: uint32 bits every output of that run must have}, hand-derived; run is "none",
"listed" or "all", see runs())."""
import numpy as np

import pd_cases
import pd_ref
import shap_edges

F32 = np.float32
LEAF = pd_cases.LEAF
NODE = pd_cases.SPARSE_NODE_DTYPE


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """Equal in every bit where `want` is not NaN, NaN where it is (x86 makes the negative default NaN, the GPU the positive one;
    payloads are not compared).  For cases that can hold NaN only."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(bits(got)[~nan], bits(want)[~nan]) and np.isnan(got[nan]).all())


def forest(nodes, trees, covers, num_cols, num_classes=1, **more):
    fo = dict(nodes=np.asarray(nodes, dtype=NODE), trees=np.asarray(trees, np.int32), covers=np.asarray(covers, np.float32),
              num_cols=num_cols, num_classes=num_classes, missing=pd_cases.MISSING, cats=None, categories=None, members_left=(),
              cat_features=())
    fo.update(more)
    return fo


def split_features(fo):
    """The features the reachable and unreachable internal nodes of the trees split on, ascending."""
    b = np.ascontiguousarray(fo["nodes"]["bits"][int(fo["trees"][0]):] if len(fo["trees"]) else fo["nodes"]["bits"][:0])
    return sorted({int(x) & pd_ref.FID_MASK for x in b if x >= 0})


def runs(case):
    """(run, targets, grid) three times: no targets, the listed ones, every split feature a target."""
    G = case["grid"].shape[0]
    yield "none", [], np.zeros((G, 0), F32)
    yield "listed", list(case["targets"]), case["grid"]
    feats = split_features(case)
    grid = case["grid_all"] if "grid_all" in case else pd_cases.random_grid(case, feats, G, seed=3)
    yield "all", feats, grid


def want_f32(fo, feats, grid):
    return pd_ref.pd_f32(fo["nodes"], fo["trees"], fo["covers"], feats, grid, fo["missing"], fo["num_classes"], fo["cats"])


def want_f64(fo, feats, grid):
    """(pd float64, bound) of pd_ref."""
    pd, A = pd_ref.pd_f64(fo["nodes"], fo["trees"], fo["covers"], feats, grid, fo["missing"], fo["num_classes"], fo["cats"])
    return pd, pd_ref.bound(fo["nodes"], fo["trees"], A)


# ---- tree-order sums ----
ORDER_CASES = [(15, 1), (16, 1), (17, 1), (18, 1), (31, 1), (32, 1), (33, 1), (49, 1), (51, 3), (96, 3), (99, 3)]
ORDER_TARGETS = [1, 4]
ORDER_G = 130  # three tiles, the last with two points


def order_forest(T, C, seed=None):
    """T trees of depth <= 3 on 6 columns, no zero covers; tree t's leaves times 10^u_t, u_t uniform in [-3, 3).  The seed
    40 + T meets the three conditions of tests/test_pd_edges_ref.py for every entry of ORDER_CASES."""
    seed = 40 + T if seed is None else seed
    fo = pd_cases.random_forest(seed=seed, num_trees=T, num_cols=6, max_depth=3, leaf_prob=0.25, num_classes=C, zero_cover_prob=0)
    rng = np.random.default_rng(1000 + seed)
    scale = (10.0 ** rng.uniform(-3, 3, T)).astype(F32)
    ends = list(fo["trees"][1:]) + [fo["nodes"].size]
    for t in range(T):
        sl = slice(int(fo["trees"][t]), int(ends[t]))
        leaf = fo["nodes"]["bits"][sl] < 0
        fo["nodes"]["val"][sl] = np.where(leaf, fo["nodes"]["val"][sl] * scale[t], fo["nodes"]["val"][sl])
    return fo


def order_case(T, C, G=ORDER_G, seed=None):
    fo = order_forest(T, C, seed)
    fo["targets"] = list(ORDER_TARGETS)
    fo["grid"] = pd_cases.random_grid(fo, ORDER_TARGETS, G, seed=T)
    return fo


def tree_values(fo, feats, grid):
    """[T, G] float32: acc of every tree at every grid point (pd_ref._walk)."""
    targets, grid, covers, splits = pd_ref._prepare(fo["nodes"], fo["trees"], fo["covers"], feats, grid, fo["cats"])
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([pd_ref._walk(fo["nodes"], int(r), covers, targets, grid, fo["missing"], splits, F32)[0] for r in fo["trees"]])


def ordered_sum(vals, order):
    """The float32 sum from +0.0f of vals[order[0]], vals[order[1]], ..."""
    s = np.zeros(vals.shape[1], F32)
    for j in order:
        s = s + vals[j]
    return s


# ---- IEEE cases ----
def stump(fid, covers, leaves, num_cols, thr=0.0):
    sn = np.zeros(3, dtype=NODE)
    sn[0] = (thr, fid, 1)
    sn[1] = (leaves[0], LEAF, 0)
    sn[2] = (leaves[1], LEAF, 0)
    cv = np.array([F32(covers[0]) + F32(covers[1]), covers[0], covers[1]], F32)
    return sn, cv


def _full(G, nt, v):
    return np.full((G, nt), v, F32)


def tiny_fraction():
    """fl = 2^-100 / 2^40 = 2^-140 (subnormal), fr = 1: acc = 2^-140 * 2^120 + 1 * 3 = 3 + 2^-20, exact in float32.  With
    subnormals flushed fl is 0, the left leaf is not visited and the value is 3."""
    sn, cv = stump(1, (2.0 ** -100, 2.0 ** 40), (2.0 ** 120, 3.0), num_cols=2)
    e = bits(F32(3.0 + 2.0 ** -20))
    return forest(sn, [0], cv, 2, id="tiny_fraction", targets=[0], grid=_full(5, 1, 0.5), expect={"none": e, "listed": e})


def subnormal_sum():
    """fl = 1/4, fr = 3/4: 2^-132 + 3 * 2^-142 = (131072 + 384) * 2^-149: products and sum subnormal, all exact."""
    sn, cv = stump(1, (1.0, 3.0), (2.0 ** -130, 2.0 ** -140), num_cols=2)
    e = np.uint32(0x00020180)
    return forest(sn, [0], cv, 2, id="subnormal_sum", targets=[0], grid=_full(5, 1, 0.5), expect={"none": e, "listed": e})


UNDERFLOW_DEPTH = 32


def weight_underflow():
    """The 32-chain with fl = 1/32 at every level: the left weight is 2^-5d, 2^-145 at level 29 and exactly 0 from level 30 on
    (2^-150 is half the smallest subnormal: ties to even).  The fractions are not 0, so the walk goes on, and the bottom-left
    leaf +inf adds 0 * inf = NaN.  With every split a target and the grid at -1 the leaf is reached with w = 1: +inf."""
    fo = pd_cases.chain(UNDERFLOW_DEPTH)
    for d in range(UNDERFLOW_DEPTH):
        fo["covers"][2 * d + 1], fo["covers"][2 * d + 2] = 1.0, 31.0
    fo["nodes"]["val"][2 * UNDERFLOW_DEPTH - 1] = np.inf
    grid_all = np.where(np.random.default_rng(8).random((5, 32)) < 0.9, -1.0, 1.0).astype(F32)
    grid_all[0] = -1.0
    fo.update(id="weight_underflow", targets=[32], grid=_full(5, 1, 0.0), grid_all=grid_all, expect={})
    return fo


def minus_zero():
    """+0 + (w * -0) = +0 + -0 = +0 at every add from +0.0f, in the walk and in the sum over trees."""
    sn, cv = stump(0, (1.0, 1.0), (-0.0, -0.0), num_cols=1)
    grid = np.array([[-1.0], [1.0], [np.nan], [pd_cases.MISSING]], F32)
    e = np.uint32(0)
    return forest(sn, [0], cv, 1, id="minus_zero", targets=[0], grid=grid, grid_all=grid, expect={"none": e, "listed": e, "all": e})


def inf_trees():
    """Root leaves, two classes: class 0 adds +inf and -inf (NaN), class 1 adds 3e38 twice (+inf)."""
    sn = np.zeros(4, dtype=NODE)
    for t, v in enumerate((np.inf, 3e38, -np.inf, 3e38)):
        sn[t] = (v, LEAF, 0)
    return forest(sn, [0, 1, 2, 3], np.ones(4, F32), 1, num_classes=2, id="inf_trees", targets=[0], grid=_full(5, 1, 0.0), expect={})


MIX_LEAVES = np.array([3e38, -3e38, np.inf, -np.inf, np.nan, -0.0, 1e-45, 2.0 ** -126, 1.5, -0.375], F32)


# one NaN leaf makes its class NaN at every point that reaches it, so the four classes draw from four pools: everything; what
# overflows; what stays at and below the smallest normal number; +inf beside ordinary values
MIX_POOLS = (MIX_LEAVES, MIX_LEAVES[[0, 1, 8, 9]], np.array([-0.0, 1e-45, 2.0 ** -126, -2.0 ** -126, 3e-39], F32), MIX_LEAVES[[2, 5, 8, 9]])


def ieee_mix():
    """8 random trees in 4 classes; the leaves of class c from MIX_POOLS[c], child covers from shap_edges' pools where create
    accepts the pair (the pools are >= 0 and finite with a positive sum; a pair whose float32 sum overflows is drawn again)."""
    fo = pd_cases.random_forest(seed=71, num_trees=8, num_cols=6, max_depth=3, leaf_prob=0.25, num_classes=4, zero_cover_prob=0)
    rng = np.random.default_rng(72)
    dealt = 0
    nd, cv = fo["nodes"], fo["covers"]
    ends = list(fo["trees"][1:]) + [nd.size]
    with np.errstate(over="ignore"):
        for t, root in enumerate(fo["trees"]):
            for i in range(int(root), int(ends[t])):
                if nd["bits"][i] < 0:
                    nd["val"][i] = rng.choice(MIX_POOLS[t % 4]) if t % 4 else MIX_LEAVES[dealt % MIX_LEAVES.size]
                    dealt += t % 4 == 0  # class 0 (two trees of at least four leaves) is dealt every value in turn
                    continue
                l = int(root) + int(nd["left_idx"][i])
                while True:
                    a, b = shap_edges.cover_pair(rng, "mixed")
                    if np.isfinite(F32(a) + F32(b)):
                        break
                cv[l], cv[l + 1] = a, b
    fo.update(id="ieee_mix", targets=[1, 4], grid=pd_cases.random_grid(fo, [1, 4], 70, seed=73), expect={})
    return fo


IEEE_CASES = {f.__name__: f for f in (tiny_fraction, subnormal_sum, weight_underflow, minus_zero, inf_trees, ieee_mix)}
FINITE_IEEE = ("tiny_fraction", "subnormal_sum", "minus_zero")


# ---- structure cases ----
def root_leaves():
    sn = np.zeros(5, dtype=NODE)
    for t in range(5):
        sn[t] = (0.5 + t, LEAF, 0)
    return forest(sn, np.arange(5), np.ones(5, F32), 2, id="root_leaves", targets=[1], grid=_full(70, 1, 0.25), expect={})


def stumps_and_leaves():
    """Depth 0 and depth 1 in turn, two classes: class 0 gets leaf, stump, leaf; class 1 stump, leaf, stump."""
    rng = np.random.default_rng(5)
    nodes, covers, trees = [], [], []
    for t in range(6):
        trees.append(sum(len(n) for n in nodes))
        if t in (0, 3, 4):
            sn = np.zeros(1, dtype=NODE)
            sn[0] = (F32(rng.normal()), LEAF, 0)
            cv = np.ones(1, F32)
        else:
            sn, cv = stump(t % 3, rng.uniform(1, 9, 2).astype(F32), rng.normal(size=2).astype(F32), 3, thr=0.25)
        nodes.append(sn)
        covers.append(cv)
    fo = forest(np.concatenate(nodes), trees, np.concatenate(covers), 3, num_classes=2, id="stumps_and_leaves", targets=[2, 0], expect={})
    fo["grid"] = pd_cases.random_grid(fo, [2, 0], 70, seed=6)
    return fo


def no_trees(C):
    return forest(np.zeros(0, dtype=NODE), np.zeros(0, np.int32), np.zeros(0, F32), 4, num_classes=C, id=f"no_trees_C{C}", targets=[2],
                  grid=_full(70, 1, 0.5), expect={})


def prefix(C, with_prefix=True):
    """Six random trees behind three leaf records with NaN covers that belong to no tree; with_prefix=False: the plain twin."""
    fo = pd_cases.random_forest(seed=81, num_trees=6, num_cols=6, max_depth=3, leaf_prob=0.25, num_classes=C, zero_cover_prob=0)
    fo.update(id=f"prefix_C{C}", targets=[0, 3], grid=pd_cases.random_grid(fo, [0, 3], 70, seed=82), expect={})
    if with_prefix:
        pre = np.zeros(3, dtype=NODE)
        pre["val"], pre["bits"] = (7.0, -7.0, np.inf), LEAF
        fo["nodes"] = np.concatenate([pre, fo["nodes"]])
        fo["covers"] = np.concatenate([np.full(3, np.nan, F32), fo["covers"]])
        fo["trees"] = fo["trees"] + np.int32(3)
    return fo


def unreachable(plain=False):
    """Two trees.  Tree 0: the root's children are nodes 1 (internal, children 4 and 5) and 2 (a leaf); node 3, between them, is
    an internal node with children 6 and 7 that nothing points to, and their covers are NaN and -1.  plain=True: nodes 3, 6 and
    7 are leaves with cover 1."""
    sn = np.zeros(8, dtype=NODE)
    sn[0] = (0.25, 0, 1)
    sn[1] = (-0.5, 1, 4)
    sn[2] = (2.0, LEAF, 0)
    sn[3] = (9.0, LEAF, 0) if plain else (0.0, 2, 6)
    sn[4] = (-1.25, LEAF, 0)
    sn[5] = (0.75, LEAF, 0)
    sn[6] = (100.0, LEAF, 0)
    sn[7] = (-100.0, LEAF, 0)
    cv = np.array([10, 6, 4, 1, 1.5, 4.5, 1 if plain else np.nan, 1 if plain else -1], F32)
    sn2, cv2 = stump(2, (2.0, 5.0), (0.5, -3.0), 3)
    fo = forest(np.concatenate([sn, sn2]), [0, 8], np.concatenate([cv, cv2]), 3, id="unreachable", targets=[1], expect={})
    fo["grid"] = np.array([[-1.0], [-0.5], [0.0], [np.nan], [pd_cases.MISSING]], F32)
    return fo


HIGH_FID = (1 << 29) + 1


def high_fid():
    """No category sets: the feature id has 30 bits.  One stump on feature 2^29 + 1, x >= 0.5 right, covers 1 / 3: as a target
    the branch (10 or 20); with target 1 -- what a 29-bit mask would make of it -- the mean 0.25 * 10 + 0.75 * 20 = 17.5."""
    sn, cv = stump(HIGH_FID, (1.0, 3.0), (10.0, 20.0), HIGH_FID + 1, thr=0.5)
    grid = np.array([[0.0], [0.5], [1.0], [np.nan]], F32)
    return forest(sn, [0], cv, HIGH_FID + 1, id="high_fid", targets=[HIGH_FID], grid=grid, target_lists=[[HIGH_FID], [1]],
                  expect={(HIGH_FID,): bits(F32([10, 20, 20, 10])), (1,): bits(F32([17.5] * 4))})


STRUCTURE_CASES = {"root_leaves": root_leaves, "stumps_and_leaves": stumps_and_leaves, "prefix_C1": lambda: prefix(1),
                   "prefix_C2": lambda: prefix(2), "unreachable": unreachable}
TWINS = {"prefix_C1": lambda: prefix(1, False), "prefix_C2": lambda: prefix(2, False), "unreachable": lambda: unreachable(True)}
