"""The edge cases of the vector-leaf handle's walk (vector.hip, forms 27 and 28) and TreeSHAP (vector_contribs_kernel<KB> of
vector_shap.hip), shared by tests/test_vector_edges_ref.py (the references against each other and the shapes the cases rely on,
no GPU) and tests/test_vector_edges_gpu.py (the kernels against the same references): test infrastructure, not product.

  paths     vine31 (one vine on features 0 .. 30 of 40 columns that continues on the left: pre-order meets the two deepest
            leaves first, so the first bin is two 32-lane paths), vine40_on_31 (40 levels on features k % 31: 31 distinct
            features, merged), mixed_len (paths of 2 .. 32 lanes sharing bins, more than 4 bins), each with K in {2, 9} and
            three cover sets; one_col_rounds (stumps on one column: a bin of 32 paths, 32 rounds)
  tiles     one 3-tree forest of depth <= 4 spread over num_cols columns (the first and the last one used), K = 9, at the
            num_cols on both sides of every step of the class-block and tile-row rule (TILE_COLS); K = 2 at 568 / 569 and
            K in {4, 5, 7, 16} at 8 columns
  walk      5 trees on columns 0, 1, num_cols - 2, num_cols - 1 at num_cols 639, 640 (the whole LDS) and 641 (no tile)
  branch    thresholds and data from shap_edges' pools under every `missing` of shap_edges.MISSINGS, K in {1, 3}
  covers    shap_edges.cover_pair's modes on irregular trees, K = 3; the roots' covers are NaN: nothing reads a parent's cover
  leaves    the five_k9 trees over a leaf table of +-3e38, +-1e38, +-inf, NaN, -0.0, 1.0 and 1e-45; and one of -0.0 alone
  K         1023 and 1024 outputs on 3 small trees
  nocols    num_cols = 0: T in {1, 5} single-leaf trees, K in {1, 9}
  deep      a vine of depth 300 beside a stump and a single leaf in one 4-tree window

A case is a dict(forest, covers {label: float32 [num_nodes]}, data, missing); a forest is tests/vector_ref.py's dict.  poly is
the float64 reference of TreeSHAP that needs no subsets: the extend / unwound-sum recursion of tests/contribs_ref.py once per
leaf path, for all K leaf values.  tile_shape restates the class-block and tile-row rule of vector_shap_build."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contribs_ref as cr  # noqa: E402
import shap_edges as se  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

F32 = np.float32
U = 2.0 ** -24
MISSING = vr.MISSING
ROWS = 65
LDS_BUDGET = 80 * 1024   # kVecShapLdsBudget
LDS_DEVICE = 160 * 1024  # the LDS of a CDNA4 compute unit
MIN_ROWS = 4             # kVecShapMinRows
WIDE = np.longdouble     # what poly's recursion runs in: the unwound sum of a 32-element path loses 5 to 6 digits

# num_cols of the tiles cases -> the (KB, R) the rule gives with K = 9
TILE_COLS = {9: (8, 64), 10: (8, 32), 77: (8, 8), 78: (8, 4), 155: (8, 4), 156: (4, 4), 301: (4, 4), 302: (2, 4), 568: (2, 4),
             569: (1, 4), 620: (1, 4), 621: (1, 4), 1024: (1, 4), 1025: (1, 2), 4096: (1, 1), 4097: (1, 1), 8192: (1, 1)}
TILE_REFUSED = 8193
TILE_FORCED = (9, 77, 155, 301, 568, 620, 621, 1024, 4096, 8192)  # one num_cols per row of the issue's table, under every forced KB
TILE_KS = (4, 5, 7, 16)  # at 8 columns: the automatic KB is the largest of 8, 4, 2 below 2 K
WALK_COLS = (639, 640, 641)
COVER_MODES = se.COVER_MODES
LEAF_POOL = np.array([3e38, -3e38, 1e38, -1e38, np.inf, -np.inf, np.nan, -0.0, 1.0, 1e-45], F32)
BIG_KS = (1023, 1024)
PATH_LABELS = ("consistent", "unrelated", "mid")


# ---- the rule of vector_shap_build / tile_rows ----
def tile_rows(F, kb, min_rows):
    per_row, r = (1 + 4 * kb) * F * 4, 64
    while r > 1 and r * per_row > LDS_BUDGET:
        r //= 2
    if kb == 1:
        return r
    return r if (r * per_row <= LDS_BUDGET and r >= min_rows) else 0


def tile_shape(cols, K, forced=None):
    """(KB, R, bytes of dynamic LDS) of a handle of num_cols = cols and K outputs; forced = TAHOE_VECTOR_SHAP_KB"""
    if forced in (1, 2, 4, 8):
        kb = forced if tile_rows(cols, forced, 1) else 1
    else:
        kb = next((c for c in (8, 4, 2) if c < 2 * K and tile_rows(cols, c, MIN_ROWS)), 1)
    R = tile_rows(cols, kb, 1)
    return kb, R, (1 + 4 * kb) * R * cols * 4


def batches(R):
    """Row counts around a tile of R rows"""
    return sorted({r for r in (1, R - 1, R, R + 1, ROWS) if 1 <= r <= ROWS})


# ---- forests ----
def with_classes(forest, k):
    """The first k outputs of every leaf"""
    return dict(forest, leaves=np.ascontiguousarray(forest["leaves"][:, :k]), k=k)


def random_spec(rng, cols, nv, max_depth, leaf_prob, thr_pool=vr.GRID, depth=0):
    if depth >= max_depth or (depth > 0 and rng.random() < leaf_prob):
        return int(rng.integers(0, nv))
    return (int(rng.integers(0, cols)), float(rng.choice(thr_pool)), bool(rng.integers(0, 2)),
            random_spec(rng, cols, nv, max_depth, leaf_prob, thr_pool, depth + 1),
            random_spec(rng, cols, nv, max_depth, leaf_prob, thr_pool, depth + 1))


def vine(rng, feats, nv, side):
    """One internal node per entry of feats, root first; the chain continues on `side` and the other child is a leaf.  Most
    thresholds keep a row on the chain."""
    spec = int(rng.integers(0, nv))
    stay = float(vr.GRID[-1] if side == "left" else vr.GRID[0])
    for fid in reversed(list(feats)):
        thr = stay if rng.random() < 0.8 else float(rng.choice(vr.GRID))
        leaf, dl = int(rng.integers(0, nv)), bool(rng.integers(0, 2))
        spec = (int(fid), thr, dl, spec, leaf) if side == "left" else (int(fid), thr, dl, leaf, spec)
    return spec


def remap(forest, columns, cols):
    """The forest with feature j renamed columns[j], on cols columns"""
    nodes = forest["nodes"].copy()
    inner = nodes["bits"] >= 0
    b = nodes["bits"][inner].astype(np.int64)
    nodes["bits"][inner] = ((b & ~np.int64(vr.FID_MASK)) | np.asarray(columns, np.int64)[b & vr.FID_MASK]).astype(np.int32)
    return dict(forest, nodes=nodes, cols=cols)


def spread(data_small, columns, cols, seed):
    """[rows, cols] of the usual mix whose columns `columns` are data_small's"""
    x = vr.make_data(data_small.shape[0], cols, seed)
    x[:, np.asarray(columns)] = data_small
    return x


def mid_covers(forest, seed):
    """Child covers (r, 1 - r) with r in [0.3, 0.7]; the roots' are 1"""
    nodes = forest["nodes"]
    rng = np.random.default_rng(seed)
    cv = np.ones(nodes.size, F32)
    bounds = list(forest["trees"]) + [nodes.size]
    for t in range(forest["trees"].size):
        lo = int(bounds[t])
        for i in range(lo, int(bounds[t + 1])):
            if nodes["bits"][i] >= 0:
                r = rng.uniform(0.3, 0.7)
                li = lo + int(nodes["left_idx"][i])
                cv[li], cv[li + 1] = r, 1.0 - r
    return cv


def pair_covers(forest, mode, seed):
    """Child covers from shap_edges.cover_pair(mode) under every internal node; the roots' covers are NaN"""
    nodes = forest["nodes"]
    rng = np.random.default_rng(seed)
    cv = np.full(nodes.size, np.nan, F32)
    bounds = list(forest["trees"]) + [nodes.size]
    for t in range(forest["trees"].size):
        lo = int(bounds[t])
        for i in range(lo, int(bounds[t + 1])):
            if nodes["bits"][i] >= 0:
                li = lo + int(nodes["left_idx"][i])
                cv[li], cv[li + 1] = se.cover_pair(rng, mode)
    return cv


def _three_covers(forest, seed):
    return {"consistent": vsr.consistent_covers(forest, seed), "unrelated": vsr.unrelated_covers(forest, seed + 1),
            "mid": mid_covers(forest, seed + 2)}


def _case(forest, covers, data, missing=MISSING):
    return dict(forest=forest, covers=covers, data=data, missing=missing)


TILE_BASE_COLS = 8


def tile_columns(cols):
    """The 8 columns the tiles forest uses at num_cols = cols: column 0, the last one, six spread between them"""
    return np.round(np.linspace(0, cols - 1, TILE_BASE_COLS)).astype(np.int64)


def _tile_base():
    """3 trees of depth <= 4 on 8 features with 16 outputs; trees 0 and 1 split on features 0 and 7 at the root"""
    forest = vr.make_named([4, 3, 4], TILE_BASE_COLS, 16, seed=6100)
    nodes = forest["nodes"].copy()
    for t, fid in ((0, 0), (1, TILE_BASE_COLS - 1)):
        r = int(forest["trees"][t])
        assert nodes["bits"][r] >= 0
        nodes["bits"][r] = (int(nodes["bits"][r]) & ~vr.FID_MASK) | fid
    forest = dict(forest, nodes=nodes)
    return _case(forest, {"consistent": vsr.consistent_covers(forest, 6101)}, vr.make_data(ROWS, TILE_BASE_COLS, seed=6102))


def _walk_base():
    forest = vr.make_named([4, "stump", 3, "leaf", 4], 4, 9, seed=6200)
    return _case(forest, {}, vr.make_data(ROWS, 4, seed=6201))


def _base(name):
    head, _, arg = name.partition(":")
    if head == "vine31":
        rng = np.random.default_rng(6000)
        forest = vr.make([vine(rng, range(31), 13, "left")], vr.mixed_leaves(rng, 13, 9), 9, 40)
        return _case(forest, _three_covers(forest, 6001), vr.make_data(ROWS, 40, seed=6004))
    if head == "vine40_on_31":
        rng = np.random.default_rng(6010)
        forest = vr.make([vine(rng, [k % 31 for k in range(40)], 13, "right")], vr.mixed_leaves(rng, 13, 9), 9, 31)
        return _case(forest, _three_covers(forest, 6011), vr.make_data(ROWS, 31, seed=6014))
    if head == "mixed_len":
        rng = np.random.default_rng(6020)
        specs = [vine(rng, rng.permutation(40)[:31], 13, "right"), random_spec(rng, 40, 13, 4, 0.3), vr.stump(rng, 40, 13),
                 random_spec(rng, 40, 13, 3, 0.3), vine(rng, rng.permutation(40)[:12], 13, "left")]
        forest = vr.make(specs, vr.mixed_leaves(rng, 13, 9), 9, 40)
        return _case(forest, _three_covers(forest, 6021), vr.make_data(ROWS, 40, seed=6024))
    if head == "one_col_rounds":
        rng = np.random.default_rng(6030)
        forest = vr.make([vr.stump(rng, 1, 13) for _ in range(17)], vr.mixed_leaves(rng, 13, 3), 3, 1)
        return _case(forest, _three_covers(forest, 6031), vr.make_data(ROWS, 1, seed=6034))
    if head == "tilebase":
        return _tile_base()
    if head == "walkbase":
        return _walk_base()
    if head == "branch":
        missing = se.MISSINGS[arg]
        rng = np.random.default_rng(6300 + list(se.MISSINGS).index(arg))
        specs = [random_spec(rng, 4, 11, 4, 0.25, se.threshold_pool(missing)) for _ in range(5)]
        forest = vr.make(specs, vr.mixed_leaves(rng, 11, 3), 3, 4)
        return _case(forest, {"consistent": vsr.consistent_covers(forest, 6310)}, se.random_data(rng, ROWS, 4, missing), missing)
    if head == "covers":
        rng = np.random.default_rng(6400)
        specs = [random_spec(rng, 5, 11, d, 0.25) for d in (4, 3, 4, 2)]
        forest = vr.make(specs, vr.mixed_leaves(rng, 11, 3), 3, 5)
        return _case(forest, {arg: pair_covers(forest, arg, 6410 + COVER_MODES.index(arg))}, vr.make_data(ROWS, 5, seed=6402))
    if head == "leaves":
        forest, data, cv = vsr.case("five_k9")
        rng = np.random.default_rng(6500)
        table = rng.choice(LEAF_POOL, forest["leaves"].shape) if arg == "ieee" else np.full(forest["leaves"].shape, -0.0)
        return _case(dict(forest, leaves=np.ascontiguousarray(table, F32)), {"consistent": cv["consistent"]}, data[:ROWS])
    if head == "K":
        rng = np.random.default_rng(6600)
        specs = [random_spec(rng, 5, 11, 3, 0.3), vr.stump(rng, 5, 11), random_spec(rng, 5, 11, 2, 0.3)]
        forest = vr.make(specs, vr.mixed_leaves(rng, 11, max(BIG_KS)), max(BIG_KS), 5)
        return _case(forest, {"consistent": vsr.consistent_covers(forest, 6601)}, vr.make_data(ROWS, 5, seed=6602))
    if head == "nocols":
        T = int(arg[1:])
        rng = np.random.default_rng(6700 + T)
        forest = vr.make([int(rng.integers(0, 7)) for _ in range(T)], vr.mixed_leaves(rng, 7, 9), 9, 0)
        return _case(forest, {"unrelated": vsr.unrelated_covers(forest, 6701)}, np.zeros((ROWS, 0), F32))
    assert head == "deep"
    rng = np.random.default_rng(6800)
    specs = [vr.chain(rng, 6, 11, depth=300), vr.stump(rng, 6, 11), int(rng.integers(0, 11)), random_spec(rng, 6, 11, 3, 0.3)]
    forest = vr.make(specs, vr.mixed_leaves(rng, 11, 3), 3, 6)
    data = vr.make_data(ROWS, 6, seed=6801)
    data[0], data[1] = 3.0, -3.0  # above and below every threshold: the whole chain, and its first step alone
    return _case(forest, {}, data)


PATH_CASES = [f"{n}:k{k}" for n in ("vine31", "vine40_on_31", "mixed_len") for k in (9, 2)] + ["one_col_rounds"]
LONG_CASES = PATH_CASES[:6]
TILE_CASES = [f"tiles:{c}" for c in TILE_COLS] + ["tiles:568:k2", "tiles:569:k2"] + [f"tiles:8:k{k}" for k in TILE_KS]
WALK_CASES = [f"walk:{c}" for c in WALK_COLS]
BRANCH_CASES = [f"branch:{m}:k{k}" for m in se.MISSINGS for k in (3, 1)]
COVER_CASES = [f"covers:{m}" for m in COVER_MODES]
LEAF_CASES = ["leaves:ieee", "leaves:negzero"]
K_CASES = [f"K:{k}" for k in BIG_KS]
NOCOLS_CASES = [f"nocols:T{t}:k{k}" for t in (1, 5) for k in (1, 9)]
DEEP_CASE = "deep"
SHAP_CASES = PATH_CASES + TILE_CASES + BRANCH_CASES + COVER_CASES + K_CASES  # TreeSHAP is held to poly on these
BRUTE_CASES = ["one_col_rounds", "tiles:8:k4", "tiles:8:k16"] + BRANCH_CASES + COVER_CASES + ["K:1023"]  # num_cols <= 8
_bases, _cases, _polys = {}, {}, {}


def _split(name):
    """-> (base name, K or None, num_cols or None)"""
    parts = name.split(":")
    k = int(parts[-1][1:]) if parts[-1][0] == "k" and parts[-1][1:].isdigit() else None
    if k is not None:
        parts = parts[:-1]
    if parts[0] == "tiles":
        return "tilebase", k or 9, int(parts[1])
    if parts[0] == "walk":
        return "walkbase", None, int(parts[1])
    if parts[0] == "K":
        return "K", int(parts[1]), None
    return ":".join(parts), k, None


def _base_of(base):
    if base not in _bases:
        c = _bases[base] = _base(base)
        for a in (c["forest"]["nodes"], c["forest"]["trees"], c["forest"]["leaves"], c["data"], *c["covers"].values()):
            a.setflags(write=False)
    return _bases[base]


def case(name):
    """The case, computed once and read-only"""
    if name not in _cases:
        base, k, cols = _split(name)
        c = _base_of(base)
        forest, data = c["forest"], c["data"]
        if k is not None:
            forest = with_classes(forest, k)
        if base == "tilebase" and cols != TILE_BASE_COLS:
            forest, data = remap(forest, tile_columns(cols), cols), spread(data, tile_columns(cols), cols, 6103)
        if base == "walkbase":
            columns = [0, 1, cols - 2, cols - 1]
            forest, data = remap(forest, columns, cols), spread(data, columns, cols, 6202)
        for a in (forest["nodes"], forest["leaves"], data):
            a.setflags(write=False)
        _cases[name] = dict(c, forest=forest, data=data)
    return _cases[name]


# ---- float64 TreeSHAP without subsets ----
def leaf_paths(forest, covers):
    """Per tree the leaves in pre-order (left first): [(vector index, [(fid, z, [(thr, def_left, right), ...]) per distinct feature
    in order of first appearance])]; z is the product of the cover ratios of the feature's edges (float64)"""
    nodes, trees = forest["nodes"], forest["trees"]
    out = []
    for root in trees:
        root = int(root)
        per_tree, stack = [], [(0, ())]
        while stack:
            i, edges = stack.pop()
            n = nodes[root + i]
            if n["bits"] < 0:
                elems = {}
                for node, right in edges:
                    m = nodes[root + node]
                    li = root + int(m["left_idx"])
                    wl, wr = float(covers[li]), float(covers[li + 1])
                    e = elems.setdefault(int(m["bits"]) & vr.FID_MASK, [1.0, []])
                    e[0] *= (wr if right else wl) / (wl + wr)
                    e[1].append((m["val"], bool(int(m["bits"]) & vr.DEF_LEFT), right))
                per_tree.append((int(n["left_idx"]), [(f, z, ed) for f, (z, ed) in elems.items()]))
                continue
            li = int(n["left_idx"])
            stack += [(li + 1, edges + ((i, True),)), (li, edges + ((i, False),))]
        out.append(per_tree)
    return out


def expectation(forest, covers):
    """[K] float64: sum over the trees of E_t, every leaf vector times the product of the cover ratios on its path"""
    e = np.zeros(forest["k"])
    for per_tree in leaf_paths(forest, covers):
        for vec, elems in per_tree:
            e += forest["leaves"][vec].astype(np.float64) * float(np.prod([z for _, z, _ in elems]))
    return e


def poly(forest, covers, x, missing=MISSING, avg=False, global_bias=0.0):
    """-> (phi, A, N): phi float64 [rows, K, cols + 1], the bias column vector_shap_ref.bias_column's; A the sum of the absolute
    per-path terms behind each value (its bias column |bias|); N [K, cols + 1] their number.  One run of
    contribs_ref._poly_chunk per leaf path with a unit leaf, on the path's own columns, scaled by the K leaf values.  The
    recursion runs in WIDE (long double) and the result is rounded to float64: in float64 the row sums of the 31-feature vines
    miss the float64 margins by up to 8e-10 of the largest value, in long double by 2.5e-13."""
    x = np.ascontiguousarray(x, F32)
    K, F, T = forest["k"], forest["cols"], forest["trees"].size
    rows = x.shape[0]
    phiT, AT, N = np.zeros((K, F + 1, rows), WIDE), np.zeros((K, F + 1, rows), WIDE), np.zeros((K, F + 1))
    for per_tree in leaf_paths(forest, covers):
        for vec, elems in per_tree:
            if not elems:
                continue
            L = len(elems) + 1
            used = [f for f, _, _ in elems]
            unit, a, n = np.zeros((L - 1, rows), WIDE), np.zeros((L - 1, rows), WIDE), np.zeros(L - 1)
            local = [(1.0, [(j, z, ed) for j, (_, z, ed) in enumerate(elems)])]
            cr._poly_chunk(local, L, x[:, used], missing, unit, a, n, WIDE)
            leaf = forest["leaves"][vec].astype(WIDE)
            phiT[:, used, :] += leaf[:, None, None] * unit[None]
            AT[:, used, :] += np.abs(leaf)[:, None, None] * a[None]
            N[:, used] += n[None]
    phi = np.ascontiguousarray(phiT.transpose(2, 0, 1), np.float64)
    A = np.ascontiguousarray(AT.transpose(2, 0, 1), np.float64)
    if avg and T:
        phi /= T
        A /= T
    phi[:, :, F] = vsr.bias_column(forest, covers, avg, global_bias)
    A[:, :, F] = np.abs(phi[:, :, F])
    return phi, A, N


def poly_raw(name, label):
    """poly of the case under covers[label], RAW and without bias (AVG and the bias only scale and shift it), computed once per
    family of cases that differ in K or num_cols alone and sliced: every output is computed on its own, and a column that no
    tree uses is 0"""
    base, k, cols = _split(name)
    if (base, label) not in _polys:
        c = _base_of(base)
        r = poly(c["forest"], c["covers"][label], c["data"], c["missing"])
        for a in r:
            a.setflags(write=False)
        _polys[(base, label)] = r
    phi, A, N = _polys[(base, label)]
    if k is not None:
        phi, A, N = phi[:, :k], A[:, :k], N[:k]
    if base == "tilebase" and cols != TILE_BASE_COLS:
        columns = np.append(tile_columns(cols), cols)
        wide = [np.zeros(a.shape[:-1] + (cols + 1,)) for a in (phi, A, N)]
        for w, a in zip(wide, (phi, A, N)):
            w[..., columns] = a
        phi, A, N = wide
    return phi, A, N


def margins64(forest, data, missing=MISSING):
    """[rows, K] float64: the sum over the trees of the leaf vector tests/vector_ref.vector_ref ends on"""
    _, leaf, _ = vr.vector_ref(forest, data, missing)
    nodes, trees = forest["nodes"], forest["trees"]
    out = np.zeros((data.shape[0], forest["k"]))
    for t, root in enumerate(trees):
        out += forest["leaves"][nodes["left_idx"][int(root) + leaf[:, t].astype(np.int64)]].astype(np.float64)
    return out
