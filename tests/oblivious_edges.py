"""The edge cases of the oblivious handle's explanations and walks, shared by tests/test_oblivious_edges_capi.py (the references
against each other, no GPU) and tests/test_oblivious_edges_gpu.py (the kernels against the same references): test
infrastructure, not product.

  elements  one tree of depth M on M distinct features for every M = 1 .. 16 (each ob_shap_tree<M, ., .> of
            oblivious_shap.hip), depth 16 on M in {7, 9, 13} repeated features, and one forest whose trees of different M share
            columns; class counts 1, 5 (a full class block and one of a single class) and 8 (two full blocks)
  covers    leaf-cover pools on one forest: zeros, 1e-30 .. 1e30, ratios within 1e-8 of 1, float32 subnormals, covers whose
            float32 sum overflows, and products on both sides of the 2^-121 cut
  branch    thresholds and data from shap_edges' pools (+-0, +-inf, NaN, subnormals, the sentinel, the edges of the missing
            band) under every `missing` of shap_edges.MISSINGS
  leaves    the covers forest with leaves near FLT_MAX: Saabas deltas that overflow
  inter     SHAP interaction values only: no tree, trees of depth 0 alone, three used columns of 300, one column (no pair), and
            the multi forest with exactly one full class block (K = 4)

A case is a dict(forest, covers, data, missing, avg, bias, cut); cut says that its covers may put a zero fraction below 2^-121,
so that its bar carries the floor (the cover cases; every other case is held to the bar alone).  reference(name) adds poly's
(phi, A, N), emulate's and saabas' phi, computed once and read-only.  The cases of one element count share one forest of the most classes any of them needs and slice
its leaves: every class is computed on its own, so the references of the widest forest serve them all.

inter_reference(name) does the same for predict_interactions with tests/oblivious_inter_ref.py: 'poly' = (Phi, A, N) in float64
and 'emulate', the kernel's bits.  A family of 13 or more elements keeps its first 3 rows there (poly holds M 2^D rows doubles
per conditioned element), which still leaves 61 lanes past the batch; poly is left out at M = 16 alone, where it takes 18 s
(8 s at M = 15): the m:16 cases are held to emulate's bits and to the structural properties."""
from __future__ import annotations

import numpy as np

import oblivious_inter_ref as oir
import oblivious_ref as obr
import oblivious_shap_ref as osr
import shap_edges as se

F32 = np.float32
U = 2.0 ** -24
MISSING = obr.MISSING

ELEMENT_COUNTS = tuple(range(1, 17))
MERGED = (7, 9, 13)                      # depth 16 on this many distinct features
MULTI_DEPTHS = [7, 9, 8, 11, 7]
COVER_DEPTHS = [0, 1, 6, 8, 3, 6]        # the depth-8 tree is on 8 distinct features
COVER_POOLS = ("int", "zero", "most", "span", "near_one", "subnormal", "f32_overflow", "cut", "mixed")
# the pools in which every subtree cover is a positive finite float32: only there can the heap expansion carry the same covers
# as node weights.  The others hold zero covers (the expansion's 1/2 : 1/2 mix under a node of weight 0 is this handle's rule,
# not the dense one's), subnormal sums, or sums past FLT_MAX.
EXPANSION_POOLS = ("int", "span", "near_one")
OVERFLOW_LEAVES = np.array([3e38, -3e38, 1e38, -1e38, 1.0, -0.0], F32)
WIDE_COLS, WIDE_USED, WIDE_DEPTHS = 300, (0, 149, 299), [3, 5, 2]
WIDE_FIDS = [0, 1, 0, 1, 2, 0, 2, 1, 2, 0]  # of WIDE_USED, level by level: every pair shares a tree, features repeat within one
INTER_DEEP = 13       # from this many elements on the interaction references keep INTER_DEEP_ROWS rows
INTER_DEEP_ROWS = 3
INTER_POLY_MAX = 15   # the most elements of an element case with a float64 poly (module docstring)


def element_classes(M):
    return (1, 5, 8) if M in (7, 16) else (1, 5)


def element_rows(M):
    return 65 if M <= 10 else 5  # poly holds (M + 1) 2^M rows doubles; both counts leave lanes past the batch


def inter_rows(name):
    """How many of the case's rows the interaction references and tests use"""
    parts = name.split(":")
    M = int(parts[1]) if parts[0] == "m" else 0
    return INTER_DEEP_ROWS if M >= INTER_DEEP else case(name)["data"].shape[0]


def has_inter_poly(name):
    parts = name.split(":")
    return parts[0] != "m" or int(parts[1]) <= INTER_POLY_MAX


def with_classes(forest, k):
    """The first k outputs of every leaf"""
    leaves = np.asarray(forest["leaves"], F32).reshape(-1, forest["k"])[:, :k]
    return dict(forest, leaves=np.ascontiguousarray(leaves).reshape(-1), k=k)


def make_covers(forest, pool, seed):
    """One float32 cover per leaf from the pool (module docstring); 'int', 'most' and 'zero' are oblivious_shap_ref's"""
    rng = np.random.default_rng(seed)
    n = int((1 << np.asarray(forest["depths"], np.int64)).sum())
    if pool in ("int", "half", "most", "zero"):
        return osr.make_covers(forest, pool, seed)
    if pool == "span":
        c = 10.0 ** rng.uniform(-30, 30, n)
    elif pool == "near_one":
        c = np.where(rng.random(n) < 1 / 3, 1e8, 1.0)
    elif pool == "subnormal":
        c = rng.choice(np.array([1e-45, 1e-40, 1.1754944e-38, 0.0, 1.0]), n)
    elif pool == "f32_overflow":
        c = rng.choice(np.array([3e38, 2e38, 1e38, 1.0]), n)
    elif pool == "cut":
        c = rng.choice(np.array([1.0, 2.0 ** -60, 2.0 ** -61, 2.0 ** -121, 2.0 ** -122]), n)
    else:
        assert pool == "mixed"
        pools = [p for p in COVER_POOLS if p != "mixed"]
        each = np.stack([make_covers(forest, p, seed + 1 + i) for i, p in enumerate(pools)])
        c = each[rng.integers(0, len(pools), n), np.arange(n)]
    return np.asarray(c, F32)


def _case(forest, covers, data, missing=MISSING, avg=False, bias=0.0, cut=False):
    return dict(forest=forest, covers=covers, data=data, missing=missing, avg=avg, bias=bias, cut=cut)


def _base(name):
    """The widest forest of a family of cases, which differ in their class count alone"""
    head, _, arg = name.partition(":")
    if head == "m":
        M = int(arg)
        forest = obr.make_forest([M], M, max(element_classes(M)), seed=4000 + M)
        forest["fids"][:] = np.arange(M)
        return _case(forest, osr.make_covers(forest, "half", seed=4100 + M), obr.make_data(element_rows(M), M, seed=4200 + M))
    if head == "merged":
        M = int(arg)
        forest = obr.make_forest([16], M, 1, seed=4300 + M)
        forest["fids"][:] = np.arange(16) % M
        return _case(forest, osr.make_covers(forest, "half", seed=4400 + M), obr.make_data(3, M, seed=4500 + M))
    if head == "multi":
        forest = obr.make_forest(MULTI_DEPTHS, 12, 3, seed=4600)
        return _case(forest, osr.make_covers(forest, "half", seed=4601), obr.make_data(65, 12, seed=4602), avg=arg == "avg",
                     bias=-0.375)
    if head in ("covers", "leaves"):
        forest = obr.make_forest(COVER_DEPTHS, 8, 3 if head == "covers" else 2, seed=4700)
        s = int(np.sum(COVER_DEPTHS[:3]))
        forest["fids"][s:s + 8] = np.arange(8)
        if head == "leaves":
            forest["leaves"] = np.random.default_rng(4703).choice(OVERFLOW_LEAVES, forest["leaves"].size).astype(F32)
            arg = "half"
        return _case(forest, make_covers(forest, arg, seed=4710 + COVER_POOLS.index(arg) if arg in COVER_POOLS else 4709),
                     obr.make_data(65, 8, seed=4702), cut=head == "covers")
    if head == "inter":
        return _inter_base(arg)
    assert head == "branch"
    missing = se.MISSINGS[arg]
    rng = np.random.default_rng(4800 + list(se.MISSINGS).index(arg))
    forest = obr.make_forest([1, 2, 3, 4, 5, 6] * 4, 6, 2, seed=4810)
    forest["thr"] = rng.choice(se.threshold_pool(missing), forest["thr"].size).astype(F32)
    forest["def_left"] = rng.integers(0, 2, forest["thr"].size).astype(bool)
    return _case(forest, osr.make_covers(forest, "half", seed=4820), se.random_data(rng, 257, 6, missing), missing=missing)


def _inter_base(arg):
    """The interaction-only families (module docstring)"""
    if arg == "none:empty":
        forest = obr.make_forest([], 4, 2, seed=4900)
        return _case(forest, np.zeros(0, F32), obr.make_data(65, 4, seed=4901), bias=0.25)
    if arg == "none:depth0":
        forest = obr.make_forest([0, 0, 0], 4, 3, seed=4910)
        return _case(forest, osr.make_covers(forest, "half", seed=4911), obr.make_data(65, 4, seed=4912), avg=True, bias=0.25)
    if arg == "wide":
        forest = obr.make_forest(WIDE_DEPTHS, len(WIDE_USED), 5, seed=4920)
        forest["fids"] = np.asarray(WIDE_USED)[WIDE_FIDS]
        forest["cols"] = WIDE_COLS
        return _case(forest, osr.make_covers(forest, "half", seed=4921), obr.make_data(65, WIDE_COLS, seed=4922))
    if arg == "one_col":
        forest = obr.make_forest([1, 4], 1, 2, seed=4930)
        return _case(forest, osr.make_covers(forest, "half", seed=4931), obr.make_data(65, 1, seed=4932))
    assert arg == "k4"  # multi:avg's splits, covers and data under leaves of 4 classes (make_forest draws the leaves last)
    forest = obr.make_forest(MULTI_DEPTHS, 12, 4, seed=4600)
    return _case(forest, osr.make_covers(forest, "half", seed=4601), obr.make_data(65, 12, seed=4602), avg=True, bias=-0.375)


ELEMENT_CASES = [f"m:{M}:k{k}" for M in ELEMENT_COUNTS for k in element_classes(M)]
MERGED_CASES = [f"merged:{M}" for M in MERGED]
MULTI_CASES = ["multi:sum", "multi:avg"]
COVER_CASES = [f"covers:{p}" for p in COVER_POOLS]
BRANCH_CASES = [f"branch:{m}" for m in se.MISSINGS]
LEAF_CASE = "leaves:overflow"
SHAP_CASES = ELEMENT_CASES + MERGED_CASES + MULTI_CASES + COVER_CASES + BRANCH_CASES  # TreeSHAP is checked on these
INTER_ONLY_CASES = ["inter:none:empty", "inter:none:depth0", "inter:wide:k1", "inter:wide:k5", "inter:one_col", "inter:k4"]
INTER_CASES = SHAP_CASES + [LEAF_CASE] + INTER_ONLY_CASES  # predict_interactions is checked on these
_bases, _refs, _inter_refs = {}, {}, {}


def _split(name):
    parts = name.split(":")
    if parts[0] == "m" or parts[:2] == ["inter", "wide"]:
        return ":".join(parts[:2]), int(parts[2][1:])
    return name, None


def _base_of(name):
    if name not in _bases:
        _bases[name] = _base(name)
        for a in (_bases[name]["covers"], _bases[name]["data"]):
            a.setflags(write=False)
    return _bases[name]


def case(name):
    base, k = _split(name)
    c = _base_of(base)
    return c if k is None else dict(c, forest=with_classes(c["forest"], k))


def reference(name, shap=True):
    """case(name) with 'poly' = (phi, A, N) and 'emulate' (shap=True) and 'saabas'; computed once per family, sliced per case"""
    base, k = _split(name)
    c = _base_of(base)
    key = (base, shap)
    if key not in _refs:
        args = (c["forest"], c["covers"], c["data"])
        kw = dict(missing=c["missing"], avg=c["avg"], global_bias=c["bias"])
        r = dict(saabas=osr.saabas(*args, **kw))
        if shap:
            r["poly"] = osr.poly(*args, **kw)
            r["emulate"] = osr.emulate(*args, **kw)
        for a in (r["saabas"],) + r.get("poly", ()) + ((r["emulate"],) if shap else ()):
            a.setflags(write=False)
        _refs[key] = r
    r = _refs[key]
    out = dict(case(name), saabas=r["saabas"][:, :k])
    if shap:
        out.update(poly=tuple(a[:, :k] for a in r["poly"]), emulate=r["emulate"][:, :k])
    return out


def inter_reference(name):
    """case(name) on its first inter_rows(name) rows with 'emulate' = oblivious_inter_ref.emulate's Phi and 'poly' = its poly's
    (Phi, A, N), or None where has_inter_poly(name) says no; computed once per family, read-only, sliced on the class axis"""
    base, k = _split(name)
    c = _base_of(base)
    rows = inter_rows(name)
    if base not in _inter_refs:
        args = (c["forest"], c["covers"], c["data"][:rows])
        kw = dict(missing=c["missing"], avg=c["avg"], global_bias=c["bias"])
        with np.errstate(all="ignore"):
            r = dict(emulate=oir.emulate(*args, **kw))
        r["poly"] = oir.poly(*args, **kw) if has_inter_poly(name) else None
        for a in (r["emulate"],) + (r["poly"] or ()):
            a.setflags(write=False)
        _inter_refs[base] = r
    r = _inter_refs[base]
    return dict(case(name), data=c["data"][:rows], emulate=r["emulate"][:, :k],
                poly=None if r["poly"] is None else tuple(a[:, :k] for a in r["poly"]))


def depth_of(forest):
    return int(max(forest["depths"], default=0))


def bar(c, A, N):
    """(bound, floor), [rows, K, F + 1]: the TreeSHAP bar of tests/test_oblivious_shap_gpu.py, (N + 4 (D + 2)) 2^-24 A, plus,
    in a case whose covers reach the cut, the floor (N + 4 (D + 2)) 2^-121 max |leaf| (/ T with AVG) -- shap_edges.floor_term's
    argument: create's cut of a zero fraction below 2^-121 moves a term by at most 2^-121 |leaf|, and a rounding below the
    normal range adds less.  Covers that are 0 or integers up to 2^10 give no zero fraction in (0, 2^-121): no floor there."""
    forest = c["forest"]
    D, T = depth_of(forest), len(forest["depths"])
    L = float(np.abs(np.asarray(forest["leaves"], np.float64)).max()) if np.size(forest["leaves"]) else 0.0
    if c["avg"] and T > 0:
        L /= T
    n = N + 4 * (D + 2)
    floor = n * se.Z_MIN * L if c["cut"] else np.zeros_like(A)
    return n * U * A + floor, floor


def inter_bar(c, A, N):
    """(bound, floor), [rows, K, F + 1, F + 1]: the off-diagonal bar of tests/test_oblivious_inter_gpu.py with bar's floor.  An
    entry is the float32 sum of N terms whose absolute values sum to A, and a term carries the rounding of a conditioned extend
    and unwind of at most D + 1 steps, of the conditioning factor, of w * cf and of the product with the leaf -- 6 (D + 2)
    roundings are that test's count: n = N + 6 (D + 2), bound = n 2^-24 A + floor.  floor = n 2^-121 max |leaf| (/ T with AVG)
    in a case whose covers reach the cut (create's cut of a zero fraction below 2^-121 moves a term by at most 2^-121 |leaf|,
    bar's argument with this n) and 0 in every other case.  No margin beyond that."""
    forest = c["forest"]
    D, T = depth_of(forest), len(forest["depths"])
    L = float(np.abs(np.asarray(forest["leaves"], np.float64)).max()) if np.size(forest["leaves"]) else 0.0
    if c["avg"] and T > 0:
        L /= T
    n = N + 6 * (D + 2)
    floor = n * se.Z_MIN * L if c["cut"] else np.zeros_like(A)
    return n * U * A + floor, floor


def element_z(c):
    """Every (tree, leaf, element) z of the case, float64, flat"""
    out = [np.zeros(0)]
    for t, D, fids, sl, lv, cv in osr._trees(c["forest"], c["covers"]):
        _, ratio = osr.heap(D, cv)
        out.append(osr.shap_tables(D, fids, ratio)[2].reshape(-1))
    return np.concatenate(out)


def branches_taken(c):
    """(missing, compare): how many (row, split) decisions of the case take the missing branch, and the compare"""
    forest, x = c["forest"], c["data"]
    with np.errstate(invalid="ignore"):
        miss = np.abs(x[:, np.asarray(forest["fids"], np.int64)] - F32(c["missing"])) <= F32(1e-6)
    return int(miss.sum()), int((~miss).sum())
