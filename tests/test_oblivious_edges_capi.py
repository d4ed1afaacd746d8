"""The references of tests/test_oblivious_edges_gpu.py against each other, on exactly its cases (tests/oblivious_edges.py).  No
GPU.

  - oblivious_shap_ref.emulate, the float32 restatement the kernel is compared with bit for bit, against the float64 poly within
    the bar the GPU file keeps, (N + 4 (D + 2)) 2^-24 A + floor: the restatement alone stays inside it, with the ratio printed;
  - poly against the subset brute force on every cover pool;
  - the preconditions that keep the GPU cases from passing vacuously: terms counted, products on both sides of the 2^-121 cut,
    both branches of the rule taken, Saabas deltas that overflow;
  - the same for predict_interactions (tests/oblivious_inter_ref.py): emulate inside oblivious_edges.inter_bar of poly off the
    diagonal and its rows adding up to oblivious_shap_ref.poly's phi, poly against the subset brute force on every cover pool
    and on the inter:* cases, and what those cases are for."""
import os
import sys

import re

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oblivious_edges as oe  # noqa: E402
import oblivious_inter_ref as oir  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402
import shap_edges as se  # noqa: E402


@pytest.mark.parametrize("name", oe.SHAP_CASES)
def test_the_float32_restatement_stays_inside_the_bar(name):
    c = oe.reference(name)
    want, A, N = c["poly"]
    got = c["emulate"]
    assert got.dtype == np.float32 and got.shape == want.shape
    assert N.max() > 0, f"{name}: no leaf weighs any row"
    bound, floor = oe.bar(c, A, N)
    assert np.all(floor <= 1e-30), f"{name}: the floor {floor.max():.3e} could mask a normal-range error"
    assert np.all(np.isfinite(got)), name
    err, bound = np.abs(got.astype(np.float64) - want)[:, :, :-1], bound[:, :, :-1]
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"{name}: emulate against poly, max err / bound = {worst:.4f}")
    assert np.all(err <= bound), f"{name}: bound exceeded {worst:.3f}x at {np.argwhere(err > bound)[:5]}"
    assert np.array_equal(se.bits(got[:, :, -1]), se.bits(want[:, :, -1].astype(np.float32))), f"{name}: bias column"


@pytest.mark.parametrize("name", oe.COVER_CASES)
def test_poly_equals_brute_force_on_every_cover_pool(name):
    c = oe.reference(name)
    forest = c["forest"]
    s = np.concatenate([[0], np.cumsum(forest["depths"])])
    assert max(np.unique(forest["fids"][a:b]).size for a, b in zip(s[:-1], s[1:])) == 8  # brute's limit, reached
    want = osr.brute(forest, c["covers"], c["data"])
    got = c["poly"][0]
    scale = np.abs(want).sum(axis=-1, keepdims=True)
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got)), name
    rel = float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max())
    print(f"{name}: poly against brute, max err / sum |phi| = {rel:.3e}")
    assert np.all(np.abs(got - want) <= 1e-12 * scale), f"{name}: {rel:.3e}"


def test_the_cover_pools_reach_what_they_are_for():
    z = {p: oe.element_z(oe.case(f"covers:{p}")) for p in oe.COVER_POOLS}
    cut = z["cut"]
    assert np.any((cut >= se.Z_MIN) & (cut <= 2.0 ** -100)), "no z in [2^-121, 2^-100]: nothing is kept just above the cut"
    assert np.any((cut > 0) & (cut < se.Z_MIN)), "no positive z below 2^-121: nothing is cut"
    assert np.any(cut == 2.0 ** -121) and np.any(cut == 2.0 ** -122), "the cut is not met from either side"
    assert np.any(np.abs(z["near_one"] - 1.0) <= 1e-8) and np.any((z["near_one"] > 0) & (z["near_one"] <= 1e-7))
    assert z["span"].min() < 1e-30 and np.all(z["zero"] <= 0.5) and np.all(oe.case("covers:zero")["covers"] == 0)
    f = lambda p: oe.case(f"covers:{p}")["covers"]  # noqa: E731
    tiny = float(np.finfo(np.float32).tiny)
    assert np.any((f("subnormal") > 0) & (f("subnormal") < tiny))
    with np.errstate(over="ignore"):
        assert np.isinf(np.add.reduce(f("f32_overflow"), dtype=np.float32)), "the float32 sum of the covers does not overflow"
    assert np.isfinite(f("f32_overflow").astype(np.float64).sum())
    for p in oe.EXPANSION_POOLS:  # what lets the heap expansion carry the same covers
        for t, D, fids, sl, lv, cv in osr._trees(oe.case(f"covers:{p}")["forest"], f(p)):
            cover, _ = osr.heap(D, cv)
            w = np.concatenate(cover).astype(np.float32)
            assert np.all(np.isfinite(w)) and np.all(w >= tiny), p
    mixed = f("mixed")
    assert np.any(mixed == 0) and np.any(mixed > 1e38) and np.any((mixed > 0) & (mixed < 1e-38))


@pytest.mark.parametrize("name", oe.BRANCH_CASES)
def test_the_branch_cases_take_both_branches(name):
    c = oe.case(name)
    missing, compare = oe.branches_taken(c)
    assert compare > 0
    if np.isnan(c["missing"]):
        # |x - NaN| <= 1e-6 holds for no x: a NaN sentinel switches the missing branch off, and that is the rule under test
        assert missing == 0
    else:
        assert missing > 0
    thr, x = c["forest"]["thr"], c["data"]
    assert np.isnan(thr).any() and np.isinf(thr).any() and np.any((thr != 0) & (np.abs(thr) < 1e-38))
    assert np.any(np.signbit(thr) & (thr == 0)) and np.isnan(x).any() and np.isinf(x).any()
    if np.isfinite(c["missing"]):
        assert np.any(thr == np.float32(c["missing"])), "no threshold equals the sentinel"
    leaf = oe.reference(name)["poly"][2]
    assert leaf.max() > 0


def test_the_overflow_leaves_overflow_the_deltas():
    c = oe.reference(oe.LEAF_CASE, shap=False)
    phi = c["saabas"][:, :, :-1]
    assert np.isinf(phi).any() and np.isnan(phi).any() and np.isfinite(phi).any()
    assert np.any(np.signbit(c["forest"]["leaves"]) & (c["forest"]["leaves"] == 0))


def test_every_instantiation_is_named():
    """One case per M = 1 .. 16 of ob_shap_tree, its features distinct; every M that oblivious_inter_kernel switches to an
    ob_inter_tree<M, KB> has such a case of one class (KB = 1) and one of more (KB = kObShapClasses), both among the cases that
    predict_interactions is checked on"""
    for M in oe.ELEMENT_COUNTS:
        forest = oe.case(f"m:{M}:k1")["forest"]
        assert list(forest["depths"]) == [M] and np.unique(forest["fids"]).size == M
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tahoe_amd", "csrc", "oblivious_shap.hip")).read()
    block = int(re.search(r"constexpr int kObShapClasses = (\d+);", src).group(1))
    assert block == osr.CLASS_BLOCK == 4
    assert "oblivious_inter_kernel<1>" in src and "oblivious_inter_kernel<kObShapClasses>" in src  # KB is 1 or the block
    inter = sorted(int(m) for m in re.findall(r"TAHOE_OB_INTER_CASE\((\d+)\)", src))
    assert inter == list(range(2, 17)), inter
    for M in inter:
        met = set()
        for k in oe.element_classes(M):
            name = f"m:{M}:k{k}"
            assert name in oe.INTER_CASES
            forest = oe.case(name)["forest"]
            assert list(forest["depths"]) == [M] and np.unique(forest["fids"]).size == M and forest["k"] == k
            assert forest["leaves"].size == k << M
            met.add(1 if k == 1 else block)
        assert met == {1, block}, (M, met)
        assert any(k > block and k % block for k in oe.element_classes(M)), f"m = {M}: no partial class block"
    for M in oe.MERGED:
        forest = oe.case(f"merged:{M}")["forest"]
        assert list(forest["depths"]) == [16] and np.unique(forest["fids"]).size == M


# ------------------------------------------------------------------------------------------------ interaction values
INTER_POLY_CASES = [n for n in oe.INTER_CASES if oe.has_inter_poly(n)]


@pytest.mark.parametrize("name", INTER_POLY_CASES)
def test_the_float32_interaction_restatement_stays_inside_the_bar(name):
    """emulate against poly off the diagonal within inter_bar (where leaves overflow: on emulate's finite entries), the corner
    and the zeroes, and every row's sum against oblivious_shap_ref.poly's phi within the sum of the two bars"""
    c = oe.inter_reference(name)
    want, A, N = c["poly"]
    got = c["emulate"]
    F = c["forest"]["cols"]
    assert got.dtype == np.float32 and got.shape == want.shape == (oe.inter_rows(name), c["forest"]["k"], F + 1, F + 1)
    bound, floor = oe.inter_bar(c, A, N)
    assert np.all(floor <= 1e-30), f"{name}: the floor {floor.max():.3e} could mask a normal-range error"
    finite = np.isfinite(got)
    assert name == oe.LEAF_CASE or finite.all(), name
    off = ~np.eye(F + 1, dtype=bool) & finite
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.where(bound > 0, bound, 1.0))[off].max()) if off.any() else 0.0
    print(f"{name}: emulate against poly, max err / bound = {worst:.4f}")
    assert np.all(err[off] <= bound[off]), f"{name}: bound exceeded {worst:.3f}x at {np.argwhere(off & (err > bound))[:5]}"
    assert np.array_equal(se.bits(got[:, :, F, F]), se.bits(want[:, :, F, F].astype(np.float32))), f"{name}: bias corner"
    assert not se.bits(got[:, :, F, :F]).any() and not se.bits(got[:, :, :F, F]).any(), f"{name}: row / column F"
    unused = np.setdiff1d(np.arange(F), c["forest"]["fids"])
    assert not se.bits(got[:, :, unused, :]).any() and not se.bits(got[:, :, :, unused]).any(), f"{name}: unused columns"
    assert np.array_equal(se.bits(got), se.bits(got.swapaxes(-1, -2))) or name == oe.LEAF_CASE, f"{name}: not symmetric"
    with np.errstate(all="ignore"):
        shap = oe.reference(name)
    rows = got.shape[0]
    phi, A1, N1 = (a[:rows] for a in shap["poly"])
    tol = oe.bar(c, A1, N1)[0][:, :, :F] + np.where(~np.eye(F + 1, dtype=bool), bound, 0.0)[:, :, :F, :F].sum(axis=-1)
    whole = finite[:, :, :F, :F].all(axis=-1)
    with np.errstate(invalid="ignore"):
        total = got.astype(np.float64)[:, :, :F, :F].sum(axis=-1)
    miss = np.abs(total - phi[:, :, :F])
    print(f"{name}: row sums against phi, max err / tol = {float((miss / np.where(tol > 0, tol, 1.0))[whole].max()) if whole.any() else 0.0:.4f}")
    assert np.all(miss[whole] <= tol[whole]), f"{name}: the rows do not add up to phi"


@pytest.mark.parametrize("name", oe.COVER_CASES + oe.INTER_ONLY_CASES)
def test_interaction_poly_equals_brute_force(name):
    """The form and tolerance of test_poly_equals_brute_force_on_every_cover_pool, on the first 9 rows"""
    c = oe.inter_reference(name)
    want = oir.brute(c["forest"], c["covers"], c["data"][:9], missing=c["missing"], avg=c["avg"], global_bias=c["bias"])
    got = c["poly"][0][:9]
    scale = np.abs(want).sum(axis=-1, keepdims=True)
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got)), name
    rel = float((np.abs(got - want) / np.where(scale > 0, scale, 1.0)).max())
    print(f"{name}: poly against brute, max err / sum |Phi[i]| = {rel:.3e}")
    assert np.all(np.abs(got - want) <= 1e-12 * scale), f"{name}: {rel:.3e}"


def test_the_interaction_cases_reach_what_they_are_for():
    emu = oe.inter_reference(oe.LEAF_CASE)["emulate"]
    assert (~np.isfinite(emu)).any() and np.isfinite(emu).any(), "leaves:overflow: no non-finite entry in emulate"
    cut = oe.element_z(oe.case("covers:cut"))
    assert np.any((cut > 0) & (cut < se.Z_MIN)) and np.any((cut >= se.Z_MIN) & (cut <= 2.0 ** -100))
    assert np.any(cut == 2.0 ** -121) and np.any(cut == 2.0 ** -122), "the cut is not met from either side"
    assert oe.inter_bar(oe.case("covers:cut"), np.ones(1), np.ones(1))[1] > 0, "covers:cut carries no floor"
    assert not oe.inter_bar(oe.case("multi:sum"), np.ones(1), np.ones(1))[1].any(), "a floor outside the cover cases"
    off = lambda n: oe.inter_reference(n)["poly"][0][:, :, :-1, :-1] * ~np.eye(oe.case(n)["forest"]["cols"], dtype=bool)  # noqa: E731
    for k in (1, 5):
        c = oe.inter_reference(f"inter:wide:k{k}")
        forest = c["forest"]
        assert forest["cols"] == oe.WIDE_COLS == 300 and forest["k"] == k and c["data"].shape == (65, 300)
        assert list(forest["depths"]) == [3, 5, 2] and sorted(set(forest["fids"])) == [0, 149, 299], "not exactly 3 used columns"
        used = np.ix_(*[np.arange(65), np.arange(k), [0, 149, 299], [0, 149, 299]])
        pairs = np.abs(off(f"inter:wide:k{k}")[used]).max(axis=0)  # [K, 3, 3]
        assert np.all(pairs[:, ~np.eye(3, dtype=bool)] > 0), "a pair of the used columns never interacts"
    c = oe.inter_reference("inter:one_col")
    assert c["forest"]["cols"] == 1 and list(c["forest"]["depths"]) == [1, 4]
    assert not c["poly"][0][:, :, 0, 1].any() and not c["poly"][0][:, :, 1, 0].any() and np.abs(c["poly"][0][:, :, 0, 0]).max() > 0
    for name, depths, k in (("inter:none:empty", [], 2), ("inter:none:depth0", [0, 0, 0], 3)):
        c = oe.inter_reference(name)
        assert list(c["forest"]["depths"]) == depths and c["forest"]["k"] == k and c["forest"]["fids"].size == 0
        Phi = c["poly"][0].copy()
        assert np.all(Phi[:, :, -1, -1] != 0)
        Phi[:, :, -1, -1] = 0
        assert not Phi.any(), f"{name}: more than the bias corner"
    c = oe.inter_reference("inter:k4")
    assert c["forest"]["k"] == osr.CLASS_BLOCK and np.abs(off("inter:k4")).max(axis=(0, 2, 3)).min() > 0
    multi = oe.case("multi:avg")
    assert all(np.array_equal(c["forest"][key], multi["forest"][key]) for key in ("depths", "fids", "thr", "def_left"))
    for name in oe.BRANCH_CASES:
        c = oe.inter_reference(name)
        missing, compare = oe.branches_taken(c)
        assert compare > 0 and (missing > 0) != bool(np.isnan(c["missing"])), name
        assert c["poly"][2].max() > 0 and np.abs(off(name)).max() > 0, name
