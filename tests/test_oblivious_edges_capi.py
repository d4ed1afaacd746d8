"""The references of tests/test_oblivious_edges_gpu.py against each other, on exactly its cases (tests/oblivious_edges.py).  No
GPU.

  - oblivious_shap_ref.emulate, the float32 restatement the kernel is compared with bit for bit, against the float64 poly within
    the bar the GPU file keeps, (N + 4 (D + 2)) 2^-24 A + floor: the restatement alone stays inside it, with the ratio printed;
  - poly against the subset brute force on every cover pool;
  - the preconditions that keep the GPU cases from passing vacuously: terms counted, products on both sides of the 2^-121 cut,
    both branches of the rule taken, Saabas deltas that overflow."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oblivious_edges as oe  # noqa: E402
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
    """One case per M = 1 .. 16 of ob_shap_tree, its features distinct"""
    for M in oe.ELEMENT_COUNTS:
        forest = oe.case(f"m:{M}:k1")["forest"]
        assert list(forest["depths"]) == [M] and np.unique(forest["fids"]).size == M
    for M in oe.MERGED:
        forest = oe.case(f"merged:{M}")["forest"]
        assert list(forest["depths"]) == [16] and np.unique(forest["fids"]).size == M
