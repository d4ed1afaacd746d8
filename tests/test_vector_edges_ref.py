"""The references and fixtures of the vector-leaf edge tests against each other (no GPU): tests/vector_edges.poly against the
subset brute force of tests/vector_shap_ref.py wherever num_cols <= 8, its row sums against float64 margins on the long paths,
and every structural condition the GPU tests rely on -- a bin of two 32-lane paths, 31 distinct features after merging, a bin
that adds in 32 rounds, paths of 2 .. 32 lanes sharing more than 4 bins, the (KB, R, bytes) of the class-block rule on both
sides of each of its steps -- so that a change to the fixtures cannot silently remove an edge."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shap_edges as se  # noqa: E402
import vector_edges as ve  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

X_ROWS = 5  # the brute force costs 2^cols walks per tree whatever the number of rows


def lanes(b):
    return [len(p) + 1 for p in b]


# ------------------------------------------------------------------------------------------------ poly
@pytest.mark.parametrize("name", vsr.SMALL)
def test_poly_equals_the_brute_force_on_the_named_forests(name):
    forest, data, covers = vsr.case(name)
    x = data[:X_ROWS]
    for label, cv in covers.items():
        want = vsr.contribs(forest, cv, x, avg=True, global_bias=0.375)
        got, A, N = ve.poly(forest, cv, x, avg=True, global_bias=0.375)
        assert got.shape == want.shape == A.shape and N.shape == got.shape[1:]
        F = forest["cols"]
        scale = np.abs(want).max() if want.size else 0.0
        assert np.all(np.abs(got[:, :, :F] - want[:, :, :F]) <= 1e-12 * scale), (name, label)
        assert np.all(np.abs(got[:, :, F] - want[:, :, F]) <= 1e-6 * (scale + 1.0))  # (poly's bias column is rounded to float32)
        assert np.all(A + 1e-12 * scale >= np.abs(got))


@pytest.mark.parametrize("name", ve.BRUTE_CASES)
def test_poly_equals_the_brute_force_on_the_edge_cases(name):
    c = ve.case(name)
    forest, x = c["forest"], c["data"][:X_ROWS]
    F = forest["cols"]
    assert F <= 8
    if forest["k"] > 16:
        forest = ve.with_classes(forest, 16)  # (every output is computed on its own)
    for label, cv in c["covers"].items():
        want = vsr.contribs(forest, cv, x, c["missing"])
        got = ve.poly_raw(name, label)[0][:X_ROWS, :forest["k"]]
        scale = np.abs(want).max()
        assert scale > 0 and np.all(np.abs(got[:, :, :F] - want[:, :, :F]) <= 1e-12 * scale), (name, label)


@pytest.mark.parametrize("name", ve.LONG_CASES)
def test_row_sums_of_poly_are_the_float64_margins_on_the_long_paths(name):
    c = ve.case(name)
    forest, F = c["forest"], c["forest"]["cols"]
    margin = ve.margins64(forest, c["data"])
    for label in ve.PATH_LABELS:
        phi = ve.poly_raw(name, label)[0]
        total = phi[:, :, :F].sum(-1) + ve.expectation(forest, c["covers"][label])[None]
        scale = np.maximum(np.abs(margin), np.abs(phi[:, :, :F]).max(-1))
        rel = np.abs(total - margin) / scale
        print(f"{name} {label}: row sum against the margin, max relative difference {rel.max():.3e}")
        assert np.all(rel <= 1e-12), (name, label, rel.max())


def test_a_tiles_case_is_the_base_forest_on_other_columns():
    base, wide = ve.case("tiles:8:k16"), ve.case("tiles:4097")
    cols = ve.tile_columns(4097)
    assert np.array_equal(wide["data"][:, cols].view(np.uint32), base["data"].view(np.uint32))
    got = ve.poly(wide["forest"], wide["covers"]["consistent"], wide["data"][:X_ROWS])[0]
    want = ve.poly_raw("tiles:4097", "consistent")[0][:X_ROWS]
    assert got.shape == want.shape == (X_ROWS, 9, 4098) and np.array_equal(got[:, :, :4097], want[:, :, :4097])
    assert np.array_equal(got[:, :, 4097], vsr.bias_column(wide["forest"], wide["covers"]["consistent"])[None].repeat(X_ROWS, 0))


# ------------------------------------------------------------------------------------------------ the shapes of the path cases
def test_vine31_fills_its_first_bin_with_two_32_lane_paths():
    forest = ve.case("vine31:k9")["forest"]
    ps, bs = vsr.paths(forest), vsr.bins(forest)
    assert forest["cols"] == 40 and forest["trees"].size == 1 and len(ps) == 32
    assert lanes(bs[0][0]) == [32, 32] and sorted(ps[0]) == list(range(31)) == sorted(ps[1])
    assert max(len(p) for p in ps) == 31
    # the same vine continuing on the right packs [31, 32], [32] lanes instead: no bin of two full paths
    rng = np.random.default_rng(1)
    other = vr.make([ve.vine(rng, range(31), 13, "right")], vr.mixed_leaves(rng, 13, 2), 2, 40)
    assert not any(lanes(b) == [32, 32] for b, _ in vsr.bins(other))
    for k in (9, 2):
        assert ve.case(f"vine31:k{k}")["forest"]["k"] == k


def test_vine40_on_31_merges_40_levels_into_31_elements():
    forest = ve.case("vine40_on_31:k9")["forest"]
    ps = vsr.paths(forest)
    _, _, steps = vr.vector_ref(forest, ve.case("vine40_on_31:k9")["data"])
    assert len(ps) == 41 and max(len(p) for p in ps) == 31 and sum(len(p) == 31 for p in ps) >= 10
    assert all(len(set(p)) == len(p) for p in ps) and forest["cols"] == 31
    inner = forest["nodes"][forest["nodes"]["bits"] >= 0]
    assert inner.size == 40 and np.array_equal(np.sort(inner["bits"] & vr.FID_MASK), np.sort(np.arange(40) % 31))


def test_one_col_rounds_adds_a_bin_in_32_rounds():
    forest = ve.case("one_col_rounds")["forest"]
    bs = vsr.bins(forest)
    assert forest["cols"] == 1 and len(bs) == 2
    assert len(bs[0][0]) == 32 and bs[0][1] == 32 and lanes(bs[0][0]) == [2] * 32


def test_mixed_len_shares_bins_among_paths_of_2_to_32_lanes():
    forest = ve.case("mixed_len:k9")["forest"]
    bs = vsr.bins(forest)
    every = [n for b, _ in bs for n in lanes(b)]
    assert set(every) >= set(range(2, 33)) and len(bs) > 4
    assert sum(len(set(lanes(b))) >= 2 for b, _ in bs) > 4  # bins that mix lengths
    assert any(rounds > 1 for _, rounds in bs)
    assert any(sum(lanes(b)) == 64 for b, _ in bs) or max(sum(lanes(b)) for b, _ in bs) >= 60
    # a short path behind a 32-lane one: the bin takes 31 extend steps, and root lane + step passes lane 63 (the kernel's clamp)
    starts = [(int(np.sum(lanes(b)[:i])), max(lanes(b))) for b, _ in bs for i in range(len(b))]
    assert any(gs + steps - 1 > 63 for gs, steps in starts)


def test_covers_of_the_path_cases():
    forest, cv = ve.case("vine31:k9")["forest"], ve.case("vine31:k9")["covers"]
    assert set(cv) == set(ve.PATH_LABELS)
    nodes = forest["nodes"]
    for i in np.nonzero(nodes["bits"] >= 0)[0]:
        li = int(nodes["left_idx"][i])
        r = float(cv["mid"][li]) / (float(cv["mid"][li]) + float(cv["mid"][li + 1]))
        assert 0.3 <= r <= 0.7


# ------------------------------------------------------------------------------------------------ the class-block rule
def test_tile_rule_gives_the_documented_shapes():
    # 64 features -> KB = 8, R = 8, 33 x 8 x 64 x 4 = 67 584 B; 81 920 B at KB = 1 with R = 64
    assert ve.tile_shape(64, 8) == (8, 8, 67584) and ve.tile_shape(64, 10) == (8, 8, 67584)
    assert ve.tile_shape(64, 1) == (1, 64, 81920)
    assert ve.tile_shape(700, 9)[:2] == (1, 4)
    # forced blocks at 700 columns: 2 and 4 leave 2 rows and 1 row, 8 leaves none and falls back to 1
    assert [ve.tile_shape(700, 9, kb)[:2] for kb in (1, 2, 4, 8)] == [(1, 4), (2, 2), (4, 1), (1, 4)]
    for cols, (kb, R) in ve.TILE_COLS.items():
        got = ve.tile_shape(cols, 9)
        assert got[:2] == (kb, R), (cols, got)
        assert got[2] == (1 + 4 * kb) * R * cols * 4 <= ve.LDS_DEVICE
        assert got[2] <= ve.LDS_BUDGET or (kb, R) == (1, 1)
    assert ve.tile_shape(77, 9)[2] == 81312 and ve.tile_shape(78, 9)[2] > ve.LDS_BUDGET // 2
    assert ve.tile_shape(4096, 9)[2] == ve.LDS_BUDGET and ve.tile_shape(8192, 9)[2] == ve.LDS_DEVICE == 163840
    assert 5 * ve.TILE_REFUSED * 4 > ve.LDS_DEVICE  # 20 B per column
    # forced 8: one row at 620 columns, none at 621
    assert ve.tile_shape(620, 9, 8) == (8, 1, 81840) and ve.tile_shape(621, 9, 8)[:2] == (1, 4)
    # K = 2 keeps KB = 2 up to 568 columns; the automatic KB is the largest of 8, 4, 2 below 2 K
    assert ve.tile_shape(568, 2)[:2] == (2, 4) and ve.tile_shape(569, 2)[:2] == (1, 4)
    assert [ve.tile_shape(8, k)[0] for k in (1, 2, 3, 4, 5, 7, 8, 16)] == [1, 2, 4, 4, 8, 8, 8, 8]
    # every step of the rule has a case on both sides
    steps = [(a, b) for a, b in zip(sorted(ve.TILE_COLS), sorted(ve.TILE_COLS)[1:]) if b == a + 1]
    assert [a for a, _ in steps] == [9, 77, 155, 301, 568, 620, 1024, 4096]
    for a, b in steps:
        assert ve.TILE_COLS[a] != ve.TILE_COLS[b] or a in (620, 4096), (a, b)
    for cols in ve.TILE_FORCED:
        assert cols in ve.TILE_COLS
    # the row counts around a tile
    assert ve.batches(64) == [1, 63, 64, 65] and ve.batches(4) == [1, 3, 4, 5, 65] and ve.batches(1) == [1, 2, 65]


def test_tiles_cases_use_the_first_and_the_last_column():
    for name in ve.TILE_CASES:
        c = ve.case(name)
        forest = c["forest"]
        cols = forest["cols"]
        inner = forest["nodes"][forest["nodes"]["bits"] >= 0]
        fids = set((inner["bits"] & vr.FID_MASK).tolist())
        assert {0, cols - 1} <= fids and max(fids) == cols - 1 and c["data"].shape == (ve.ROWS, cols), name
        assert forest["trees"].size == 3 and vr.vector_ref(forest, c["data"][:3])[2].max() <= 4
        assert np.unique(ve.tile_columns(cols)).size == ve.TILE_BASE_COLS
    assert ve.case("tiles:568:k2")["forest"]["k"] == 2 and ve.case("tiles:8:k16")["forest"]["k"] == 16


def test_walk_cases_split_on_the_outer_columns():
    for cols in ve.WALK_COLS:
        c = ve.case(f"walk:{cols}")
        inner = c["forest"]["nodes"][c["forest"]["nodes"]["bits"] >= 0]
        assert set((inner["bits"] & vr.FID_MASK).tolist()) == {0, 1, cols - 2, cols - 1}
        assert c["forest"]["trees"].size == 5 and c["forest"]["k"] == 9
    assert 640 * 64 * 4 == ve.LDS_DEVICE and 640 % 4 == 0 and 639 % 4 != 0


# ------------------------------------------------------------------------------------------------ branch, covers, leaves, K
def test_branch_cases_take_both_rules_and_hold_the_special_values():
    for m, missing in se.MISSINGS.items():
        c = ve.case(f"branch:{m}:k3")
        nodes, x = c["forest"]["nodes"], c["data"]
        inner = nodes[nodes["bits"] >= 0]
        thr = inner["val"]
        assert np.isnan(thr).any() and np.isinf(thr).any() and (np.abs(thr[np.isfinite(thr)]) < 1.2e-38).any()
        assert c["forest"]["trees"].size == 5 and c["forest"]["cols"] == 4
        with np.errstate(invalid="ignore"):
            miss = np.abs(x - np.float32(missing)) <= np.float32(1e-6)
        assert np.isnan(x).any() and np.isinf(x).any()
        if np.isfinite(missing):
            assert miss.any() and (~miss).any()
            if abs(np.spacing(np.float32(missing))) < 1e-6:  # the band holds float32 values other than the sentinel: they are drawn
                assert (miss & (x != np.float32(missing))).any()
        else:
            assert not miss.any()
        assert ve.case(f"branch:{m}:k1")["forest"]["k"] == 1


def test_cover_cases_hold_what_their_modes_say():
    for mode in ve.COVER_MODES:
        c = ve.case(f"covers:{mode}")
        forest, cv = c["forest"], c["covers"][mode]
        assert np.isnan(cv[forest["trees"]]).all() and np.isfinite(np.delete(cv, forest["trees"])).all()
        zs = np.array([z for per_tree in ve.leaf_paths(forest, cv) for _, elems in per_tree for _, z, _ in elems])
        assert np.isfinite(zs).all() and (zs >= 0).all() and (zs <= 1).all()
        if mode == "zero":
            assert (zs == 0).any()
        if mode == "tiny":
            assert ((zs > 0) & (zs < se.Z_MIN)).any()
        if mode == "near_one":
            assert (zs > 1 - 1e-7).any() and ((zs > 0) & (zs < 1e-7)).any()
        if mode == "f32_overflow":
            assert np.isinf(np.float32(3e38) + np.float32(3e38)) and (cv[np.isfinite(cv)] >= 2e38).any()


def test_leaf_cases():
    c = ve.case("leaves:ieee")
    lv = c["forest"]["leaves"]
    assert np.isnan(lv).any() and np.isposinf(lv).any() and np.isneginf(lv).any() and (np.abs(lv) == np.float32(3e38)).any()
    assert (lv.view(np.uint32) == 0x80000000).any() and (lv == np.float32(1e-45)).any()
    sums = vr.vector_ref(c["forest"], c["data"])[0]
    assert np.isnan(sums).any() and np.isinf(sums).any() and np.isfinite(sums).any()
    z = ve.case("leaves:negzero")
    assert (z["forest"]["leaves"].view(np.uint32) == 0x80000000).all()
    assert not vr.vector_ref(z["forest"], z["data"])[0].view(np.uint32).any()  # +0.0 + -0.0 = +0.0


def test_k_nocols_and_deep_cases():
    for k in ve.BIG_KS:
        c = ve.case(f"K:{k}")
        assert c["forest"]["k"] == k == c["forest"]["leaves"].shape[1] and c["forest"]["trees"].size == 3
    for name in ve.NOCOLS_CASES:
        c = ve.case(name)
        forest = c["forest"]
        assert forest["cols"] == 0 and (forest["nodes"]["bits"] < 0).all() and forest["nodes"].size == forest["trees"].size
        assert not vsr.paths(forest) and not vsr.bins(forest) and ve.tile_shape(0, forest["k"])[1:] == (64, 0)
        sums, leaf, steps = vr.vector_ref(forest, c["data"])
        assert not leaf.any() and not steps.any()
        want = forest["leaves"][forest["nodes"]["left_idx"]].astype(np.float32)
        acc = np.zeros(forest["k"], np.float32)
        for v in want:
            acc = acc + v
        assert np.array_equal(sums.view(np.uint32), np.broadcast_to(acc, sums.shape).view(np.uint32))
    c = ve.case(ve.DEEP_CASE)
    steps = vr.vector_ref(c["forest"], c["data"])[2]
    assert c["forest"]["trees"].size == 4 and steps[0, 0] == 300 and steps[1, 0] == 1 and steps[:, 2].max() == 0
    assert len(set(steps[:, 0].tolist())) > 5
