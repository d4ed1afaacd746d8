"""SHAP interaction values on vector-leaf handles without a GPU (tests/vector_inter_ref.py): the class-block / tile-row / form rule
of vector_inter_build restated and its steps, the triangle index of the slab form, and the float64 conditioned recursion run once
per path for all K outputs against the float64 brute force the sparse SHAP tests use (tests/sparse_shap_ref.interactions), on the
T x K-tree expansion: 1e-12 of the largest value."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_shap_ref as ssr  # noqa: E402
import vector_inter_ref as vir  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402


@pytest.mark.parametrize("F", [0, 1, 2, 3, 8, 18, 36, 51, 71])
def test_the_triangle_index_is_a_bijection(F):
    got = [vir.tri_index(a, b, F) for a in range(F) for b in range(a + 1, F)]
    assert got == list(range(vir.pairs(F)))  # row-major, onto [0, F (F - 1) / 2)


def test_the_steps_of_the_rule():
    for F, want in vir.STEPS.items():
        assert vir.shape(F, 9)[:3] == want, F
    # the form is the sparse handle's: (F + 4 F^2) floats within 80 KiB
    assert [F for F in range(200) if vir.shape(F, 9)[0]] == list(range(72))
    # the class block: 8 to 36 columns, 4 to 51, 2 to 71 (one row of KB triangles per wave and the row within 80 KiB)
    kb = [vir.shape(F, 9)[1] for F in range(72)]
    assert kb == [8] * 37 + [4] * 15 + [2] * 20
    # ... and at KB 8 the rows of a tile
    rows = [vir.shape(F, 9)[2] for F in range(37)]
    assert rows[18] == 4 and rows[19] == 2 and rows[25] == 2 and rows[26] == 1 and rows[36] == 1 and max(rows) == 32
    assert all(a >= b for a, b in zip(rows, rows[1:]))
    for F in range(0, 200):
        for K in (1, 2, 3, 4, 5, 8, 9, 1024):
            slabs, kb, R, lds = vir.shape(F, K)
            assert kb in (1, 2, 4, 8) and kb < 2 * K and 1 <= R <= 32 and R & (R - 1) == 0
            assert lds <= vir.LDS_BUDGET
            if slabs:
                assert lds == R * (F + 4 * kb * vir.pairs(F)) * 4
                assert R == 32 or 2 * lds > vir.LDS_BUDGET  # the largest power of two that fits
                assert kb == 8 or kb * 2 >= 2 * K or vir.slab_row_bytes(F, 2 * kb) > vir.LDS_BUDGET  # the largest block
            else:
                assert (kb, R, lds) == (next(c for c in (8, 4, 2, 1) if c < 2 * K), 1, 16 * F)


def test_the_class_block_follows_k_and_the_knob():
    assert [vir.shape(8, K)[1] for K in (1, 2, 3, 4, 5, 7, 16)] == [1, 2, 4, 4, 8, 8, 8]
    assert [vir.shape(700, K)[1] for K in (1, 2, 3, 4, 5, 7, 16)] == [1, 2, 4, 4, 8, 8, 8]
    for forced in (1, 2, 4, 8):
        assert vir.shape(8, 9, forced)[1] == forced and vir.shape(700, 9, forced)[1] == forced  # in place: no LDS per class
        assert vir.shape(8, 1, forced)[1] == forced  # forcing is not bounded by K: the spare classes of a block idle
    assert [vir.shape(60, 9, f)[1] for f in (1, 2, 4, 8)] == [1, 2, 1, 1]  # a block that leaves no row falls back to 1
    assert [vir.shape(40, 9, f)[1] for f in (1, 2, 4, 8)] == [1, 2, 4, 1]
    # a device with less LDS than the budget: the form and the block both follow it
    assert vir.shape(63, 9, lds=64 * 1024)[:3] == (True, 2, 1) and vir.shape(64, 9, lds=64 * 1024)[:3] == (False, 8, 1)
    assert vir.shape(30, 9, lds=64 * 1024)[:3] == (True, 8, 1) and vir.shape(30, 9)[:3] == (True, 8, 1)
    assert vir.shape(31, 9, lds=64 * 1024)[:3] == (True, 8, 1) and vir.shape(32, 9, lds=64 * 1024)[:3] == (True, 8, 1)
    assert vir.shape(33, 9, lds=64 * 1024)[:3] == (True, 4, 1) and vir.shape(33, 9)[:3] == (True, 8, 1)


def test_batches_surround_the_tile():
    assert vir.batches(8, 9) == [1, 15, 16, 17, 33] and vir.batches(18, 9) == [1, 3, 4, 5, 33]
    assert vir.batches(36, 9) == [1, 2, 33] and vir.batches(72, 9) == [1, 3, 4, 5]


def test_two_col_rounds_is_one_pair_in_21_rounds():
    c = vir.case("two_col_rounds")
    b = vsr.bins(c["forest"])
    assert [len(p) for p, _ in b] == [21, 21, 21, 21]
    assert all(q == [0, 1] for p, _ in b for q in p)  # every path: x0 then x1, so one pair, once per path of a bin


@pytest.mark.parametrize("name", ["stump_k3", "three_k1", "four_k8", "five_k9", "nine_k17", "repeat_k3", "zero_side_k3",
                                  "tiny_ratio_k3", "two_col_rounds"])
def test_one_recursion_per_path_meets_the_brute_force_on_the_expansion(name):
    if name == "two_col_rounds":
        c = vir.case(name)
        forest, data, covers = c["forest"], c["data"], c["covers"]
    else:
        forest, data, covers = vsr.case(name)
    K, F = forest["k"], forest["cols"]
    x = data[:12]
    sn, tr = vr.expand(forest)
    for label, cv in covers.items():
        got = vir.interactions(forest, cv, x)
        want = ssr.interactions(sn, tr, vsr.tile_covers(forest, cv), x, F, vr.MISSING, K)
        assert got.shape == want.shape == (12, K, F, F)
        # 1e-12 of the largest value, and of 1 where the values are smaller: the leaves span 1e-3 .. 1e4, float64 carries 1.1e-16
        scale = max(np.abs(want).max(), 1.0)
        err = np.abs(got - want).max()
        print(f"{name} {label}: max |path - brute| = {err:.3e}, largest value {np.abs(want).max():.3e}")
        assert err <= 1e-12 * scale, (name, label, err)
        assert (np.abs(want).max() > 0) == any(len(p) > 1 for p in vsr.paths(forest))  # a pair needs a path with two features
