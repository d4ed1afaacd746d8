"""The references of the vector-leaf interventional TreeSHAP tests against each other (no GPU): the subset brute force of
tests/vector_iv_ref.py against its per-path closed form on every forest of num_cols <= 8, the closed form on the vector forest
against the closed form evaluated class by class on the K-fold expansion -- so the GPU tests may use the closed form -- and the
class-block / tile-row rule restated there at every shape the GPU cases rely on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vector_edges as ve  # noqa: E402
import vector_iv_ref as vir  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

ROWS, B = 9, 5


def inputs(name):
    forest, data, _ = vsr.case(name)
    bg = vr.make_data(B, forest["cols"], seed=900 + forest["cols"])
    return forest, data[:ROWS], bg


@pytest.mark.parametrize("name", vsr.SMALL)
def test_brute_force_and_closed_form_agree(name):
    forest, x, bg = inputs(name)
    for avg, bias in ((False, 0.0), (True, 0.375)):
        b = vir.brute(forest, x, bg, avg=avg, global_bias=bias)
        p, A, N = vir.paths(forest, x, bg, avg=avg, global_bias=bias)
        scale = np.abs(b).sum(axis=-1, keepdims=True) + 1e-300
        assert np.all(np.abs(b - p) <= 1e-12 * scale), name
        assert np.all(A[:, :, :-1] + 1e-300 >= np.abs(p[:, :, :-1]) * (1 - 1e-12))
        # efficiency: a row's values and the bias sum to its margin
        T = forest["trees"].size
        margin = ve.margins64(forest, x) / (T if avg and T else 1) + bias
        assert np.all(np.abs(b.sum(axis=-1) - margin) <= 1e-12 * scale[..., 0]), name


@pytest.mark.parametrize("name", vsr.NAMES)
def test_closed_form_equals_the_expansion_class_by_class(name):
    forest, x, bg = inputs(name)
    p, _, N = vir.paths(forest, x, bg, avg=True, global_bias=-0.25)
    e = vir.paths_expansion(forest, x, bg, avg=True, global_bias=-0.25)
    scale = np.abs(p).sum(axis=-1, keepdims=True) + 1e-300
    assert np.all(np.abs(p - e) <= 1e-12 * scale), name
    assert N.shape == (forest["k"], forest["cols"] + 1) and np.all(N == N[:1])  # every output sees the same paths


def test_the_rule_at_the_shapes_the_gpu_cases_rely_on():
    for cols, (kb, R, wlds) in vir.TILE_COLS.items():
        got = vir.iv_shape(cols, 9)
        assert got[:3] == (kb, R, wlds), (cols, got)
        assert got[3] <= (vir.LDS_BUDGET if cols <= 3891 else vir.LDS_DEVICE), cols
    # the steps are steps: neighbouring entries differ in exactly the way the table says, and one column more than the last fits nothing
    cols = sorted(vir.TILE_COLS)
    assert [(a, b) for a, b in zip(cols, cols[1:]) if b == a + 1] == [(73, 74), (147, 148), (294, 295), (589, 590), (1144, 1145),
                                                                        (2161, 2162), (3891, 3892), (7987, 7988)]
    assert 5 * vir.TILE_REFUSED * 4 > vir.LDS_DEVICE >= 5 * 8192 * 4
    # K decides the widest block: the largest of 8, 4, 2 below 2 K
    assert [vir.iv_shape(8, k)[0] for k in (1, 2, 3, 4, 5, 8, 9, 17, 1024)] == [1, 2, 4, 4, 8, 8, 8, 8, 8]
    # K == 1 walks the row steps of the existing kernel's rule
    assert [vir.iv_shape(c, 1)[:2] for c in (486, 487, 972, 973, 1945, 1946)] == [(1, 8), (1, 4), (1, 4), (1, 2), (1, 2), (1, 1)]
    # a forced block that leaves no row falls back to 1
    assert vir.iv_shape(590, 9, forced=8)[0] == 1 and vir.iv_shape(589, 9, forced=8)[:2] == (8, 1)
    assert vir.iv_shape(700, 9)[:2] == (4, 1) and vir.iv_shape(700, 9, forced=2)[:2] == (2, 2)  # wide_k9
    # the named forests of the knob test: every forced block is honoured on them but the widest ones on wide_k9
    for name in ("nine_k17", "five_k9", "four_k8", "stump_k3", "nine_k1", "repeat_k3"):
        forest = vsr.case(name)[0]
        assert [vir.iv_shape(forest["cols"], forest["k"], forced=kb)[:2] for kb in (1, 2, 4, 8)] == [(1, 8), (2, 8), (4, 8), (8, 8)]
