"""tests/vector_approx_ref.py without a GPU: the restated definition against approx_contribs_ref.sparse on the K-fold expansion for
every case tests/test_vector_approx_gpu.py uses (K == 1: on the same trees), the float64 deltas of every path telescoping to
leaf - E(root), the float32 reference within (N + 1) 2^-24 S of the float64 sums (the bound of tests/test_shap_edges_capi.py), the
form-rule helper against a written-out table, and the preconditions that keep the GPU cases from passing vacuously."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_contribs_ref as acr  # noqa: E402
import shap_edges as se  # noqa: E402
import vector_approx_ref as var  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

U = 2.0 ** -24
NAMED = ["five_k9", "four_k8", "wide_k9", "repeat_k3", "zero_side_k3", "tiny_ratio_k3", "nine_k1"]


def cases():
    """[(label, forest, data, covers, missing)] of every case of the GPU tests"""
    out = []
    for name in NAMED:
        forest, data, covers = vsr.case(name)
        out += [(f"{name}:{label}", forest, data, cv, vr.MISSING) for label, cv in covers.items()]
    for K in (1, 3, 8, 9, 17):
        out.append((f"k{K}", *var.k_case(K), vr.MISSING))
    out.append(("k1023", *var.k_case(1023, cols=3, kinds=(3, "stump", 2)), vr.MISSING))
    for T in (0, 1, 3, 5):
        out.append((f"t{T}", *var.k_case(9, kinds=(4, "stump", 5, "leaf", 3)[:T], seed=7200), vr.MISSING))
    for K, cols in ((9, 8), (17, 5), (9, 64), (3, 318)):
        out.append((f"knobs_k{K}_c{cols}", *var.k_case(K, cols=cols, rows=var.WIDE_ROWS), vr.MISSING))
    out.append(("leaves_only", *var.leaves_only_case(), vr.MISSING))
    out.append(("vine", *var.vine_case(), vr.MISSING))
    for cols in (1, 317, 318, 319, 320):
        out.append((f"wide_{cols}", *var.wide_case(cols), vr.MISSING))
    for label, m in se.MISSINGS.items():
        out.append((f"pool_{label}", *var.pool_case(m), m))
    for kind in ("subnormal", "overflow"):
        out.append((kind, *var.value_case(kind), vr.MISSING))
    return out


CASES = cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("label,forest,data,covers,missing", CASES, ids=[c[0] for c in CASES])
def test_reference_equals_the_sparse_reference_on_the_expansion(label, forest, data, covers, missing):
    data = data[:65] if forest["k"] > 100 else data
    for avg, gb in ((False, 0.0), (True, 0.375)):
        got = var.contribs(forest, covers, data, missing=missing, avg=avg, global_bias=gb)
        sn, tr = vr.expand(forest)
        want = acr.sparse(sn, tr, vsr.tile_covers(forest, covers), forest["cols"], data, missing, num_classes=forest["k"], avg=avg,
                          global_bias=gb)
        se.assert_same_bits(got, want, f"{label} avg={avg}: the expansion")
        if forest["k"] == 1:
            same = acr.sparse(forest_as_sparse(forest), forest["trees"], covers, forest["cols"], data, missing, avg=avg, global_bias=gb)
            se.assert_same_bits(got, same, f"{label} avg={avg}: the same trees")


def forest_as_sparse(forest):
    nodes = forest["nodes"].copy()
    leaf = nodes["bits"] < 0
    nodes["val"][leaf] = forest["leaves"][nodes["left_idx"][leaf], 0]
    nodes["left_idx"][leaf] = 0
    return nodes


FINITE = [c for c in CASES if c[0] != "overflow"]  # (that one is not finite by construction: test_overflow_case_is_partly_finite)


@pytest.mark.parametrize("label,forest,data,covers,missing", FINITE, ids=[c[0] for c in FINITE])
def test_float64_deltas_telescope_and_bound_the_float32_sums(label, forest, data, covers, missing):
    for t, leaf, total, want, mag in var.path_deltas64(forest, covers):  # at most 301 float64 roundings of at most mag each
        assert np.all(np.abs(total - want) <= 302 * 2.0 ** -52 * (mag + np.abs(want))), (label, t, leaf)
    data = data[:65]
    phi, S, N = var.contribs(forest, covers, data, missing=missing, scale=True)
    assert np.isfinite(phi).all(), f"{label}: the reference is finite on this case"
    err = np.abs(phi.astype(np.float64) - var.direct64(forest, covers, data, missing=missing))[..., :-1]
    tol = ((N[:, None] + 1) * U * S)[:, :, None]
    assert np.all(err <= tol), f"{label}: worst {np.max(err / np.maximum(tol, 1e-300)):.3g} of the bound"


def test_overflow_case_is_partly_finite():
    forest, data, covers = var.value_case("overflow")
    phi = var.contribs(forest, covers, data)[:, :, :-1]
    share = np.mean(~np.isfinite(phi))
    assert 0.0 < share < 1.0, share
    assert np.isnan(phi).any() and np.isposinf(phi).any() and np.isneginf(phi).any()


def test_subnormal_case_has_subnormal_sums():
    forest, data, covers = var.value_case("subnormal")
    for avg in (False, True):
        phi = var.contribs(forest, covers, data, avg=avg)[:, :, :-1]
        assert np.any((phi != 0) & (np.abs(phi) < se.FLT_MIN))


@pytest.mark.parametrize("cols,K,kb,form,want", [
    # (class block, slab?, waves per workgroup) at 160 KiB of LDS
    (64, 1, None, None, (1, True, 3)),      # 16.6 KB per wave slab
    (64, 8, None, None, (2, True, 1)),      # KB 8: 133 KB, KB 4: 67 KB, KB 2: 33 KB per wave slab
    (64, 10, None, None, (2, True, 1)),
    (200, 8, None, None, (1, True, 1)),     # KB 1: 51 KB: above the 40 KB cut, but KB 1 is the floor
    (8, 9, None, None, (8, True, 3)),       # 18.7 KB per wave slab: three in the 64-KB budget
    (5, 3, None, None, (4, True, 4)),
    (318, 9, None, None, (1, True, 1)),     # two wave slabs of one output: 163328 B, the last width that fits
    (319, 9, None, None, (4, False, 4)),     # in place: class block 4
    (700, 9, None, None, (4, False, 4)),
    (700, 2, None, None, (2, False, 4)),
    (64, 8, 8, 1, (8, True, 1)),            # forced: one 133-KB wave slab
    (64, 8, 8, None, (8, False, 4)),        # forced class block alone: two wave slabs do not fit
    (64, 8, 4, None, (4, True, 1)),
    (64, 8, 2, 2, (2, False, 4)),
    (318, 3, 2, 1, (2, True, 1)),           # 163584 B: one wave slab just fits
    (318, 3, 4, 1, (4, False, 4)),
])
def test_form_rule_matches_a_written_out_table(cols, K, kb, form, want):
    assert var.form_rule(cols, K, kb, form) == want
