"""SHAP interaction values (tahoe_forest_predict_interactions) without a GPU: the symbol, the NULL-handle refusal, and the two
float64 references of tests/interactions_ref.py against each other, against tests/contribs_ref.py and against the oracle's
float64 sums."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contribs_ref  # noqa: E402
import interactions_ref  # noqa: E402

INVALID_ARG = 1
MISSING = -999.0


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def random_forest(ta, rng, T, D, cols, nan_thr=0.05):
    """synth_forest with random covers, early leaves, a root-leaf tree 0 and some NaN thresholds."""
    nodes = ta.synth_forest(T, D, cols, seed=int(rng.integers(1 << 30)), leaf_prob=0.15)
    nodes["weight"] = rng.uniform(0.05, 1.0, nodes.size).astype(np.float32)
    internal = (nodes["bits"].view(np.uint32) >> 31) == 0
    nodes["val"][internal & (rng.random(nodes.size) < nan_thr)] = np.nan
    nodes["bits"][0] = nodes["bits"][0] | np.int32(-2 ** 31)
    return nodes


def random_rows(ta, rng, rows, cols):
    return ta.synth_data(rows, cols, seed=int(rng.integers(1 << 30)), missing_prob=0.1, missing=MISSING, nan_prob=0.05)


def test_symbol_is_exported_and_bound(ta):
    assert "tahoe_forest_predict_interactions" in ta.capi.EXPORTED_SYMBOLS
    assert hasattr(ta.lib, "tahoe_forest_predict_interactions")
    assert hasattr(ta.Forest, "predict_interactions")
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    assert " tahoe_forest_predict_interactions" in syms


def test_predict_interactions_on_null_handle(ta):
    assert ta.lib.tahoe_forest_predict_interactions(None, None, None, 0, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_predict_interactions(None, None, None, 10, None) == INVALID_ARG


@pytest.mark.parametrize("seed", range(5))
def test_references_agree(ta, seed):
    rng = np.random.default_rng(seed)
    T, D, cols = 5, int(rng.integers(2, 6)), int(rng.integers(2, 7))
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 30, cols)
    for C_, avg, bias in ((1, False, 0.0), (1, True, 0.5), (5, True, -0.25)):
        b = interactions_ref.brute(nodes, T, D, cols, x, MISSING, num_classes=C_, avg=avg, global_bias=bias)
        p, A, N = interactions_ref.poly(nodes, T, D, cols, x, MISSING, num_classes=C_, avg=avg, global_bias=bias)
        scale = np.abs(b).sum(axis=(-1, -2), keepdims=True) + 1e-300
        assert np.all(np.abs(b - p) <= 1e-12 * scale), np.max(np.abs(b - p) / scale)
        off = ~np.eye(cols + 1, dtype=bool)
        off[cols, :] = off[:, cols] = False
        assert np.all(A[..., off] >= np.abs(p[..., off]) - 1e-12 * scale[..., 0])
        assert np.all(N[:, ~off] == 0) and np.all(A[..., ~off] == 0)


@pytest.mark.parametrize("seed", range(3))
def test_references_are_symmetric_and_rows_sum_to_phi(ta, seed):
    rng = np.random.default_rng(20 + seed)
    T, D, cols = 6, 4, 5
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 40, cols)
    phi = contribs_ref.brute(nodes, T, D, cols, x, MISSING, num_classes=2, avg=True, global_bias=0.125)
    scale = np.abs(phi).sum(axis=-1) + 1e-300
    for ref in (interactions_ref.brute, lambda *a, **k: interactions_ref.poly(*a, **k)[0]):
        m = ref(nodes, T, D, cols, x, MISSING, num_classes=2, avg=True, global_bias=0.125)
        assert np.array_equal(m, m.swapaxes(-1, -2))
        rowsum = m[:, :, :cols, :cols].sum(axis=-1)
        assert np.all(np.abs(rowsum - phi[:, :, :cols]) <= 1e-12 * scale[..., None])
        assert np.all(m[:, :, cols, :cols] == 0) and np.all(m[:, :, :cols, cols] == 0)
        assert np.array_equal(m[:, :, cols, cols], phi[:, :, cols])


def test_off_diagonals_are_not_trivial(ta):
    """The small forests above do have interactions (a reference that returned zeros would pass the sums)."""
    rng = np.random.default_rng(3)
    nodes = random_forest(ta, rng, 6, 4, 4)
    x = random_rows(ta, rng, 30, 4)
    m = interactions_ref.brute(nodes, 6, 4, 4, x, MISSING)
    off = m[:, 0, :4, :4] * (1 - np.eye(4))
    assert np.count_nonzero(off) > 0.3 * off.size


def test_matrix_sums_to_the_oracle_margin(ta):
    from oracle import oracle

    rng = np.random.default_rng(11)
    T, D, cols = 8, 5, 4  # few columns: features repeat on paths
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 48, cols)
    want = oracle.predict_f64(nodes, T, D, x, MISSING)
    p, A, _ = interactions_ref.poly(nodes, T, D, cols, x, MISSING)
    got = p[:, 0].sum(axis=(-1, -2))
    # the bias is float32; the rest is float64
    assert np.all(np.abs(got - want) <= 1e-6 * (np.abs(want) + A[:, 0].sum(axis=(-1, -2)) + 1)), np.max(np.abs(got - want))
