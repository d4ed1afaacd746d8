"""Interventional TreeSHAP (tahoe_forest_set_background, tahoe_forest_predict_contribs_interventional) without a GPU: the
symbols, the NULL-handle refusals, and the two float64 references of tests/interventional_ref.py against each other, against
f(x) - f(r) and on r = x."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interventional_ref as ivr  # noqa: E402

INVALID_ARG = 1
MISSING = -999.0
SYMBOLS = ("tahoe_forest_set_background", "tahoe_forest_predict_contribs_interventional")


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def test_symbols_are_exported_and_bound(ta):
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    for name in SYMBOLS:
        assert name in ta.capi.EXPORTED_SYMBOLS
        assert hasattr(ta.lib, name)
        assert " " + name in syms, name
    assert hasattr(ta.Forest, "set_background") and hasattr(ta.Forest, "predict_contribs_interventional")
    assert ta.lib.tahoe_abi_version() == 2


def test_null_handle_is_refused(ta):
    assert ta.lib.tahoe_forest_set_background(None, None, 0, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_set_background(None, None, 10, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_predict_contribs_interventional(None, None, None, 0, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_predict_contribs_interventional(None, None, None, 10, None) == INVALID_ARG
    assert "null forest" in ta.lib.tahoe_last_error().decode()


def random_forest(ta, rng, T, D, cols, nan_thr=0.05):
    """synth_forest with early leaves, a root-leaf tree and some NaN thresholds (covers are not read by this game)."""
    nodes = ta.synth_forest(T, D, cols, seed=int(rng.integers(1 << 30)), leaf_prob=0.15)
    internal = (nodes["bits"].view(np.uint32) >> 31) == 0
    nodes["val"][internal & (rng.random(nodes.size) < nan_thr)] = np.nan
    nodes["bits"][0] = nodes["bits"][0] | np.int32(-2 ** 31)  # tree 0 is a single leaf ...
    nodes["val"][0] = 0.375  # ... with a finite value
    return nodes


def random_rows(ta, rng, rows, cols):
    return ta.synth_data(rows, cols, seed=int(rng.integers(1 << 30)), missing_prob=0.1, missing=MISSING, nan_prob=0.05)


@pytest.mark.parametrize("seed", range(5))
def test_references_agree(ta, seed):
    rng = np.random.default_rng(seed)
    T, D, cols = 5, int(rng.integers(1, 6)), int(rng.integers(2, 7))
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 12, cols)
    bg = random_rows(ta, rng, 5, cols)
    for C_, avg, bias in ((1, False, 0.0), (1, True, 0.5), (5, True, -0.25)):
        b = ivr.brute(nodes, T, D, cols, x, bg, MISSING, num_classes=C_, avg=avg, global_bias=bias)
        p, A, N = ivr.paths(nodes, T, D, cols, x, bg, MISSING, num_classes=C_, avg=avg, global_bias=bias)
        scale = np.abs(b).sum(axis=-1, keepdims=True) + 1e-300
        assert np.all(np.abs(b - p) <= 1e-12 * scale), np.max(np.abs(b - p) / scale)
        assert np.all(A >= np.abs(p) - 1e-12 * scale)
        assert np.all(N[:, -1] == 0)


def test_each_pair_sums_to_the_difference_of_outputs(ta):
    from oracle import oracle

    rng = np.random.default_rng(11)
    T, D, cols = 8, 5, 4  # few columns: features repeat on paths
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 32, cols)
    bg = random_rows(ta, rng, 6, cols)
    fx = oracle.predict_f64(nodes, T, D, x, MISSING)
    fr = oracle.predict_f64(nodes, T, D, bg, MISSING)
    for r in range(bg.shape[0]):
        p, A, _ = ivr.paths(nodes, T, D, cols, x, bg[r:r + 1], MISSING)
        got = p[:, 0, :cols].sum(axis=1)
        assert np.all(np.abs(got - (fx - fr[r])) <= 1e-12 * (A[:, 0, :cols].sum(axis=1) + np.abs(fx) + abs(fr[r]))), r


def test_background_equal_to_the_row_gives_zero(ta):
    rng = np.random.default_rng(12)
    T, D, cols = 6, 4, 5
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 10, cols)
    for k in range(x.shape[0]):
        p, _, _ = ivr.paths(nodes, T, D, cols, x[k:k + 1], x[k:k + 1], MISSING)
        assert np.all(p[:, :, :cols] == 0.0), k


def test_weights(ta):
    # W+(a, b) = (a-1)! b! / (a+b)! = 1 / (a C(a+b, b)).  One live path pays out f(x) - f(r) on it: a W+(a, b) - b W+(b, a) is
    # 1 when only x reaches the leaf (b = 0), -1 when only r does (a = 0), 0 when neither does
    for a in range(0, 20):
        for b in range(0, 20):
            if a >= 1:
                assert ivr.weight(a, b) == pytest.approx(1.0 / (a * math.comb(a + b, b)), rel=1e-15)
            want = 1.0 if b == 0 and a > 0 else (-1.0 if a == 0 and b > 0 else 0.0)
            assert a * ivr.weight(a, b) - b * ivr.weight(b, a) == pytest.approx(want, abs=1e-15)


def test_bias_is_float64_then_float32(ta):
    from oracle import oracle

    rng = np.random.default_rng(5)
    T, D, cols = 6, 4, 3
    nodes = random_forest(ta, rng, T, D, cols)
    bg = random_rows(ta, rng, 9, cols)
    b = ivr.bias_f32(nodes, T, D, bg, MISSING, num_classes=2, avg=True, global_bias=0.125)
    want = []
    for c in range(2):
        raw = oracle.predict(ivr.sub_forest(nodes, T, 2, c), 3, D, bg, MISSING)[0]
        want.append(np.float32(sum(float(v) for v in raw) / 9 / 3 + 0.125))
    assert b.dtype == np.float32 and list(b) == want
