"""Interventional TreeSHAP (tahoe_forest_set_background, tahoe_forest_predict_contribs_interventional) on the GPU against the
float64 references of tests/interventional_ref.py.  Needs an MI355X.

Bound: |phi_gpu - phi_64| <= (N + B + 8) 2^-24 A per output, A = (1 / B) sum over (path, background row) of |leaf x weight|
(divided by Tc with AVG; interventional_ref.paths), N = the paths feeding the output, B = the background rows.  Derivation: a
term leaf x W(a, b) of one (path, background row) pair carries the rounding of W (1 ulp), of the in-order float32 sum of the
B weights of its path element (B - 1; all weights of one sum have one sign, so this is relative to their sum), of the product
with the leaf (1), of the slab sum over the wave's paths on that feature (<= N - 1), of the four-slab sum (3), and of the two
divisions (2): N + B + 5 to first order, 3 more for the second-order terms.
Exact: the bias column bit for bit against the host formula on Forest.predict_raw(bg); B = 1 with the background equal to the
row gives +0.0 everywhere but the bias; a feature no tree uses gives +0.0.  Additivity: sum_i phi_i + bias against the library's
margin within the bound plus the float32 error of the margin and of the background's raw sums.  Bitwise: repeat calls, any
batch / permutation / prefix, every strategy, the re-layout, the same background set again, and class c of a multi-class handle
against a handle on class c's sub-forest."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interventional_ref as ivr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
U = 2.0 ** -24
INVALID_ARG, UNSUPPORTED = 1, 7


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(env, a):
    return env[1].from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def gpu_phi(env, forest, x):
    ta, torch = env
    out = forest.predict_contribs_interventional(dev(env, x))
    torch.cuda.synchronize()
    phi = out.cpu().numpy()
    return phi if phi.ndim == 3 else phi[:, None, :]


def abs_leaf_sums(nodes, T, D, data, num_classes):
    """sum over class c's trees of |the leaf the row reaches| (float64), [rows, C]."""
    from oracle import oracle

    a = nodes.copy()
    leaf = (a["bits"].view(np.uint32) >> 31) == 1
    a["val"][leaf] = np.abs(a["val"][leaf])
    return np.stack([oracle.predict_f64(ivr.sub_forest(a, T, num_classes, c), T // num_classes, D, data, MISSING)
                     for c in range(num_classes)], axis=1)


def check(env, nodes, T, D, F, x, bg, num_classes=1, output=0, bias=0.0, label="", brute=False):
    ta, torch = env
    avg = (output & ta.OUT_AVG) != 0
    f = ta.Forest(nodes, T, D, F, missing=MISSING, output=output, global_bias=bias, num_classes=num_classes, contribs=True)
    bgd = dev(env, bg)
    f.set_background(bgd)
    got = gpu_phi(env, f, x).astype(np.float64)
    want, A, N = ivr.paths(nodes, T, D, F, x, bg, MISSING, num_classes=num_classes, avg=avg, global_bias=bias)
    B = bg.shape[0]
    if brute:
        b = ivr.brute(nodes, T, D, F, x, bg, MISSING, num_classes=num_classes, avg=avg, global_bias=bias)
        scale = np.abs(b).sum(axis=-1, keepdims=True) + 1e-300
        assert np.all(np.abs(b - want) <= 1e-12 * scale), label
        want = b
    gamma = (N[None, :, :] + B + 8) * U
    err = np.abs(got - want)[:, :, :-1]
    bound = (gamma * A)[:, :, :-1]
    scale = np.abs(want).sum(axis=-1) + 1e-30
    rel = float(np.max(err.max(axis=-1) / scale))
    assert np.all(err <= bound), f"{label}: max |phi - phi64| / sum|phi64| = {rel:.3e}; bound exceeded at {np.argwhere(err > bound)[:5]}"
    # bias column bit for bit: the host formula on the library's own raw sums of the background
    raw = ta.Forest(nodes, T, D, F, missing=MISSING, num_classes=num_classes).predict_raw(bgd).cpu().numpy()
    raw = raw.reshape(B, num_classes)
    Tc = T // num_classes
    want_bias = np.array([ivr.bias_from_raw(raw[:, c], Tc, avg, bias) for c in range(num_classes)]).astype(np.float32)
    assert np.array_equal(bits(got[:, :, -1].astype(np.float32)), bits(np.broadcast_to(want_bias, got[:, :, -1].shape))), label
    # ... which the float32 oracle gives as well
    assert np.array_equal(bits(want_bias), bits(ivr.bias_f32(nodes, T, D, bg, MISSING, num_classes, avg, bias))), label
    # additivity against the library's margins (AVG and bias applied, no sigmoid / softmax)
    m = ta.Forest(nodes, T, D, F, missing=MISSING, output=output & ta.OUT_AVG, global_bias=bias, num_classes=num_classes)
    margin = m.predict(dev(env, x)).cpu().numpy().astype(np.float64).reshape(x.shape[0], num_classes)
    div = Tc if avg and Tc > 0 else 1
    sx = abs_leaf_sums(nodes, T, D, x, num_classes) / div
    sr = abs_leaf_sums(nodes, T, D, bg, num_classes).mean(axis=0)[None, :] / div
    tol = (bound.sum(axis=-1) + (Tc + 4) * U * (sx + sr) + 4 * U * (np.abs(margin) + np.abs(got[:, :, -1]) + abs(bias)))
    assert np.all(np.abs(got.sum(axis=-1) - margin) <= tol), f"{label}: additivity"
    m.close()
    return f, got, rel


@pytest.mark.parametrize("seed", range(3))
def test_small_shapes_brute_force(env, seed):
    ta, _ = env
    rng = np.random.default_rng(200 + seed)
    T, D, F = int(rng.integers(2, 16)), int(rng.integers(1, 6)), int(rng.integers(2, 8))
    nodes = ta.synth_forest(T, D, F, seed=seed, leaf_prob=0.15)
    internal = (nodes["bits"].view(np.uint32) >> 31) == 0
    nodes["val"][internal & (rng.random(nodes.size) < 0.05)] = np.nan
    x = ta.synth_data(37, F, seed=seed + 7, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    bg = ta.synth_data(6, F, seed=seed + 8, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    check(env, nodes, T, D, F, x, bg, label=f"brute T={T} D={D} F={F}", brute=True)


def test_k1_shape(env):
    import bench

    ta, _ = env
    _, (nodes, T, D, F), data = bench.baseline_workload(ta, "K1")
    check(env, nodes, T, D, F, np.ascontiguousarray(data[:16]), np.ascontiguousarray(data[5000:5064]), label="K1 B=64")


def test_hist_forest_with_missing_and_nan(env):
    ta, _ = env
    nodes = ta.synth_forest_hist(60, 8, 32, seed=5, feature_seed=6)
    x = ta.synth_data_hist(40, 32, seed=7, feature_seed=6, missing_prob=0.05, missing=MISSING)
    bg = ta.synth_data_hist(24, 32, seed=8, feature_seed=6, missing_prob=0.05, missing=MISSING)
    rng = np.random.default_rng(3)
    x[rng.random(x.shape) < 0.03] = np.nan
    bg[rng.random(bg.shape) < 0.03] = np.nan
    check(env, nodes, 60, 8, 32, x, bg, label="hist 60x8 F=32")


def test_repeated_features_on_paths(env):
    ta, _ = env
    nodes = ta.synth_forest(40, 9, 3, seed=17, leaf_prob=0.05)  # 9 levels on 3 features: every path repeats features
    x = ta.synth_data(50, 3, seed=18, missing_prob=0.05, missing=MISSING, nan_prob=0.02)
    bg = ta.synth_data(33, 3, seed=19, missing_prob=0.05, missing=MISSING, nan_prob=0.02)
    check(env, nodes, 40, 9, 3, x, bg, label="repeats F=3")


@pytest.mark.parametrize("F", [600, 8192])
def test_wide_rows(env, F):
    ta, _ = env
    nodes = ta.synth_forest(10, 7, F, seed=F, leaf_prob=0.05)
    x = ta.synth_data(11, F, seed=F + 1, missing_prob=0.02, missing=MISSING, nan_prob=0.01)
    bg = ta.synth_data(9, F, seed=F + 2, missing_prob=0.02, missing=MISSING, nan_prob=0.01)
    check(env, nodes, 10, 7, F, x, bg, label=f"wide F={F}")


@pytest.mark.parametrize("C", [3, 10])
def test_multiclass(env, C):
    ta, torch = env
    T, D, F = 4 * C, 6, 16
    nodes = ta.synth_forest_hist(T, D, F, seed=C, feature_seed=C + 1)
    x = ta.synth_data_hist(45, F, seed=C + 2, feature_seed=C + 1, missing_prob=0.03, missing=MISSING)
    bg = ta.synth_data_hist(20, F, seed=C + 3, feature_seed=C + 1, missing_prob=0.03, missing=MISSING)
    out = ta.OUT_AVG | ta.OUT_SOFTMAX
    f, got, _ = check(env, nodes, T, D, F, x, bg, num_classes=C, output=out, bias=0.375, label=f"C={C}")
    for c in range(C):
        g = ta.Forest(ivr.sub_forest(nodes, T, C, c), T // C, D, F, missing=MISSING, output=ta.OUT_AVG, global_bias=0.375,
                      contribs=True)
        g.set_background(dev(env, bg))
        one = gpu_phi(env, g, x)[:, 0, :]
        assert np.array_equal(bits(one), bits(got[:, c, :].astype(np.float32))), c
        g.close()


def test_background_equal_to_the_row_gives_plus_zero(env):
    ta, _ = env
    nodes = ta.synth_forest(30, 7, 12, seed=31, leaf_prob=0.1)
    x = ta.synth_data(20, 12, seed=32, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    f = ta.Forest(nodes, 30, 7, 12, missing=MISSING, contribs=True)
    for k in range(x.shape[0]):
        f.set_background(dev(env, x[k:k + 1]))
        phi = gpu_phi(env, f, x[k:k + 1])
        assert np.all(bits(phi[:, :, :-1]) == 0), k  # +0.0, not -0.0


def test_unused_feature_is_zero(env):
    ta, _ = env
    T, D, F = 25, 6, 9
    nodes = ta.synth_forest(T, D, F, seed=41, leaf_prob=0.1)
    internal = (nodes["bits"].view(np.uint32) >> 31) == 0
    fid = nodes["bits"].view(np.uint32) & 0x3FFFFFFF
    assert np.any(internal & (fid == 4))
    nodes["bits"][internal & (fid == 4)] += 1  # feature 4 -> 5: no tree uses 4
    x = ta.synth_data(30, F, seed=42, missing_prob=0.05, missing=MISSING)
    bg = ta.synth_data(10, F, seed=43, missing_prob=0.05, missing=MISSING)
    f = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True)
    f.set_background(dev(env, bg))
    phi = gpu_phi(env, f, x)
    assert np.all(bits(phi[:, :, 4]) == 0)
    assert np.any(phi[:, :, 5] != 0)


@pytest.fixture(scope="module")
def k_forest(env):
    ta, torch = env
    T, D, F = 40, 8, 24
    nodes = ta.synth_forest_hist(T, D, F, seed=21, feature_seed=22)
    x = ta.synth_data_hist(333, F, seed=23, feature_seed=22, missing_prob=0.03, missing=MISSING)
    bg = ta.synth_data_hist(37, F, seed=24, feature_seed=22, missing_prob=0.03, missing=MISSING)
    f = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True)
    f.set_background(dev(env, bg))
    return nodes, T, D, F, x, bg, f, gpu_phi(env, f, x)


def test_repeat_calls_are_bitwise_identical(env, k_forest):
    nodes, T, D, F, x, bg, f, ref = k_forest
    for _ in range(3):
        assert np.array_equal(bits(gpu_phi(env, f, x)), bits(ref))


def test_rows_do_not_depend_on_the_batch(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, bg, f, ref = k_forest
    assert tuple(f.predict_contribs_interventional(torch.empty((0, F), device="cuda")).shape) == (0, F + 1)
    perm = np.random.default_rng(1).permutation(x.shape[0])
    assert np.array_equal(bits(gpu_phi(env, f, x[perm])), bits(ref[perm]))
    for n in (1, 2, 7, 8, 9, 67, 130):
        assert np.array_equal(bits(gpu_phi(env, f, x[:n])), bits(ref[:n])), n
    for r in (0, 5, 332):
        assert np.array_equal(bits(gpu_phi(env, f, x[r:r + 1])), bits(ref[r:r + 1])), r


def test_strategy_has_no_effect(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, bg, f, ref = k_forest
    for s in (ta.STRATEGY_DIRECT, ta.STRATEGY_ROWTILE, ta.STRATEGY_TILEBLOCK, ta.STRATEGY_TILERING, ta.STRATEGY_QRING,
              ta.STRATEGY_AUTO):
        f.set_strategy(s)
        f.set_background(dev(env, bg))  # the bias is computed under any strategy setting ...
        if s != ta.STRATEGY_AUTO:
            assert f.get_strategy(100) == s
        assert np.array_equal(bits(gpu_phi(env, f, x)), bits(ref)), s
    f.set_strategy(ta.STRATEGY_QRING)
    f.set_background(dev(env, bg))
    assert f.get_strategy(100) == ta.STRATEGY_QRING  # ... and leaves the setting as it was
    f.set_strategy(ta.STRATEGY_AUTO)


def test_relayout_gives_the_same_bits(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, bg, f, ref = k_forest
    g = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True, relayout=True)
    assert g.info().relayout == 1
    g.set_background(dev(env, bg))
    assert np.array_equal(bits(gpu_phi(env, g, x)), bits(ref))


def test_background_replaced_cleared_and_counted(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, bg, f, ref = k_forest
    g = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True)
    base = g.info().device_bytes
    g.set_background(dev(env, bg[:5]))
    other = gpu_phi(env, g, x)
    assert not np.array_equal(bits(other), bits(ref))
    assert g.info().device_bytes > base
    g.set_background(dev(env, bg))  # replaced; the caller's tensor may go away
    torch.cuda.synchronize()
    assert np.array_equal(bits(gpu_phi(env, g, x)), bits(ref))
    g.set_background(dev(env, bg))  # the same background again
    assert np.array_equal(bits(gpu_phi(env, g, x)), bits(ref))
    g.set_background(None)
    assert g.info().device_bytes == base
    out = torch.full((4, F + 1), 7.0, device="cuda")
    xd = dev(env, x[:4])
    assert ta.lib.tahoe_forest_predict_contribs_interventional(g._h, out.data_ptr(), xd.data_ptr(), 4, None) == UNSUPPORTED
    assert "background" in ta.lib.tahoe_last_error().decode()
    g.set_background(dev(env, bg))
    assert ta.lib.tahoe_forest_set_background(g._h, None, 0, None) == 0  # (NULL, 0) clears
    assert ta.lib.tahoe_forest_predict_contribs_interventional(g._h, out.data_ptr(), xd.data_ptr(), 4, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.all(out == 7.0).item()


def test_graph_capture_after_set_background(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, bg, f, ref = k_forest
    xd = dev(env, x)
    out = torch.empty((x.shape[0], F + 1), device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        f.predict_contribs_interventional(xd, out=out, stream=s)
    out.zero_()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(ref[:, 0, :]))


def test_refusals(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, bg, f, ref = k_forest
    xd, bgd = dev(env, x), dev(env, bg)
    out = torch.full((x.shape[0], F + 1), 7.0, device="cuda")
    n = x.shape[0]
    plain = ta.Forest(nodes, T, D, F, missing=MISSING)
    assert ta.lib.tahoe_forest_set_background(plain._h, bgd.data_ptr(), bg.shape[0], None) == UNSUPPORTED
    assert "TAHOE_CREATE_CONTRIBS" in ta.lib.tahoe_last_error().decode()
    assert ta.lib.tahoe_forest_predict_contribs_interventional(plain._h, out.data_ptr(), xd.data_ptr(), n, None) == UNSUPPORTED
    assert "TAHOE_CREATE_CONTRIBS" in ta.lib.tahoe_last_error().decode()
    sn, tr = ta.capi.dense_to_sparse(nodes, T, D)
    sp = ta.capi.SparseForest(sn, tr, F, missing=MISSING)
    assert ta.lib.tahoe_forest_set_background(sp._h, bgd.data_ptr(), bg.shape[0], None) == UNSUPPORTED
    assert ta.lib.tahoe_forest_predict_contribs_interventional(sp._h, out.data_ptr(), xd.data_ptr(), n, None) == UNSUPPORTED
    assert "sparse" in ta.lib.tahoe_last_error().decode()
    nobg = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True)
    assert ta.lib.tahoe_forest_predict_contribs_interventional(nobg._h, out.data_ptr(), xd.data_ptr(), n, None) == UNSUPPORTED
    assert "no background" in ta.lib.tahoe_last_error().decode()
    # NULL arguments and overflows
    assert ta.lib.tahoe_forest_predict_contribs_interventional(f._h, None, xd.data_ptr(), 5, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_predict_contribs_interventional(f._h, out.data_ptr(), None, 5, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_predict_contribs_interventional(f._h, None, None, 0, None) == 0
    assert ta.lib.tahoe_forest_predict_contribs_interventional(f._h, out.data_ptr(), xd.data_ptr(), 2 ** 62, None) == INVALID_ARG
    assert "overflow" in ta.lib.tahoe_last_error().decode()
    assert ta.lib.tahoe_forest_set_background(f._h, None, 5, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_set_background(f._h, bgd.data_ptr(), 2 ** 62, None) == INVALID_ARG
    assert "overflow" in ta.lib.tahoe_last_error().decode()
    torch.cuda.synchronize()
    assert torch.all(out == 7.0).item()  # nothing was launched
    # the refused calls kept f's background
    assert np.array_equal(bits(gpu_phi(env, f, x)), bits(ref))
