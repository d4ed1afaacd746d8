"""Per-feature contributions (tahoe_forest_predict_contribs) on the GPU against the float64 references of tests/contribs_ref.py.
Needs an MI355X.

Bars: |phi_gpu - phi_64| <= gamma * A per output, A = sum of |per-path terms| feeding it (contribs_ref.poly), gamma =
(n_terms + 4 (depth + 2)) 2^-24: a float32 recursive sum of n_terms terms, each carrying the rounding of an extend / unwind of at
most depth + 2 steps.  The bias column bit for bit (float64 on the host, rounded once).  Additivity against the library's own
margin within the same bound plus the margin's own float32 sum.  Bitwise: repeat calls, any batch / permutation / prefix,
every strategy, the re-layout, and class c of a multi-class handle against a handle on class c's sub-forest."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contribs_ref  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
U = 2.0 ** -24


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def gpu_phi(env, forest, x):
    ta, torch = env
    out = forest.predict_contribs(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    torch.cuda.synchronize()
    phi = out.cpu().numpy()
    return phi if phi.ndim == 3 else phi[:, None, :]


def check(env, nodes, T, D, F, x, num_classes=1, output=0, bias=0.0, label="", brute=False):
    ta, torch = env
    avg = (output & ta.OUT_AVG) != 0
    f = ta.Forest(nodes, T, D, F, missing=MISSING, output=output, global_bias=bias, num_classes=num_classes, contribs=True)
    got = gpu_phi(env, f, x).astype(np.float64)
    want, A, N = contribs_ref.poly(nodes, T, D, F, x, MISSING, num_classes=num_classes, avg=avg, global_bias=bias)
    if brute:
        want = contribs_ref.brute(nodes, T, D, F, x, MISSING, num_classes=num_classes, avg=avg, global_bias=bias)
    gamma = (N[None, :, :] + 4 * (D + 2)) * U
    err = np.abs(got - want)[:, :, :-1]
    bound = (gamma * A)[:, :, :-1]
    scale = np.abs(want).sum(axis=-1) + 1e-30
    rel = float(np.max(err.max(axis=-1) / scale))
    assert np.all(err <= bound), f"{label}: max |phi - phi64| / sum|phi64| = {rel:.3e}; bound exceeded at {np.argwhere(err > bound)[:5]}"
    # bias column bit for bit
    b = contribs_ref.bias_f32(nodes, T, D, num_classes, avg, bias)
    assert np.array_equal(bits(got[:, :, -1].astype(np.float32)), bits(np.broadcast_to(b, got[:, :, -1].shape))), label
    # additivity against the library's margins (AVG and bias applied, no sigmoid / softmax)
    m = ta.Forest(nodes, T, D, F, missing=MISSING, output=output & ta.OUT_AVG, global_bias=bias, num_classes=num_classes)
    margin = m.predict(torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64).reshape(x.shape[0], num_classes)
    Tc = T // num_classes
    tol = (gamma * A)[:, :, :-1].sum(axis=-1) + (Tc + 4) * U * (A.sum(axis=-1) + np.abs(margin)) + F * U * np.abs(got).sum(-1)
    assert np.all(np.abs(got.sum(axis=-1) - margin) <= tol), f"{label}: additivity"
    m.close()
    return f, got, rel


@pytest.mark.parametrize("seed", range(4))
def test_small_shapes_brute_force(env, seed):
    ta, _ = env
    rng = np.random.default_rng(100 + seed)
    T, D, F = int(rng.integers(2, 21)), int(rng.integers(1, 6)), int(rng.integers(2, 9))
    nodes = ta.synth_forest(T, D, F, seed=seed, leaf_prob=0.15)
    nodes["weight"] = rng.uniform(0.05, 1.0, nodes.size).astype(np.float32)
    internal = (nodes["bits"].view(np.uint32) >> 31) == 0
    nodes["val"][internal & (rng.random(nodes.size) < 0.05)] = np.nan
    x = ta.synth_data(131, F, seed=seed + 7, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    check(env, nodes, T, D, F, x, label=f"brute T={T} D={D} F={F}", brute=True)


def test_hist_forest_100x8_on_32(env):
    ta, _ = env
    nodes = ta.synth_forest_hist(100, 8, 32, seed=5, feature_seed=6)
    x = ta.synth_data_hist(150, 32, seed=7, feature_seed=6, missing_prob=0.02, missing=MISSING)
    check(env, nodes, 100, 8, 32, x, label="hist 100x8 F=32")


def test_synth_forest_30x12_on_256(env):
    ta, _ = env
    nodes = ta.synth_forest(30, 12, 256, seed=9, leaf_prob=0.05)
    x = ta.synth_data(70, 256, seed=10, missing_prob=0.02, missing=MISSING, nan_prob=0.01)
    check(env, nodes, 30, 12, 256, x, label="synth 30x12 F=256")


@pytest.mark.parametrize("F", [600, 3072])
def test_wide_rows(env, F):
    ta, _ = env
    nodes = ta.synth_forest(12, 7, F, seed=F, leaf_prob=0.05)
    x = ta.synth_data(37, F, seed=F + 1, missing_prob=0.02, missing=MISSING, nan_prob=0.01)
    check(env, nodes, 12, 7, F, x, label=f"wide F={F}")


@pytest.mark.parametrize("C", [3, 10])
def test_multiclass(env, C):
    ta, torch = env
    T, D, F = 4 * C, 6, 16
    nodes = ta.synth_forest_hist(T, D, F, seed=C, feature_seed=C + 1)
    x = ta.synth_data_hist(90, F, seed=C + 2, feature_seed=C + 1, missing_prob=0.03, missing=MISSING)
    out = ta.OUT_AVG | ta.OUT_SOFTMAX
    f, got, _ = check(env, nodes, T, D, F, x, num_classes=C, output=out, bias=0.375, label=f"C={C}")
    per = nodes.size // T
    for c in range(C):
        sub = np.ascontiguousarray(nodes.reshape(T, per)[c::C]).reshape(-1)
        g = ta.Forest(sub, T // C, D, F, missing=MISSING, output=ta.OUT_AVG, global_bias=0.375, contribs=True)
        one = gpu_phi(env, g, x)[:, 0, :]
        assert np.array_equal(bits(one), bits(got[:, c, :].astype(np.float32))), c
        g.close()


@pytest.fixture(scope="module")
def k_forest(env):
    ta, torch = env
    T, D, F = 40, 8, 24
    nodes = ta.synth_forest_hist(T, D, F, seed=21, feature_seed=22)
    x = ta.synth_data_hist(333, F, seed=23, feature_seed=22, missing_prob=0.03, missing=MISSING)
    f = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True)
    return nodes, T, D, F, x, f, gpu_phi(env, f, x)


def test_repeat_calls_are_bitwise_identical(env, k_forest):
    nodes, T, D, F, x, f, ref = k_forest
    for _ in range(3):
        assert np.array_equal(bits(gpu_phi(env, f, x)), bits(ref))


def test_rows_do_not_depend_on_the_batch(env, k_forest):
    nodes, T, D, F, x, f, ref = k_forest
    perm = np.random.default_rng(1).permutation(x.shape[0])
    assert np.array_equal(bits(gpu_phi(env, f, x[perm])), bits(ref[perm]))
    for n in (1, 2, 63, 64, 65, 130, 257):
        assert np.array_equal(bits(gpu_phi(env, f, x[:n])), bits(ref[:n])), n
    for r in (0, 5, 332):
        assert np.array_equal(bits(gpu_phi(env, f, x[r:r + 1])), bits(ref[r:r + 1])), r


def test_strategy_has_no_effect(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, f, ref = k_forest
    for s in (ta.STRATEGY_DIRECT, ta.STRATEGY_ROWTILE, ta.STRATEGY_TILEBLOCK, ta.STRATEGY_TILERING, ta.STRATEGY_QRING,
              ta.STRATEGY_AUTO):
        f.set_strategy(s)
        assert np.array_equal(bits(gpu_phi(env, f, x)), bits(ref)), s


def test_relayout_gives_the_same_bits(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, f, ref = k_forest
    g = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True, relayout=True)
    assert g.info().relayout == 1
    assert np.array_equal(bits(gpu_phi(env, g, x)), bits(ref))


def test_tables_count_in_device_bytes(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, f, ref = k_forest
    a = ta.Forest(nodes, T, D, F, missing=MISSING)
    assert f.info().device_bytes > a.info().device_bytes


def test_refusals(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, f, ref = k_forest
    xd = torch.from_numpy(x).cuda()
    out = torch.zeros((x.shape[0], F + 1), device="cuda")
    plain = ta.Forest(nodes, T, D, F, missing=MISSING)
    assert ta.lib.tahoe_forest_predict_contribs(plain._h, out.data_ptr(), xd.data_ptr(), x.shape[0], None) == 7
    assert "TAHOE_CREATE_CONTRIBS" in ta.lib.tahoe_last_error().decode()
    sn, tr = ta.capi.dense_to_sparse(nodes, T, D)
    sp = ta.capi.SparseForest(sn, tr, F, missing=MISSING)
    assert ta.lib.tahoe_forest_predict_contribs(sp._h, out.data_ptr(), xd.data_ptr(), x.shape[0], None) == 7
    assert "sparse" in ta.lib.tahoe_last_error().decode()
    torch.cuda.synchronize()
    assert torch.count_nonzero(out).item() == 0  # nothing was launched
    assert ta.lib.tahoe_forest_predict_contribs(f._h, None, xd.data_ptr(), 5, None) == 1
    assert ta.lib.tahoe_forest_predict_contribs(f._h, out.data_ptr(), None, 5, None) == 1
    assert ta.lib.tahoe_forest_predict_contribs(f._h, None, None, 0, None) == 0


@pytest.mark.parametrize("name,kw", [("tahoe_forest_predict_contribs", {"contribs": True}),
                                     ("tahoe_forest_predict_contribs_approx", {"approx_contribs": True})])
def test_huge_rows_overflow(env, k_forest, name, kw):
    ta, torch = env
    nodes, T, D, F, x, f, ref = k_forest
    g = ta.Forest(nodes, T, D, F, missing=MISSING, **kw)
    xd = torch.from_numpy(x).cuda()
    out = torch.full((x.shape[0], F + 1), 7.0, device="cuda")
    huge = (1 << 64) // (4 * (F + 1)) + 1  # rows x (F + 1) x 4 overflows size_t
    assert getattr(ta.lib, name)(g._h, out.data_ptr(), xd.data_ptr(), huge, None) == 1
    assert "overflow" in ta.lib.tahoe_last_error().decode()
    torch.cuda.synchronize()
    assert torch.all(out == 7.0).item()  # nothing was launched
    g.close()


def test_zero_rows(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, f, ref = k_forest
    assert tuple(f.predict_contribs(torch.empty((0, F), device="cuda")).shape) == (0, F + 1)


def test_graph_capture_after_reserve(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, f, ref = k_forest
    f.reserve(x.shape[0])
    xd = torch.from_numpy(x).cuda()
    out = torch.empty((x.shape[0], F + 1), device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        f.predict_contribs(xd, out=out, stream=s)
    out.zero_()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(ref[:, 0, :]))
