"""SHAP interaction values (tahoe_forest_predict_interactions) on the GPU against the float64 references of
tests/interactions_ref.py.  Needs an MI355X.

Off-diagonal bar: |Phi_gpu - Phi_64| <= gamma * A per entry, A = sum of |per-path terms| feeding it (interactions_ref.poly),
gamma = (N + 6 (depth + 2)) 2^-24.  N is the count of float32 adds into the entry (a recursive sum of N terms).  The 6 per path
step bounds a term's own rounding: the conditioned extend and unwind run at most depth + 1 steps each, and a lane's weight or
running total takes at most 4 roundings per step (the bound test_contribs_gpu.py uses for the same recursions); the term then
takes 4 more products (o_j - z_j, the leaf, o_k - z_k, 1/2, one of them exact), the AVG division and, in the LDS form, 3 slab
merges: 8 roundings, <= 2 (depth + 2) as soon as a tree has a pair (depth >= 2).  The data does not enter the constant.

Exact bits: symmetry, the diagonal recomputed on the host in float32 from the GPU off-diagonals and predict_contribs, the bias
corner, +0.0 in row and column F and for an unused feature, and every reproducibility property of predict_contribs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contribs_ref  # noqa: E402
import interactions_ref  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
U = 2.0 ** -24
K_STEP = 6


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gpu_inter(env, forest, x):
    ta, torch = env
    out = forest.predict_interactions(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    torch.cuda.synchronize()
    m = out.cpu().numpy()
    return m if m.ndim == 4 else m[:, None]


def gpu_phi(env, forest, x):
    ta, torch = env
    out = forest.predict_contribs(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    torch.cuda.synchronize()
    phi = out.cpu().numpy()
    return phi if phi.ndim == 3 else phi[:, None, :]


def host_diagonal(m, phi):
    """float32: phi_i - (0.0f + M[i][0] + ... + M[i][F-1], j != i, ascending)."""
    F = m.shape[-1] - 1
    off = m[..., :F, :F].astype(np.float32)
    want = np.empty(m.shape[:-2] + (F,), np.float32)
    for i in range(F):
        cols = [j for j in range(F) if j != i]
        terms = np.concatenate([np.zeros(m.shape[:-2] + (1,), np.float32), off[..., i, cols]], axis=-1)
        s = np.add.accumulate(terms, axis=-1, dtype=np.float32)[..., -1]
        want[..., i] = phi[..., i].astype(np.float32) - s
    return want


def check_exact(env, f, got, x):
    """Bits that follow from the definition: symmetry, diagonal, bias corner, zero row / column F."""
    F = got.shape[-1] - 1
    assert np.array_equal(bits(got), bits(got.swapaxes(-1, -2))), "not exactly symmetric"
    phi = gpu_phi(env, f, x)
    idx = np.arange(F)
    assert np.array_equal(bits(got[..., idx, idx]), bits(host_diagonal(got, phi))), "diagonal"
    assert np.array_equal(bits(got[..., F, F]), bits(phi[..., F])), "bias corner"
    assert not np.any(bits(got[..., F, :F])) and not np.any(bits(got[..., :F, F])), "row / column F not +0.0"
    return phi


def check(env, nodes, T, D, F, x, num_classes=1, output=0, bias=0.0, label="", brute=False):
    ta, torch = env
    avg = (output & ta.OUT_AVG) != 0
    f = ta.Forest(nodes, T, D, F, missing=MISSING, output=output, global_bias=bias, num_classes=num_classes, contribs=True)
    got32 = gpu_inter(env, f, x)
    got = got32.astype(np.float64)
    want, A, N = interactions_ref.poly(nodes, T, D, F, x, MISSING, num_classes=num_classes, avg=avg, global_bias=bias)
    if brute:
        b = interactions_ref.brute(nodes, T, D, F, x, MISSING, num_classes=num_classes, avg=avg, global_bias=bias)
        # brute's v(S) differences leave ~1e-18 where no path holds the pair (poly: exactly 0): brute checks poly, poly the GPU
        assert np.allclose(b, want, rtol=0, atol=1e-12 * (np.abs(b).sum() + 1)), label
    off = ~np.eye(F + 1, dtype=bool)
    off[F, :] = off[:, F] = False
    gamma = (N[None] + K_STEP * (D + 2)) * U
    err = np.abs(got - want)[..., off]
    bound = (gamma * A)[..., off]
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    assert np.all(err <= bound), f"{label}: bound exceeded at {np.argwhere(err > bound)[:5]}; max err / bound {worst:.3e}"
    assert np.count_nonzero(want[..., off]) > 0, f"{label}: a forest without interactions tests nothing"
    phi = check_exact(env, f, got32, x)
    # additivity: the matrix sums to the library's margin (AVG and bias applied, no sigmoid / softmax).  Bound: the diagonal's
    # float32 sums (F + 1 roundings of at most sum |M| per row) plus predict_contribs' own additivity bound (test_contribs_gpu)
    m = ta.Forest(nodes, T, D, F, missing=MISSING, output=output & ta.OUT_AVG, global_bias=bias, num_classes=num_classes)
    margin = m.predict(torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64).reshape(x.shape[0], num_classes)
    m.close()
    cw, cA, cN = contribs_ref.poly(nodes, T, D, F, x, MISSING, num_classes=num_classes, avg=avg, global_bias=bias)
    cg = (cN[None] + 4 * (D + 2)) * U
    Tc = T // num_classes
    phi64 = phi.astype(np.float64)
    tol = ((cg * cA)[..., :-1].sum(-1) + (Tc + 4) * U * (cA.sum(-1) + np.abs(margin)) + F * U * np.abs(phi64).sum(-1)
           + (F + 2) * U * np.abs(got).sum(axis=(-1, -2)))
    assert np.all(np.abs(got.sum(axis=(-1, -2)) - margin) <= tol), f"{label}: additivity"
    return f, got32


@pytest.mark.parametrize("seed", range(4))
def test_small_shapes_brute_force(env, seed):
    ta, _ = env
    rng = np.random.default_rng(300 + seed)
    T, D, F = int(rng.integers(2, 13)), int(rng.integers(2, 6)), int(rng.integers(3, 9))
    nodes = ta.synth_forest(T, D, F, seed=seed, leaf_prob=0.15)
    nodes["weight"] = rng.uniform(0.05, 1.0, nodes.size).astype(np.float32)
    internal = (nodes["bits"].view(np.uint32) >> 31) == 0
    nodes["val"][internal & (rng.random(nodes.size) < 0.05)] = np.nan
    x = ta.synth_data(71, F, seed=seed + 7, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    check(env, nodes, T, D, F, x, label=f"brute T={T} D={D} F={F}", brute=True)


def test_hist_forest_100x8_on_32(env):
    """F = 32: the LDS-slab form."""
    ta, _ = env
    nodes = ta.synth_forest_hist(100, 8, 32, seed=5, feature_seed=6)
    x = ta.synth_data_hist(40, 32, seed=7, feature_seed=6, missing_prob=0.02, missing=MISSING)
    check(env, nodes, 100, 8, 32, x, label="hist 100x8 F=32")


def test_synth_forest_30x12_on_256(env):
    """F = 256: the in-place form."""
    ta, _ = env
    nodes = ta.synth_forest(30, 12, 256, seed=9, leaf_prob=0.05)
    x = ta.synth_data(12, 256, seed=10, missing_prob=0.02, missing=MISSING, nan_prob=0.01)
    check(env, nodes, 30, 12, 256, x, label="synth 30x12 F=256")


def test_wide_rows_600(env):
    ta, _ = env
    nodes = ta.synth_forest(12, 7, 600, seed=600, leaf_prob=0.05)
    x = ta.synth_data(9, 600, seed=601, missing_prob=0.02, missing=MISSING, nan_prob=0.01)
    check(env, nodes, 12, 7, 600, x, label="wide F=600")


@pytest.mark.parametrize("C", [3, 10])
def test_multiclass(env, C):
    ta, torch = env
    T, D, F = 4 * C, 6, 16
    nodes = ta.synth_forest_hist(T, D, F, seed=C, feature_seed=C + 1)
    x = ta.synth_data_hist(50, F, seed=C + 2, feature_seed=C + 1, missing_prob=0.03, missing=MISSING)
    out = ta.OUT_AVG | ta.OUT_SOFTMAX
    f, got = check(env, nodes, T, D, F, x, num_classes=C, output=out, bias=0.375, label=f"C={C}")
    per = nodes.size // T
    for c in range(C):
        sub = np.ascontiguousarray(nodes.reshape(T, per)[c::C]).reshape(-1)
        g = ta.Forest(sub, T // C, D, F, missing=MISSING, output=ta.OUT_AVG, global_bias=0.375, contribs=True)
        assert np.array_equal(bits(gpu_inter(env, g, x)[:, 0]), bits(got[:, c])), c
        g.close()


@pytest.mark.parametrize("F", [12, 200])
def test_unused_feature_is_all_zero(env, F):
    """A column no tree splits on: its row, column and diagonal are +0.0 (F = 12 LDS form, F = 200 in place)."""
    ta, _ = env
    T, D = 10, 5
    nodes = ta.synth_forest(T, D, F - 1, seed=F, leaf_prob=0.1)  # features 0 .. F - 2: column F - 1 is unused
    x = ta.synth_data(33, F, seed=F + 1, missing_prob=0.05, missing=MISSING, nan_prob=0.02)
    f = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True)
    got = gpu_inter(env, f, x)
    u = F - 1
    assert not np.any(bits(got[..., u, :])) and not np.any(bits(got[..., :, u]))
    check_exact(env, f, got, x)


@pytest.fixture(scope="module", params=["lds", "in_place"])
def k_forest(env, request):
    ta, torch = env
    T, D, F = (40, 8, 24) if request.param == "lds" else (16, 7, 90)
    nodes = ta.synth_forest_hist(T, D, F, seed=21, feature_seed=22)
    x = ta.synth_data_hist(133, F, seed=23, feature_seed=22, missing_prob=0.03, missing=MISSING)
    f = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True)
    return nodes, T, D, F, x, f, gpu_inter(env, f, x)


def test_repeat_calls_are_bitwise_identical(env, k_forest):
    nodes, T, D, F, x, f, ref = k_forest
    for _ in range(3):
        assert np.array_equal(bits(gpu_inter(env, f, x)), bits(ref))
    check_exact(env, f, ref, x)


def test_rows_do_not_depend_on_the_batch(env, k_forest):
    nodes, T, D, F, x, f, ref = k_forest
    perm = np.random.default_rng(1).permutation(x.shape[0])
    assert np.array_equal(bits(gpu_inter(env, f, x[perm])), bits(ref[perm]))
    for n in (1, 2, 3, 9, 17, 33, 67, 130):
        assert np.array_equal(bits(gpu_inter(env, f, x[:n])), bits(ref[:n])), n
    for r in (0, 5, 132):
        assert np.array_equal(bits(gpu_inter(env, f, x[r:r + 1])), bits(ref[r:r + 1])), r


def test_strategy_and_relayout_have_no_effect(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, f, ref = k_forest
    for s in (ta.STRATEGY_DIRECT, ta.STRATEGY_ROWTILE, ta.STRATEGY_TILEBLOCK, ta.STRATEGY_TILERING, ta.STRATEGY_QRING,
              ta.STRATEGY_AUTO):
        f.set_strategy(s)
        assert np.array_equal(bits(gpu_inter(env, f, x)), bits(ref)), s
    g = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True, relayout=True)
    assert g.info().relayout == 1
    assert np.array_equal(bits(gpu_inter(env, g, x)), bits(ref))
    g.close()


def test_batches_of_0_1_and_67_rows(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, f, ref = k_forest
    assert tuple(f.predict_interactions(torch.empty((0, F), device="cuda")).shape) == (0, F + 1, F + 1)
    for n in (1, 67):
        out = f.predict_interactions(torch.from_numpy(x[40:40 + n]).cuda())
        assert tuple(out.shape) == (n, F + 1, F + 1)
        assert np.array_equal(bits(out.cpu().numpy()), bits(ref[40:40 + n, 0]))


def test_graph_capture_without_reserve(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, f, ref = k_forest
    g_forest = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True)  # fresh handle: nothing reserved
    xd = torch.from_numpy(x).cuda()
    out = torch.empty((x.shape[0], F + 1, F + 1), device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        g_forest.predict_interactions(xd, out=out, stream=s)
    out.fill_(7.0)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(ref[:, 0]))
    g_forest.close()


def test_refusals(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, f, ref = k_forest
    xd = torch.from_numpy(x).cuda()
    n = x.shape[0]
    out = torch.full((n, F + 1, F + 1), 7.0, device="cuda")
    call = ta.lib.tahoe_forest_predict_interactions
    plain = ta.Forest(nodes, T, D, F, missing=MISSING)
    assert call(plain._h, out.data_ptr(), xd.data_ptr(), n, None) == 7
    assert "TAHOE_CREATE_CONTRIBS" in ta.lib.tahoe_last_error().decode()
    sn, tr = ta.capi.dense_to_sparse(nodes, T, D)
    sp = ta.capi.SparseForest(sn, tr, F, missing=MISSING)
    assert call(sp._h, out.data_ptr(), xd.data_ptr(), n, None) == 7
    assert "sparse" in ta.lib.tahoe_last_error().decode()
    assert call(f._h, None, xd.data_ptr(), 5, None) == 1
    assert call(f._h, out.data_ptr(), None, 5, None) == 1
    assert call(f._h, None, None, 0, None) == 0
    assert call(f._h, out.data_ptr(), xd.data_ptr(), 0, None) == 0
    huge = (1 << 64) // (4 * (F + 1) * (F + 1)) + 1  # rows x (F + 1)^2 x 4 overflows size_t
    assert call(f._h, out.data_ptr(), xd.data_ptr(), huge, None) == 1
    assert "overflow" in ta.lib.tahoe_last_error().decode()
    torch.cuda.synchronize()
    assert torch.all(out == 7.0).item()  # nothing was launched
    plain.close()
