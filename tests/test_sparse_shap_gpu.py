"""TreeSHAP on sparse handles (tahoe_sparse_forest_create_ex with TAHOE_CREATE_CONTRIBS) on the GPU.  Needs an MI355X.

Bitwise: a dense handle and the sparse handle of its tahoe_dense_to_sparse_ex conversion hold the same path bins, so contributions,
interactions and interventional values agree bit for bit (single- and multi-class, every strategy setting); class c of a
multi-class sparse handle against a single-class sparse handle on class c's sub-forest; a row alone against the same row in a batch.
Accuracy: irregular deep forests (depth 4..24 on 8 features, 40-level vines that repeat features) with random positive covers
against the float64 brute force of tests/sparse_shap_ref.py, within gamma x (sum over paths of |leaf| x path length), gamma =
(paths + 4 (depth + 2)) 2^-24 -- the kind of bar the dense SHAP tests use, with an upper bound of their sum of |terms|."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_shap_ref as ref  # noqa: E402

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


def run_all(env, f, x, bg):
    """(contribs, interactions, interventional) as numpy, each with a class axis."""
    ta, torch = env
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    phi = f.predict_contribs(xd).cpu().numpy()
    inter = f.predict_interactions(xd).cpu().numpy()
    f.set_background(torch.from_numpy(np.ascontiguousarray(bg)).cuda())
    iv = f.predict_contribs_interventional(xd).cpu().numpy()
    f.check()
    if f.num_classes == 1:
        phi, inter, iv = phi[:, None], inter[:, None], iv[:, None]
    return phi, inter, iv


def all_strategies(ta, f):
    out = []
    for s in (ta.STRATEGY_AUTO, ta.STRATEGY_DIRECT, ta.STRATEGY_ROWTILE, ta.STRATEGY_TILEBLOCK, ta.STRATEGY_QRING):
        try:
            f.set_strategy(s)
            out.append(s)
        except ta.TahoeError:
            pass
    return out


@pytest.mark.parametrize("case", ["k1_like", "multiclass"])
def test_dense_and_converted_sparse_give_the_same_bits(env, case):
    ta, torch = env
    if case == "k1_like":
        T, D, F, nc, out, bias = 40, 8, 24, 1, ta.OUT_AVG, 0.25
    else:
        T, D, F, nc, out, bias = 12, 6, 16, 3, ta.OUT_AVG | ta.OUT_SOFTMAX, -0.5
    nodes = ta.synth_forest_hist(T, D, F, seed=51, feature_seed=52)
    x = ta.synth_data_hist(200, F, seed=53, feature_seed=52, missing_prob=0.03, missing=MISSING)
    bg = ta.synth_data_hist(37, F, seed=54, feature_seed=52, missing_prob=0.03, missing=MISSING)
    dense = ta.Forest(nodes, T, D, F, missing=MISSING, output=out, global_bias=bias, num_classes=nc, contribs=True)
    want = run_all(env, dense, x, bg)
    sn, tr, cv = ta.capi.dense_to_sparse(nodes, T, D, covers=True)
    sp = ta.capi.SparseForest(sn, tr, F, missing=MISSING, output=out, global_bias=bias, covers=cv, num_classes=nc,
                              contribs=True)
    assert sp.info().device_bytes > 0
    strategies = all_strategies(ta, sp)
    assert len(strategies) == 5
    for s in strategies:
        sp.set_strategy(s)
        got = run_all(env, sp, x, bg)
        for name, a, b in zip(("contribs", "interactions", "interventional"), got, want):
            assert np.array_equal(bits(a), bits(b)), (case, name, s)
    sp.close()
    dense.close()


def _random_covers(sn, seed):
    return np.random.default_rng(seed).uniform(0.05, 1.0, sn.size).astype(np.float32)


def _vines(ta, T, depth, F, seed):
    """T vines `depth` levels deep on features k % F (a leaf on one side of every inner node, the side drawn at random)."""
    rng = np.random.default_rng(seed)
    parts, roots, off = [], [], 0
    for t in range(T):
        sn = np.zeros(2 * depth + 1, dtype=ta.capi.SPARSE_NODE_DTYPE)
        nxt = 0
        for k in range(depth):
            i = nxt
            sn[i] = (np.float32(rng.uniform(-1, 1)), ((k + t) % F) | (int(rng.integers(2)) << 30), 2 * k + 1)
            leaf_right = bool(rng.integers(2))
            leaf_pos = 2 * k + 1 + (1 if leaf_right else 0)
            sn[leaf_pos] = (np.float32(rng.uniform(-1, 1)), np.int32(-(1 << 31)), 0)
            nxt = 2 * k + 1 + (0 if leaf_right else 1)
        sn[nxt] = (np.float32(rng.uniform(-1, 1)), np.int32(-(1 << 31)), 0)
        parts.append(sn)
        roots.append(off)
        off += sn.size
    return np.concatenate(parts), np.array(roots, np.int32)


def _check_against_brute(env, sn, tr, F, nc, x, bg, out, bias, label):
    ta, torch = env
    cv = _random_covers(sn, 7)
    f = ta.capi.SparseForest(sn, tr, F, missing=MISSING, output=out, global_bias=bias, covers=cv, num_classes=nc, contribs=True)
    phi, inter, iv = run_all(env, f, x, bg)
    avg = (out & ta.OUT_AVG) != 0
    scale, depth, paths = ref.bound_scale(sn, tr, nc)
    gamma = (paths + 4 * (depth + 2)) * U
    tol = gamma * scale / ((tr.size // nc) if avg else 1)  # [C]
    # path-dependent contributions; the bias column is exact in float64, rounded once
    want = ref.contribs(sn, tr, cv, x, F, MISSING, nc, avg, bias)
    err = np.abs(phi[:, :, :F].astype(np.float64) - want[:, :, :F])
    assert np.all(err <= tol[None, :, None]), f"{label}: contribs max err {err.max():.3e} > {tol.max():.3e}"
    b = ref.bias_column(sn, tr, cv, nc, avg, bias)
    assert np.array_equal(bits(phi[:, :, F]), bits(np.broadcast_to(b, phi[:, :, F].shape))), label
    # additivity against the handle's own margins
    xd = torch.from_numpy(x).cuda()
    m = ta.capi.SparseForest(sn, tr, F, missing=MISSING, output=out & ta.OUT_AVG, global_bias=bias, num_classes=nc)
    margin = m.predict(xd).cpu().numpy().astype(np.float64).reshape(x.shape[0], nc)
    assert np.all(np.abs(phi.astype(np.float64).sum(-1) - margin) <= 2 * tol[None, :] + 1e-5 * np.abs(margin) + 1e-6), label
    # interactions off the diagonal; the diagonal is phi_i minus the row's off-diagonal sum
    want_i = ref.interactions(sn, tr, cv, x, F, MISSING, nc, avg)
    off = ~np.eye(F, dtype=bool)
    err = np.abs(inter[:, :, :F, :F].astype(np.float64) - want_i)[:, :, off]
    assert np.all(err <= 2 * tol[None, :, None]), f"{label}: interactions max err {err.max():.3e}"
    assert np.array_equal(bits(inter[:, :, F, :F]), bits(np.zeros_like(inter[:, :, F, :F]))), label
    assert np.array_equal(bits(inter[:, :, F, F]), bits(phi[:, :, F])), label
    # interventional against the same background (bias column from the library's float32 background sums)
    bg_raw = m.predict_raw(torch.from_numpy(bg).cuda()).cpu().numpy().reshape(bg.shape[0], nc)
    want_v = ref.interventional(sn, tr, x, bg, F, MISSING, nc, avg, bias, bg_raw=bg_raw)
    err = np.abs(iv[:, :, :F].astype(np.float64) - want_v[:, :, :F])
    assert np.all(err <= tol[None, :, None]), f"{label}: interventional max err {err.max():.3e}"
    assert np.array_equal(bits(iv[:, :, F]), bits(want_v[:, :, F].astype(np.float32))), label
    m.close()
    return f, cv, phi, inter, iv


@pytest.mark.parametrize("seed", range(3))
def test_irregular_deep_forest_against_brute_force(env, seed):
    ta, _ = env
    F = 8
    sn, tr = ta.capi.synth_sparse_forest(6, F, 4, 24, 0.5, 300, 600 + seed)
    x = ta.synth_data(9, F, seed=seed, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    bg = ta.synth_data(6, F, seed=seed + 50, missing_prob=0.1, missing=MISSING)
    f, *_ = _check_against_brute(env, sn, tr, F, 1, x, bg, 0, 0.125, f"irregular seed {seed}")
    f.close()


def test_vines_forty_levels_deep(env):
    ta, _ = env
    F = 8
    sn, tr = _vines(ta, 4, 40, F, 71)
    x = ta.synth_data(9, F, seed=72, missing_prob=0.1, missing=MISSING)
    bg = ta.synth_data(5, F, seed=73)
    f, *_ = _check_against_brute(env, sn, tr, F, 1, x, bg, 0, 0.0, "vines")
    f.close()


def test_classes_match_single_class_sub_forests(env):
    ta, torch = env
    F, nc = 8, 3
    sn, tr = ta.capi.synth_sparse_forest(9, F, 4, 16, 0.45, 300, 81)
    x = ta.synth_data(9, F, seed=82, missing_prob=0.1, missing=MISSING)
    bg = ta.synth_data(6, F, seed=83)
    out = ta.OUT_AVG | ta.OUT_SOFTMAX
    f, cv, phi, inter, iv = _check_against_brute(env, sn, tr, F, nc, x, bg, out, 0.5, "classes")
    for c in range(nc):
        s, t, c_cv = ref.sub_forest(sn, tr, c, nc, covers=cv)
        g = ta.capi.SparseForest(s, t, F, missing=MISSING, output=ta.OUT_AVG, global_bias=0.5, covers=c_cv, contribs=True)
        one = run_all(env, g, x, bg)
        for name, a, b in zip(("contribs", "interactions", "interventional"), one, (phi, inter, iv)):
            assert np.array_equal(bits(a[:, 0]), bits(b[:, c])), (name, c)
        g.close()
    f.close()


def test_a_row_alone_gives_the_bits_of_the_batch(env):
    ta, torch = env
    F = 24
    sn, tr = ta.capi.synth_sparse_forest(60, F, 4, 20, 0.32, 65535, 91)
    cv = _random_covers(sn, 92)
    x = ta.synth_data(150, F, seed=93, missing_prob=0.05, missing=MISSING, nan_prob=0.02)
    bg = ta.synth_data(20, F, seed=94)
    f = ta.capi.SparseForest(sn, tr, F, missing=MISSING, covers=cv, contribs=True)
    batch = run_all(env, f, x, bg)
    again = run_all(env, f, x, bg)
    for a, b in zip(batch, again):
        assert np.array_equal(bits(a), bits(b))
    for r in (0, 77, 149):
        one = run_all(env, f, x[r:r + 1], bg)
        for name, a, b in zip(("contribs", "interactions", "interventional"), one, batch):
            assert np.array_equal(bits(a[0]), bits(b[r])), (name, r)
    f.close()


def test_refusal_without_the_flag_names_sparse(env):
    ta, torch = env
    F = 8
    sn, tr = ta.capi.synth_sparse_forest(6, F, 4, 12, 0.4, 300, 95)
    f = ta.capi.SparseForest(sn, tr, F, num_classes=3)
    x = torch.zeros((4, F), device="cuda")
    out = torch.zeros((4, 3, F + 1), device="cuda")
    assert ta.lib.tahoe_forest_predict_contribs(f._h, out.data_ptr(), x.data_ptr(), 4, None) == 7
    assert "sparse" in ta.lib.tahoe_last_error().decode()
    assert ta.lib.tahoe_forest_set_background(f._h, x.data_ptr(), 4, None) == 7
    assert "sparse" in ta.lib.tahoe_last_error().decode()
    torch.cuda.synchronize()
    assert torch.count_nonzero(out).item() == 0
    f.close()
