"""Saabas contributions (tahoe_forest_predict_contribs_approx) on the GPU against the numpy restatement of
tests/approx_contribs_ref.py, bit for bit.  Needs an MI355X.

Bitwise against the reference: random small forests (missing values, NaN, +-inf, rows on thresholds, shallow leaves, root-leaf
trees), histogram forests, widths 3 / 256 / 3072 / 10000, multi-class with AVG and global_bias, sparse handles (irregular forests,
a 40-level vine on 40 features).  Bitwise properties: repeat calls, a row alone / a prefix / a permutation of a batch, every
strategy, re-layout, class c against its sub-forest, dense -> sparse conversion, CONTRIBS|APPROX handles.  Additivity against
predict_raw within (2 N + T + 8) 2^-24 (S + |bias| + sum |leaf|), N the adds and S the sum of |delta| of the row (float32: a rounded
delta and a rounded add per step, the margin's own sum, the bias rounding)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_contribs_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
U = 2.0 ** -24
LEAF = -(1 << 31)


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
    out = forest.predict_contribs_approx(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    torch.cuda.synchronize()
    phi = out.cpu().numpy()
    return phi if phi.ndim == 3 else phi[:, None, :]


def assert_bits(got, want, label):
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        r, c, i = bad[0]
        raise AssertionError(f"{label}: {len(bad)} outputs differ, first at row {r} class {c} col {i}: {got[r, c, i]!r} vs "
                             f"{want[r, c, i]!r}")


def random_forest(ta, rng, T, D, cols, nan_thr=0.05):
    """synth_forest with random covers, early leaves, a root-leaf tree (tree 0) and some NaN / infinite thresholds."""
    nodes = ta.synth_forest(T, D, cols, seed=int(rng.integers(1 << 30)), leaf_prob=0.2)
    nodes["weight"] = rng.uniform(0.05, 1.0, nodes.size).astype(np.float32)
    internal = (nodes["bits"].view(np.uint32) >> 31) == 0
    nodes["val"][internal & (rng.random(nodes.size) < nan_thr)] = np.nan
    nodes["val"][internal & (rng.random(nodes.size) < nan_thr)] = np.inf
    nodes["val"][internal & (rng.random(nodes.size) < nan_thr)] = -np.inf
    nodes["bits"][0] = nodes["bits"][0] | np.int32(LEAF)
    return nodes


def random_rows(ta, rng, nodes, rows, cols):
    """synth_data with the missing sentinel and NaN, then +-inf and values equal to thresholds the forest uses (ties)."""
    x = ta.synth_data(rows, cols, seed=int(rng.integers(1 << 30)), missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    x[rng.random(x.shape) < 0.03] = np.inf
    x[rng.random(x.shape) < 0.03] = -np.inf
    thr = nodes["val"][np.isfinite(nodes["val"])]
    if thr.size:
        tie = rng.random(x.shape) < 0.1
        x[tie] = rng.choice(thr, int(tie.sum()))
    return x


def check_dense(env, nodes, T, D, F, x, num_classes=1, output=0, bias=0.0, label="", relayout=False):
    ta, torch = env
    avg = (output & ta.OUT_AVG) != 0
    f = ta.Forest(nodes, T, D, F, missing=MISSING, output=output, global_bias=bias, num_classes=num_classes,
                  approx_contribs=True, relayout=relayout)
    got = gpu_phi(env, f, x)
    want, S, N = ref.dense(nodes, T, D, F, x, MISSING, num_classes=num_classes, avg=avg, global_bias=bias, scale=True)
    assert_bits(got, want, label)
    check_additivity(env, f, x, got, S, N, T // num_classes, nodes["val"], label)
    return f, got


def check_additivity(env, f, x, got, S, N, Tc, vals, label):
    ta, torch = env
    margin = f.predict_raw(torch.from_numpy(np.ascontiguousarray(x)).cuda()).cpu().numpy().astype(np.float64)
    margin = margin.reshape(got.shape[0], got.shape[1])
    div = Tc if (f.params.output & ta.OUT_AVG) else 1
    margin = margin / div + f.params.global_bias
    leaf_abs = Tc * float(np.nanmax(np.abs(vals[np.isfinite(vals)]), initial=0.0)) / div
    s = got.astype(np.float64).sum(axis=-1)
    tol = (2 * N + Tc + 8) * U * (S / div + np.abs(got[:, :, -1]) + leaf_abs) + 1e-30
    assert np.all(np.abs(s - margin) <= tol), f"{label}: additivity, worst {np.max(np.abs(s - margin) / tol):.3g} of the bound"


@pytest.mark.parametrize("seed", range(6))
def test_random_small_forests(env, seed):
    ta, _ = env
    rng = np.random.default_rng(300 + seed)
    T, D, F = int(rng.integers(2, 25)), int(rng.integers(0, 8)), int(rng.integers(1, 9))
    nodes = random_forest(ta, rng, T, D, F)
    x = random_rows(ta, rng, nodes, int(rng.integers(1, 300)), F)
    for output, bias in ((0, 0.0), (ta.OUT_AVG | ta.OUT_SIGMOID, 0.25)):
        check_dense(env, nodes, T, D, F, x, output=output, bias=bias, label=f"seed {seed} T={T} D={D} F={F} out={output}")


def test_hist_forest_100x8_on_32(env):
    ta, _ = env
    nodes = ta.synth_forest_hist(100, 8, 32, seed=5, feature_seed=6)
    x = ta.synth_data_hist(700, 32, seed=7, feature_seed=6, missing_prob=0.02, missing=MISSING)
    check_dense(env, nodes, 100, 8, 32, x, label="hist 100x8 F=32")


@pytest.mark.parametrize("F", [3, 256, 3072, 10000])
def test_widths(env, F):
    ta, _ = env
    rng = np.random.default_rng(F)
    T, D = 20, 9
    nodes = ta.synth_forest(T, D, F, seed=F, leaf_prob=0.05)
    nodes["weight"] = rng.uniform(0.05, 1.0, nodes.size).astype(np.float32)
    x = ta.synth_data(130, F, seed=F + 1, missing_prob=0.02, missing=MISSING, nan_prob=0.01)
    check_dense(env, nodes, T, D, F, x, label=f"F={F}")


@pytest.mark.parametrize("C", [3, 10])
def test_multiclass_and_sub_forests(env, C):
    ta, _ = env
    T, D, F = 6 * C, 7, 16
    nodes = ta.synth_forest_hist(T, D, F, seed=C, feature_seed=C + 1)
    x = ta.synth_data_hist(200, F, seed=C + 2, feature_seed=C + 1, missing_prob=0.03, missing=MISSING)
    out = ta.OUT_AVG | ta.OUT_SOFTMAX
    f, got = check_dense(env, nodes, T, D, F, x, num_classes=C, output=out, bias=0.375, label=f"C={C}")
    per = nodes.size // T
    for c in range(C):
        sub = np.ascontiguousarray(nodes.reshape(T, per)[c::C]).reshape(-1)
        g = ta.Forest(sub, T // C, D, F, missing=MISSING, output=ta.OUT_AVG, global_bias=0.375, approx_contribs=True)
        assert_bits(gpu_phi(env, g, x), got[:, c:c + 1, :], f"class {c}")
        g.close()


@pytest.fixture(scope="module")
def k_forest(env):
    ta, torch = env
    T, D, F = 60, 10, 40
    nodes = ta.synth_forest_hist(T, D, F, seed=21, feature_seed=22)
    x = ta.synth_data_hist(1000, F, seed=23, feature_seed=22, missing_prob=0.03, missing=MISSING)
    f = ta.Forest(nodes, T, D, F, missing=MISSING, approx_contribs=True)
    got = gpu_phi(env, f, x)
    assert_bits(got, ref.dense(nodes, T, D, F, x, MISSING), "k_forest")
    return nodes, T, D, F, x, f, got


def test_repeat_calls_are_bitwise_identical(env, k_forest):
    nodes, T, D, F, x, f, want = k_forest
    for _ in range(3):
        assert_bits(gpu_phi(env, f, x), want, "repeat")


def test_rows_do_not_depend_on_the_batch(env, k_forest):
    nodes, T, D, F, x, f, want = k_forest
    assert_bits(gpu_phi(env, f, x[17:18]), want[17:18], "row alone")
    assert_bits(gpu_phi(env, f, x[:77]), want[:77], "prefix")
    perm = np.random.default_rng(3).permutation(x.shape[0])
    assert_bits(gpu_phi(env, f, x[perm]), want[perm], "permutation")


def test_strategy_has_no_effect(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, f, want = k_forest
    g = ta.Forest(nodes, T, D, F, missing=MISSING, approx_contribs=True)
    for s in range(6):
        g.set_strategy(s)
        assert_bits(gpu_phi(env, g, x), want, f"strategy {s}")
    g.close()


def test_relayout_gives_the_same_bits(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, f, want = k_forest
    g = ta.Forest(nodes, T, D, F, missing=MISSING, approx_contribs=True, relayout=True)
    assert g.info().relayout == 1 and g.info().relayout_swaps > 0
    assert_bits(gpu_phi(env, g, x), want, "relayout")
    g.close()
    # multi-class and re-layout together
    C = 4
    m = ta.Forest(nodes, T, D, F, missing=MISSING, num_classes=C, approx_contribs=True, relayout=True, output=ta.OUT_AVG)
    assert_bits(gpu_phi(env, m, x), ref.dense(nodes, T, D, F, x, MISSING, num_classes=C, avg=True), "relayout C=4")
    m.close()


def test_with_the_exact_flag(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, f, want = k_forest
    both = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True, approx_contribs=True)
    exact = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True)
    a = gpu_phi(env, both, x)
    assert_bits(a, want, "CONTRIBS|APPROX approx")
    e1 = both.predict_contribs(env[1].from_numpy(x).cuda()).cpu().numpy()
    e2 = exact.predict_contribs(env[1].from_numpy(x).cuda()).cpu().numpy()
    assert np.array_equal(bits(e1), bits(e2))
    assert np.array_equal(bits(e1[:, -1]), bits(a[:, 0, -1]))  # the two bias columns
    both.close()
    exact.close()


def test_additivity_against_predict_raw(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, f, got = k_forest
    _, S, N = ref.dense(nodes, T, D, F, x, MISSING, scale=True)
    check_additivity(env, f, x, got, S, N, T, nodes["val"], "k_forest")


def test_refusals_and_zero_rows(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, f, want = k_forest
    plain = ta.Forest(nodes, T, D, F, missing=MISSING, contribs=True)
    out = torch.zeros((4, F + 1), device="cuda")
    xd = torch.from_numpy(x[:4]).cuda()
    st = ta.lib.tahoe_forest_predict_contribs_approx(plain._h, out.data_ptr(), xd.data_ptr(), 4, None)
    assert st == 7 and "TAHOE_CREATE_APPROX_CONTRIBS" in ta.lib.tahoe_last_error().decode()
    assert ta.lib.tahoe_forest_predict_contribs_approx(plain._h, None, None, 0, None) == 7  # the flag before rows == 0
    assert ta.lib.tahoe_forest_predict_contribs_approx(f._h, None, None, 0, None) == 0
    assert ta.lib.tahoe_forest_predict_contribs_approx(f._h, None, xd.data_ptr(), 4, None) == 1
    assert ta.lib.tahoe_forest_predict_contribs_approx(f._h, out.data_ptr(), None, 4, None) == 1
    assert ta.lib.tahoe_forest_predict_contribs_approx(f._h, out.data_ptr(), xd.data_ptr(), (1 << 64) // 8, None) == 1
    torch.cuda.synchronize()
    assert not out.any().item()  # nothing launched
    assert tuple(f.predict_contribs_approx(torch.empty((0, F), device="cuda")).shape) == (0, F + 1)
    sn, tr, cv = ta.capi.dense_to_sparse(nodes, T, D, covers=True)
    sp = ta.capi.SparseForest(sn, tr, F, missing=MISSING, covers=cv, contribs=True)
    assert ta.lib.tahoe_forest_predict_contribs_approx(sp._h, out.data_ptr(), xd.data_ptr(), 4, None) == 7
    sp.close()
    plain.close()


def test_graph_capture(env, k_forest):
    ta, torch = env
    nodes, T, D, F, x, f, want = k_forest
    xd = torch.from_numpy(x).cuda()
    out = torch.empty((x.shape[0], F + 1), device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        f.predict_contribs_approx(xd, out=out, stream=s)
    out.zero_()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want[:, 0, :]))


def test_tables_count_in_device_bytes(env, k_forest):
    ta, _ = env
    nodes, T, D, F, x, f, want = k_forest
    plain = ta.Forest(nodes, T, D, F, missing=MISSING)
    assert f.info().device_bytes >= plain.info().device_bytes + T * ((1 << D) - 1) * 16
    plain.close()
    sn, tr, cv = ta.capi.dense_to_sparse(nodes, T, D, covers=True)
    a = ta.capi.SparseForest(sn, tr, F, missing=MISSING, covers=cv)
    b = ta.capi.SparseForest(sn, tr, F, missing=MISSING, covers=cv, approx_contribs=True)
    assert b.info().device_bytes >= a.info().device_bytes + sn.size * 8
    a.close()
    b.close()


# ---- sparse handles ----
@pytest.mark.parametrize("C", [1, 3])
def test_dense_and_converted_sparse_give_the_same_bits(env, C):
    ta, _ = env
    rng = np.random.default_rng(70 + C)
    T, D, F = 12 * C, 8, 20
    nodes = random_forest(ta, rng, T, D, F)
    x = random_rows(ta, rng, nodes, 500, F)
    out = ta.OUT_AVG if C > 1 else 0
    f, want = check_dense(env, nodes, T, D, F, x, num_classes=C, output=out, bias=-0.5, label=f"dense C={C}")
    sn, tr, cv = ta.capi.dense_to_sparse(nodes, T, D, covers=True)
    sp = ta.capi.SparseForest(sn, tr, F, missing=MISSING, covers=cv, num_classes=C, output=out, global_bias=-0.5,
                              approx_contribs=True)
    for s in (0, 1, 2, 3, 5):  # the strategies a sparse handle serves
        sp.set_strategy(s)
        assert_bits(gpu_phi(env, sp, x), want, f"sparse C={C} strategy {s}")
    sp.close()
    f.close()


@pytest.mark.parametrize("seed", range(3))
def test_irregular_sparse_forests(env, seed):
    ta, _ = env
    F = 24
    sn, tr = ta.capi.synth_sparse_forest(30, F, 4, 24, 0.3, 2000, 600 + seed)
    cv = np.random.default_rng(seed).uniform(0.05, 1.0, sn.size).astype(np.float32)
    x = ta.synth_data(400, F, seed=seed, missing_prob=0.05, missing=MISSING, nan_prob=0.02)
    for C, out, bias in ((1, 0, 0.0), (3, ta.OUT_AVG, 0.125)):
        f = ta.capi.SparseForest(sn, tr, F, missing=MISSING, covers=cv, num_classes=C, output=out, global_bias=bias,
                                 approx_contribs=True)
        want = ref.sparse(sn, tr, cv, F, x, MISSING, num_classes=C, avg=bool(out), global_bias=bias)
        assert_bits(gpu_phi(env, f, x), want, f"irregular seed {seed} C={C}")
        f.close()


def test_deep_vine_on_40_features(env):
    ta, _ = env
    rng = np.random.default_rng(9)
    depth, F, T = 40, 40, 3
    parts, roots, off = [], [], 0
    for t in range(T):
        sn = np.zeros(2 * depth + 1, dtype=ta.capi.SPARSE_NODE_DTYPE)
        nxt = 0
        for k in range(depth):
            i = nxt
            leaf_right = bool(rng.integers(2))
            thr = 0.9 if leaf_right else -0.9  # small values take the long branch: left of +0.9, right of -0.9
            sn[i] = (np.float32(thr + rng.uniform(-0.05, 0.05)), ((k + t) % F) | (int(rng.integers(2)) << 30), 2 * k + 1)
            sn[2 * k + 1 + int(leaf_right)] = (np.float32(rng.uniform(-1, 1)), np.int32(LEAF), 0)
            nxt = 2 * k + 1 + (0 if leaf_right else 1)
        sn[nxt] = (np.float32(rng.uniform(-1, 1)), np.int32(LEAF), 0)
        parts.append(sn)
        roots.append(off)
        off += sn.size
    sn, tr = np.concatenate(parts), np.array(roots, np.int32)
    cv = rng.uniform(0.05, 1.0, sn.size).astype(np.float32)
    x = ta.synth_data(300, F, seed=5, missing_prob=0.05, missing=MISSING, nan_prob=0.02)
    x[np.isfinite(x) & (x != MISSING)] *= np.float32(0.5)  # most rows stay on the long branch for many levels
    f = ta.capi.SparseForest(sn, tr, F, missing=MISSING, covers=cv, approx_contribs=True)
    want, S, N = ref.sparse(sn, tr, cv, F, x, MISSING, scale=True)
    assert N.max() > 31  # paths longer than the exact flag allows
    got = gpu_phi(env, f, x)
    assert_bits(got, want, "vine")
    check_additivity(env, f, x, got, S, N, T, sn["val"], "vine")
    f.close()


# ---- one full forest ----
def test_k3_full_batch(env):
    """K3 (1000 trees x depth 12 on 256 features), 1 M rows: every output finite and additive against predict_raw; a 20 k-row
    slice bit-exact against the reference."""
    ta, torch = env
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench

    _, (nodes, T, D, F), data = bench.baseline_workload(ta, "K3")
    nodes = ta.capi.set_probability_weights(nodes, T, D)
    try:
        f = ta.Forest(nodes, T, D, F, missing=bench.MISSING, approx_contribs=True)
    except ta.TahoeError:  # a reachable node no row of the generator reaches: both children weigh 0
        nodes = nodes.copy()
        nodes["weight"] += np.float32(1e-6)
        f = ta.Forest(nodes, T, D, F, missing=bench.MISSING, approx_contribs=True)
    xd = torch.from_numpy(data).cuda()
    phi = f.predict_contribs_approx(xd)
    raw = f.predict_raw(xd)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(phi).all().item())
    s = phi.double().sum(dim=1)
    # rigorous: at most T x D adds per row, each |delta| <= 2 max |leaf|, so every partial sum is below S = 2 T D max |leaf|
    maxleaf = float(np.max(np.abs(nodes["val"][(nodes["bits"].view(np.uint32) >> 31) == 1])))
    tol = (2 * T * D + T + 8) * U * (2 * T * D * maxleaf + phi[:, F].double().abs())
    err = (s - raw.double()).abs()
    assert bool((err <= tol).all().item()), float((err / tol).max().item())
    del s, err
    lo = 123_457
    sl = np.ascontiguousarray(data[lo:lo + 20_000])
    want = ref.dense(nodes, T, D, F, sl, bench.MISSING)
    assert_bits(phi[lo:lo + 20_000].cpu().numpy()[:, None, :], want, "K3 slice")
    f.close()
