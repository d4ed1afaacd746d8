"""The four explanation calls on sparse handles with categorical splits (TAHOE_CREATE_CAT_CONTRIBS) on the GPU.  Needs an MI355X.

Bitwise: a forest of integer thresholds and its two categorical restatements (tests/cat_shap_cases.twin) hold the same path bins
and the same node deltas, so contributions, interactions, interventional values and Saabas contributions agree bit for bit; a row
alone against the batch, class c against class c's sub-forest, a background set twice.
Accuracy: random sets of 0 / 1 / 2 / 5 words mixed with numeric nodes against the float64 brute force of tests/cat_shap_ref.py,
within the bars of tests/test_sparse_shap_gpu.py -- gamma x (sum over paths of |leaf| x path length), gamma = (paths + 4 (depth +
2)) 2^-24, twice that for interactions: they depend on the trees' structure and leaves only, so they carry over.  Saabas against
its float32 restatement, bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cat_shap_cases as cases  # noqa: E402
import cat_shap_ref as cref  # noqa: E402
import sparse_shap_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = cases.MISSING
U = 2.0 ** -24
LEAF = np.int32(-(1 << 31))


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
    """(contribs, interactions, interventional, saabas, margins) as numpy, each with a class axis."""
    ta, torch = env
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    phi = f.predict_contribs(xd).cpu().numpy()
    inter = f.predict_interactions(xd).cpu().numpy()
    f.set_background(torch.from_numpy(np.ascontiguousarray(bg)).cuda())
    iv = f.predict_contribs_interventional(xd).cpu().numpy()
    sa = f.predict_contribs_approx(xd).cpu().numpy()
    raw = f.predict_raw(xd).cpu().numpy().reshape(x.shape[0], -1)
    f.check()
    if f.num_classes == 1:
        phi, inter, iv, sa = phi[:, None], inter[:, None], iv[:, None], sa[:, None]
    return phi, inter, iv, sa, raw


NAMES = ("contribs", "interactions", "interventional", "saabas", "margins")


def make(ta, sn, tr, F, covers, cats=None, left=(), nc=1, out=0, bias=0.0):
    return ta.capi.SparseForest(sn, tr, F, missing=MISSING, output=out, global_bias=bias, covers=covers, num_classes=nc,
                                contribs=True, approx_contribs=True, categories=cats, members_left=left)


def strategies(ta, f):
    ok = []
    for s in (ta.STRATEGY_AUTO, ta.STRATEGY_DIRECT, ta.STRATEGY_ROWTILE, ta.STRATEGY_TILEBLOCK, ta.STRATEGY_QRING):
        try:
            f.set_strategy(s)
            ok.append(s)
        except ta.TahoeError:
            pass
    return ok


# ---- 1. threshold twins ----

@pytest.fixture(scope="module")
def twin(env):
    ta, _ = env
    F = 6
    sn, tr, ge, lt = cases.twin(ta, 12, F, 11)
    cv = np.random.default_rng(12).uniform(0.05, 1.0, sn.size).astype(np.float32)
    return F, sn, tr, ge, lt, cv


@pytest.mark.parametrize("nc", [1, 3])
def test_threshold_twins_bit_for_bit(env, twin, nc):
    ta, _ = env
    F, sn, tr, ge, lt, cv = twin
    out, bias = (ta.OUT_AVG, 0.25) if nc == 3 else (0, 0.0)
    x, bg = cases.twin_rows(70, F, 13), cases.twin_rows(9, F, 14)
    a = make(ta, sn, tr, F, cv, nc=nc, out=out, bias=bias)
    b = make(ta, sn, tr, F, cv, ge, nc=nc, out=out, bias=bias)
    bare = ta.capi.SparseForest(sn, tr, F, missing=MISSING, output=out, global_bias=bias, num_classes=nc, categories=ge)
    assert b.info().device_bytes > bare.info().device_bytes  # the path tables and the element sets are counted
    bare.close()
    want = run_all(env, a, x, bg)
    sb = strategies(ta, b)
    assert ta.STRATEGY_QRING not in sb and len(sb) == 4
    for s in sb:
        b.set_strategy(s)
        for name, got, w in zip(NAMES, run_all(env, b, x, bg), want):
            assert np.array_equal(bits(got), bits(w)), (name, s)
    # members to the left, sets {c < k}: the rules agree on non-negative integers only
    x, bg = cases.twin_rows(70, F, 15, odd=False), cases.twin_rows(9, F, 16, odd=False)
    c = make(ta, sn, tr, F, cv, lt, left=set(lt), nc=nc, out=out, bias=bias)
    want = run_all(env, a, x, bg)
    for s in strategies(ta, c):
        c.set_strategy(s)
        for name, got, w in zip(NAMES, run_all(env, c, x, bg), want):
            assert np.array_equal(bits(got), bits(w)), (name, s, "members left")
    for f in (a, b, c):
        f.close()


# ---- 2. brute force, 3. Saabas ----

@pytest.mark.parametrize("F,seed", [(5, 3), (8, 5)])
def test_mixed_forest_against_brute_force(env, F, seed):
    """Measured on an MI355X (max error / bar): see the figures the test prints."""
    ta, torch = env
    forest, cv = cases.mixed(ta, F, seed)
    sn, tr = forest.sn, forest.tr
    x, bg = cases.mixed_rows(9, F, seed + 1), cases.mixed_rows(6, F, seed + 2)
    bias = 0.125
    f = make(ta, sn, tr, F, cv, forest.cats, forest.left, bias=bias)
    phi, inter, iv, sa, raw = run_all(env, f, x, bg)
    scale, depth, paths = ref.bound_scale(sn, tr, 1)
    tol = (paths + 4 * (depth + 2)) * U * scale  # [1]
    want = cref.contribs(forest, cv, x, F, MISSING, 1, False, bias)
    err = np.abs(phi[:, :, :F].astype(np.float64) - want[:, :, :F])
    print(f"F {F}: contribs max err {err.max():.3e}, bar {tol.max():.3e}")
    assert np.all(err <= tol[None, :, None])
    assert np.array_equal(bits(phi[:, :, F]), bits(np.broadcast_to(ref.bias_column(sn, tr, cv, 1, False, bias), phi[:, :, F].shape)))
    # additivity against a categorical handle's own margins
    m = ta.capi.SparseForest(sn, tr, F, missing=MISSING, global_bias=bias, categories=forest.cats, members_left=forest.left)
    margin = m.predict(torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64).reshape(x.shape[0], 1)
    assert np.array_equal(bits(raw), bits(m.predict_raw(torch.from_numpy(x).cuda()).cpu().numpy().reshape(raw.shape)))
    assert np.all(np.abs(phi.astype(np.float64).sum(-1) - margin) <= 2 * tol[None, :] + 1e-5 * np.abs(margin) + 1e-6)
    # interactions: off the diagonal against the index, exactly symmetric, +0.0f in the bias row and column
    want_i = cref.interactions(forest, cv, x, F, MISSING)
    off = ~np.eye(F, dtype=bool)
    err = np.abs(inter[:, :, :F, :F].astype(np.float64) - want_i)[:, :, off]
    print(f"F {F}: interactions max err {err.max():.3e}, bar {2 * tol.max():.3e}")
    assert np.all(err <= 2 * tol[None, :, None])
    assert np.array_equal(bits(inter), bits(inter.transpose(0, 1, 3, 2)))
    assert np.array_equal(bits(inter[:, :, F, :F]), bits(np.zeros_like(inter[:, :, F, :F])))
    assert np.array_equal(bits(inter[:, :, F, F]), bits(phi[:, :, F]))
    # interventional; its bias from the library's own background sums
    bg_raw = m.predict_raw(torch.from_numpy(bg).cuda()).cpu().numpy().reshape(bg.shape[0], 1)
    want_v = cref.interventional(forest, x, bg, F, MISSING, 1, False, bias, bg_raw=bg_raw)
    err = np.abs(iv[:, :, :F].astype(np.float64) - want_v[:, :, :F])
    print(f"F {F}: interventional max err {err.max():.3e}, bar {tol.max():.3e}")
    assert np.all(err <= tol[None, :, None])
    assert np.array_equal(bits(iv[:, :, F]), bits(want_v[:, :, F].astype(np.float32)))
    # Saabas: the float32 restatement, bit for bit
    assert np.array_equal(bits(sa), bits(cref.saabas(forest, cv, F, x, MISSING, 1, False, bias)))
    m.close()
    f.close()


def test_saabas_alone_with_classes(env):
    """TAHOE_CREATE_APPROX_CONTRIBS | TAHOE_CREATE_CAT_CONTRIBS without the path tables, three classes with AVG."""
    ta, torch = env
    F = 5
    forest, cv = cases.mixed(ta, F, 7)  # 6 trees: 2 per class
    x = cases.mixed_rows(70, F, 8)
    f = ta.capi.SparseForest(forest.sn, forest.tr, F, missing=MISSING, output=ta.OUT_AVG, global_bias=-0.5, covers=cv, num_classes=3,
                             approx_contribs=True, categories=forest.cats, members_left=forest.left)
    got = f.predict_contribs_approx(torch.from_numpy(x).cuda()).cpu().numpy()
    f.check()
    assert np.array_equal(bits(got), bits(cref.saabas(forest, cv, F, x, MISSING, 3, True, -0.5)))
    f.close()


# ---- 4. reproducibility ----

def test_rows_classes_and_backgrounds_reproduce(env):
    ta, torch = env
    F, nc = 5, 3
    forest, cv = cases.mixed(ta, F, 21)
    x, bg = cases.mixed_rows(70, F, 22), cases.mixed_rows(9, F, 23)
    f = make(ta, forest.sn, forest.tr, F, cv, forest.cats, forest.left, nc=nc, out=ta.OUT_AVG, bias=0.5)
    batch = run_all(env, f, x, bg)
    again = run_all(env, f, x, bg)  # a second call, the same background set again
    for name, a, b in zip(NAMES, batch, again):
        assert np.array_equal(bits(a), bits(b)), name
    for r in (0, 33, 69):
        for name, a, b in zip(NAMES, run_all(env, f, x[r:r + 1], bg), batch):
            assert np.array_equal(bits(a[0]), bits(b[r])), (name, r)
    for c in range(nc):
        sub, sub_cv = forest.sub(c, nc, cv)
        g = make(ta, sub.sn, sub.tr, F, sub_cv, sub.cats, sub.left, out=ta.OUT_AVG, bias=0.5)
        for name, a, b in zip(NAMES, run_all(env, g, x, bg), batch):
            assert np.array_equal(bits(a[:, 0]), bits(b[:, c])), (name, c)
        g.close()
    f.close()


# ---- 5. pool edges ----

def _stump(ta, ids):
    """f0 in ids ? right : left, then a numeric node on f1 on the right."""
    sn = np.zeros(5, dtype=ta.capi.SPARSE_NODE_DTYPE)
    sn[0] = (0.0, 0, 1)
    sn[1] = (-1.0, LEAF, 0)
    sn[2] = (0.5, 1 | 1 << 30, 3)
    sn[3] = (0.25, LEAF, 0)
    sn[4] = (2.0, LEAF, 0)
    return cref.CatForest(sn, np.zeros(1, np.int32), {0: ids}), np.array([1.0, 0.3, 0.7, 0.2, 0.5], np.float32)


@pytest.mark.parametrize("ids", [[3, 63], []], ids=["last_set_ends_the_pool", "no_words"])
def test_pool_edges(env, ids):
    ta, torch = env
    forest, cv = _stump(ta, ids)
    F = 2
    x = np.array([[63, 1], [3, 0], [62, 1], [64, 1], [31, MISSING], [MISSING, 1], [np.nan, 0], [-1, 1], [2.0 ** 24, 1], [95, 0]],
                 np.float32)
    bg = x[::-1][:4].copy()
    f = make(ta, forest.sn, forest.tr, F, cv, forest.cats)
    phi, inter, iv, sa, raw = run_all(env, f, x, bg)
    scale, depth, paths = ref.bound_scale(forest.sn, forest.tr, 1)
    tol = (paths + 4 * (depth + 2)) * U * scale
    want = cref.contribs(forest, cv, x, F, MISSING)
    assert np.all(np.abs(phi[:, :, :F] - want[:, :, :F]) <= tol[None, :, None])
    want_v = cref.interventional(forest, x, bg, F, MISSING, bg_raw=raw[::-1][:4])
    assert np.all(np.abs(iv[:, :, :F] - want_v[:, :, :F]) <= tol[None, :, None])
    assert np.all(np.abs(inter[:, :, 0, 1] - cref.interactions(forest, cv, x, F, MISSING)[:, :, 0, 1]) <= 2 * tol[None, :])
    assert np.array_equal(bits(sa), bits(cref.saabas(forest, cv, F, x, MISSING)))
    f.close()


def test_the_flag_without_splits_is_create_ex(env):
    ta, torch = env
    F = 6
    sn, tr, _, _ = cases.twin(ta, 12, F, 31)
    cv = np.random.default_rng(32).uniform(0.05, 1.0, sn.size).astype(np.float32)
    x, bg = cases.twin_rows(70, F, 33), cases.twin_rows(9, F, 34)
    plain = make(ta, sn, tr, F, cv)
    plain_bytes = plain.info().device_bytes  # before run_all sets a background, which counts as well
    want = run_all(env, plain, x, bg)
    # tahoe_sparse_forest_create_cat with the flag and an empty split list (the Python class never sends that)
    flagged = ta.capi.SparseForest.__new__(ta.capi.SparseForest)
    flagged.params = ta.ForestParams(int(sn.size), 0, int(tr.size), F, 0, 0, 0.0, 0.0, 0, MISSING)
    flagged._h = C.c_void_p()
    cats, _keep = ta.capi.pack_categorical({})
    flags = ta.CREATE_CONTRIBS | ta.CREATE_APPROX_CONTRIBS | ta.CREATE_CAT_CONTRIBS
    assert ta.lib.tahoe_sparse_forest_create_cat(C.byref(flagged._h), tr.ctypes.data, sn.ctypes.data, cv.ctypes.data,
                                                 C.byref(flagged.params), 1, flags, C.byref(cats)) == 0
    flagged.num_trees, flagged.depth, flagged.num_cols, flagged.num_classes = int(tr.size), 0, F, 1
    assert flagged.info().device_bytes == plain_bytes
    assert len(strategies(ta, flagged)) == 5  # QRING included: no splits
    flagged.set_strategy(ta.STRATEGY_AUTO)
    for name, a, b in zip(NAMES, run_all(env, flagged, x, bg), want):
        assert np.array_equal(bits(a), bits(b)), name
    flagged.close()
    plain.close()
