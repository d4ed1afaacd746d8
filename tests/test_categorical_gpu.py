"""Categorical splits on sparse handles (tahoe_sparse_forest_create_cat) on the GPU: sums and leaf indices bit for bit
tests/categorical_ref.py under AUTO, DIRECT, ROWTILE and TILEBLOCK; QRING refused; classes with SOFTMAX; predict_accumulate and
predict_host; an equivalence with the plain sparse handle that does not rest on the reference; num_splits == 0 gives _ex's bits.
Needs an MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref  # noqa: E402
import test_categorical_capi as capi_t  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
FLOAT_FORMS = ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK")


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def strategy(ta, name):
    return getattr(ta, "STRATEGY_" + name)


def cat_forest(ta, T, cols, cat_feats, seed, min_depth=4, max_depth=16, max_cats=1000, universe=1100):
    """synth_sparse_forest with every inner node on a feature of cat_feats made categorical: a random set of 1..max_cats
    categories out of [0, universe); members_left drawn for a third of them."""
    sn, tr = ta.capi.synth_sparse_forest(T, cols, min_depth, max_depth, 0.32, 65535, seed)
    rng = np.random.default_rng(seed)
    b = sn["bits"].view(np.uint32)
    inner = np.flatnonzero((b >> 31) == 0)
    fid = b[inner] & ((1 << 30) - 1)
    chosen = inner[np.isin(fid, cat_feats)]
    cats = {int(i): rng.choice(universe, size=int(rng.integers(1, max_cats + 1)), replace=False) for i in chosen}
    ml = {int(i) for i in chosen if rng.random() < 1 / 3}
    return sn, tr, cats, ml


def cat_data(ta, rows, cols, cat_feats, seed, universe=1100):
    """synth_data with the categorical columns replaced by a mix of valid categories, non-integers, negatives (-0.0 too),
    NaN, the sentinel and values past every bitset."""
    data = ta.synth_data(rows, cols, seed=seed, missing_prob=0.03, missing=MISSING, nan_prob=0.02)
    rng = np.random.default_rng(seed)
    for f in cat_feats:
        u = rng.random(rows)
        v = rng.integers(0, universe, rows).astype(np.float32)
        v = np.where(u < 0.15, v + np.float32(0.5), v)
        v = np.where((u >= 0.60) & (u < 0.68), rng.choice(np.array([-0.0, -0.5, -1.0, -3.0, -1e9], np.float32), rows), v)
        v = np.where((u >= 0.68) & (u < 0.74), np.float32(np.nan), v)
        v = np.where((u >= 0.74) & (u < 0.80), np.float32(MISSING), v)
        v = np.where((u >= 0.80) & (u < 0.88), rng.choice(np.array([1100.0, 4096.0, 1e7, 3e7, np.inf], np.float32), rows), v)
        data[:, f] = v
    return np.ascontiguousarray(data, dtype=np.float32)


def ref(ta, sn, tr, data, cats, ml, **kw):
    _, (node, offset, words, mla) = ta.capi.pack_categorical(cats, ml)
    return categorical_ref.predict(sn, tr, data, MISSING, node, offset, words, mla, **kw)


def test_every_float_strategy_matches_the_reference(env):
    ta, torch = env
    cols, feats = 32, [1, 5, 9, 17, 30]
    sn, tr, cats, ml = cat_forest(ta, 60, cols, feats, seed=11)
    assert len(cats) > 500 and 0 < len(ml) < len(cats)
    rows = 3001
    data = cat_data(ta, rows, cols, feats, seed=12)
    want, want_leaf = ref(ta, sn, tr, data, cats, ml)
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, categories=cats, members_left=ml)
    assert f.get_strategy(rows) == ta.STRATEGY_TILEBLOCK and f.kernel_form(rows) == "sparse_top"
    x = torch.from_numpy(data).cuda()
    for name in FLOAT_FORMS:
        f.set_strategy(strategy(ta, name))
        raw = f.predict_raw(x)
        leaf, sums = f.predict_leaf_idx(x)
        leaf2, none = f.predict_leaf_idx(x, want_sums=False)
        f.check()
        assert np.array_equal(bits(raw.cpu().numpy()), bits(want)), name
        assert np.array_equal(bits(sums.cpu().numpy()), bits(want)), name
        assert np.array_equal(leaf.cpu().numpy().view(np.uint32), want_leaf), name
        assert none is None and np.array_equal(leaf2.cpu().numpy().view(np.uint32), want_leaf), name
    f.close()


def test_qring_is_refused_and_auto_falls_back(env):
    ta, torch = env
    cols, feats = 16, [0, 3]
    sn, tr, cats, ml = cat_forest(ta, 400, cols, feats, seed=21)
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, categories=cats, members_left=ml)
    plain = ta.capi.SparseForest(sn, tr, cols, missing=MISSING)
    assert plain.get_strategy(200_000) == ta.STRATEGY_QRING  # the same shape without splits would take QRING
    with pytest.raises(ta.TahoeError) as e:
        f.set_strategy(ta.STRATEGY_QRING)
    assert e.value.status == 7 and "categorical" in str(e.value)
    assert ta.lib.tahoe_forest_get_strategy(f._h, 200_000) == ta.STRATEGY_TILEBLOCK
    assert f.kernel_form(200_000) == "sparse_top"
    for name in FLOAT_FORMS:
        f.set_strategy(strategy(ta, name))
    f.close()
    plain.close()


def test_known_answers_on_every_float_strategy(env):
    ta, torch = env
    sn, tr, node, offset, words, ml = capi_t.three_trees(ta)
    data = np.array([k[0] for k in capi_t.KNOWN], np.float32)
    want_leaf = np.array([k[1] for k in capi_t.KNOWN], np.uint32)
    want = np.array([capi_t._want(k[1]) for k in capi_t.KNOWN], np.float32)
    cats = {0: [2, 33], 3: [0, 5], 8: []}
    f = ta.capi.SparseForest(sn, tr, 2, missing=MISSING, categories=cats, members_left={3})
    x = torch.from_numpy(data).cuda()
    for name in FLOAT_FORMS:
        f.set_strategy(strategy(ta, name))
        leaf, sums = f.predict_leaf_idx(x)
        f.check()
        assert np.array_equal(leaf.cpu().numpy().view(np.uint32), want_leaf), name
        assert np.array_equal(bits(sums.cpu().numpy()), bits(want)), name
    f.close()


def test_classes_with_softmax(env):
    ta, torch = env
    nc, cols, feats = 3, 24, [2, 7, 11, 20]
    sn, tr, cats, ml = cat_forest(ta, 17 * nc, cols, feats, seed=31)
    rows = 2500
    data = cat_data(ta, rows, cols, feats, seed=32)
    want, want_leaf = ref(ta, sn, tr, data, cats, ml, num_classes=nc)
    e = np.exp(want.astype(np.float64) - want.max(axis=1, keepdims=True))
    want_p = e / e.sum(axis=1, keepdims=True)
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, output=ta.OUT_SOFTMAX, num_classes=nc, categories=cats,
                             members_left=ml)
    assert f.num_classes == nc
    x = torch.from_numpy(data).cuda()
    for name in FLOAT_FORMS:
        f.set_strategy(strategy(ta, name))
        raw = f.predict_raw(x)
        p = f.predict(x)
        leaf, sums = f.predict_leaf_idx(x)
        f.check()
        assert tuple(raw.shape) == (rows, nc)
        assert np.array_equal(bits(raw.cpu().numpy()), bits(want)), name
        assert np.array_equal(bits(sums.cpu().numpy()), bits(want)), name
        assert np.array_equal(leaf.cpu().numpy().view(np.uint32), want_leaf), name
        assert np.allclose(p.cpu().numpy(), want_p, rtol=1e-5, atol=1e-7), name
    f.close()


def test_accumulate_and_host_with_one_class(env):
    ta, torch = env
    cols, feats = 20, [0, 4, 13]
    sn, tr, cats, ml = cat_forest(ta, 45, cols, feats, seed=41)
    rows = 4100
    data = cat_data(ta, rows, cols, feats, seed=42)
    init = np.random.default_rng(43).uniform(-2, 2, rows).astype(np.float32)
    want, _ = ref(ta, sn, tr, data, cats, ml)
    want_acc, _ = ref(ta, sn, tr, data, cats, ml, init=init)
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, categories=cats, members_left=ml)
    x = torch.from_numpy(data).cuda()
    for name in FLOAT_FORMS:
        f.set_strategy(strategy(ta, name))
        acc = torch.from_numpy(init.copy()).cuda()
        f.predict_accumulate(x, acc)
        h = np.full(rows, 7.0, np.float32)
        f.predict_host(data, h, chunk_rows=1024)
        f.check()
        assert np.array_equal(bits(acc.cpu().numpy()), bits(want_acc)), name
        assert np.array_equal(bits(h), bits(want)), name
    f.close()


@pytest.mark.parametrize("complement", [False, True])
def test_threshold_splits_restated_as_sets_give_the_plain_handle_bits(env, complement):
    """On categorical columns holding integers in [0, K) (and, for the sets {k..K-1} going right, NaN, negatives and the
    sentinel), x >= k and x >= k - 0.5 are the set {k, ..., K-1} with members right, or its complement {0, ..., k-1} with
    members left.  The categorical handle must give the plain sparse handle's bits."""
    ta, torch = env
    cols, feats, K = 24, [1, 6, 15, 22], 300
    sn, tr = ta.capi.synth_sparse_forest(70, cols, 4, 18, 0.32, 65535, 51)
    rng = np.random.default_rng(52)
    b = sn["bits"].view(np.uint32)
    inner = np.flatnonzero((b >> 31) == 0)
    chosen = inner[np.isin(b[inner] & ((1 << 30) - 1), feats)]
    k = rng.integers(0, K + 1, chosen.size)
    thr = np.where(rng.random(chosen.size) < 0.5, k, k - 0.5).astype(np.float32)
    num = sn.copy()
    num["val"][chosen] = thr
    if complement:
        cats = {int(i): range(int(kk)) for i, kk in zip(chosen, k)}
        ml = {int(i) for i in chosen}
    else:
        cats = {int(i): range(int(kk), K) for i, kk in zip(chosen, k)}
        ml = set()
    cats = {i: list(c) for i, c in cats.items()}
    rows = 3100
    data = ta.synth_data(rows, cols, seed=53, missing_prob=0.03, missing=MISSING, nan_prob=0.02)
    for f_ in feats:
        u = rng.random(rows)
        v = rng.integers(0, K, rows).astype(np.float32)
        v = np.where(u < 0.05, np.float32(MISSING), v)
        if not complement:
            v = np.where((u >= 0.05) & (u < 0.10), np.float32(np.nan), v)
            # below every threshold (k - 0.5 >= -0.5); -0.0 is category 0 and >= -0.5 alike
            v = np.where((u >= 0.10) & (u < 0.15), rng.choice(np.array([-0.0, -0.75, -1.0, -7.0], np.float32), rows), v)
        data[:, f_] = v
    data = np.ascontiguousarray(data, dtype=np.float32)
    x = torch.from_numpy(data).cuda()
    plain = ta.capi.SparseForest(num, tr, cols, missing=MISSING)
    cat = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, categories=cats, members_left=ml)  # vals of sn are ignored
    for name in FLOAT_FORMS:
        plain.set_strategy(strategy(ta, name))
        cat.set_strategy(strategy(ta, name))
        a_leaf, a_sums = plain.predict_leaf_idx(x)
        b_leaf, b_sums = cat.predict_leaf_idx(x)
        plain.check()
        cat.check()
        assert np.array_equal(a_leaf.cpu().numpy(), b_leaf.cpu().numpy()), name
        assert np.array_equal(bits(a_sums.cpu().numpy()), bits(b_sums.cpu().numpy())), name
    plain.close()
    cat.close()


def test_no_splits_gives_the_ex_handle(env):
    ta, torch = env
    cols = 32
    sn, tr = ta.capi.synth_sparse_forest(90, cols, 4, 24, 0.32, 65535, 61)
    data = ta.synth_data(5000, cols, seed=62, missing_prob=0.05, missing=MISSING, nan_prob=0.01)
    x = torch.from_numpy(data).cuda()
    ex = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, num_classes=3, output=ta.OUT_SOFTMAX)
    params = ta.ForestParams(int(sn.size), 0, int(tr.size), cols, 0, ta.OUT_SOFTMAX, 0.0, 0.0, 0, MISSING)
    new = ta.capi.SparseForest.__new__(ta.capi.SparseForest)
    new.params, new._h = params, C.c_void_p()
    empty = ta.capi.CategoricalSplits(0, None, None, None, None)
    assert ta.lib.tahoe_sparse_forest_create_cat(C.byref(new._h), tr.ctypes.data, sn.ctypes.data, None, C.byref(params), 3, 0,
                                                 C.byref(empty)) == 0
    new.num_trees, new.depth, new.num_cols, new.num_classes = int(tr.size), 0, cols, 3
    assert new.info().device_bytes == ex.info().device_bytes
    for name in FLOAT_FORMS + ("QRING",):
        ex.set_strategy(strategy(ta, name))
        new.set_strategy(strategy(ta, name))
        assert ex.kernel_form(5000) == new.kernel_form(5000)
        a_leaf, a_sums = ex.predict_leaf_idx(x)
        b_leaf, b_sums = new.predict_leaf_idx(x)
        a, b = ex.predict(x), new.predict(x)
        ex.check()
        new.check()
        assert np.array_equal(a_leaf.cpu().numpy(), b_leaf.cpu().numpy()), name
        assert np.array_equal(bits(a_sums.cpu().numpy()), bits(b_sums.cpu().numpy())), name
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), name
    new.close()
    ex.close()
