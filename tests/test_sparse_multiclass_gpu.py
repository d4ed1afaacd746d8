"""Multi-class sparse handles (tahoe_sparse_forest_create_ex) on the GPU: per-class float32 sums bit for bit the CPU oracle on each
class's sub-forest (trees c, c + C, ...), leaf indices in the caller's numbering, under every strategy of a sparse handle;
QRING tree groups that cut inside classes; a dense multi-class forest converted to sparse; C == 1 against the old entry point;
the refusals of predict_accumulate / predict_host.  Needs an MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_shap_ref  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def class_sums(sn, tr, data, num_classes):
    """[rows, C] float32: oracle.sparse_predict on every class's sub-forest."""
    out = np.empty((data.shape[0], num_classes), np.float32)
    for c in range(num_classes):
        s, t = sparse_shap_ref.sub_forest(sn, tr, c, num_classes)
        out[:, c], _ = oracle.sparse_predict(s, t, data, MISSING, threads=8)
    return out


def strategies(ta, f):
    out = [ta.STRATEGY_AUTO, ta.STRATEGY_DIRECT, ta.STRATEGY_ROWTILE, ta.STRATEGY_TILEBLOCK, ta.STRATEGY_QRING]
    avail = []
    for s in out:
        try:
            f.set_strategy(s)
            avail.append(s)
        except ta.TahoeError:
            pass
    f.set_strategy(ta.STRATEGY_AUTO)
    return avail


@pytest.mark.parametrize("num_classes", [3, 7])
def test_irregular_forest_every_strategy(env, num_classes):
    ta, torch = env
    T, cols, rows = 12 * num_classes, 32, 3000
    sn, tr = ta.capi.synth_sparse_forest(T, cols, 4, 24, 0.32, 65535, 300 + num_classes)
    data = ta.synth_data(rows, cols, seed=num_classes, missing_prob=0.05, missing=MISSING, nan_prob=0.02)
    want = class_sums(sn, tr, data, num_classes)
    _, want_leaf = oracle.sparse_predict(sn, tr, data, MISSING, want_leaf=True, threads=8)
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, num_classes=num_classes)
    assert f.num_classes == num_classes and ta.lib.tahoe_forest_num_classes(f._h) == num_classes
    got = strategies(ta, f)
    assert set(got) >= {ta.STRATEGY_AUTO, ta.STRATEGY_DIRECT, ta.STRATEGY_ROWTILE, ta.STRATEGY_TILEBLOCK, ta.STRATEGY_QRING}
    x = torch.from_numpy(data).cuda()
    for s in got:
        f.set_strategy(s)
        raw = f.predict_raw(x)
        f.check()
        assert tuple(raw.shape) == (rows, num_classes)
        assert np.array_equal(bits(raw.cpu().numpy()), bits(want)), s
        leaf, sums = f.predict_leaf_idx(x)
        f.check()
        assert np.array_equal(leaf.cpu().numpy().view(np.uint32), want_leaf), s
        assert np.array_equal(bits(sums.cpu().numpy()), bits(want)), s
        leaf2, none = f.predict_leaf_idx(x, want_sums=False)
        f.check()
        assert none is None and np.array_equal(leaf2.cpu().numpy().view(np.uint32), want_leaf), s
    f.close()


@pytest.mark.parametrize("num_classes", [2, 3])
def test_qring_tree_groups_cut_inside_classes(env, num_classes):
    """The > 32767-threshold forest of test_sparse.py (48 trees, 2 features: two or more quantisation groups) read as classes:
    group boundaries at 24 (two groups), 16 / 32 (three) or 12 / 24 / 36 (four) fall inside a class for C = 2 or 3."""
    ta, torch = env
    cols = 2
    sn, tr = ta.capi.synth_sparse_forest(48, cols, 10, 14, 0.05, 65535, 91)
    rows = 5000
    data = ta.synth_data(rows, cols, seed=92, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    data[7, 0], data[8, 1], data[9, 0] = np.inf, -np.inf, -0.0
    want = class_sums(sn, tr, data, num_classes)
    _, want_leaf = oracle.sparse_predict(sn, tr, data, MISSING, want_leaf=True, threads=8)
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, num_classes=num_classes)
    f.set_strategy(ta.STRATEGY_QRING)
    x = torch.from_numpy(data).cuda()
    for n in (1, 63, 64, 65, 191, 193, 385, 4097, 5000):
        leaf, sums = f.predict_leaf_idx(x[:n].contiguous())
        raw = f.predict_raw(x[:n].contiguous())
        f.check()
        assert np.array_equal(leaf.cpu().numpy().view(np.uint32), want_leaf[:n]), n
        assert np.array_equal(bits(sums.cpu().numpy()), bits(want[:n])), n
        assert np.array_equal(bits(raw.cpu().numpy()), bits(want[:n])), n
    f.close()


@pytest.mark.parametrize("output,bias", [("avg", 0.375), ("sigmoid", 0.0), ("softmax", -0.25)])
def test_dense_multiclass_converted_to_sparse(env, output, bias):
    ta, torch = env
    nc, D, F = 3, 8, 16
    T = 5 * nc
    out = {"avg": ta.OUT_AVG, "sigmoid": ta.OUT_SIGMOID, "softmax": ta.OUT_SOFTMAX | ta.OUT_AVG}[output]
    nodes = ta.synth_forest_hist(T, D, F, seed=31, feature_seed=32)
    data = ta.synth_data_hist(2500, F, seed=33, feature_seed=32, missing_prob=0.03, missing=MISSING)
    x = torch.from_numpy(data).cuda()
    dense = ta.Forest(nodes, T, D, F, missing=MISSING, output=out, global_bias=bias, num_classes=nc)
    want_pred = dense.predict(x).cpu().numpy()
    want_raw = dense.predict_raw(x).cpu().numpy()
    dense.check()
    sn, tr = ta.capi.dense_to_sparse(nodes, T, D)
    assert np.array_equal(bits(want_raw), bits(class_sums(sn, tr, data, nc)))
    sp = ta.capi.SparseForest(sn, tr, F, missing=MISSING, output=out, global_bias=bias, num_classes=nc)
    for s in strategies(ta, sp):
        sp.set_strategy(s)
        pred = sp.predict(x)
        raw = sp.predict_raw(x)
        sp.check()
        assert np.array_equal(bits(pred.cpu().numpy()), bits(want_pred)), (output, s)
        assert np.array_equal(bits(raw.cpu().numpy()), bits(want_raw)), (output, s)
    sp.close()
    dense.close()


def test_one_class_ex_matches_the_old_entry_point(env):
    ta, torch = env
    cols = 32
    sn, tr = ta.capi.synth_sparse_forest(90, cols, 4, 24, 0.32, 65535, 44)
    data = ta.synth_data(5000, cols, seed=45, missing_prob=0.05, missing=MISSING, nan_prob=0.01)
    x = torch.from_numpy(data).cuda()
    out = ta.OUT_AVG | ta.OUT_SIGMOID
    old = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, output=out, global_bias=0.5)
    params = ta.ForestParams(int(sn.size), 0, int(tr.size), cols, 0, out, 0.0, 0.5, 0, MISSING)
    new = ta.capi.SparseForest.__new__(ta.capi.SparseForest)
    new.params, new._h = params, C.c_void_p()
    assert ta.lib.tahoe_sparse_forest_create_ex(C.byref(new._h), tr.ctypes.data, sn.ctypes.data, None, C.byref(params), 1, 0) == 0
    new.num_trees, new.depth, new.num_cols, new.num_classes = int(tr.size), 0, cols, 1
    assert ta.lib.tahoe_forest_num_classes(new._h) == 1
    assert new.info().device_bytes == old.info().device_bytes
    for s in strategies(ta, old):
        old.set_strategy(s)
        new.set_strategy(s)
        assert old.kernel_form(5000) == new.kernel_form(5000)
        a_leaf, a_sums = old.predict_leaf_idx(x)
        b_leaf, b_sums = new.predict_leaf_idx(x)
        a, b = old.predict(x), new.predict(x)
        old.check()
        new.check()
        assert np.array_equal(a_leaf.cpu().numpy(), b_leaf.cpu().numpy()), s
        assert np.array_equal(bits(a_sums.cpu().numpy()), bits(b_sums.cpu().numpy())), s
        assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), s
    # the accumulate and host paths stay served with one class
    acc = old.predict_raw(x)
    new.predict_accumulate(x, acc)
    h = np.empty(5000, np.float32)
    new.predict_host(data, h)
    new.check()
    new.close()
    old.close()


def test_accumulate_and_host_are_refused_with_classes(env):
    ta, torch = env
    cols = 16
    sn, tr = ta.capi.synth_sparse_forest(9, cols, 4, 12, 0.32, 65535, 46)
    data = ta.synth_data(300, cols, seed=47)
    x = torch.from_numpy(data).cuda()
    f = ta.capi.SparseForest(sn, tr, cols, num_classes=3)
    sums = torch.full((300, 3), 7.0, device="cuda")
    assert ta.lib.tahoe_forest_predict_accumulate(f._h, sums.data_ptr(), x.data_ptr(), 300, None) == 7
    assert "multi-class" in ta.lib.tahoe_last_error().decode()
    preds = np.full(300 * 3, 7.0, np.float32)
    assert ta.lib.tahoe_forest_predict_host(f._h, preds.ctypes.data, data.ctypes.data, 300, 0) == 7
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all()) and bool((preds == 7.0).all())  # nothing was written
    f.check()
    f.close()
