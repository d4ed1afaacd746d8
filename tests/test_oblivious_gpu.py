"""Oblivious forests on the GPU (tahoe_oblivious_forest_create).  Every comparison is for equal bits:
  - against tests/oblivious_ref.py under forced DIRECT, forced ROWTILE and AUTO: raw sums, leaf indices, every batch size;
  - against the library itself: the heap expansion on a dense handle (K == 1) and on a multi-class handle of T x K trees (K > 1),
    output transforms included -- both sides run the same epilogue kernels;
  - accumulate, the refusals, profiling, device bytes, graph capture.
Shapes are the smallest at which the kernels can go wrong: rows around the 64-row tile, tree counts that are no multiple of the
four trees in flight, depths 0 .. 16 mixed, num_cols with and without the 16-byte staging reads and one whose tile cannot fit
LDS, leaf dimensions across the 8-class block.  Needs an MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oblivious_ref as obr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = obr.MISSING
UNSUPPORTED = 7
ROWS = 130
BATCHES = (1, 63, 64, 65, 130)
_cache = {}

# name -> (depths, num_cols, K)
FORESTS = {
    "one_tree": ([6], 1, 1),
    "all_depth0_k2": ([0, 0, 0], 3, 2),
    "all_depth16": ([16, 16, 16], 40, 1),
    "mixed_k1": ([0, 1, 2, 6, 16], 5, 1),
    "mixed_k3": ([0, 1, 2, 6, 16], 5, 3),
    "nine_k1": ([6, 2, 1, 0, 1, 6, 2, 1, 0], 40, 1),
    "five_k8": ([2, 6, 0, 1, 6], 40, 8),
    "nine_k9": ([6, 2, 1, 0, 1, 6, 2, 1, 0], 40, 9),
    "nine_k17": ([2, 6, 0, 1, 6, 1, 2, 0, 6], 3, 17),
}


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def case(name):
    """(forest, data [ROWS, cols], reference sums [ROWS, K], reference leaves [ROWS, T]), computed once and read-only"""
    if name not in _cache:
        depths, cols, k = FORESTS[name]
        forest = obr.make_forest(depths, cols, k, seed=1000 + len(name))
        data = obr.make_data(ROWS, cols, seed=7 + cols)
        sums, leaf = obr.ref_of(forest, data)
        for a in (data, sums, leaf):
            a.setflags(write=False)
        _cache[name] = (forest, data, sums, leaf)
    return _cache[name]


def handle(ta, forest, **kw):
    return ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], forest["cols"],
                              leaf_dim=forest["k"], missing=MISSING, **kw)


def cut(forest, lo, hi):
    """Trees lo .. hi - 1 of a forest"""
    d = forest["depths"].astype(np.int64)
    s = np.concatenate([[0], np.cumsum(d)])
    v = np.concatenate([[0], np.cumsum(1 << d)]) * forest["k"]
    return dict(forest, depths=forest["depths"][lo:hi], fids=forest["fids"][s[lo]:s[hi]], thr=forest["thr"][s[lo]:s[hi]],
                def_left=forest["def_left"][s[lo]:s[hi]], leaves=forest["leaves"][v[lo]:v[hi]])


def shaped(sums, k):
    return sums[:, 0] if k == 1 else sums


def dense_handle(ta, forest, **kw):
    """The heap expansion on a handle of tahoe_forest_create (K == 1) or, tree t * K + k carrying class k's leaves, of
    tahoe_forest_create_multiclass"""
    k, T = forest["k"], len(forest["depths"])
    per_class = [obr.dense_of(forest, c) for c in range(k)]
    D = per_class[0][1]
    nodes = np.stack([n.reshape(T, -1) for n, _ in per_class], axis=1).reshape(-1)
    return ta.Forest(nodes, T * k, D, forest["cols"], missing=MISSING, num_classes=k, **kw)


# ------------------------------------------------------------------------------------------------ 1: against the reference
@pytest.mark.parametrize("name", list(FORESTS))
def test_sums_and_leaves_match_the_reference(env, name):
    ta, torch = env
    forest, data, want, want_leaf = case(name)
    k = forest["k"]
    f = handle(ta, forest)
    assert f.num_classes == k
    x = torch.from_numpy(data.copy()).cuda()
    got = {}
    for strat in ("DIRECT", "ROWTILE", "AUTO"):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert f.kernel_form(ROWS) == ("oblivious_direct" if strat == "DIRECT" else "oblivious_tile")
        for r in BATCHES:
            xr = x[:r].contiguous()
            sums = f.predict_raw(xr)
            leaf, lsums = f.predict_leaf_idx(xr)
            assert tuple(sums.shape) == ((r, k) if k > 1 else (r,))
            assert np.array_equal(bits(sums), bits(shaped(want[:r], k))), (strat, r)
            assert np.array_equal(bits(lsums), bits(shaped(want[:r], k))), (strat, r)
            assert np.array_equal(bits(leaf), want_leaf[:r].view(np.uint32)), (strat, r)
            leaf_only, none = f.predict_leaf_idx(xr, want_sums=False)
            assert none is None and np.array_equal(bits(leaf_only), want_leaf[:r].view(np.uint32))
        alone = f.predict_raw(x[ROWS - 1:ROWS].clone())  # a row alone and inside a batch
        assert np.array_equal(bits(alone), bits(shaped(want[ROWS - 1:], k))), strat
        got[strat] = bits(f.predict_raw(x))
    assert np.array_equal(got["DIRECT"], got["ROWTILE"]) and np.array_equal(got["AUTO"], got["ROWTILE"])
    f.check()
    f.close()


def test_a_tile_that_cannot_fit_lds_runs_direct(env):
    ta, torch = env
    lds = C.c_int()
    assert ta.lib.tahoe_device_lds_bytes(C.byref(lds)) == 0
    cols = lds.value // 256 + 1  # one 64-row float32 tile is 256 bytes per column
    forest = obr.make_forest([2, 6, 1], cols, 1, seed=77)
    data = obr.make_data(65, cols, seed=78)
    want, want_leaf = obr.ref_of(forest, data)
    f = handle(ta, forest)
    assert f.kernel_form(65) == "oblivious_direct" and f.get_strategy(65) == ta.STRATEGY_DIRECT
    with pytest.raises(ta.TahoeError) as e:
        f.set_strategy(ta.STRATEGY_ROWTILE)
    assert e.value.status == UNSUPPORTED
    x = torch.from_numpy(data.copy()).cuda()
    leaf, sums = f.predict_leaf_idx(x)
    assert np.array_equal(bits(sums), bits(want[:, 0])) and np.array_equal(bits(leaf), want_leaf.view(np.uint32))
    assert np.array_equal(bits(f.predict_raw(x)), bits(want[:, 0]))
    f.check()
    f.close()


@pytest.mark.parametrize("k", [1, 9])
def test_the_widest_tile_that_fits_runs(env, k):
    """All of the device's LDS as one tile: past the 64 KiB a kernel may ask for without hipFuncSetAttribute"""
    ta, torch = env
    lds = C.c_int()
    assert ta.lib.tahoe_device_lds_bytes(C.byref(lds)) == 0
    cols = lds.value // 256
    assert cols * 256 > 64 * 1024
    forest = obr.make_forest([2, 6, 1, 0, 6], cols, k, seed=79)
    forest["fids"][:3] = (cols - 1, 0, cols - 2)  # the last rows of the tile are read
    data = obr.make_data(65, cols, seed=80)
    want, want_leaf = obr.ref_of(forest, data)
    f = handle(ta, forest)
    assert f.kernel_form(65) == "oblivious_tile" and f.get_strategy(65) == ta.STRATEGY_ROWTILE
    x = torch.from_numpy(data.copy()).cuda()
    leaf, sums = f.predict_leaf_idx(x)
    assert np.array_equal(bits(sums), bits(shaped(want, k))) and np.array_equal(bits(leaf), want_leaf.view(np.uint32))
    assert np.array_equal(bits(f.predict_raw(x)), bits(shaped(want, k)))
    f.check()
    f.close()


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_rows_off_the_16_byte_boundary_take_the_plain_staging_loop(env, shift):
    """num_cols is a multiple of 4, but the batch starts `shift` floats past a 16-byte boundary: no float4 row reads"""
    ta, torch = env
    forest, data, want, want_leaf = case("nine_k1")
    cols = forest["cols"]
    assert cols % 4 == 0
    buf = torch.full((ROWS * cols + 4,), float("nan"), device="cuda")
    x = buf[shift:shift + ROWS * cols].view(ROWS, cols)
    x.copy_(torch.from_numpy(data.copy()))
    assert x.is_contiguous() and buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 4 * shift
    f = handle(ta, forest)
    f.set_strategy(ta.STRATEGY_ROWTILE)
    leaf, sums = f.predict_leaf_idx(x)
    assert np.array_equal(bits(sums), bits(want[:, 0])) and np.array_equal(bits(leaf), want_leaf.view(np.uint32))
    assert np.array_equal(bits(f.predict_raw(x[:65])), bits(want[:65, 0]))
    f.check()
    f.close()


@pytest.mark.parametrize("strat", ["TILEBLOCK", "TILERING", "QRING"])
def test_other_strategies_are_refused(env, strat):
    ta, _ = env
    f = handle(ta, case("mixed_k1")[0])
    with pytest.raises(ta.TahoeError) as e:
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
    assert e.value.status == UNSUPPORTED and "oblivious" in str(e.value)
    f.close()


# ------------------------------------------------------------------------------------------------ 2: the expansion, K == 1
@pytest.mark.parametrize("output,bias", [("RAW", 0.0), ("AVG", 0.25), ("THRESHOLD", 0.0), ("SIGMOID", -0.5), ("AVG|SIGMOID", 0.0)])
@pytest.mark.parametrize("name", ["one_tree", "mixed_k1", "nine_k1"])
def test_single_output_equals_the_dense_expansion(env, name, output, bias):
    ta, torch = env
    forest, data, want, _ = case(name)
    out = 0
    for o in output.split("|"):
        out |= getattr(ta, "OUT_" + o)
    kw = dict(output=out, threshold=0.5, global_bias=bias)
    f, g = handle(ta, forest, **kw), dense_handle(ta, forest, **kw)
    x = torch.from_numpy(data.copy()).cuda()
    a, b = f.predict(x), g.predict(x)
    assert np.array_equal(bits(a), bits(b))
    if output == "RAW":
        assert np.array_equal(bits(a), bits(want[:, 0]))
    else:
        assert not np.array_equal(bits(a), bits(want[:, 0]))  # the transform ran
    f.check()
    f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ 3: the expansion, K > 1
@pytest.mark.parametrize("name", ["all_depth0_k2", "mixed_k3", "five_k8", "nine_k9", "nine_k17"])
def test_vector_leaves_equal_the_multiclass_expansion(env, name):
    ta, torch = env
    forest, data, want, _ = case(name)
    T = len(forest["depths"])
    x = torch.from_numpy(data.copy()).cuda()
    f, g = handle(ta, forest), dense_handle(ta, forest)
    margins = f.predict_raw(x)
    assert np.array_equal(bits(margins), bits(g.predict_raw(x))) and np.array_equal(bits(margins), bits(want))
    f.close()
    g.close()
    kw = dict(output=ta.OUT_SOFTMAX, global_bias=0.125)
    f, g = handle(ta, forest, **kw), dense_handle(ta, forest, **kw)
    p = f.predict(x)
    assert np.array_equal(bits(p), bits(g.predict(x)))
    ok = np.isfinite(want).all(axis=1)
    assert ok.any() and np.allclose(p.cpu().numpy()[ok].sum(axis=1), 1.0, atol=1e-5)
    f.close()
    g.close()
    f = handle(ta, forest, output=ta.OUT_AVG)  # every tree feeds every class: the divisor is T
    assert np.array_equal(bits(f.predict(x)), bits(want / np.float32(T)))
    f.close()


# ------------------------------------------------------------------------------------------------ 4: accumulate
@pytest.mark.parametrize("strat", ["DIRECT", "ROWTILE"])
def test_accumulate_continues_the_sum(env, strat):
    ta, torch = env
    forest, data, want, _ = case("nine_k1")
    x = torch.from_numpy(data.copy()).cuda()
    first, second = handle(ta, cut(forest, 0, 4)), handle(ta, cut(forest, 4, 9))
    for h in (first, second):
        h.set_strategy(getattr(ta, "STRATEGY_" + strat))
    sums = first.predict_raw(x)
    assert not np.array_equal(bits(sums), bits(want[:, 0]))
    second.predict_accumulate(x, sums)
    assert np.array_equal(bits(sums), bits(want[:, 0]))
    first.close()
    second.close()


def test_accumulate_is_refused_for_vector_leaves(env):
    ta, torch = env
    forest, data, _, _ = case("mixed_k3")
    f = handle(ta, forest)
    x = torch.from_numpy(data.copy()).cuda()
    sums = torch.full((ROWS, 3), 7.0, device="cuda")
    st = ta.lib.tahoe_forest_predict_accumulate(f._h, sums.data_ptr(), x.data_ptr(), ROWS, None)
    torch.cuda.synchronize()
    assert st == UNSUPPORTED and bool((sums == 7.0).all())
    f.close()


# ------------------------------------------------------------------------------------------------ 5: out of scope
def test_entry_points_out_of_scope_are_refused(env):
    ta, torch = env
    forest, data, _, _ = case("mixed_k1")
    cols = forest["cols"]
    f = handle(ta, forest)
    x = torch.from_numpy(data.copy()).cuda()
    lib, h = ta.lib, f._h
    out = torch.full((ROWS * (cols + 1) * (cols + 1),), 7.0, device="cuda")
    indptr = torch.arange(0, ROWS + 1, dtype=torch.int64, device="cuda")
    indices = torch.zeros(ROWS, dtype=torch.int32, device="cuda")
    host_out = np.full(ROWS, 7.0, np.float32)
    rounds = np.array([1, 2], np.int32)
    form, chunk = C.c_int(-5), C.c_size_t(99)
    calls = {
        "tahoe_forest_predict_csr": lambda: lib.tahoe_forest_predict_csr(h, out.data_ptr(), indptr.data_ptr(), indices.data_ptr(),
                                                                         x.data_ptr(), ROWS, ROWS, None),
        "tahoe_forest_reserve_csr": lambda: lib.tahoe_forest_reserve_csr(h, ROWS, ROWS),
        "tahoe_forest_get_csr_plan": lambda: lib.tahoe_forest_get_csr_plan(h, ROWS, ROWS, C.byref(form), C.byref(chunk)),
        "tahoe_forest_predict_host": lambda: lib.tahoe_forest_predict_host(h, host_out.ctypes.data, data.ctypes.data, ROWS, 0),
        "tahoe_forest_set_stages": lambda: lib.tahoe_forest_set_stages(h, rounds.ctypes.data, 2),
        "tahoe_forest_predict_staged": lambda: lib.tahoe_forest_predict_staged(h, out.data_ptr(), x.data_ptr(), ROWS, None),
        "tahoe_forest_predict_contribs": lambda: lib.tahoe_forest_predict_contribs(h, out.data_ptr(), x.data_ptr(), ROWS, None),
        "tahoe_forest_predict_interactions": lambda: lib.tahoe_forest_predict_interactions(h, out.data_ptr(), x.data_ptr(), ROWS, None),
        "tahoe_forest_predict_contribs_interventional":
            lambda: lib.tahoe_forest_predict_contribs_interventional(h, out.data_ptr(), x.data_ptr(), ROWS, None),
        "tahoe_forest_predict_contribs_approx": lambda: lib.tahoe_forest_predict_contribs_approx(h, out.data_ptr(), x.data_ptr(), ROWS, None),
        "tahoe_forest_set_background": lambda: lib.tahoe_forest_set_background(h, x.data_ptr(), ROWS, None),
    }
    for name, call in calls.items():
        assert call() == UNSUPPORTED, name
        msg = lib.tahoe_last_error().decode()
        assert "oblivious" in msg and name in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and (host_out == 7.0).all()
    assert form.value == 0 and chunk.value == 0  # TAHOE_FORM_NONE
    assert f.staged_strategy(ROWS) == 0
    f.reserve(1 << 20)  # served: nothing to size
    f.check()
    assert np.array_equal(bits(f.predict_raw(x)), bits(case("mixed_k1")[2][:, 0]))  # the handle is as it was
    f.close()


# ------------------------------------------------------------------------------------------------ 6 - 9
def test_profiling_info_and_graph_capture(env):
    ta, torch = env
    forest, data, want, _ = case("nine_k9")
    f = handle(ta, forest)
    x = torch.from_numpy(data.copy()).cuda()
    info = f.info()
    assert info.device_bytes >= 8 * forest["fids"].size + 4 * forest["leaves"].size
    assert info.depth == 6 and info.is_sparse == 0 and info.num_trees == 9 and info.num_cols == 40
    f.set_profiling(3)
    for _ in range(3):
        f.predict_raw(x)
    times = f.kernel_times_ms()
    assert times.shape == (3,) and (times > 0).all()
    f.set_profiling(0)

    out = torch.empty((ROWS, 9), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f.predict(x, preds=out)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f.predict(x, preds=out)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(want))
        out.zero_()
    f.check()
    f.close()


def test_empty_forest_and_empty_batch(env):
    ta, torch = env
    f = ta.ObliviousForest([], [], [], [], [], 3, leaf_dim=2, missing=MISSING)
    x = torch.from_numpy(obr.make_data(5, 3, seed=1)).cuda()
    assert not bits(f.predict_raw(x)).any()
    f.close()
    f = handle(ta, case("all_depth0_k2")[0])  # (3 columns as well)
    assert tuple(f.predict_raw(x[:0].contiguous()).shape) == (0, 2)
    f.check()
    f.close()
