"""Vector-leaf forests on the GPU (tahoe_vector_forest_create).  Every comparison is for equal bits:
  - against tests/vector_ref.py under forced DIRECT and forced ROWTILE: raw sums and leaf indices at every batch size;
  - against the library itself: the T x K-tree expansion on a multi-class SparseForest (K > 1) or the same trees on a plain
    SparseForest (K == 1), output transforms included -- both sides run the same epilogue kernels;
  - the strategy rule, the refusals, profiling, device bytes, graph capture.
Shapes are the smallest at which the kernels can go wrong: rows around the 64-row tile and the 256-row workgroup, tree counts
around the four trees in flight, a depth-24 chain beside stumps and single leaves in one window, leaf dimensions across the
8-class block, num_cols with and without the 16-byte staging reads and one whose tile cannot fit LDS.  Needs an MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vector_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = vr.MISSING
UNSUPPORTED = 7
ROWS = vr.ROWS
BATCHES = (1, 63, 64, 65, 200, 257)
FORM_DIRECT, FORM_TILE = 27, 28


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def handle(ta, forest, **kw):
    return ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=MISSING, **kw)


def expansion_handle(ta, forest, **kw):
    """The T x K-tree expansion on a handle of tahoe_sparse_forest_create_ex(num_classes = K); K == 1: tahoe_sparse_forest_create"""
    nodes, trees = vr.expand(forest)
    kw.setdefault("threshold", 0.5)
    return ta.capi.SparseForest(nodes, trees, forest["cols"], missing=MISSING, num_classes=forest["k"], **kw)


def shaped(sums, k):
    return sums[:, 0] if k == 1 else sums


# ------------------------------------------------------------------------------------------------ 1: sums and leaf indices
@pytest.mark.parametrize("name", list(vr.FORESTS))
def test_sums_and_leaves_match_the_reference_and_the_expansion(env, name):
    ta, torch = env
    forest, data, want, want_leaf, _ = vr.case(name)
    k, T = forest["k"], forest["trees"].size
    f, g = handle(ta, forest), expansion_handle(ta, forest)
    assert f.num_classes == k and f.num_trees == T
    x = torch.from_numpy(data.copy()).cuda()
    theirs = {}
    for r in BATCHES:
        xr = x[:r].contiguous()
        if T == 0:  # (no tree, no leaf index: a [rows, 0] tensor has no address to pass)
            theirs[r] = (bits(g.predict_raw(xr)),)
            assert not theirs[r][0].any()
            continue
        leaf, sums = g.predict_leaf_idx(xr)
        theirs[r] = (bits(g.predict_raw(xr)), bits(sums), bits(leaf).reshape(r, T * k)[:, ::k])
        assert np.array_equal(theirs[r][0], bits(shaped(want[:r], k))), r  # (the expansion agrees with the restatement)
    got = {}
    for strat in ("DIRECT", "ROWTILE"):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert f.kernel_form(ROWS) == ("vector_direct" if strat == "DIRECT" else "vector_tile")
        for r in BATCHES:
            xr = x[:r].contiguous()
            sums = f.predict_raw(xr)
            assert tuple(sums.shape) == ((r, k) if k > 1 else (r,))
            assert np.array_equal(bits(sums), bits(shaped(want[:r], k))) and np.array_equal(bits(sums), theirs[r][0]), (strat, r)
            if T == 0:
                continue
            leaf, lsums = f.predict_leaf_idx(xr)
            assert tuple(lsums.shape) == tuple(sums.shape)
            assert tuple(leaf.shape) == (r, T)
            assert np.array_equal(bits(sums), bits(shaped(want[:r], k))), (strat, r)
            assert np.array_equal(bits(lsums), bits(shaped(want[:r], k))), (strat, r)
            assert np.array_equal(bits(leaf), want_leaf[:r].view(np.uint32)), (strat, r)
            assert np.array_equal(bits(sums), theirs[r][0]) and np.array_equal(bits(lsums), theirs[r][1]), (strat, r)
            assert np.array_equal(bits(leaf), theirs[r][2]), (strat, r)
            leaf_only, none = f.predict_leaf_idx(xr, want_sums=False)
            assert none is None and np.array_equal(bits(leaf_only), want_leaf[:r].view(np.uint32))
        for i in (0, 100, ROWS - 1):  # a row alone and inside a batch
            alone = f.predict_raw(x[i:i + 1].clone())
            assert np.array_equal(bits(alone), bits(shaped(want[i:i + 1], k))), (strat, i)
        got[strat] = bits(f.predict_raw(x))
    assert np.array_equal(got["DIRECT"], got["ROWTILE"])
    f.check()
    f.close()
    g.close()


@pytest.mark.parametrize("name", ["four_k8", "nine_k1"])
@pytest.mark.parametrize("strat", ["DIRECT", "ROWTILE"])
def test_rows_off_the_16_byte_boundary_take_the_plain_staging_loop(env, name, strat):
    """num_cols is a multiple of 4, but the batch starts one float past a 16-byte boundary: no float4 row reads"""
    ta, torch = env
    forest, data, want, want_leaf, _ = vr.case(name)
    k, cols = forest["k"], forest["cols"]
    assert cols % 4 == 0
    buf = torch.full((ROWS * cols + 4,), float("nan"), device="cuda")
    x = buf[1:1 + ROWS * cols].view(ROWS, cols)
    x.copy_(torch.from_numpy(data.copy()))
    assert x.is_contiguous() and buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 4
    f, g = handle(ta, forest), expansion_handle(ta, forest)
    f.set_strategy(getattr(ta, "STRATEGY_" + strat))
    leaf, sums = f.predict_leaf_idx(x)
    assert np.array_equal(bits(sums), bits(shaped(want, k))) and np.array_equal(bits(leaf), want_leaf.view(np.uint32))
    assert np.array_equal(bits(sums), bits(g.predict_raw(x)))
    assert np.array_equal(bits(f.predict_raw(x[:65])), bits(shaped(want[:65], k)))
    f.check()
    f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ 2: output bits
def out_bits(ta, output):
    out = 0
    for o in output.split("|"):
        out |= getattr(ta, "OUT_" + o)
    return out


@pytest.mark.parametrize("output", ["RAW", "AVG", "SIGMOID", "THRESHOLD"])
@pytest.mark.parametrize("name", ["three_k1", "nine_k1"])
def test_single_output_bits_equal_the_sparse_handle(env, name, output):
    ta, torch = env
    forest, data, want, _, _ = vr.case(name)
    kw = dict(output=out_bits(ta, output), threshold=0.5, global_bias=0.25)
    f, g = handle(ta, forest, **kw), expansion_handle(ta, forest, **kw)
    x = torch.from_numpy(data.copy()).cuda()
    for strat in ("DIRECT", "ROWTILE"):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        a = f.predict(x)
        assert tuple(a.shape) == (ROWS,)
        assert np.array_equal(bits(a), bits(g.predict(x))), strat
        assert not np.array_equal(bits(a), bits(want[:, 0]))  # the transform ran
        assert np.array_equal(bits(f.predict_raw(x)), bits(want[:, 0]))
    f.check()
    f.close()
    g.close()


@pytest.mark.parametrize("output", ["RAW", "AVG", "SOFTMAX", "AVG|SOFTMAX"])
@pytest.mark.parametrize("name", ["stump_k3", "four_k8", "five_k9", "nine_k17"])
def test_vector_output_bits_equal_the_multiclass_expansion(env, name, output):
    ta, torch = env
    forest, data, want, _, _ = vr.case(name)
    k, T = forest["k"], forest["trees"].size
    kw = dict(output=out_bits(ta, output), global_bias=0.125)
    f, g = handle(ta, forest, **kw), expansion_handle(ta, forest, **kw)
    x = torch.from_numpy(data.copy()).cuda()
    for strat in ("DIRECT", "ROWTILE"):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        p = f.predict(x)
        assert tuple(p.shape) == (ROWS, k)
        assert np.array_equal(bits(p), bits(g.predict(x))), strat
        assert not np.array_equal(bits(p), bits(want))  # the transform ran
    if "SOFTMAX" in output:
        ok = np.isfinite(want).all(axis=1)
        assert ok.any() and np.allclose(p.cpu().numpy()[ok].sum(axis=1), 1.0, atol=1e-5)
    if output == "AVG":  # every tree feeds every class: the divisor is T
        assert np.array_equal(bits(p), bits(want / np.float32(T) + np.float32(0.125)))
    f.check()
    f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ 3: the strategy rule
def test_a_tile_that_cannot_fit_lds_runs_direct(env):
    ta, torch = env
    cols = 700  # 256 B per column: 179200 B, past the 160 KiB of LDS
    forest = vr.make_named([4, "stump", "leaf", 6, 3], cols, 3, seed=77)
    data = vr.make_data(65, cols, seed=78)
    want, want_leaf, _ = vr.vector_ref(forest, data)
    f = handle(ta, forest)
    assert f.get_strategy(65) == ta.STRATEGY_DIRECT and ta.lib.tahoe_forest_get_kernel_form(f._h, 65) == FORM_DIRECT
    for strat in ("ROWTILE", "TILEBLOCK", "TILERING", "QRING"):
        with pytest.raises(ta.TahoeError) as e:
            f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert e.value.status == UNSUPPORTED and "vector-leaf" in str(e.value), strat
    assert f.get_strategy(65) == ta.STRATEGY_DIRECT
    x = torch.from_numpy(data.copy()).cuda()
    leaf, sums = f.predict_leaf_idx(x)
    assert np.array_equal(bits(sums), bits(want)) and np.array_equal(bits(leaf), want_leaf.view(np.uint32))
    assert np.array_equal(bits(f.predict_raw(x)), bits(want))
    f.check()
    f.close()


def test_auto_takes_the_tile_where_it_fits(env):
    ta, torch = env
    forest, data, want, _, _ = vr.case("four_k8")
    f = handle(ta, forest)
    assert f.get_strategy(ROWS) == ta.STRATEGY_ROWTILE and ta.lib.tahoe_forest_get_kernel_form(f._h, ROWS) == FORM_TILE
    assert f.kernel_form(ROWS) == "vector_tile"
    for strat in ("TILEBLOCK", "TILERING", "QRING"):
        with pytest.raises(ta.TahoeError) as e:
            f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert e.value.status == UNSUPPORTED and "vector-leaf" in str(e.value), strat
    x = torch.from_numpy(data.copy()).cuda()
    assert np.array_equal(bits(f.predict_raw(x)), bits(want))  # under AUTO
    f.close()


# ------------------------------------------------------------------------------------------------ 4: out of scope
@pytest.mark.parametrize("name", ["nine_k1", "five_k9"])
def test_entry_points_out_of_scope_are_refused(env, name):
    ta, torch = env
    forest, data, want, _, _ = vr.case(name)
    cols, k = forest["cols"], forest["k"]
    f = handle(ta, forest)
    x = torch.from_numpy(data.copy()).cuda()
    lib, h = ta.lib, f._h
    out = torch.full((ROWS * k * (cols + 1) * (cols + 1),), 7.0, device="cuda")
    indptr = torch.arange(0, ROWS + 1, dtype=torch.int64, device="cuda")
    indices = torch.zeros(ROWS, dtype=torch.int32, device="cuda")
    host_out = np.full(ROWS * k, 7.0, np.float32)
    rounds = np.array([1, 2], np.int32)
    form, chunk = C.c_int(-5), C.c_size_t(99)
    calls = {
        "tahoe_forest_predict_accumulate": lambda: lib.tahoe_forest_predict_accumulate(h, out.data_ptr(), x.data_ptr(), ROWS, None),
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
    for fn, call in calls.items():
        assert call() == UNSUPPORTED, fn
        msg = lib.tahoe_last_error().decode()
        assert "vector-leaf" in msg and fn in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and (host_out == 7.0).all()
    assert form.value == 0 and chunk.value == 0  # TAHOE_FORM_NONE
    assert f.staged_strategy(ROWS) == 0
    f.reserve(1 << 20)  # served: nothing to size
    f.check()
    assert np.array_equal(bits(f.predict_raw(x)), bits(shaped(want, k)))  # the handle is as it was
    f.close()


# ------------------------------------------------------------------------------------------------ 5: info, profiling, capture
def test_profiling_info_and_graph_capture(env):
    ta, torch = env
    forest, data, want, _, _ = vr.case("five_k9")
    f = handle(ta, forest)
    x = torch.from_numpy(data.copy()).cuda()
    info = f.info()
    assert info.device_bytes >= 12 * forest["nodes"].size + 4 * forest["trees"].size + 4 * forest["leaves"].size
    assert info.depth == 24 and info.is_sparse == 0 and info.num_trees == 5 and info.num_cols == 8
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


def test_empty_batch(env):
    ta, torch = env
    forest, data, _, _, _ = vr.case("four_k8")
    f = handle(ta, forest)
    x = torch.from_numpy(data.copy()).cuda()
    assert tuple(f.predict_raw(x[:0].contiguous()).shape) == (0, 8)
    f.check()
    f.close()
