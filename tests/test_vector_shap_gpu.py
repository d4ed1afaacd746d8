"""TreeSHAP on vector-leaf handles (tahoe_vector_forest_create_ex with TAHOE_CREATE_CONTRIBS) on the GPU.  Needs an MI355X.

Bitwise: predict_contribs of the native handle against the T x K-tree expansion on tahoe_sparse_forest_create_ex(num_classes = K,
TAHOE_CREATE_CONTRIBS) whose copies of tree t carry tree t's covers (K == 1: the same trees on a sparse handle) -- every forest of
tests/vector_shap_ref.py, both cover generators, batches around the row tiles, three output settings; every class block the
kernel is built for and both ways of running the blocks; a row alone, an unaligned input, two calls, a graph replay.
Accuracy: against the float64 brute force within the bar tests/test_sparse_shap_gpu.py uses, built the same way on the expansion:
gamma x (sum over paths of |leaf| x path length), gamma = (paths + 4 (depth + 2)) 2^-24, divided by T with AVG; local accuracy
against the handle's own margins within that test's expression.
Shapes: the forests are small on purpose -- rows around the 64-row tile, K on both sides of the 8-class block, 700 columns for the
smallest tiles, a chain whose bins add in several rounds, covers of 0 and below the 2^-121 cut."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_shap_ref as ssr  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = vsr.MISSING
ROWS = vsr.ROWS
BATCHES = (1, 63, 64, 65, 257)
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 7
U = 2.0 ** -24
KNOBS = ("TAHOE_VECTOR_SHAP_KB", "TAHOE_VECTOR_SHAP_GRID")


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def native(ta, forest, covers=None, contribs=True, **kw):
    return ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=MISSING, covers=covers,
                           contribs=contribs, **kw)


def expansion(ta, forest, covers=None, contribs=True, **kw):
    """The T x K-tree expansion on tahoe_sparse_forest_create_ex(num_classes = K); every copy of tree t carries tree t's covers"""
    nodes, trees = vr.expand(forest)
    kw.setdefault("threshold", 0.5)
    return ta.capi.SparseForest(nodes, trees, forest["cols"], missing=MISSING, num_classes=forest["k"],
                                covers=None if covers is None else vsr.tile_covers(forest, covers), contribs=contribs, **kw)


def out_bits(ta, output):
    out = 0
    for o in output.split("|"):
        out |= getattr(ta, "OUT_" + o)
    return out


def phi_shape(forest, rows):
    return (rows,) + ((forest["k"],) if forest["k"] > 1 else ()) + (forest["cols"] + 1,)


# ------------------------------------------------------------------------------------------------ 1: the expansion's bits
@pytest.mark.parametrize("name,label", vsr.cover_cases())
def test_contribs_equal_the_expansion_bit_for_bit(env, name, label):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cv = covers[label]
    x = torch.from_numpy(data.copy()).cuda()
    for output in ("RAW", "AVG", "AVG|SIGMOID"):
        kw = dict(output=out_bits(ta, output), global_bias=0.375)
        f, g = native(ta, forest, cv, **kw), expansion(ta, forest, cv, **kw)
        for r in BATCHES:
            xr = x[:r].contiguous()
            a, b = f.predict_contribs(xr), g.predict_contribs(xr)
            assert tuple(a.shape) == tuple(b.shape) == phi_shape(forest, r)
            assert np.array_equal(bits(a), bits(b)), (output, r)
        assert np.isfinite(a.cpu().numpy()).all()
        f.check()
        f.close()
        g.close()


@pytest.mark.parametrize("name", ["nine_k17", "five_k9", "four_k8", "stump_k3", "nine_k1", "wide_k9", "repeat_k3"])
def test_class_block_and_grid_change_no_bit(env, monkeypatch, name):
    """Every vector_contribs_kernel<KB>, with the class blocks in a workgroup's loop and over gridDim.y (the knobs are read at
    create)"""
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cv = next(iter(covers.values()))
    x = torch.from_numpy(data.copy()).cuda()
    kw = dict(output=ta.OUT_AVG, global_bias=-0.25)
    g = expansion(ta, forest, cv, **kw)
    want = bits(g.predict_contribs(x))
    g.close()
    for kb in (1, 2, 4, 8):
        for grid in (0, 1):
            monkeypatch.setenv("TAHOE_VECTOR_SHAP_KB", str(kb))
            monkeypatch.setenv("TAHOE_VECTOR_SHAP_GRID", str(grid))
            f = native(ta, forest, cv, **kw)
            assert np.array_equal(bits(f.predict_contribs(x)), want), (kb, grid)
            assert np.array_equal(bits(f.predict_contribs(x[:65].contiguous())), want[:65]), (kb, grid)
            f.check()
            f.close()


# ------------------------------------------------------------------------------------------------ 2: accuracy
@pytest.mark.parametrize("name", vsr.SMALL)
def test_contribs_against_the_float64_brute_force(env, name):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    K, F, T = forest["k"], forest["cols"], forest["trees"].size
    rows = 65
    x = data[:rows]
    xd = torch.from_numpy(x.copy()).cuda()
    sn, tr = vr.expand(forest)
    scale, depth, paths = ssr.bound_scale(sn, tr, K)
    gamma = (paths + 4 * (depth + 2)) * U
    for label, cv in covers.items():
        raw = vsr.contribs(forest, cv, x)  # float64, RAW and no bias: AVG and the bias only scale and shift it
        for avg, bias in ((False, 0.125), (True, -0.5)):
            out = ta.OUT_AVG if avg else 0
            tol = gamma * scale / (T if avg and T else 1)  # [K]
            want = raw / (T if avg and T else 1)
            f = native(ta, forest, cv, output=out, global_bias=bias)
            phi = f.predict_contribs(xd).cpu().numpy().reshape(rows, K, F + 1)
            err = np.abs(phi[:, :, :F].astype(np.float64) - want[:, :, :F])
            print(f"{name} {label} avg={avg}: max err {err.max() if err.size else 0.0:.3e}, bar {tol.max():.3e}")
            assert np.all(err <= tol[None, :, None]), f"{name} {label}: contribs max err {err.max():.3e} > {tol.max():.3e}"
            b = vsr.bias_column(forest, cv, avg, bias)
            assert np.array_equal(bits(phi[:, :, F]), bits(np.broadcast_to(b, (rows, K)))), (name, label, avg)
            # local accuracy against the handle's own margins (predict divides by T with AVG: no trees, no margin to meet)
            if T or not avg:
                m = native(ta, forest, None, contribs=False, output=out, global_bias=bias)
                margin = m.predict(xd).cpu().numpy().astype(np.float64).reshape(rows, K)
                assert np.all(np.abs(phi.astype(np.float64).sum(-1) - margin) <= 2 * tol[None, :] + 1e-5 * np.abs(margin) + 1e-6), (name, label, avg)
                m.close()
            f.check()
            f.close()


# ------------------------------------------------------------------------------------------------ 3: determinism
@pytest.mark.parametrize("name", ["five_k9", "nine_k1", "repeat_k3"])
def test_two_calls_a_row_alone_and_the_strategy(env, name):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cv = next(iter(covers.values()))
    f = native(ta, forest, cv, output=ta.OUT_AVG, global_bias=0.5)
    x = torch.from_numpy(data.copy()).cuda()
    batch = bits(f.predict_contribs(x))
    assert np.array_equal(bits(f.predict_contribs(x)), batch)
    for r in (0, 63, 64, 200, ROWS - 1):
        assert np.array_equal(bits(f.predict_contribs(x[r:r + 1].clone()))[0], batch[r]), r
    for strat in ("DIRECT", "ROWTILE"):  # the call does not use the strategy
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert np.array_equal(bits(f.predict_contribs(x)), batch), strat
    f.check()
    f.close()


@pytest.mark.parametrize("name", ["four_k8", "nine_k1"])
def test_rows_one_float_off_a_16_byte_boundary(env, name):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cols = forest["cols"]
    assert cols % 4 == 0
    f = native(ta, forest, covers["consistent"])
    aligned = torch.from_numpy(data.copy()).cuda()
    buf = torch.full((ROWS * cols + 4,), float("nan"), device="cuda")
    x = buf[1:1 + ROWS * cols].view(ROWS, cols)
    x.copy_(aligned)
    assert x.is_contiguous() and buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 4
    assert np.array_equal(bits(f.predict_contribs(x)), bits(f.predict_contribs(aligned)))
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------------ 4: capture, device bytes
def test_graph_capture_and_device_bytes(env):
    ta, torch = env
    forest, data, covers = vsr.case("five_k9")
    cv, K, cols = covers["consistent"], forest["k"], forest["cols"]
    f, plain = native(ta, forest, cv), native(ta, forest, None, contribs=False)
    x = torch.from_numpy(data.copy()).cuda()
    want = bits(f.predict_contribs(x))

    nb = len(vsr.bins(forest))
    assert nb > 4
    table = nb * 64 * 20 + nb * 4 + K * 4  # elements (16 B) and 1 - z per lane, bin_info, the bias column
    assert f.info().device_bytes - plain.info().device_bytes == table
    g, g_plain = expansion(ta, forest, cv), expansion(ta, forest, None, contribs=False)
    assert g.info().device_bytes - g_plain.info().device_bytes > K * nb * 64 * 20 > table
    for h in (plain, g, g_plain):
        h.close()

    out = torch.empty(phi_shape(forest, ROWS), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f.predict_contribs(x, out=out)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f.predict_contribs(x, out=out)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), want)
        out.zero_()
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------------ 5: edge forests
def test_a_root_leaf_tree_adds_only_to_the_bias(env):
    ta, torch = env
    forest, data, covers = vsr.case("single_leaf_k1")
    f = native(ta, forest, covers["unrelated"], global_bias=0.25)
    phi = f.predict_contribs(torch.from_numpy(data.copy()).cuda()).cpu().numpy()
    leaf = forest["leaves"][forest["nodes"]["left_idx"][0], 0]
    assert phi.shape == (ROWS, 2) and not bits(phi[:, 0]).any()
    assert np.array_equal(bits(phi[:, 1]), bits(np.full(ROWS, np.float32(float(leaf) + 0.25), np.float32)))
    f.close()
    # ... and beside other trees: taking the root-leaf tree out changes the bias column alone
    forest, data, covers = vsr.case("three_k1")
    cv = covers["consistent"]
    assert forest["nodes"]["bits"][forest["trees"][2]] < 0 and forest["trees"].size == 3
    last = int(forest["trees"][2])
    without = dict(forest, nodes=forest["nodes"][:last], trees=forest["trees"][:2])
    x = torch.from_numpy(data.copy()).cuda()
    f, g = native(ta, forest, cv), native(ta, without, cv[:last])
    a, b = f.predict_contribs(x).cpu().numpy(), g.predict_contribs(x).cpu().numpy()
    assert np.array_equal(bits(a[:, :-1]), bits(b[:, :-1])) and not np.array_equal(bits(a[:, -1]), bits(b[:, -1]))
    f.close()
    g.close()


@pytest.mark.parametrize("name", ["zero_side_k3", "tiny_ratio_k3"])
def test_extreme_covers_give_finite_values_with_the_expansions_bits(env, name):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cv = covers["fixed"]
    x = torch.from_numpy(data.copy()).cuda()
    f, g = native(ta, forest, cv), expansion(ta, forest, cv)
    a = f.predict_contribs(x)
    assert np.isfinite(a.cpu().numpy()).all() and a.abs().max().item() > 0
    assert np.array_equal(bits(a), bits(g.predict_contribs(x)))
    f.check()
    f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ 6: refusals
@pytest.mark.parametrize("flagged", [True, False])
def test_unserved_calls_are_refused(env, flagged):
    ta, torch = env
    forest, data, covers = vsr.case("five_k9")
    cols, k = forest["cols"], forest["k"]
    f = native(ta, forest, covers["consistent"], contribs=flagged)
    x = torch.from_numpy(data.copy()).cuda()
    lib, h = ta.lib, f._h
    out = torch.full((ROWS * k * (cols + 1) * (cols + 1),), 7.0, device="cuda")
    calls = {
        "tahoe_forest_predict_interactions": lambda: lib.tahoe_forest_predict_interactions(h, out.data_ptr(), x.data_ptr(), ROWS, None),
        "tahoe_forest_predict_contribs_interventional":
            lambda: lib.tahoe_forest_predict_contribs_interventional(h, out.data_ptr(), x.data_ptr(), ROWS, None),
        "tahoe_forest_predict_contribs_approx": lambda: lib.tahoe_forest_predict_contribs_approx(h, out.data_ptr(), x.data_ptr(), ROWS, None),
        "tahoe_forest_set_background": lambda: lib.tahoe_forest_set_background(h, x.data_ptr(), ROWS, None),
    }
    if not flagged:
        calls["tahoe_forest_predict_contribs"] = lambda: lib.tahoe_forest_predict_contribs(h, out.data_ptr(), x.data_ptr(), ROWS, None)
    for fn, call in calls.items():
        assert call() == UNSUPPORTED, fn
        msg = lib.tahoe_last_error().decode()
        assert "vector-leaf" in msg and fn in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    if flagged:
        assert lib.tahoe_forest_predict_contribs(h, None, None, 0, None) == OK  # rows == 0
        assert lib.tahoe_forest_predict_contribs(h, None, x.data_ptr(), ROWS, None) == INVALID_ARG
        assert "null argument" in lib.tahoe_last_error().decode()
        assert lib.tahoe_forest_predict_contribs(h, out.data_ptr(), None, ROWS, None) == INVALID_ARG
        assert lib.tahoe_forest_predict_contribs(h, out.data_ptr(), x.data_ptr(), C.c_size_t(1 << 62).value, None) == INVALID_ARG
        assert "overflow" in lib.tahoe_last_error().decode()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
        assert tuple(f.predict_contribs(x[:0].contiguous()).shape) == (0, k, cols + 1)
    f.check()
    f.close()


def test_contribs_without_covers_raises_as_the_sparse_handle_does(env):
    ta, _ = env
    forest, _, _ = vsr.case("four_k8")
    with pytest.raises(ta.TahoeError) as e:
        native(ta, forest, None, contribs=True)
    assert e.value.status == INVALID_ARG and "needs covers" in str(e.value)
    nodes, trees = vr.expand(forest)
    with pytest.raises(ta.TahoeError) as e2:
        ta.capi.SparseForest(nodes, trees, forest["cols"], num_classes=forest["k"], contribs=True)
    assert e2.value.status == e.value.status
