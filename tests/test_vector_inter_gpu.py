"""SHAP interaction values on vector-leaf handles (tahoe_vector_forest_create_ex with TAHOE_CREATE_CONTRIBS |
TAHOE_CREATE_VECTOR_INTERACTIONS) on the GPU.  Needs an MI355X.

Bitwise: predict_interactions of the native handle against the T x K-tree expansion on tahoe_sparse_forest_create_ex(num_classes =
K, TAHOE_CREATE_CONTRIBS) whose copies of tree t carry tree t's covers (K == 1: the same trees on a sparse handle) -- every forest
of tests/vector_shap_ref.py, both cover generators, batches around the row tile, three output settings; wide_k9 (700 columns)
runs the in-place form at 1 and 5 rows, every other forest the LDS triangles; every class block the kernel is built for and both
ways of running the blocks on one forest of each form.  The matrix: exactly symmetric, the diagonal phi_i minus the row's
off-diagonal float32 sum in ascending order, row and column num_cols +0.0 but the corner, the corner predict_contribs' bias.  A row
alone, two calls, an unaligned input, a graph replay, device_bytes of the handle without the flag, refusals that launch nothing.
Accuracy: off the diagonal against the float64 recursion of tests/vector_inter_ref.py (held to the brute force on the expansion
to 1e-12 by tests/test_vector_inter_ref.py) within the interactions bar of tests/test_sparse_shap_gpu.py, built the same way on
the expansion: 2 gamma x (sum over paths of |leaf| x path length), gamma = (paths + 4 (depth + 2)) 2^-24, divided by T with AVG.
The test prints the largest error as a fraction of the bar (DESIGN.md section 28 records it)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_shap_ref as ssr  # noqa: E402
import vector_inter_ref as vir  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = vsr.MISSING
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 7
U = 2.0 ** -24
KNOBS = ("TAHOE_VECTOR_SHAP_KB", "TAHOE_VECTOR_SHAP_GRID")
SLAB_FOREST, INPLACE_FOREST = "nine_k17", "wide_k9"


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


def native(ta, forest, covers=None, interactions=True, **kw):
    return ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=MISSING, covers=covers,
                           interactions=interactions, **kw)


def expansion(ta, forest, covers, **kw):
    """The T x K-tree expansion on tahoe_sparse_forest_create_ex(num_classes = K); every copy of tree t carries tree t's covers"""
    nodes, trees = vr.expand(forest)
    kw.setdefault("threshold", 0.5)
    return ta.capi.SparseForest(nodes, trees, forest["cols"], missing=MISSING, num_classes=forest["k"],
                                covers=vsr.tile_covers(forest, covers), contribs=True, **kw)


def out_bits(ta, output):
    out = 0
    for o in output.split("|"):
        out |= getattr(ta, "OUT_" + o)
    return out


def mat_shape(forest, rows):
    return (rows,) + ((forest["k"],) if forest["k"] > 1 else ()) + (forest["cols"] + 1,) * 2


def row_counts(forest):
    if forest["cols"] > 71:
        return (1, 5)
    return tuple(vir.batches(forest["cols"], forest["k"])) + (65,)


# ------------------------------------------------------------------------------------------------ 1: the expansion's bits
@pytest.mark.parametrize("name,label", vsr.cover_cases())
def test_interactions_equal_the_expansion_bit_for_bit(env, name, label):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cv = covers[label]
    slabs = vir.shape(forest["cols"], forest["k"])[0]
    assert slabs == (name != "wide_k9")
    x = torch.from_numpy(data[:65].copy()).cuda()
    for output in ("RAW", "AVG", "AVG|SIGMOID"):
        kw = dict(output=out_bits(ta, output), global_bias=0.375)
        f, g = native(ta, forest, cv, **kw), expansion(ta, forest, cv, **kw)
        for r in row_counts(forest):
            xr = x[:r].contiguous()
            a, b = f.predict_interactions(xr), g.predict_interactions(xr)
            assert tuple(a.shape) == tuple(b.shape) == mat_shape(forest, r)
            assert np.array_equal(bits(a), bits(b)), (output, r)
            del a, b
        # predict_contribs keeps its bits beside the new call
        assert np.array_equal(bits(f.predict_contribs(x)), bits(g.predict_contribs(x))), output
        f.check()
        f.close()
        g.close()


@pytest.mark.parametrize("name", [SLAB_FOREST, INPLACE_FOREST])
def test_class_block_and_grid_change_no_bit(env, monkeypatch, name):
    """Every vector_interactions_kernel<KB, form>, with the class blocks in a workgroup's loop and over gridDim.y (the knobs are
    read at create)"""
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cv = next(iter(covers.values()))
    rows = row_counts(forest)[-2]  # 33 (slabs), 1 (in place) ...
    rows = max(rows, 5)            # ... at least 5: more rows than waves in place
    x = torch.from_numpy(data[:rows].copy()).cuda()
    kw = dict(output=ta.OUT_AVG, global_bias=-0.25)
    g = expansion(ta, forest, cv, **kw)
    want = bits(g.predict_interactions(x))
    g.close()
    for kb in (1, 2, 4, 8):
        assert vir.shape(forest["cols"], forest["k"], kb)[1] == kb  # the forced block leaves a row
        for grid in (0, 1):
            monkeypatch.setenv("TAHOE_VECTOR_SHAP_KB", str(kb))
            monkeypatch.setenv("TAHOE_VECTOR_SHAP_GRID", str(grid))
            f = native(ta, forest, cv, **kw)
            assert np.array_equal(bits(f.predict_interactions(x)), want), (kb, grid)
            f.check()
            f.close()


# ------------------------------------------------------------------------------------------------ 2: the matrix
@pytest.mark.parametrize("name", ["five_k9", "nine_k1", "repeat_k3", "wide_k9"])
def test_symmetry_diagonal_and_the_bias_row(env, name):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cv = next(iter(covers.values()))
    K, F = forest["k"], forest["cols"]
    rows = 5 if F > 71 else 33
    x = torch.from_numpy(data[:rows].copy()).cuda()
    f = native(ta, forest, cv, output=ta.OUT_AVG, global_bias=0.5)
    m = f.predict_interactions(x).cpu().numpy().reshape(rows, K, F + 1, F + 1)
    phi = f.predict_contribs(x).cpu().numpy().reshape(rows, K, F + 1)
    f.check()
    f.close()
    assert np.array_equal(bits(m), bits(m.transpose(0, 1, 3, 2)))  # exactly symmetric
    assert not bits(m[:, :, F, :F]).any() and not bits(m[:, :, :F, F]).any()  # +0.0f, sign included
    assert np.array_equal(bits(m[:, :, F, F]), bits(phi[:, :, F]))
    # diagonal: phi_i - (the row's off-diagonal sum, ascending from 0.0f), all in float32
    body = m[:, :, :F, :F]
    acc = np.zeros((rows, K, F), np.float32)
    idx = np.arange(F)
    for j in range(F):
        acc = np.where(idx != j, acc + body[:, :, :, j], acc).astype(np.float32)
    diag = body[:, :, idx, idx]
    assert np.array_equal(bits(diag), bits((phi[:, :, :F] - acc).astype(np.float32)))
    assert np.abs(body).max() > 0


# ------------------------------------------------------------------------------------------------ 3: accuracy
@pytest.mark.parametrize("name", vsr.SMALL)
def test_interactions_against_the_float64_reference(env, name):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    K, F, T = forest["k"], forest["cols"], forest["trees"].size
    rows = 33
    x = data[:rows]
    xd = torch.from_numpy(x.copy()).cuda()
    sn, tr = vr.expand(forest)
    scale, depth, paths = ssr.bound_scale(sn, tr, K)
    gamma = (paths + 4 * (depth + 2)) * U
    off = ~np.eye(F, dtype=bool)
    for label, cv in covers.items():
        raw = vir.interactions(forest, cv, x)  # float64, RAW: AVG only divides it
        for avg, bias in ((False, 0.125), (True, -0.5)):
            tol = gamma * scale / (T if avg and T else 1)  # [K]: the contribs bar; interactions are held to twice it
            want = raw / (T if avg and T else 1)
            f = native(ta, forest, cv, output=ta.OUT_AVG if avg else 0, global_bias=bias)
            m = f.predict_interactions(xd).cpu().numpy().reshape(rows, K, F + 1, F + 1)
            f.check()
            f.close()
            err = np.abs(m[:, :, :F, :F].astype(np.float64) - want)[:, :, off].reshape(rows, K, -1)
            frac = (err / np.maximum(2 * tol, 1e-300)[None, :, None]).max() if err.size else 0.0
            print(f"{name} {label} avg={avg}: max err {err.max() if err.size else 0.0:.3e}, bar {2 * tol.max():.3e}, "
                  f"largest fraction of the bar {frac:.4f}")
            assert np.all(err <= 2 * tol[None, :, None]), f"{name} {label}: interactions max err {err.max():.3e} > {2 * tol.max():.3e}"


# ------------------------------------------------------------------------------------------------ 4: determinism
@pytest.mark.parametrize("name", ["five_k9", "nine_k1", "wide_k9"])
def test_two_calls_and_a_row_alone(env, name):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cv = next(iter(covers.values()))
    rows = 6 if forest["cols"] > 71 else 65
    f = native(ta, forest, cv, output=ta.OUT_AVG, global_bias=0.5)
    x = torch.from_numpy(data[:rows].copy()).cuda()
    batch = bits(f.predict_interactions(x))
    assert np.array_equal(bits(f.predict_interactions(x)), batch)
    for r in (0, 3, 4, rows - 1):
        assert np.array_equal(bits(f.predict_interactions(x[r:r + 1].clone()))[0], batch[r]), r
    for strat in ("DIRECT", "ROWTILE") if forest["cols"] <= 640 else ("DIRECT",):  # the call does not use the strategy
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert np.array_equal(bits(f.predict_interactions(x)), batch), strat
    f.check()
    f.close()


@pytest.mark.parametrize("name", ["four_k8", "nine_k1"])
def test_rows_one_float_off_a_16_byte_boundary(env, name):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cols, rows = forest["cols"], 33
    assert cols % 4 == 0
    f = native(ta, forest, covers["consistent"])
    aligned = torch.from_numpy(data[:rows].copy()).cuda()
    buf = torch.full((rows * cols + 4,), float("nan"), device="cuda")
    x = buf[1:1 + rows * cols].view(rows, cols)
    x.copy_(aligned)
    assert x.is_contiguous() and buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 4
    assert np.array_equal(bits(f.predict_interactions(x)), bits(f.predict_interactions(aligned)))
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------------ 5: capture, device bytes
def test_graph_capture_and_device_bytes(env):
    ta, torch = env
    forest, data, covers = vsr.case("five_k9")
    cv, rows = covers["consistent"], 33
    f = native(ta, forest, cv)
    plain = ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=MISSING, covers=cv,
                            contribs=True)
    both = native(ta, forest, cv, interventional=True)
    iv = ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=MISSING, covers=cv,
                         contribs=True, interventional=True)
    assert f.info().device_bytes == plain.info().device_bytes  # no table of its own
    assert both.info().device_bytes == iv.info().device_bytes
    x = torch.from_numpy(data[:rows].copy()).cuda()
    want = bits(f.predict_interactions(x))
    assert np.array_equal(bits(both.predict_interactions(x)), want)
    # the handle without the flag is what it was: same contributions, and it refuses the call (test 6)
    assert np.array_equal(bits(f.predict_contribs(x)), bits(plain.predict_contribs(x)))
    for h in (plain, both, iv):
        h.close()

    out = torch.empty(mat_shape(forest, rows), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f.predict_interactions(x, out=out)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f.predict_interactions(x, out=out)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), want)
        out.zero_()
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------------ 6: refusals
@pytest.mark.parametrize("flags", ["contribs", "interventional", "contribs+interventional", "none"])
def test_handles_without_the_flag_refuse_and_launch_nothing(env, flags):
    ta, torch = env
    forest, data, covers = vsr.case("five_k9")
    cols, k, rows = forest["cols"], forest["k"], 9
    f = ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=MISSING,
                        covers=covers["consistent"], contribs="contribs" in flags, interventional="interventional" in flags)
    x = torch.from_numpy(data[:rows].copy()).cuda()
    out = torch.full((rows * k * (cols + 1) * (cols + 1),), 7.0, device="cuda")
    assert ta.lib.tahoe_forest_predict_interactions(f._h, out.data_ptr(), x.data_ptr(), rows, None) == UNSUPPORTED
    msg = ta.lib.tahoe_last_error().decode()
    assert "vector-leaf" in msg and "tahoe_forest_predict_interactions" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    f.check()
    f.close()


def test_entry_checks_of_the_served_call(env):
    ta, torch = env
    forest, data, covers = vsr.case("five_k9")
    cols, k, rows = forest["cols"], forest["k"], 9
    f = native(ta, forest, covers["consistent"])
    x = torch.from_numpy(data[:rows].copy()).cuda()
    lib, h = ta.lib, f._h
    out = torch.full((rows * k * (cols + 1) * (cols + 1),), 7.0, device="cuda")
    assert lib.tahoe_forest_predict_interactions(h, None, None, 0, None) == OK  # rows == 0 comes first
    assert lib.tahoe_forest_predict_interactions(h, None, x.data_ptr(), rows, None) == INVALID_ARG
    assert "null argument" in lib.tahoe_last_error().decode()
    assert lib.tahoe_forest_predict_interactions(h, out.data_ptr(), None, rows, None) == INVALID_ARG
    assert lib.tahoe_forest_predict_interactions(h, out.data_ptr(), x.data_ptr(), C.c_size_t(1 << 62).value, None) == INVALID_ARG
    assert "overflow" in lib.tahoe_last_error().decode()
    # the calls the handle does not serve keep their refusal
    for fn in ("tahoe_forest_predict_contribs_approx", "tahoe_forest_predict_contribs_interventional"):
        assert getattr(lib, fn)(h, out.data_ptr(), x.data_ptr(), rows, None) == UNSUPPORTED, fn
        msg = lib.tahoe_last_error().decode()
        assert "vector-leaf" in msg and fn in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert tuple(f.predict_interactions(x[:0].contiguous()).shape) == (0, k, cols + 1, cols + 1)
    f.check()
    f.close()


def test_interactions_without_covers_raises(env):
    ta, _ = env
    forest, _, _ = vsr.case("four_k8")
    with pytest.raises(ta.TahoeError) as e:
        native(ta, forest, None)
    assert e.value.status == INVALID_ARG and "needs covers" in str(e.value)
