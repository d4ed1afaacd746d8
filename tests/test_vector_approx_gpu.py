"""Saabas contributions on vector-leaf handles (tahoe_vector_forest_create_ex with TAHOE_CREATE_VECTOR_APPROX) on the GPU.  Needs
an MI355X.  Every test creates a handle with the flag, which the library refused before the flag existed.

Bitwise throughout: predict_contribs_approx of the native handle against tests/vector_approx_ref.py (the definition in numpy) and
against the T x K-tree expansion on tahoe_sparse_forest_create_ex(num_classes = K, TAHOE_CREATE_APPROX_CONTRIBS) whose copies of
tree t carry tree t's covers (K == 1: the same trees).  A NaN need only be a NaN at the same place (shap_edges.assert_same_bits).
Every call of the native handle goes through run(): it writes into the head of a buffer 256 rows longer whose tail must come back
untouched.  Shapes are small on purpose: rows around one and two workgroups, K on both sides of every class block, num_cols on
both sides of the form rule's edge."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shap_edges as se  # noqa: E402
import vector_approx_ref as var  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = vr.MISSING
ROWS = vr.ROWS
BATCHES = (1, 63, 64, 65, 129, 257)
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 7
U = 2.0 ** -24
KNOBS = ("TAHOE_VECTOR_SHAP_KB", "TAHOE_APPROX_FORM", "TAHOE_VECTOR_SHAP_GRID")
GUARD_ROWS = 256
GUARD = np.float32(-12345.678)
FN = "tahoe_forest_predict_contribs_approx"


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    n = C.c_int(0)
    assert ta.lib.tahoe_device_lds_bytes(C.byref(n)) == 0 and n.value == var.LDS_LIMIT
    return ta, torch


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def native(ta, forest, covers, missing=MISSING, approx=True, **kw):
    return ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=missing, covers=covers,
                           approx_contribs=approx, **kw)


def expansion(ta, forest, covers, missing=MISSING, **kw):
    nodes, trees = vr.expand(forest)
    kw.setdefault("threshold", 0.5)
    return ta.capi.SparseForest(nodes, trees, forest["cols"], missing=missing, num_classes=forest["k"],
                                covers=vsr.tile_covers(forest, covers), approx_contribs=True, **kw)


def run(env, f, x):
    """predict_contribs_approx of x (numpy or device tensor) into the head of a guarded buffer -> numpy [rows, K, cols + 1]"""
    ta, torch = env
    xd = x if hasattr(x, "is_cuda") else torch.from_numpy(np.array(x, np.float32)).cuda()
    n, K, F1 = xd.shape[0], f.num_classes, f.num_cols + 1
    shape = (n + GUARD_ROWS,) + ((K,) if K > 1 else ()) + (F1,)
    big = torch.full(shape, float(GUARD), device="cuda")
    out = f.predict_contribs_approx(xd, out=big[:n])
    assert tuple(out.shape) == (n,) + shape[1:]
    torch.cuda.synchronize()
    a = big.cpu().numpy().reshape(n + GUARD_ROWS, K, F1)
    assert not (bits(a[n:]) != bits(GUARD)).any(), f"values written past the batch's {n} rows"
    return a[:n]


def same(got, want, label):
    se.assert_same_bits(got, np.asarray(want).reshape(got.shape), label)


def settings(ta):
    return ((0, 0.0), (ta.OUT_AVG, 0.375))


# ------------------------------------------------------------------------------------- 1: named cases, batch sizes, the expansion
@pytest.mark.parametrize("name", ["five_k9", "four_k8", "wide_k9", "repeat_k3", "zero_side_k3", "tiny_ratio_k3", "nine_k1"])
def test_named_cases_equal_the_reference_and_the_expansion(env, name):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    for label, cv in covers.items():
        for output, gb in settings(ta):
            want = var.contribs(forest, cv, data, avg=bool(output), global_bias=gb)
            f, g = native(ta, forest, cv, output=output, global_bias=gb), expansion(ta, forest, cv, output=output, global_bias=gb)
            for r in BATCHES:
                got = run(env, f, data[:r])
                same(got, want[:r], f"{name} {label} out={output} rows={r}: reference")
                same(got, g.predict_contribs_approx(torch.from_numpy(data[:r].copy()).cuda()).cpu().numpy(),
                     f"{name} {label} out={output} rows={r}: expansion")
            f.check()
            f.close()
            g.close()


# ------------------------------------------------------------------------------------- 2: class blocks
@pytest.mark.parametrize("K", [1, 3, 8, 9, 17])
def test_partial_class_blocks(env, K):
    ta, torch = env
    forest, data, cv = var.k_case(K)
    for output, gb in settings(ta):
        f, g = native(ta, forest, cv, output=output, global_bias=gb), expansion(ta, forest, cv, output=output, global_bias=gb)
        got = run(env, f, data)
        same(got, var.contribs(forest, cv, data, avg=bool(output), global_bias=gb), f"K={K}: reference")
        same(got, g.predict_contribs_approx(torch.from_numpy(data.copy()).cuda()).cpu().numpy(), f"K={K}: expansion")
        f.check()
        f.close()
        g.close()


def test_k_1023_at_three_columns(env):
    ta, torch = env
    forest, data, cv = var.k_case(1023, cols=3, kinds=(3, "stump", 2))
    f, g = native(ta, forest, cv, output=ta.OUT_AVG), expansion(ta, forest, cv, output=ta.OUT_AVG)
    got = run(env, f, data[:65])
    same(got, var.contribs(forest, cv, data[:65], avg=True), "K=1023: reference")
    same(got, g.predict_contribs_approx(torch.from_numpy(data[:65].copy()).cuda()).cpu().numpy(), "K=1023: expansion")
    f.check()
    f.close()
    g.close()


@pytest.mark.parametrize("T", [0, 1, 3, 5])
def test_tree_counts(env, T):
    ta, _ = env
    forest, data, cv = var.k_case(9, kinds=(4, "stump", 5, "leaf", 3)[:T], seed=7200)
    for output, gb in settings(ta):
        f = native(ta, forest, cv, output=output, global_bias=gb)
        same(run(env, f, data), var.contribs(forest, cv, data, avg=bool(output), global_bias=gb), f"T={T} out={output}")
        f.check()
        f.close()


def test_single_leaf_trees_add_nothing(env):
    ta, _ = env
    forest, data, cv = var.leaves_only_case()
    for output, gb in settings(ta):
        f = native(ta, forest, cv, output=output, global_bias=gb)
        got = run(env, f, data)
        assert not bits(got[:, :, :-1]).any(), "zeros in every bit"
        b = vsr.bias_column(forest, cv, bool(output), gb)
        assert np.array_equal(bits(got[:, :, -1]), bits(np.broadcast_to(b, got.shape[:2])))
        f.close()


def test_a_depth_300_vine_beside_a_stump_and_a_leaf(env):
    ta, torch = env
    forest, data, cv = var.vine_case()
    f, g = native(ta, forest, cv), expansion(ta, forest, cv)
    got = run(env, f, data)
    same(got, var.contribs(forest, cv, data), "vine: reference")
    same(got, g.predict_contribs_approx(torch.from_numpy(data.copy()).cuda()).cpu().numpy(), "vine: expansion")
    f.check()
    f.close()
    g.close()


# ------------------------------------------------------------------------------------- 3: forms
@pytest.mark.parametrize("K,cols", [(9, 8), (17, 5), (9, 64), (3, 318)])
def test_class_block_and_form_knobs_change_no_bit(env, monkeypatch, K, cols):
    ta, _ = env
    forest, data, cv = var.k_case(K, cols=cols, rows=var.WIDE_ROWS)
    f = native(ta, forest, cv, output=ta.OUT_AVG, global_bias=-0.25)
    want = run(env, f, data)
    same(want, var.contribs(forest, cv, data, avg=True, global_bias=-0.25), "unforced: reference")
    f.close()
    for kb in (1, 2, 4, 8):
        for form in (1, 2):
            for grid in (1, 0):
                for k, v in zip(KNOBS, (kb, form, grid)):
                    monkeypatch.setenv(k, str(v))
                f = native(ta, forest, cv, output=ta.OUT_AVG, global_bias=-0.25)
                w = var.form_rule(cols, K, kb, form)[2]
                for r in (1, 64 * w - 1, 64 * w + 1, 128 * w + 1):
                    same(run(env, f, data[:r]), want[:r], f"KB={kb} form={form} grid={grid} rows={r}")
                f.check()
                f.close()


def test_form_rule_edges_are_where_the_helper_says(env):
    """The widths the next test runs at: the last slab width, the first in-place width, one either side"""
    assert [var.form_rule(c, 9)[1] for c in (317, 318, 319, 320)] == [True, True, False, False]
    assert var.form_rule(318, 9) == (1, True, 1) and var.form_rule(319, 9) == (4, False, 4) and var.form_rule(1, 9) == (8, True, 4)


@pytest.mark.parametrize("cols", [1, 317, 318, 319, 320])
def test_num_cols_at_the_edges_of_the_form_rule(env, cols):
    ta, _ = env
    forest, data, cv = var.wide_case(cols)
    w = var.form_rule(cols, forest["k"])[2]
    want = var.contribs(forest, cv, data, avg=True, global_bias=0.5)
    f = native(ta, forest, cv, output=ta.OUT_AVG, global_bias=0.5)
    for r in (1, 64 * w - 1, 64 * w + 1, 128 * w + 1):
        same(run(env, f, data[:r]), want[:r], f"cols={cols} rows={r}")
    f.check()
    f.close()


# ------------------------------------------------------------------------------------- 4: the branch rule
@pytest.mark.parametrize("missing", list(se.MISSINGS))
def test_branch_rule_on_the_edge_pools(env, missing):
    ta, torch = env
    m = se.MISSINGS[missing]
    forest, data, cv = var.pool_case(m)
    f, g = native(ta, forest, cv, missing=m), expansion(ta, forest, cv, missing=m)
    got = run(env, f, data)
    same(got, var.contribs(forest, cv, data, missing=m), f"missing={missing}: reference")
    same(got, g.predict_contribs_approx(torch.from_numpy(data.copy()).cuda()).cpu().numpy(), f"missing={missing}: expansion")
    f.check()
    f.close()
    g.close()


# ------------------------------------------------------------------------------------- 5: values
def test_subnormal_deltas_are_not_flushed(env):
    ta, _ = env
    forest, data, cv = var.value_case("subnormal")
    for output, gb in ((0, 0.0), (ta.OUT_AVG, 0.0)):
        want = var.contribs(forest, cv, data, avg=bool(output))
        feats = want[:, :, :-1]
        assert np.any((feats != 0) & (np.abs(feats) < se.FLT_MIN)), "the case has subnormal sums"
        f = native(ta, forest, cv, output=output, global_bias=gb)
        got = run(env, f, data)
        assert np.array_equal(bits(got), bits(want)), f"out={output}"
        f.check()
        f.close()


def test_overflowing_deltas_give_the_references_inf_and_nan(env):
    ta, _ = env
    forest, data, cv = var.value_case("overflow")
    want = var.contribs(forest, cv, data)
    assert np.isinf(want).any() and np.isnan(want).any() and np.isfinite(want).any()
    f = native(ta, forest, cv)
    got = run(env, f, data)
    same(got, want, "overflow")
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])
    f.check()  # no error flag
    same(run(env, f, data), want, "overflow, the next call")
    f.close()
    # ... and the next call of a benign handle is exact
    forest, data, cv = var.k_case(3)
    f = native(ta, forest, cv)
    same(run(env, f, data), var.contribs(forest, cv, data), "after the overflow")
    f.close()


# ------------------------------------------------------------------------------------- 6: properties
def test_bias_column_and_the_other_explanations_on_a_handle_with_every_flag(env):
    ta, torch = env
    forest, data, covers = vsr.case("five_k9")
    cv = covers["consistent"]
    x = torch.from_numpy(data[:65].copy()).cuda()
    kw = dict(contribs=True, interventional=True, interactions=True, output=ta.OUT_AVG, global_bias=0.125)
    f, g = native(ta, forest, cv, **kw), native(ta, forest, cv, approx=False, **kw)
    got = run(env, f, data[:65])
    same(got, var.contribs(forest, cv, data[:65], avg=True, global_bias=0.125), "all flags: reference")
    phi = f.predict_contribs(x).cpu().numpy()
    assert np.array_equal(bits(got[:, :, -1]), bits(phi[:, :, -1])), "bias column against predict_contribs"
    assert np.array_equal(bits(phi), bits(g.predict_contribs(x)))
    assert np.array_equal(bits(f.predict_interactions(x)), bits(g.predict_interactions(x)))
    for h in (f, g):
        h.set_background(x[:20].contiguous())
    assert np.array_equal(bits(f.predict_contribs_interventional(x)), bits(g.predict_contribs_interventional(x)))
    assert np.array_equal(bits(f.predict(x)), bits(g.predict(x)))
    for h in (f, g):
        h.check()
        h.close()


@pytest.mark.parametrize("name", ["five_k9", "nine_k17", "nine_k1"])
def test_rows_sum_to_predict_raw(env, name):
    """The feature columns of a row against the float64 total of the row's exact deltas (vector_approx_ref.direct64) within
    (N + 1) 2^-24 S -- N float32 adds of deltas rounded once, S the sum of |delta| over the adds -- and, with the bias, against
    predict_raw of the same handle within that bound plus what predict_raw and the bias column round themselves: T float32
    adds of leaf values and one rounding of the bias, (T + 1) 2^-24 (sum |leaf| + |bias|)."""
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cv = covers["consistent"]
    T = forest["trees"].size
    f = native(ta, forest, cv)
    got = run(env, f, data).astype(np.float64)
    _, S, N = var.contribs(forest, cv, data, scale=True)
    tol = (N[:, None] + 1) * U * S
    exact = var.direct64(forest, cv, data)[:, :, :-1].sum(-1)
    err = np.abs(got[:, :, :-1].sum(-1) - exact)
    print(f"{name}: features against the float64 deltas: worst {np.max(err / np.maximum(tol, 1e-300)):.3g} of the bound")
    assert np.all(err <= tol)
    raw = f.predict_raw(torch.from_numpy(data.copy()).cuda()).cpu().numpy().reshape(ROWS, -1).astype(np.float64)
    leaf_abs = np.abs(forest["leaves"][forest["nodes"]["left_idx"][forest["nodes"]["bits"] < 0]]).max(0).astype(np.float64) * T
    tol2 = tol + (T + 1) * U * (leaf_abs[None, :] + np.abs(got[:, :, -1]))
    err2 = np.abs(got.sum(-1) - raw)
    print(f"{name}: rows against predict_raw: worst {np.max(err2 / np.maximum(tol2, 1e-300)):.3g} of the bound")
    assert np.all(err2 <= tol2)
    f.close()


def test_a_row_alone_two_calls_the_strategy_and_an_unaligned_input(env):
    ta, torch = env
    forest, data, covers = vsr.case("four_k8")
    cols = forest["cols"]
    f = native(ta, forest, covers["unrelated"], output=ta.OUT_AVG, global_bias=0.5)
    batch = run(env, f, data)
    assert np.array_equal(bits(run(env, f, data)), bits(batch)), "two calls"
    for r in (0, 63, 64, 200, ROWS - 1):
        assert np.array_equal(bits(run(env, f, data[r:r + 1]))[0], bits(batch)[r]), r
    for strat in ("DIRECT", "ROWTILE"):  # the call does not use the strategy
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert np.array_equal(bits(run(env, f, data)), bits(batch)), strat
    assert cols % 4 == 0
    buf = torch.full((ROWS * cols + 4,), float("nan"), device="cuda")
    x = buf[1:1 + ROWS * cols].view(ROWS, cols)
    x.copy_(torch.from_numpy(data.copy()).cuda())
    assert x.is_contiguous() and buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 4
    assert np.array_equal(bits(run(env, f, x)), bits(batch)), "one float off a 16-byte boundary"
    f.check()
    f.close()


def test_graph_capture_and_device_bytes(env):
    ta, torch = env
    forest, data, covers = vsr.case("five_k9")
    cv, K, cols = covers["consistent"], forest["k"], forest["cols"]
    f, plain = native(ta, forest, cv), native(ta, forest, None, approx=False)
    kb = var.form_rule(cols, K)[0]
    assert kb == 8
    assert f.info().device_bytes - plain.info().device_bytes == var.table_bytes(forest, kb) == 4 * 16 * forest["nodes"].size + 4 * K
    plain.close()
    x = torch.from_numpy(data.copy()).cuda()
    want = run(env, f, x)
    out = torch.empty((ROWS, K, cols + 1), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f.predict_contribs_approx(x, out=out)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f.predict_contribs_approx(x, out=out)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(want))
        out.zero_()
    f.check()
    f.close()


# ------------------------------------------------------------------------------------- 7: refusals with a device
def test_refusals(env):
    ta, torch = env
    forest, data, covers = vsr.case("five_k9")
    cv, K, cols = covers["consistent"], forest["k"], forest["cols"]
    x = torch.from_numpy(data.copy()).cuda()
    out = torch.full((ROWS * K * (cols + 1),), 7.0, device="cuda")
    lib = ta.lib
    for kw in (dict(), dict(contribs=True, interventional=True, interactions=True)):
        f = native(ta, forest, cv, approx=False, **kw)
        assert lib.tahoe_forest_predict_contribs_approx(f._h, out.data_ptr(), x.data_ptr(), ROWS, None) == UNSUPPORTED
        msg = lib.tahoe_last_error().decode()
        assert "vector-leaf" in msg and FN in msg, msg
        f.close()
    f = native(ta, forest, cv)
    h = f._h
    assert lib.tahoe_forest_predict_contribs_approx(h, None, None, 0, None) == OK  # rows == 0 comes first
    assert lib.tahoe_forest_predict_contribs_approx(h, None, x.data_ptr(), ROWS, None) == INVALID_ARG
    assert "null argument" in lib.tahoe_last_error().decode()
    assert lib.tahoe_forest_predict_contribs_approx(h, out.data_ptr(), None, ROWS, None) == INVALID_ARG
    assert "null argument" in lib.tahoe_last_error().decode()
    assert lib.tahoe_forest_predict_contribs_approx(h, out.data_ptr(), x.data_ptr(), C.c_size_t(1 << 62).value, None) == INVALID_ARG
    assert "overflow" in lib.tahoe_last_error().decode()
    # the calls the flag does not serve stay refused
    assert lib.tahoe_forest_predict_contribs(h, out.data_ptr(), x.data_ptr(), ROWS, None) == UNSUPPORTED
    assert "vector-leaf" in lib.tahoe_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "nothing written on a refusal"
    assert tuple(f.predict_contribs_approx(x[:0].contiguous()).shape) == (0, K, cols + 1)
    f.check()
    f.close()
    with pytest.raises(ta.TahoeError) as e:
        native(ta, forest, None)
    assert e.value.status == INVALID_ARG and "needs covers" in str(e.value)
