"""TreeSHAP and Saabas contributions on oblivious handles (tahoe_oblivious_forest_create_ex) against tests/oblivious_shap_ref.py
and against the heap expansion on dense handles.  Needs an MI355X.

TreeSHAP bar: |phi - phi64| <= (N + 4 (D + 2)) 2^-24 A per output -- the bound and error model of tests/test_contribs_gpu.py: a
float32 recursive sum of N per-leaf terms (A = the sum of their absolute values), each carrying the rounding of an extend /
unwind of at most D + 2 steps.  The native kernel runs the same EXTEND and the same o = 1 unwinding recurrence; where o = 0 it
takes -S0 leaf for sum (0 - z) leaf with sum = S0 / z, which saves the division and its rounding, so the constant stands.  The
bias column, Saabas and everything said to be bitwise compare bits.  Every call writes into the head of a buffer 256 rows longer
whose tail must come back untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oblivious_ref as obr  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = obr.MISSING
UNSUPPORTED = 7
U = 2.0 ** -24
ROWS = 129
BATCHES = (1, 63, 64, 65, 129)
TAIL = 256
SENTINEL = 7.0
MIXED = [0, 1, 2, 6, 3, 6, 4]  # depths; on 5 columns the features repeat within a tree
_cache = {}


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


@pytest.fixture
def unforced(monkeypatch):
    monkeypatch.delenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", raising=False)
    return monkeypatch


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def lds_bytes(ta):
    lds = C.c_int()
    assert ta.lib.tahoe_device_lds_bytes(C.byref(lds)) == 0
    return lds.value


def handle(ta, forest, covers=None, **kw):
    return ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], forest["cols"],
                              leaf_dim=forest["k"], missing=MISSING, leaf_covers=covers, **kw)


def expansion_handle(ta, forest, covers, **kw):
    k, T = forest["k"], len(forest["depths"])
    per_class = [osr.expand_with_covers(forest, covers, c) for c in range(k)]
    nodes = np.stack([n.reshape(T, -1) for n, _ in per_class], axis=1).reshape(-1)
    return ta.Forest(nodes, T * k, per_class[0][1], forest["cols"], missing=MISSING, num_classes=k, **kw)


def run(env, f, call, x):
    """f.<call>(x) into the head of a longer buffer -> numpy [rows, K, F + 1]; the tail must stay as it was"""
    ta, torch = env
    rows, k, F1 = x.shape[0], f.num_classes, f.num_cols + 1
    shape = (rows + TAIL,) + ((k,) if k > 1 else ()) + (F1,)
    buf = torch.full(shape, SENTINEL, device="cuda")
    getattr(f, call)(x, out=buf[:rows])
    torch.cuda.synchronize()
    assert bool((buf[rows:] == SENTINEL).all()), f"{call} wrote past its {rows} rows"
    return buf[:rows].cpu().numpy().reshape(rows, k, F1)


def case(name, depths, cols, k, kind, rows=ROWS, avg=False, bias=0.0, fids=None):
    """(forest, covers, data, poly's (phi, A, N), saabas' phi), computed once and read-only"""
    if name not in _cache:
        forest = obr.make_forest(depths, cols, k, seed=2000 + len(name))
        if fids is not None:
            forest["fids"][:] = fids
        covers = osr.make_covers(forest, kind, seed=31 + len(name))
        data = obr.make_data(rows, cols, seed=9 + cols)
        poly = osr.poly(forest, covers, data, avg=avg, global_bias=bias)
        saabas = osr.saabas(forest, covers, data, avg=avg, global_bias=bias)
        for a in (covers, data, saabas) + poly:
            a.setflags(write=False)
        _cache[name] = (forest, covers, data, poly, saabas)
    return _cache[name]


def check_shap(env, name, batches=BATCHES, **spec):
    """predict_contribs on the case: the bar, the bias bits, additivity, and every batch size against the full batch"""
    ta, torch = env
    avg, bias = spec.get("avg", False), spec.get("bias", 0.0)
    forest, covers, data, (want, A, N), _ = case(name, **spec)
    T, D, F = len(forest["depths"]), int(max(forest["depths"], default=0)), forest["cols"]
    f = handle(ta, forest, covers, contribs=True, output=ta.OUT_AVG if avg else 0, global_bias=bias)
    x = torch.from_numpy(data.copy()).cuda()
    got32 = run(env, f, "predict_contribs", x)
    got = got32.astype(np.float64)
    gamma = (N + 4 * (D + 2)) * U
    err, bound = np.abs(got - want)[:, :, :-1], (gamma * A)[:, :, :-1]
    worst = float((err / np.where(bound > 0, bound, 1.0)).max()) if err.size else 0.0
    print(f"{name}: max err / bound = {worst:.3f}")
    assert np.all(err <= bound), f"{name}: bound exceeded {worst:.3f}x at {np.argwhere(err > bound)[:5]}"
    b = osr.bias_f32(forest, covers, avg, bias)
    assert np.array_equal(bits(got32[:, :, -1]), bits(np.broadcast_to(b, got32[:, :, -1].shape))), name
    raw = f.predict_raw(x).cpu().numpy().astype(np.float64).reshape(data.shape[0], forest["k"])
    margin = (raw / T if avg and T else raw) + float(np.float32(bias))
    tol = bound.sum(axis=-1) + (T + 4) * U * (A.sum(axis=-1) + np.abs(margin)) + F * U * np.abs(got).sum(-1)
    assert np.all(np.abs(got.sum(axis=-1) - margin) <= tol), f"{name}: additivity"
    for r in batches:
        if r < data.shape[0]:
            assert np.array_equal(bits(run(env, f, "predict_contribs", x[:r].contiguous())), bits(got32[:r])), (name, r)
    f.close()
    return got32


# ------------------------------------------------------------------------------------------------ TreeSHAP against poly
@pytest.mark.parametrize("k", [1, 3, 9])
def test_treeshap_mixed_depths(env, unforced, k):
    check_shap(env, f"mixed_k{k}", depths=MIXED, cols=5, k=k, kind="int")


@pytest.mark.parametrize("kind", ["half", "most", "zero"])
def test_treeshap_with_empty_leaves(env, unforced, kind):
    check_shap(env, f"mixed_{kind}", depths=MIXED, cols=5, k=3, kind=kind)


def test_treeshap_avg_and_global_bias(env, unforced):
    check_shap(env, "mixed_avg", depths=MIXED, cols=5, k=3, kind="half", avg=True, bias=-0.375)


def test_treeshap_depth_16_on_four_repeated_features(env, unforced):
    check_shap(env, "deep16", batches=(1,), depths=[16], cols=4, k=1, kind="half", rows=5, fids=np.arange(16) % 4)


def test_treeshap_depth_10_on_ten_features(env, unforced):
    check_shap(env, "deep10", batches=(1,), depths=[10], cols=10, k=1, kind="int", rows=5, fids=np.arange(10))


# ------------------------------------------------------------------------------------------------ Saabas
@pytest.mark.parametrize("kind", ["int", "half", "most", "zero"])
@pytest.mark.parametrize("k", [1, 3, 9])
def test_saabas_equals_the_reference_bit_for_bit(env, unforced, k, kind):
    ta, torch = env
    forest, covers, data, _, want = case(f"mixed_{kind}_k{k}_s", depths=MIXED, cols=5, k=k, kind=kind)
    f = handle(ta, forest, covers, approx_contribs=True)
    x = torch.from_numpy(data.copy()).cuda()
    full = run(env, f, "predict_contribs_approx", x)
    assert np.array_equal(bits(full), bits(want))
    for r in BATCHES[:-1]:
        assert np.array_equal(bits(run(env, f, "predict_contribs_approx", x[:r].contiguous())), bits(want[:r])), r
    f.close()


@pytest.mark.parametrize("avg", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_saabas_and_bias_equal_the_expansion_bit_for_bit(env, unforced, k, avg):
    ta, torch = env
    forest, covers, data, _, want = case(f"exp_k{k}_{avg}", depths=MIXED, cols=5, k=k, kind="int", avg=avg, bias=0.25)
    kw = dict(output=ta.OUT_AVG if avg else 0, global_bias=0.25)
    f = handle(ta, forest, covers, contribs=True, approx_contribs=True, **kw)
    g = expansion_handle(ta, forest, covers, contribs=True, approx_contribs=True, **kw)
    x = torch.from_numpy(data.copy()).cuda()
    mine = run(env, f, "predict_contribs_approx", x)
    assert np.array_equal(bits(mine), bits(run(env, g, "predict_contribs_approx", x)))
    assert np.array_equal(bits(mine), bits(want))
    shap = run(env, f, "predict_contribs", x)
    assert np.array_equal(bits(shap[:, :, -1]), bits(mine[:, :, -1]))  # one bias for both calls ...
    assert np.array_equal(bits(shap[:, :, -1]), bits(run(env, g, "predict_contribs", x)[:, :, -1]))  # ... and the expansion's
    f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ bitwise
@pytest.mark.parametrize("call,flag", [("predict_contribs", "contribs"), ("predict_contribs_approx", "approx_contribs")])
def test_repeats_rows_alone_and_permutations_give_the_same_bits(env, unforced, call, flag):
    ta, torch = env
    forest, covers, data, _, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, kind="int")
    f = handle(ta, forest, covers, **{flag: True})
    x = torch.from_numpy(data.copy()).cuda()
    first = run(env, f, call, x)
    assert np.array_equal(bits(first), bits(run(env, f, call, x)))
    for r in (0, 63, 64, ROWS - 1):
        assert np.array_equal(bits(run(env, f, call, x[r:r + 1].clone())), bits(first[r:r + 1])), r
    perm = np.random.default_rng(5).permutation(ROWS)
    assert np.array_equal(bits(run(env, f, call, x[torch.from_numpy(perm).cuda()].contiguous())), bits(first[perm]))
    f.close()


def wide_forest(used, cols, k, seed):
    """Trees of depth 6 whose splits use exactly `used` distinct features of `cols` columns"""
    trees = -(-used // 6)
    forest = obr.make_forest([6] * trees, cols, k, seed=seed)
    rng = np.random.default_rng(seed)
    fids = np.concatenate([rng.permutation(used), rng.integers(0, used, 6 * trees - used)])
    forest["fids"][:] = rng.permutation(cols)[fids]
    assert np.unique(forest["fids"]).size == used
    return forest


# widths on either side of the form boundary, per class block (oblivious_shap_ref.shap_form; 160 KiB of LDS)
FORMS = {(319, 1): "lds", (320, 1): "inplace", (159, 3): "lds", (160, 3): "inplace", (127, 9): "lds", (128, 9): "inplace"}


@pytest.mark.parametrize("used,k", list(FORMS))
def test_the_forms_agree_bit_for_bit_on_either_side_of_the_boundary(env, unforced, used, k):
    ta, torch = env
    assert osr.shap_form(used, k, 160 * 1024) == FORMS[(used, k)], "the rule in oblivious_shap_build"
    assert osr.shap_form(used, k, lds_bytes(ta)) == FORMS[(used, k)], "this device's LDS is not the 160 KiB the table is for"
    forest = wide_forest(used, used + 3, k, seed=used + k)
    covers = osr.make_covers(forest, "half", seed=used)
    data = obr.make_data(65, used + 3, seed=used + 1)
    x = torch.from_numpy(data.copy()).cuda()
    want = osr.saabas(forest, covers, data)
    got = {}
    for forced in (False, True):
        if forced:
            unforced.setenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", "1")
        f = handle(ta, forest, covers, contribs=True, approx_contribs=True)
        unforced.delenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", raising=False)
        got[forced] = (run(env, f, "predict_contribs", x), run(env, f, "predict_contribs_approx", x))
        f.close()
    assert np.array_equal(bits(got[False][0]), bits(got[True][0])) and np.array_equal(bits(got[False][1]), bits(got[True][1]))
    assert np.array_equal(bits(got[False][1]), bits(want))
    phi, A, N = osr.poly(forest, covers, data)
    err = np.abs(got[False][0].astype(np.float64) - phi)[:, :, :-1]
    assert np.all(err <= ((N + 4 * (6 + 2)) * U * A)[:, :, :-1])


@pytest.mark.parametrize("forced", [False, True])
def test_many_columns_few_used(env, unforced, forced):
    """5000 columns of which 12 are used: the LDS form by the rule (its width is the used features'), every other column 0"""
    ta, torch = env
    assert osr.shap_form(12, 1, lds_bytes(ta)) == "lds"
    forest = wide_forest(12, 5000, 1, seed=3)
    covers = osr.make_covers(forest, "int", seed=4)
    data = obr.make_data(65, 5000, seed=5)
    x = torch.from_numpy(data.copy()).cuda()
    if forced:
        unforced.setenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", "1")
    f = handle(ta, forest, covers, contribs=True, approx_contribs=True)
    unforced.delenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", raising=False)
    assert np.array_equal(bits(run(env, f, "predict_contribs_approx", x)), bits(osr.saabas(forest, covers, data)))
    got = run(env, f, "predict_contribs", x)
    phi, A, N = osr.poly(forest, covers, data)
    assert np.all(np.abs(got.astype(np.float64) - phi)[:, :, :-1] <= ((N + 4 * (6 + 2)) * U * A)[:, :, :-1])
    unused = np.setdiff1d(np.arange(5000), forest["fids"])
    assert not bits(got[:, :, unused]).any()
    f.close()


# ------------------------------------------------------------------------------------------------ other cases
@pytest.mark.parametrize("depths", [[], [0, 0, 0]])
def test_no_trees_and_single_leaves_feed_the_bias_only(env, unforced, depths):
    ta, torch = env
    forest = obr.make_forest(depths, 3, 2, seed=1)
    covers = osr.make_covers(forest, "int", seed=2)
    data = obr.make_data(65, 3, seed=3)
    x = torch.from_numpy(data.copy()).cuda()
    f = handle(ta, forest, covers, contribs=True, approx_contribs=True, global_bias=0.5)
    b = osr.bias_f32(forest, covers, False, 0.5)
    for call in ("predict_contribs", "predict_contribs_approx"):
        got = run(env, f, call, x)
        assert not bits(got[:, :, :-1]).any() and np.array_equal(bits(got[:, :, -1]), bits(np.broadcast_to(b, (65, 2))))
    f.close()


def test_zero_rows(env, unforced):
    ta, torch = env
    forest, covers, data, _, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, kind="int")
    f = handle(ta, forest, covers, contribs=True, approx_contribs=True)
    x = torch.from_numpy(data[:0].copy()).cuda()
    assert tuple(f.predict_contribs(x).shape) == (0, 3, 6) and tuple(f.predict_contribs_approx(x).shape) == (0, 3, 6)
    assert ta.lib.tahoe_forest_predict_contribs(f._h, None, None, 0, None) == 0
    f.close()


def test_both_calls_can_be_captured(env, unforced):
    ta, torch = env
    forest, covers, data, _, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, kind="int")
    f = handle(ta, forest, covers, contribs=True, approx_contribs=True)
    x = torch.from_numpy(data.copy()).cuda()
    want = run(env, f, "predict_contribs", x), run(env, f, "predict_contribs_approx", x)
    a, b = torch.zeros((ROWS, 3, 6), device="cuda"), torch.zeros((ROWS, 3, 6), device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f.predict_contribs(x, out=a)
        f.predict_contribs_approx(x, out=b)
    for _ in range(2):
        a.zero_()
        b.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(a), bits(want[0])) and np.array_equal(bits(b), bits(want[1]))
    f.close()


def test_tables_count_in_device_bytes_and_predictions_keep_their_bits(env, unforced):
    ta, torch = env
    forest, covers, data, _, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, kind="int")
    plain, flagged = handle(ta, forest), handle(ta, forest, covers, contribs=True, approx_contribs=True)
    depths = np.asarray(forest["depths"], np.int64)
    leaves = int((1 << depths).sum())
    elems = sum((1 << int(d)) * np.unique(forest["fids"][s:s + int(d)]).size
                for d, s in zip(depths, np.concatenate([[0], np.cumsum(depths)])))
    tables = 8 * elems + 4 * leaves + 4 * 3 * 2 * (leaves - depths.size)
    assert flagged.info().device_bytes >= plain.info().device_bytes + tables
    x = torch.from_numpy(data.copy()).cuda()
    assert np.array_equal(bits(plain.predict(x)), bits(flagged.predict(x)))
    assert np.array_equal(bits(plain.predict_raw(x)), bits(flagged.predict_raw(x)))
    (la, sa), (lb, sb) = plain.predict_leaf_idx(x), flagged.predict_leaf_idx(x)
    assert np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(sa), bits(sb))
    plain.close()
    flagged.close()


def test_refusals(env, unforced):
    ta, torch = env
    forest, covers, data, _, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, kind="int")
    x = torch.from_numpy(data.copy()).cuda()
    out = torch.full((ROWS * 3 * 6 * 6,), SENTINEL, device="cuda")
    lib = ta.lib

    def refused(f, names):
        for name in names:
            fn = getattr(lib, name)
            st = fn(f._h, x.data_ptr(), ROWS, None) if name == "tahoe_forest_set_background" else \
                fn(f._h, out.data_ptr(), x.data_ptr(), ROWS, None)
            msg = lib.tahoe_last_error().decode()
            assert st == UNSUPPORTED and "oblivious" in msg and name in msg, (name, st, msg)

    never = ["tahoe_forest_predict_interactions", "tahoe_forest_set_background", "tahoe_forest_predict_contribs_interventional"]
    both = handle(ta, forest, covers, contribs=True, approx_contribs=True)
    refused(both, never)
    only_shap = handle(ta, forest, covers, contribs=True)
    refused(only_shap, never + ["tahoe_forest_predict_contribs_approx"])
    only_approx = handle(ta, forest, covers, approx_contribs=True)
    refused(only_approx, never + ["tahoe_forest_predict_contribs"])
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert lib.tahoe_forest_predict_contribs(both._h, None, x.data_ptr(), ROWS, None) == 1  # TAHOE_ERR_INVALID_ARG
    for f in (both, only_shap, only_approx):
        f.check()
        f.close()
