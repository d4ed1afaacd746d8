"""Interventional TreeSHAP on vector-leaf handles (tahoe_vector_forest_create_ex with TAHOE_CREATE_INTERVENTIONAL) on the GPU.
Needs an MI355X.

Bitwise: set_background + predict_contribs_interventional of the native handle -- created with the flag alone (no covers) and
with TAHOE_CREATE_CONTRIBS beside it -- against the T x K-tree expansion on tahoe_sparse_forest_create_ex(num_classes = K,
TAHOE_CREATE_CONTRIBS) under two cover sets, bias column included: every forest of tests/vector_shap_ref.py, batches around the
8-row tile, backgrounds around the unroll of 8, three output settings; every class block the kernel is built for and both ways of
running the blocks; the edge cases of tests/vector_edges.py; num_cols on both sides of every step of the class-block / tile rule.
Accuracy: against the float64 closed form of tests/vector_iv_ref.py (itself checked against the subset brute force) within
tests/test_interventional_gpu.py's bar, |err| <= (N + B + 8) 2^-24 A per value, derived there; the bias column bit for bit against
the host formula on the handle's own raw sums of the background; additivity against the handle's margins within that test's
allowance.  The largest error seen is printed as a fraction of the bar.
Protocol: replace / clear / set again, device_bytes, a row alone, two calls, a graph replay, the strategy, every refusal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interventional_ref as ivr  # noqa: E402
import vector_edges as ve  # noqa: E402
import vector_iv_ref as vir  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = vsr.MISSING
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 7
U = 2.0 ** -24
KNOBS = ("TAHOE_VECTOR_SHAP_KB", "TAHOE_VECTOR_SHAP_GRID")
BATCHES = (1, 7, 8, 9, 65)       # around the tile of R <= 8 rows
BACKGROUNDS = (1, 7, 8, 9, 19)   # around the unroll of 8
OUTPUTS = ("RAW", "AVG", "AVG|SIGMOID")


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


def native(ta, forest, covers=None, contribs=False, interventional=True, **kw):
    return ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=MISSING, covers=covers,
                           contribs=contribs, interventional=interventional, **kw)


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


def phi_shape(forest, rows):
    return (rows,) + ((forest["k"],) if forest["k"] > 1 else ()) + (forest["cols"] + 1,)


def two_cover_sets(forest, covers):
    sets = list(covers.values())
    if len(sets) < 2:
        sets.append(vsr.unrelated_covers(forest, 77))
    return sets[:2]


def background(forest, B, seed=0):
    """B rows of the usual mix: the sentinel, a value within 1e-6 of it, NaN, +-inf, +-0.0 among grid values"""
    return vr.make_data(B, forest["cols"], seed=700 + 31 * B + seed)


def same_bits_nan_aside(a, b):
    """Equal in every bit where both are finite or infinite; NaN where the other is NaN (the payload is not compared)"""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 1: the expansion's bits
@pytest.mark.parametrize("name", vsr.NAMES)
def test_equals_the_expansion_bit_for_bit(env, name):
    ta, torch = env
    forest, data, covers = vsr.case(name)
    cv1, cv2 = two_cover_sets(forest, covers)
    x = torch.from_numpy(data[:65].copy()).cuda()
    for output in OUTPUTS:
        kw = dict(output=out_bits(ta, output), global_bias=0.375)
        handles = [native(ta, forest, **kw), native(ta, forest, cv1, contribs=True, **kw), expansion(ta, forest, cv1, **kw),
                   expansion(ta, forest, cv2, **kw)]
        for B in BACKGROUNDS:
            bg = torch.from_numpy(background(forest, B)).cuda()
            for h in handles:
                h.set_background(bg)
            for r in BATCHES:
                xr = x[:r].contiguous()
                got = [h.predict_contribs_interventional(xr) for h in handles]
                assert all(tuple(g.shape) == phi_shape(forest, r) for g in got)
                want = bits(got[2])
                assert np.array_equal(bits(got[3]), want), (output, B, r)  # the covers change no bit of the expansion
                assert np.array_equal(bits(got[0]), want), ("flag alone", output, B, r)
                assert np.array_equal(bits(got[1]), want), ("with CONTRIBS", output, B, r)
        handles[0].check()
        for h in handles:
            h.close()


# ------------------------------------------------------------------------------------------------ 2: the knobs
@pytest.mark.parametrize("name", ["nine_k17", "five_k9", "four_k8", "stump_k3", "nine_k1", "wide_k9", "repeat_k3"])
def test_class_block_and_grid_change_no_bit(env, monkeypatch, name):
    """Every vector_interventional_kernel<KB, true>, with the class blocks in a workgroup's loop and over gridDim.y (the knobs
    are read at create)"""
    ta, torch = env
    forest, data, covers = vsr.case(name)
    x = torch.from_numpy(data[:65].copy()).cuda()
    bg = torch.from_numpy(background(forest, 9)).cuda()
    kw = dict(output=ta.OUT_AVG, global_bias=-0.25)
    g = expansion(ta, forest, next(iter(covers.values())), **kw)
    g.set_background(bg)
    want = bits(g.predict_contribs_interventional(x))
    g.close()
    for kb in (1, 2, 4, 8):
        for grid in (0, 1):
            monkeypatch.setenv("TAHOE_VECTOR_SHAP_KB", str(kb))
            monkeypatch.setenv("TAHOE_VECTOR_SHAP_GRID", str(grid))
            f = native(ta, forest, **kw)
            f.set_background(bg)
            assert np.array_equal(bits(f.predict_contribs_interventional(x)), want), (kb, grid)
            assert np.array_equal(bits(f.predict_contribs_interventional(x[:9].contiguous())), want[:9]), (kb, grid)
            f.check()
            f.close()


# ------------------------------------------------------------------------------------------------ 3: accuracy
def host_bias(ta, torch, forest, f, bg, avg, bias):
    """The host formula of tahoe_forest_set_background on the handle's own raw sums of the background"""
    raw = f.predict_raw(bg).cpu().numpy().reshape(bg.shape[0], forest["k"])
    T = forest["trees"].size
    return np.array([ivr.bias_from_raw(raw[:, k], T, avg, bias) for k in range(forest["k"])]).astype(np.float32)


@pytest.mark.parametrize("name", vsr.SMALL)
def test_against_the_float64_closed_form(env, name):
    ta, torch = env
    forest, data, _ = vsr.case(name)
    K, F, T = forest["k"], forest["cols"], forest["trees"].size
    rows, B = 17, 7
    x, bgh = data[:rows], background(forest, B, seed=3)
    worst = 0.0
    for output, bias in (("RAW", 0.0), ("AVG", 0.375)):
        avg = "AVG" in output
        want, A, N = vir.paths(forest, x, bgh, avg=avg, global_bias=bias)
        brute = vir.brute(forest, x, bgh, avg=avg, global_bias=bias)  # num_cols <= 8 on every forest of SMALL
        scale = np.abs(brute).sum(axis=-1, keepdims=True) + 1e-300
        assert np.all(np.abs(brute - want) <= 1e-12 * scale), name
        f = native(ta, forest, output=out_bits(ta, output), global_bias=bias)
        bg = torch.from_numpy(bgh).cuda()
        f.set_background(bg)
        got = f.predict_contribs_interventional(torch.from_numpy(x.copy()).cuda()).cpu().numpy().reshape(rows, K, F + 1)
        err = np.abs(got.astype(np.float64) - want)[:, :, :-1]
        bound = ((N[None] + B + 8) * U * A)[:, :, :-1]
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0)))
        assert np.all(err <= bound), f"{name} {output}: bound exceeded at {np.argwhere(err > bound)[:5]}"
        # bias column: bit for bit the host formula on the handle's own predict_raw of the background
        want_bias = host_bias(ta, torch, forest, f, bg, avg, bias)
        assert np.array_equal(bits(got[:, :, -1]), bits(np.broadcast_to(want_bias, (rows, K)))), (name, output)
        # additivity against the handle's margins (AVG and bias applied); AVG over no trees is 0 / 0 in predict: no margin to meet
        if avg and not T:
            f.close()
            continue
        m = native(ta, forest, interventional=False, output=out_bits(ta, output), global_bias=bias)
        margin = m.predict(torch.from_numpy(x.copy()).cuda()).cpu().numpy().astype(np.float64).reshape(rows, K)
        m.close()
        div = T if avg and T else 1
        absf = dict(forest, leaves=np.abs(forest["leaves"]))
        sx = ve.margins64(absf, x) / div
        sr = ve.margins64(absf, bgh).mean(axis=0)[None, :] / div
        tol = bound.sum(axis=-1) + (T + 4) * U * (sx + sr) + 4 * U * (np.abs(margin) + np.abs(got[:, :, -1]) + abs(bias))
        assert np.all(np.abs(got.astype(np.float64).sum(axis=-1) - margin) <= tol), f"{name} {output}: additivity"
        f.close()
    print(f"{name}: largest |err| / bar = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 4: edges
def compare_with_expansion(env, forest, covers, x, bgh, exact=True, **kw):
    ta, torch = env
    f, g = native(ta, forest, **kw), expansion(ta, forest, covers, **kw)
    bg = torch.from_numpy(np.array(bgh, np.float32)).cuda()
    f.set_background(bg)
    g.set_background(bg)
    xd = torch.from_numpy(np.array(x, np.float32)).cuda()
    a, b = f.predict_contribs_interventional(xd), g.predict_contribs_interventional(xd)
    assert tuple(a.shape) == tuple(b.shape) == phi_shape(forest, x.shape[0])
    assert np.array_equal(bits(a), bits(b)) if exact else same_bits_nan_aside(a, b)
    f.check()
    g.close()
    return f, a


def follow_row(base, elems, follow):
    """base with the feature of every element set so that the row follows its edges (follow[j]) or fails its first one"""
    row = base.copy()
    for (fid, _, edges), yes in zip(elems, follow):
        assert len(edges) == 1
        thr, _, right = edges[0]
        row[fid] = thr + 1.0 if right == yes else thr - 1.0
    return row


def test_vine31_reaches_the_last_diagonal_of_the_weight_table(env):
    """A 32-lane path whose 31 features all differ between the row and the background row: |A| + |B'| = 31"""
    c = ve.case("vine31:k9")
    forest, data = c["forest"], c["data"]
    deepest = max(ve.leaf_paths(forest, np.ones(forest["nodes"].size, np.float32))[0], key=lambda p: len(p[1]))[1]
    assert len(deepest) == 31
    x, bgh = data[:33].copy(), data[40:49].copy()
    none, all_ = [False] * 31, [True] * 31
    split = [j < 10 for j in range(31)]
    x[0], bgh[0] = follow_row(x[0], deepest, all_), follow_row(bgh[0], deepest, none)          # W[31][0]
    x[1], bgh[1] = follow_row(x[1], deepest, split), follow_row(bgh[1], deepest, [not s for s in split])  # W[10][21], W[21][10]
    x[2] = follow_row(x[2], deepest, none)                                                   # against bgh[2] below: W[31][0] from B'
    bgh[2] = follow_row(bgh[2], deepest, all_)
    term = vir._path_terms([(f, ed) for f, _, ed in deepest], x[:3], bgh[:3], MISSING)
    assert np.isclose(term[0, 0, 0], 1 / 31) and np.isclose(term[0, 2, 2], -1 / 31) and term[0, 1, 1] != 0 and term[30, 1, 1] != 0
    f, _ = compare_with_expansion(env, forest, c["covers"]["consistent"], x, bgh, output=0, global_bias=0.0)
    f.close()


@pytest.mark.parametrize("name", ["mixed_len:k9", "one_col_rounds", "K:1024"])
def test_path_shapes_and_class_blocks_over_the_grid(env, name):
    """Short paths behind a 32-lane one; 32 rounds into one cell; 128 class blocks on gridDim.y"""
    c = ve.case(name)
    forest, data = c["forest"], c["data"]
    if name == "one_col_rounds":
        assert max(r for _, r in vsr.bins(forest)) == 32
    f, _ = compare_with_expansion(env, forest, next(iter(c["covers"].values())), data[:17], data[30:39], output=env[0].OUT_AVG,
                                  global_bias=0.5)
    f.close()


def test_root_leaves_only(env):
    """No bin: every feature column is +0.0f and the bias is the background's mean margin"""
    ta, torch = env
    rng = np.random.default_rng(8100)
    forest = vr.make([int(rng.integers(0, 7)) for _ in range(5)], vr.mixed_leaves(rng, 7, 3), 3, 4)
    x, bgh = vr.make_data(9, 4, seed=8101), vr.make_data(5, 4, seed=8102)
    f, a = compare_with_expansion(env, forest, np.ones(forest["nodes"].size, np.float32), x, bgh, output=ta.OUT_AVG, global_bias=0.25)
    got = a.cpu().numpy()
    assert np.all(bits(got[:, :, :-1]) == 0)
    want_bias = host_bias(ta, torch, forest, f, torch.from_numpy(bgh).cuda(), True, 0.25)
    assert np.array_equal(bits(got[:, :, -1]), bits(np.broadcast_to(want_bias, (9, 3))))
    f.close()


def test_ieee_leaves_equal_the_expansion(env):
    """+-3e38, +-inf, NaN, -0.0 and 1e-45 at the leaves: every bit of the expansion where it is no NaN, NaN where it is (the
    expansion gives NaN there too; payloads are not compared)"""
    c = ve.case("leaves:ieee")
    f, a = compare_with_expansion(env, c["forest"], c["covers"]["consistent"], c["data"][:17], c["data"][30:39], exact=False,
                                  output=0, global_bias=0.0)
    assert np.isnan(a.cpu().numpy()).any()  # (inf - inf and NaN leaves reach nearly every value of this case)
    f.close()
    c = ve.case("leaves:negzero")  # every leaf -0.0: the sign of every zero, exactly
    f, a = compare_with_expansion(env, c["forest"], c["covers"]["consistent"], c["data"][:17], c["data"][30:39], output=0,
                                  global_bias=0.0)
    assert np.all(a.cpu().numpy() == 0.0)
    f.close()


@pytest.mark.parametrize("cols", list(vir.TILE_COLS))
def test_tiles_on_both_sides_of_every_step_of_the_rule(env, cols):
    """One 3-tree forest, K = 9, spread over num_cols columns: (KB, R, WLDS) as tests/vector_iv_ref.TILE_COLS lists them
    (asserted without a GPU in tests/test_vector_iv_ref.py); 8192 columns read the weight table from global memory"""
    c = ve.case(f"tiles:{cols}")
    rows = 2 * vir.TILE_COLS[cols][1] + 1  # two full tiles and a row
    f, _ = compare_with_expansion(env, c["forest"], c["covers"]["consistent"], c["data"][:rows], c["data"][30:39],
                                  output=env[0].OUT_AVG, global_bias=0.5)
    f.close()


def test_one_column_too_many_is_refused(env):
    ta, _ = env
    c = ve.case(f"tiles:{vir.TILE_REFUSED}")
    with pytest.raises(ta.TahoeError) as e:
        native(ta, c["forest"])
    assert e.value.status == UNSUPPORTED and "20 B of LDS per column" in str(e.value)


# ------------------------------------------------------------------------------------------------ 5: protocol
@pytest.fixture(scope="module")
def five(env):
    ta, torch = env
    forest, data, covers = vsr.case("five_k9")
    kw = dict(output=ta.OUT_AVG, global_bias=0.375)
    f = native(ta, forest, **kw)
    x = torch.from_numpy(data[:65].copy()).cuda()
    bgh = background(forest, 19)
    f.set_background(torch.from_numpy(bgh).cuda())
    ref = bits(f.predict_contribs_interventional(x))
    return forest, covers["consistent"], kw, f, x, bgh, ref


def test_background_replaced_cleared_set_again_and_counted(env, five):
    ta, torch = env
    forest, cv, kw, f, x, bgh, ref = five
    K, nbins = forest["k"], len(vsr.bins(forest))
    g = native(ta, forest, **kw)
    base = g.info().device_bytes
    g.set_background(torch.from_numpy(bgh[:5].copy()).cuda())
    assert g.info().device_bytes == base + nbins * 5 * 8 + (1024 + K) * 4
    assert not np.array_equal(bits(g.predict_contribs_interventional(x)), ref)
    g.set_background(torch.from_numpy(bgh).cuda())  # replaced; the caller's tensor may go away
    torch.cuda.synchronize()
    assert g.info().device_bytes == base + nbins * 19 * 8 + (1024 + K) * 4
    assert np.array_equal(bits(g.predict_contribs_interventional(x)), ref)
    g.set_background(torch.from_numpy(bgh).cuda())  # the same background again
    assert np.array_equal(bits(g.predict_contribs_interventional(x)), ref)
    g.set_background(None)
    assert g.info().device_bytes == base
    with pytest.raises(ta.TahoeError) as e:
        g.predict_contribs_interventional(x)
    assert e.value.status == UNSUPPORTED and "no background" in str(e.value)
    g.close()
    # what the handle holds: the flag alone saves one_minus_z (4 B per lane) and the TreeSHAP bias (4 K B); both flags hold what
    # TAHOE_CREATE_CONTRIBS alone does; predict_contribs needs that flag
    both, contribs = native(ta, forest, cv, contribs=True, **kw), native(ta, forest, cv, contribs=True, interventional=False, **kw)
    assert both.info().device_bytes == contribs.info().device_bytes == base + nbins * 64 * 4 + K * 4
    g = native(ta, forest, **kw)
    with pytest.raises(ta.TahoeError) as e:
        g.predict_contribs(x)
    assert e.value.status == UNSUPPORTED and "vector-leaf" in str(e.value) and "tahoe_forest_predict_contribs" in str(e.value)
    want = bits(contribs.predict_contribs(x))
    assert np.array_equal(bits(both.predict_contribs(x)), want)  # one set of tables serves both calls
    both.set_background(torch.from_numpy(bgh).cuda())
    assert np.array_equal(bits(both.predict_contribs_interventional(x)), ref)
    assert np.array_equal(bits(both.predict_contribs(x)), want)
    for h in (g, both, contribs):
        h.close()


def test_rows_calls_strategy_and_graph_replay(env, five):
    ta, torch = env
    forest, cv, kw, f, x, bgh, ref = five
    assert np.array_equal(bits(f.predict_contribs_interventional(x)), ref)  # two calls
    for r in (0, 7, 64):
        assert np.array_equal(bits(f.predict_contribs_interventional(x[r:r + 1].contiguous())), ref[r:r + 1]), r
    assert tuple(f.predict_contribs_interventional(x[:0].contiguous()).shape) == phi_shape(forest, 0)
    bg = torch.from_numpy(bgh).cuda()
    for s in (ta.STRATEGY_DIRECT, ta.STRATEGY_ROWTILE, ta.STRATEGY_AUTO):
        f.set_strategy(s)
        f.set_background(bg)  # the bias is computed as DIRECT under any setting, which is left as it was
        if s != ta.STRATEGY_AUTO:
            assert f.get_strategy(100) == s
        assert np.array_equal(bits(f.predict_contribs_interventional(x)), ref), s
    out = torch.empty(phi_shape(forest, 65), device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        f.predict_contribs_interventional(x, out=out, stream=s)
    out.zero_()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), ref)


def test_refusals_launch_nothing(env, five):
    ta, torch = env
    lib = ta.lib
    forest, cv, kw, f, x, bgh, ref = five
    F, K = forest["cols"], forest["k"]
    bg = torch.from_numpy(bgh).cuda()
    out = torch.full((65 * K * (F + 1),), 7.0, device="cuda")
    name = "tahoe_forest_predict_contribs_interventional"
    assert lib.tahoe_forest_predict_contribs_interventional(None, out.data_ptr(), x.data_ptr(), 65, None) == INVALID_ARG
    assert lib.tahoe_forest_set_background(None, bg.data_ptr(), 19, None) == INVALID_ARG
    # without the flag, as before it existed: TAHOE_CREATE_CONTRIBS or not, even with NULL pointers (the flag comes first)
    for h in (native(ta, forest, interventional=False), native(ta, forest, cv, contribs=True, interventional=False)):
        assert lib.tahoe_forest_set_background(h._h, bg.data_ptr(), 19, None) == UNSUPPORTED
        msg = lib.tahoe_last_error().decode()
        assert "vector-leaf" in msg and "tahoe_forest_set_background" in msg, msg
        assert lib.tahoe_forest_predict_contribs_interventional(h._h, None, None, 65, None) == UNSUPPORTED
        msg = lib.tahoe_last_error().decode()
        assert "vector-leaf" in msg and name in msg, msg
        h.close()
    nobg = native(ta, forest)
    assert lib.tahoe_forest_predict_contribs_interventional(nobg._h, None, None, 0, None) == UNSUPPORTED  # before rows == 0
    assert "no background" in lib.tahoe_last_error().decode()
    nobg.close()
    assert lib.tahoe_forest_predict_contribs_interventional(f._h, None, None, 0, None) == OK
    assert lib.tahoe_forest_predict_contribs_interventional(f._h, None, x.data_ptr(), 5, None) == INVALID_ARG
    assert lib.tahoe_forest_predict_contribs_interventional(f._h, out.data_ptr(), None, 5, None) == INVALID_ARG
    assert lib.tahoe_forest_predict_contribs_interventional(f._h, out.data_ptr(), x.data_ptr(), 2 ** 62, None) == INVALID_ARG
    assert "overflow" in lib.tahoe_last_error().decode()
    assert lib.tahoe_forest_set_background(f._h, None, 5, None) == INVALID_ARG
    assert lib.tahoe_forest_set_background(f._h, bg.data_ptr(), 2 ** 62, None) == INVALID_ARG
    # the calls a vector-leaf handle does not serve, with the flag or without
    unserved = {
        "tahoe_forest_predict_interactions": lambda: lib.tahoe_forest_predict_interactions(f._h, out.data_ptr(), x.data_ptr(), 1, None),
        "tahoe_forest_predict_contribs_approx": lambda: lib.tahoe_forest_predict_contribs_approx(f._h, out.data_ptr(), x.data_ptr(), 65, None),
        "tahoe_forest_predict_contribs": lambda: lib.tahoe_forest_predict_contribs(f._h, out.data_ptr(), x.data_ptr(), 65, None),
        "tahoe_forest_predict_accumulate": lambda: lib.tahoe_forest_predict_accumulate(f._h, out.data_ptr(), x.data_ptr(), 65, None),
    }
    for fn, call in unserved.items():
        assert call() == UNSUPPORTED, fn
        msg = lib.tahoe_last_error().decode()
        assert "vector-leaf" in msg and fn in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    assert np.array_equal(bits(f.predict_contribs_interventional(x)), ref)  # the refused calls kept f's background
