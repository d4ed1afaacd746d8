"""Interventional TreeSHAP on oblivious handles (tahoe_oblivious_forest_create_ex with TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL;
tahoe_forest_set_background, tahoe_forest_predict_contribs_interventional) against the float64 references of
tests/oblivious_iv_ref.py and against the heap expansion on a dense handle.  Needs an MI355X.

Bound: |phi_gpu - phi_64| <= (N + 8) 2^-24 A per output, A = (1 / B) sum over (tree, occupied background leaf, subset) of
count |weight| |leaf| (divided by T with AVG; oblivious_iv_ref.paths), N = the number of those terms feeding the output.
Derivation, in the style of tests/test_interventional_gpu.py: a term weight x (float)count x leaf carries the rounding of the
weight (1), of (float)count (1; 0 below 2^24), of its two products (2), of the in-order float32 sum of the N terms (N - 1) and of
the two divisions (2): N + 5 to first order, 3 more for the second-order terms.  The kernel makes exactly these operations (the
division by div is by 1.0f without AVG), so the constant stands as derived.
Exact: the bias column bit for bit against the host formula on predict_raw(bg) of the same handle; B = 1 with the background equal
to the row gives +0.0 everywhere but the bias; a column no tree uses gives +0.0.  Additivity: sum_i phi_i + bias against the
handle's margin within the bound plus the float32 error of the margin and of the background's raw sums.  Bitwise: repeat calls, a
row alone, a permutation, a prefix, the LDS form against the in-place form, output k of a K = 5 handle against a K = 1 handle on
that output's leaves, with and without the other three flags, the same background set again, and in the feature columns the
background permuted and the background tiled twice (counts and B double: every scaling is by a power of two).
Every call writes into the head of a buffer 256 rows longer whose tail must come back untouched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interventional_ref as ivr  # noqa: E402
import oblivious_iv_ref as oiv  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, 7
U = 2.0 ** -24
TAIL = 256
SENTINEL = 7.0
MIXED = [0, 1, 2, 6, 3, 6, 4]  # depths; on 5 columns the features repeat within a tree
WEIGHT_BYTES = 2 * 17 * 17 * 4
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


def dev(env, a):
    return env[1].from_numpy(np.array(a, np.float32)).cuda()  # (a copy: the cached arrays are read-only)


def handle(ta, forest, covers=None, missing=obr.MISSING, interventional=True, **kw):
    return ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], forest["cols"],
                              leaf_dim=forest["k"], missing=missing, leaf_covers=covers, interventional=interventional, **kw)


def run(env, f, x):
    """f.predict_contribs_interventional(x) into the head of a longer buffer -> numpy [rows, K, F + 1]; the tail must stay"""
    ta, torch = env
    rows, k, F1 = x.shape[0], f.num_classes, f.num_cols + 1
    buf = torch.full((rows + TAIL,) + ((k,) if k > 1 else ()) + (F1,), SENTINEL, device="cuda")
    f.predict_contribs_interventional(x, out=buf[:rows])
    torch.cuda.synchronize()
    assert bool((buf[rows:] == SENTINEL).all()), f"the call wrote past its {rows} rows"
    return buf[:rows].cpu().numpy().reshape(rows, k, F1)


def case(name, depths=None, cols=None, k=None, rows=None, B=None, avg=False, bias=0.0, fids=None, spread=None, missing=obr.MISSING,
         brute=False):
    """(forest, data, background, paths' (phi, A, N)), computed once and read-only.  spread: the forest is made on len(spread)
    columns and its feature c becomes column spread[c] of `cols`, so that some columns stay unused."""
    if name not in _cache:
        forest = obr.make_forest(depths, cols if spread is None else len(spread), k, seed=3000 + len(name))
        if fids is not None:
            forest["fids"][:] = fids
        if spread is not None:
            forest["fids"][:] = np.asarray(spread)[np.asarray(forest["fids"])]
            forest["cols"] = cols
        data = obr.make_data(rows, cols, seed=19 + cols, missing=missing)
        bg = obr.make_data(B, cols, seed=23 + cols, missing=missing)
        ref = oiv.paths(forest, data, bg, missing, avg=avg, global_bias=bias)
        if brute:
            want = oiv.brute(forest, data, bg, missing, avg=avg, global_bias=bias)
            assert np.all(np.abs(want - ref[0]) <= 1e-12 * (np.abs(want).sum(axis=-1, keepdims=True) + 1e-300)), name
            ref = (want,) + ref[1:]
        for a in (data, bg) + ref:
            a.setflags(write=False)
        _cache[name] = (forest, data, bg, ref)
    return _cache[name]


def abs_leaf_sums(forest, data, missing):
    """sum over the trees of |leaf[idx_t][k]| (float64), [rows, K]"""
    _, leaf = obr.ref_of(forest, data, missing)
    d = np.asarray(forest["depths"], np.int64)
    lo = np.concatenate([[0], np.cumsum(1 << d)])
    lv = np.abs(np.asarray(forest["leaves"], np.float32).reshape(-1, forest["k"]).astype(np.float64))
    return sum((lv[lo[t] + leaf[:, t].astype(np.int64)] for t in range(d.size)), np.zeros((data.shape[0], forest["k"])))


def check(env, name, **spec):
    """The case on a handle with the flag alone: the bound, the bias bits, unused columns, additivity -> (got, worst err / bound)"""
    ta, torch = env
    avg, gb, missing = spec.get("avg", False), spec.get("bias", 0.0), spec.get("missing", obr.MISSING)
    forest, data, bg, (want, A, N) = case(name, **spec)
    F, T, K, B = forest["cols"], len(forest["depths"]), forest["k"], bg.shape[0]
    f = handle(ta, forest, missing=missing, output=ta.OUT_AVG if avg else 0, global_bias=gb)
    x, bgd = dev(env, data), dev(env, bg)
    f.set_background(bgd)
    got = run(env, f, x)
    err, bound = np.abs(got.astype(np.float64) - want)[:, :, :F], ((N + 8) * U * A)[:, :, :F]
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"{name}: max err / bound = {worst:.3f}")
    assert np.all(err <= bound), f"{name}: bound exceeded {worst:.3f}x at {np.argwhere(err > bound)[:5]}"
    # the bias column bit for bit: the host formula on the handle's own raw sums of the background
    raw = f.predict_raw(bgd).cpu().numpy().reshape(B, K)
    want_bias = np.array([ivr.bias_from_raw(raw[:, k], T, avg, gb) for k in range(K)]).astype(np.float32)
    assert np.array_equal(bits(got[:, :, F]), bits(np.broadcast_to(want_bias, got[:, :, F].shape))), f"{name}: bias column"
    assert np.array_equal(bits(want_bias), bits(oiv.bias(forest, bg, missing, avg, gb))), f"{name}: bias against the reference"
    unused = np.setdiff1d(np.arange(F), forest["fids"])
    assert not bits(got[:, :, unused]).any(), f"{name}: unused columns"
    # additivity against the handle's margins (AVG and bias applied; no sigmoid / softmax set)
    margin = f.predict(x).cpu().numpy().astype(np.float64).reshape(data.shape[0], K)
    div = T if avg and T > 0 else 1
    sx = abs_leaf_sums(forest, data, missing) / div
    sr = abs_leaf_sums(forest, bg, missing).mean(axis=0)[None, :] / div
    g64 = got.astype(np.float64)
    tol = bound.sum(axis=-1) + (T + 4) * U * (sx + sr) + 4 * U * (np.abs(margin) + np.abs(g64[:, :, F]) + abs(gb))
    assert np.all(np.abs(g64.sum(axis=-1) - margin) <= tol), f"{name}: additivity"
    f.close()
    return got, worst


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("seed", range(3))
def test_random_forests_against_the_definition(env, seed):
    rng = np.random.default_rng(100 + seed)
    cols = int(rng.integers(3, 9))
    depths = rng.integers(0, 6, int(rng.integers(3, 8))).tolist()
    check(env, f"brute_{seed}", depths=depths, cols=cols, k=int(rng.integers(1, 4)), rows=37, B=6, brute=True)


EVERY_M = dict(depths=list(range(1, 17)), cols=16, k=5, rows=65, B=3,
               fids=np.concatenate([np.random.default_rng(16).permutation(16)[:d] for d in range(1, 17)]))


def test_every_number_of_distinct_features_k5(env):
    """Trees of depths 1 .. 16, tree d on d distinct features of 16 columns: m = 1 .. 16, every instantiation, a ragged tile"""
    check(env, "every_m", **EVERY_M)


def every_m_k1():
    """Output 2 of the forest above as a forest of its own, with the reference's slice"""
    if "every_m_k1" not in _cache:
        forest, data, bg, (want, A, N) = case("every_m", **EVERY_M)
        one = dict(forest, k=1, leaves=np.ascontiguousarray(np.asarray(forest["leaves"]).reshape(-1, 5)[:, 2]))
        _cache["every_m_k1"] = (one, data, bg, (want[:, 2:3], A[:, 2:3], N[:, 2:3]))
    return _cache["every_m_k1"]


def test_every_number_of_distinct_features_k1_and_output_k_of_the_k5_handle(env):
    every_m_k1()
    got1, _ = check(env, "every_m_k1")
    got5, _ = check(env, "every_m", **EVERY_M)
    assert np.array_equal(bits(got5[:, 2:3]), bits(got1))


@pytest.mark.parametrize("m", range(1, 17))
def test_one_tree_of_m_distinct_features(env, m):
    """Worst error / bound per m (DESIGN section 30's table): one tree of depth m on m distinct features, K = 1 and K = 5"""
    fids = np.random.default_rng(m).permutation(16)[:m]
    for k in (1, 5):
        check(env, f"one_m{m:02d}_k{k}", depths=[m], cols=16, k=k, rows=65, B=3, fids=fids)


def test_depth_16_on_seven_repeated_features(env):
    check(env, "deep16", depths=[16], cols=7, k=1, rows=65, B=3, fids=np.arange(16) % 7)


def test_mixed_depths_avg_global_bias_and_unused_columns(env):
    got, _ = check(env, "mixed_avg", depths=[0, 1, 2, 3, 4, 5, 6, 0, 6], cols=9, k=3, rows=65, B=11, avg=True, bias=-0.375,
                   spread=[6, 0, 3, 4, 2, 8])
    assert np.abs(got[:, :, :9]).max() > 0


def test_a_large_background_on_depth_3(env):
    forest, data, bg, _ = case("b300", depths=[3, 3, 3], cols=4, k=2, rows=37, B=300)
    occ = oiv.occupancy(forest, bg)
    assert all(l.size <= 8 for l, _ in occ) and max(int(c.max()) for _, c in occ) > 1
    check(env, "b300", depths=[3, 3, 3], cols=4, k=2, rows=37, B=300)


@pytest.mark.parametrize("missing", [-999.0, 0.5, float("nan")])
def test_every_kind_of_missing(env, missing):
    check(env, f"missing_{missing}", depths=MIXED, cols=5, k=2, rows=65, B=9, missing=missing)


# ------------------------------------------------------------------------------------------------ exact
def test_a_row_against_itself_gives_zero(env):
    ta, torch = env
    forest, data, _, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, rows=129, B=7)
    f = handle(ta, forest)
    for r in (0, 5, 128):
        f.set_background(dev(env, data[r:r + 1]))
        got = run(env, f, dev(env, data[r:r + 1]))
        assert not bits(got[:, :, :5]).any(), r
        assert np.array_equal(bits(got[0, :, 5]), bits(f.predict_raw(dev(env, data[r:r + 1])).cpu().numpy().reshape(3))), r
    f.close()


# ------------------------------------------------------------------------------------------------ bitwise
def test_repeats_batches_rows_alone_and_permutations_give_the_same_bits(env):
    ta, torch = env
    forest, data, bg, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, rows=129, B=7)
    f = handle(ta, forest)
    f.set_background(dev(env, bg))
    x = dev(env, data)
    first = run(env, f, x)
    assert np.array_equal(bits(first), bits(run(env, f, x)))
    for r in (1, 63, 64, 65):
        assert np.array_equal(bits(run(env, f, x[:r].contiguous())), bits(first[:r])), r
    for r in (0, 63, 64, 128):
        assert np.array_equal(bits(run(env, f, x[r:r + 1].clone())), bits(first[r:r + 1])), r
    perm = np.random.default_rng(5).permutation(129)
    assert np.array_equal(bits(run(env, f, x[torch.from_numpy(perm).cuda()].contiguous())), bits(first[perm]))
    f.set_background(dev(env, bg))  # the same background again
    assert np.array_equal(bits(first), bits(run(env, f, x)))
    f.close()


def test_the_lds_form_and_the_in_place_form_give_the_same_bits(env, unforced):
    ta, torch = env
    got = {}
    for name, spec in (("mixed_k3", dict(depths=MIXED, cols=5, k=3, rows=129, B=7)), ("every_m", EVERY_M)):
        forest, data, bg, _ = case(name, **spec)
        for forced in (False, True):
            if forced:
                unforced.setenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", "1")
            f = handle(ta, forest)
            unforced.delenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", raising=False)
            f.set_background(dev(env, bg))
            got[forced] = run(env, f, dev(env, data))
            f.close()
        assert np.array_equal(bits(got[False]), bits(got[True])), name


def test_the_other_flags_change_no_bit(env):
    ta, torch = env
    forest, data, bg, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, rows=129, B=7)
    covers = osr.make_covers(forest, "half", seed=3)
    x, bgd = dev(env, data), dev(env, bg)
    alone = handle(ta, forest)
    alone.set_background(bgd)
    want = run(env, alone, x)
    for kw in (dict(contribs=True), dict(approx_contribs=True), dict(interactions=True),
               dict(contribs=True, approx_contribs=True, interactions=True)):
        f = handle(ta, forest, covers, **kw)
        f.set_background(bgd)
        assert np.array_equal(bits(run(env, f, x)), bits(want)), kw
        if kw.get("contribs"):  # ... and the flag changes no bit of theirs
            g = handle(ta, forest, covers, interventional=False, **kw)
            assert np.array_equal(bits(f.predict_contribs(x)), bits(g.predict_contribs(x)))
            g.close()
        f.close()
    alone.close()


def test_the_background_permuted_or_tiled_twice_changes_no_feature_column(env):
    ta, torch = env
    forest, data, bg, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, rows=129, B=7)
    f = handle(ta, forest)
    x = dev(env, data)
    f.set_background(dev(env, bg))
    want = run(env, f, x)
    f.set_background(dev(env, bg[np.random.default_rng(8).permutation(7)]))
    assert np.array_equal(bits(run(env, f, x)[:, :, :5]), bits(want[:, :, :5]))
    f.set_background(dev(env, np.concatenate([bg, bg])))
    assert np.array_equal(bits(run(env, f, x)[:, :, :5]), bits(want[:, :, :5]))
    f.close()


# ------------------------------------------------------------------------------------------------ against the library
def test_the_heap_expansion_on_a_dense_handle_agrees(env):
    ta, torch = env
    forest, data, bg, (want, A, N) = case("mixed_k1", depths=MIXED, cols=5, k=1, rows=37, B=6)
    T, F, B = len(MIXED), 5, 6
    ones = np.ones(int((1 << np.asarray(MIXED, np.int64)).sum()), np.float32)
    nodes, D = osr.expand_with_covers(forest, ones)
    _, Ad, Nd = ivr.paths(nodes, T, D, F, data, bg, obr.MISSING)
    f = handle(ta, forest)
    g = ta.Forest(nodes, T, D, F, missing=obr.MISSING, contribs=True)
    x, bgd = dev(env, data), dev(env, bg)
    f.set_background(bgd)
    g.set_background(bgd)
    mine = run(env, f, x)
    theirs = g.predict_contribs_interventional(x).cpu().numpy().reshape(37, 1, F + 1)
    bound = (N + 8) * U * A + (Nd[None] + B + 8) * U * Ad
    err = np.abs(mine.astype(np.float64) - theirs.astype(np.float64))
    assert np.all(err[:, :, :F] <= bound[:, :, :F]), (err / np.where(bound > 0, bound, 1.0))[:, :, :F].max()
    assert np.array_equal(bits(mine[:, :, F]), bits(theirs[:, :, F]))
    f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ lifecycle
def create_bytes(forest, k):
    """What the flag alone adds at create (include/tahoe_amd.h): the splits with compact ids, the used columns, the elements, the
    offsets, the bias and the three placeholders of the tables it does not build, and the weight tables"""
    d = np.asarray(forest["depths"], np.int64)
    so = np.concatenate([[0], np.cumsum(d)])
    elems = sum(np.unique(forest["fids"][so[t]:so[t + 1]]).size for t in range(d.size))
    return 8 * int(d.sum()) + 4 * np.unique(forest["fids"]).size + 8 * elems + 12 * d.size + 4 * k + 20 + WEIGHT_BYTES


def test_replace_clear_and_device_bytes(env):
    ta, torch = env
    forest, data, bg, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, rows=129, B=7)
    covers = osr.make_covers(forest, "int", seed=3)
    T, K = len(MIXED), 3
    plain, f = handle(ta, forest, interventional=False), handle(ta, forest)
    base = f.info().device_bytes
    assert base - plain.info().device_bytes == create_bytes(forest, K)
    shap, both = handle(ta, forest, covers, interventional=False, contribs=True), handle(ta, forest, covers, contribs=True)
    assert both.info().device_bytes - shap.info().device_bytes == WEIGHT_BYTES
    x = dev(env, data)
    small = data[:5]

    def bg_bytes(b):
        return 8 * sum(l.size for l, _ in oiv.occupancy(forest, b)) + 4 * (T + 1) + 4 * K

    tmp = dev(env, bg)
    f.set_background(tmp)
    del tmp
    assert f.info().device_bytes == base + bg_bytes(bg)
    want = run(env, f, x)
    f.set_background(dev(env, small))  # replaced
    assert f.info().device_bytes == base + bg_bytes(small)
    assert not np.array_equal(bits(run(env, f, x)), bits(want))
    f.set_background(dev(env, bg))
    assert f.info().device_bytes == base + bg_bytes(bg) and np.array_equal(bits(run(env, f, x)), bits(want))
    # a refusal keeps the background
    assert ta.lib.tahoe_forest_set_background(f._h, None, 5, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_set_background(f._h, x.data_ptr(), 2 ** 62, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_set_background(f._h, x.data_ptr(), 2 ** 31, None) == INVALID_ARG
    assert np.array_equal(bits(run(env, f, x)), bits(want))
    f.set_strategy(ta.STRATEGY_DIRECT)
    f.set_background(dev(env, bg))  # the strategy setting is left as it was and changes no bit
    assert f.get_strategy(129) == ta.STRATEGY_DIRECT and np.array_equal(bits(run(env, f, x)), bits(want))
    f.set_background(None)
    assert f.info().device_bytes == base
    out = torch.zeros((129, 3, 6), device="cuda")
    assert ta.lib.tahoe_forest_predict_contribs_interventional(f._h, out.data_ptr(), x.data_ptr(), 129, None) == UNSUPPORTED
    assert "no background set" in ta.lib.tahoe_last_error().decode()
    f.set_background(dev(env, bg))
    assert ta.lib.tahoe_forest_set_background(f._h, None, 0, None) == 0  # (NULL, 0) clears
    assert f.info().device_bytes == base
    for h in (plain, f, shap, both):
        h.check()
        h.close()


def test_graph_capture_after_set_background(env):
    ta, torch = env
    forest, data, bg, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, rows=129, B=7)
    f = handle(ta, forest)
    f.set_background(dev(env, bg))
    x = dev(env, data)
    want = run(env, f, x)
    out = torch.zeros((129, 3, 6), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        f.predict_contribs_interventional(x, out=out, stream=side)
    for _ in range(2):
        out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(want))
    f.close()


def test_refusals_in_order_and_zero_rows(env):
    ta, torch = env
    forest, data, bg, _ = case("mixed_k3", depths=MIXED, cols=5, k=3, rows=129, B=7)
    covers = osr.make_covers(forest, "int", seed=3)
    lib = ta.lib
    x, bgd = dev(env, data), dev(env, bg)
    out = torch.full((129 * 3 * 6,), SENTINEL, device="cuda")
    PREDICT, SET = "tahoe_forest_predict_contribs_interventional", "tahoe_forest_set_background"
    # 1. the flag is missing, whatever else the handle serves: "oblivious" and the call's name, before every other check
    for kw in (dict(), dict(contribs=True, approx_contribs=True, interactions=True)):
        f = handle(ta, forest, covers if kw else None, interventional=False, **kw)
        assert lib.tahoe_forest_set_background(f._h, None, 5, None) == UNSUPPORTED
        msg = lib.tahoe_last_error().decode()
        assert "oblivious" in msg and SET in msg, msg
        assert lib.tahoe_forest_predict_contribs_interventional(f._h, None, None, 0, None) == UNSUPPORTED
        msg = lib.tahoe_last_error().decode()
        assert "oblivious" in msg and PREDICT in msg, msg
        f.close()
    f = handle(ta, forest)
    # 2. no background, before rows == 0 and the NULL pointers
    assert lib.tahoe_forest_predict_contribs_interventional(f._h, None, None, 0, None) == UNSUPPORTED
    msg = lib.tahoe_last_error().decode()
    assert "no background set" in msg and PREDICT in msg, msg
    f.set_background(bgd)
    # 3. rows == 0, before the NULL pointers
    assert lib.tahoe_forest_predict_contribs_interventional(f._h, None, None, 0, None) == 0
    assert tuple(f.predict_contribs_interventional(x[:0].contiguous()).shape) == (0, 3, 6)
    # 4. NULL pointers, 5. a size that overflows
    assert lib.tahoe_forest_predict_contribs_interventional(f._h, None, x.data_ptr(), 129, None) == INVALID_ARG
    assert lib.tahoe_forest_predict_contribs_interventional(f._h, out.data_ptr(), None, 129, None) == INVALID_ARG
    assert "null argument" in lib.tahoe_last_error().decode()
    assert lib.tahoe_forest_predict_contribs_interventional(f._h, out.data_ptr(), x.data_ptr(), 2 ** 62, None) == INVALID_ARG
    assert "overflow" in lib.tahoe_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    f.check()
    f.close()
