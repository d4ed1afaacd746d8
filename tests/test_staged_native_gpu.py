"""Staged prediction on oblivious and vector-leaf handles created with TAHOE_CREATE_STAGED (tahoe_forest_set_stages,
tahoe_forest_predict_staged, tahoe_forest_get_staged_strategy).  Every comparison is for equal bits:
  - raw sums against numpy: the sequential float32 running sum of the reference walk's per-tree leaf vectors, read at
    rounds[s] - 1;
  - output bits against the library itself: predict on a handle of the same create call from the first rounds[s] trees;
  - category sets, a handle that also explains, the bookkeeping of set_stages, and graph capture.
Shapes are the smallest at which the stage cursor can go wrong: 11 trees (two windows of the four trees in flight and a tail of
three), stages at every position of a window, on a window's end, inside the tail and on the last tree; 130 rows (two 64-row tiles
and a tail of two; one partly filled DIRECT block); K across the 8-class block; num_cols with and without the 16-byte staging
reads.  Needs an MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oblivious_cat_ref as ocr  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import vector_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = obr.MISSING
INVALID_ARG, UNSUPPORTED = 1, 7
ROWS, T = 130, 11
DEPTHS = [0, 3, 6, 1, 2, 5, 4, 6, 3, 2, 0]  # a depth-0 tree first and last
CAT_DEPTHS = [2, 0, 6, 1, 3, 5, 4, 6, 3, 2, 0]  # (tree 0 has a split: the first stage of a forest with sets has one)
KINDS = ["leaf", 5, "stump", 8, 3, 6, "leaf", 8, 2, 7, 4]  # irregular trees of depth <= 8, two single leaves
STAGE_SETS = ([1, 2, 3, 4, 5, 8, 9, 11], [11], [4], [7], [10])
STRATEGIES = ("DIRECT", "ROWTILE", "AUTO")
assert len(DEPTHS) == len(CAT_DEPTHS) == len(KINDS) == T


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


# ---- the forests, their data and the running sums, computed once and read-only ----
def running_sums(per_tree):
    """per_tree float32 [rows, T, K] -> the float32 sum from +0.0 over the trees in order, after every tree: [rows, T, K]"""
    acc = np.zeros(per_tree[:, 0].shape, np.float32)
    out = np.empty_like(per_tree)
    for t in range(per_tree.shape[1]):
        acc = acc + per_tree[:, t]  # float32 + float32, one tree after the other
        out[:, t] = acc
    return out


def oblivious_leaf_vectors(forest, leaf):
    lo = np.concatenate([[0], np.cumsum(1 << np.asarray(forest["depths"], np.int64))])[:-1]
    return np.asarray(forest["leaves"], np.float32).reshape(-1, forest["k"])[lo[None, :] + leaf.astype(np.int64)]


def vector_leaf_vectors(forest, leaf):
    at = forest["trees"].astype(np.int64)[None, :] + leaf.astype(np.int64)
    return forest["leaves"][forest["nodes"]["left_idx"][at]]


_cache = {}


def case(kind, cols, k):
    """(forest, data [ROWS, cols], running sums [ROWS, T, K]); kind: "oblivious", "vector" or "cat" """
    key = (kind, cols, k)
    if key not in _cache:
        seed = 3400 + 10 * cols + k
        if kind == "vector":
            forest = vr.make_named(KINDS, cols, k, seed)
            data = vr.make_data(ROWS, cols, seed=seed + 1)
            sums, leaf, _ = vr.vector_ref(forest, data)
            per_tree = vector_leaf_vectors(forest, leaf)
        elif kind == "cat":
            forest = ocr.sets_forest(CAT_DEPTHS, cols, k, seed)
            data = ocr.sets_data(ROWS, cols, seed=seed + 1)
            sums, leaf = ocr.cat_ref(forest, data)
            per_tree = oblivious_leaf_vectors(forest, leaf)
        else:
            forest = obr.make_forest(DEPTHS, cols, k, seed)
            data = obr.make_data(ROWS, cols, seed=seed + 1)
            sums, leaf = obr.ref_of(forest, data)
            per_tree = oblivious_leaf_vectors(forest, leaf)
        run = running_sums(per_tree)
        assert np.array_equal(run[:, -1].view(np.uint32), sums.view(np.uint32))  # (the last running sum is the reference's own)
        for a in (data, run):
            a.setflags(write=False)
        _cache[key] = (forest, data, run)
    return _cache[key]


def want_of(run, rounds, k):
    w = run[:, np.asarray(rounds) - 1]  # [rows, S, K]
    return w[:, :, 0] if k == 1 else w


def cut(forest, n):
    """The first n trees of a forest of any of the three kinds"""
    if "nodes" in forest:
        end = int(forest["trees"][n]) if n < forest["trees"].size else forest["nodes"].size
        return dict(forest, nodes=forest["nodes"][:end], trees=forest["trees"][:n])
    d = np.asarray(forest["depths"], np.int64)
    s, v = int(d[:n].sum()), int((1 << d[:n]).sum()) * forest["k"]
    part = dict(forest, depths=forest["depths"][:n], fids=forest["fids"][:s], thr=forest["thr"][:s], def_left=forest["def_left"][:s],
                leaves=forest["leaves"][:v])
    if "cats" in forest:
        part["cats"] = {i: c for i, c in forest["cats"].items() if i < s}
        part["ml"] = frozenset(i for i in forest["ml"] if i < s)
    return part


def handle(ta, forest, **kw):
    if "nodes" in forest:
        return ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=MISSING, **kw)
    if forest.get("cats"):
        kw.update(ocr.handle_args(forest))
    return ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], forest["cols"],
                              leaf_dim=forest["k"], missing=MISSING, **kw)


# ------------------------------------------------------------------------------------------ 1, 2: raw bits against numpy
@pytest.mark.parametrize("k", [1, 3, 8, 9])
@pytest.mark.parametrize("cols", [7, 8])
@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_raw_stages_match_the_running_sums(env, kind, cols, k):
    ta, torch = env
    forest, data, run = case(kind, cols, k)
    f = handle(ta, forest, staged=True)
    x = torch.from_numpy(data.copy()).cuda()
    for rounds in STAGE_SETS:
        f.set_stages(rounds)
        want = bits(want_of(run, rounds, k))
        for strat in STRATEGIES:
            f.set_strategy(getattr(ta, "STRATEGY_" + strat))
            assert f.staged_strategy(ROWS) == (ta.STRATEGY_DIRECT if strat == "DIRECT" else ta.STRATEGY_ROWTILE)
            out = f.predict_staged(x)
            assert tuple(out.shape) == ((ROWS, len(rounds)) if k == 1 else (ROWS, len(rounds), k))
            assert np.array_equal(bits(out), want), (rounds, strat)
            if rounds is STAGE_SETS[0]:  # a row gives the same bits in any batch
                for lo, hi in ((0, 1), (0, 64), (129, 130), (66, 130)):
                    part = f.predict_staged(x[lo:hi].contiguous())
                    assert np.array_equal(bits(part), want[lo:hi]), (strat, lo, hi)
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------ 3: output bits against truncated handles
K1_OUTPUTS = [("AVG", 0.0), ("AVG|SIGMOID", 0.0), ("SIGMOID|THRESHOLD", 0.0), ("AVG|THRESHOLD", 0.375), ("RAW", -1.25)]
K3_OUTPUTS = [("RAW", 0.0), ("AVG", 0.0), ("AVG|SIGMOID", 0.0), ("SOFTMAX", 0.0), ("AVG|SOFTMAX", 0.375)]


def output_bits(ta, names):
    out = 0
    for n in names.split("|"):
        out |= getattr(ta, "OUT_" + n)
    return out


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_outputs_match_truncated_handles(env, kind, k):
    ta, torch = env
    forest, data, _ = case(kind, 8, k)
    x = torch.from_numpy(data.copy()).cuda()
    rounds = STAGE_SETS[0]
    for names, bias in (K1_OUTPUTS if k == 1 else K3_OUTPUTS):
        kw = dict(output=output_bits(ta, names), threshold=0.25, global_bias=bias)
        want = []
        for n in rounds:  # the same create call and parameters on the first n trees, without the flag
            g = handle(ta, cut(forest, n), **kw)
            want.append(bits(g.predict(x)))
            g.close()
        want = np.stack(want, axis=1)
        f = handle(ta, forest, staged=True, **kw)
        f.set_stages(rounds)
        for strat in ("DIRECT", "ROWTILE"):
            f.set_strategy(getattr(ta, "STRATEGY_" + strat))
            assert np.array_equal(bits(f.predict_staged(x)), want), (names, strat)
        f.close()


# ------------------------------------------------------------------------------------------ 4: category sets
@pytest.mark.parametrize("k", [1, 9])
def test_category_sets(env, k):
    ta, torch = env
    forest, data, run = case("cat", 8, k)
    widths = [ocr.nwords_of(c) for c in forest["cats"].values()]
    assert any(w <= 1 for w in widths) and any(w >= 2 for w in widths)  # sets in their record and sets in the pool
    assert any(i < CAT_DEPTHS[0] for i in forest["cats"])
    x = torch.from_numpy(data.copy()).cuda()
    rounds = [1, 5, 11]
    want = []
    for n in rounds:
        g = handle(ta, cut(forest, n))
        want.append(bits(g.predict(x)))
        g.close()
    want = np.stack(want, axis=1)
    assert np.array_equal(want, bits(want_of(run, rounds, k)))
    f = handle(ta, forest, staged=True)
    f.set_stages(rounds)
    for strat in ("DIRECT", "ROWTILE"):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert np.array_equal(bits(f.predict_staged(x)), want), strat
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------ 5: beside explanations
def test_staged_beside_contribs(env):
    ta, torch = env
    forest, data, run = case("oblivious", 8, 3)
    covers = np.random.default_rng(5).integers(0, 50, int((1 << np.asarray(DEPTHS, np.int64)).sum())).astype(np.float32)
    x = torch.from_numpy(data.copy()).cuda()
    rounds = STAGE_SETS[0]
    both = handle(ta, forest, leaf_covers=covers, contribs=True, staged=True)
    only_contribs = handle(ta, forest, leaf_covers=covers, contribs=True)
    only_staged = handle(ta, forest, staged=True)
    assert both.info().device_bytes == only_contribs.info().device_bytes
    both.set_stages(rounds)
    only_staged.set_stages(rounds)
    assert np.array_equal(bits(both.predict_contribs(x)), bits(only_contribs.predict_contribs(x)))
    got = bits(both.predict_staged(x))
    assert np.array_equal(got, bits(only_staged.predict_staged(x))) and np.array_equal(got, bits(want_of(run, rounds, 3)))
    with pytest.raises(ta.TahoeError) as e:  # each flag serves its own calls only
        only_contribs.set_stages(rounds)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ta.TahoeError) as e:
        only_staged.predict_contribs(x)
    assert e.value.status == UNSUPPORTED
    for f in (both, only_contribs, only_staged):
        f.close()


# ------------------------------------------------------------------------------------------ 6: bookkeeping
@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_bookkeeping(env, kind):
    ta, torch = env
    k = 3
    forest, data, run = case(kind, 8, k)
    x = torch.from_numpy(data.copy()).cuda()
    plain, f = handle(ta, forest), handle(ta, forest, staged=True)
    base = plain.info().device_bytes
    assert f.info().device_bytes == base  # the flag builds no table
    assert f.staged_strategy(ROWS) == 0
    with pytest.raises(ta.TahoeError) as e:
        f.predict_staged(x)
    assert e.value.status == UNSUPPORTED and "no stages are set" in str(e.value)

    f.set_stages([2, 6, 7])
    assert f.info().device_bytes == base + 4 * 3
    assert f.staged_strategy(ROWS) == ta.STRATEGY_ROWTILE  # AUTO: a tile of 8 columns fits LDS
    assert np.array_equal(bits(f.predict_staged(x)), bits(want_of(run, [2, 6, 7], k)))
    f.set_stages([1, 3, 5, 9, 11])  # a second call replaces the stages
    assert f.info().device_bytes == base + 4 * 5
    assert np.array_equal(bits(f.predict_staged(x)), bits(want_of(run, [1, 3, 5, 9, 11], k)))
    for bad, index in (([0], 0), ([12], 0), ([3, 3], 1), ([2, 5, 4], 2)):
        with pytest.raises(ta.TahoeError) as e:
            f.set_stages(bad)
        assert e.value.status == INVALID_ARG and f"rounds[{index}]" in str(e.value), str(e.value)
        assert f.info().device_bytes == base + 4 * 5
        assert np.array_equal(bits(f.predict_staged(x)), bits(want_of(run, [1, 3, 5, 9, 11], k)))  # the previous stages stay
    f.set_stages(None)
    assert f.info().device_bytes == base and f.staged_strategy(ROWS) == 0
    with pytest.raises(ta.TahoeError) as e:
        f.predict_staged(x)
    assert e.value.status == UNSUPPORTED and "no stages are set" in str(e.value)

    # an unflagged handle refuses as it always has
    rounds = np.array([1, 2], np.int32)
    out = torch.full((ROWS * 2 * k,), 7.0, device="cuda")
    word = "oblivious" if kind == "oblivious" else "vector-leaf"
    for name, call in (("tahoe_forest_set_stages", lambda: ta.lib.tahoe_forest_set_stages(plain._h, rounds.ctypes.data, 2)),
                       ("tahoe_forest_predict_staged",
                        lambda: ta.lib.tahoe_forest_predict_staged(plain._h, out.data_ptr(), x.data_ptr(), ROWS, None))):
        assert call() == UNSUPPORTED
        msg = ta.lib.tahoe_last_error().decode()
        assert msg.startswith(f"{name}: not served on a") and word in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and plain.staged_strategy(ROWS) == 0
    assert plain.info().device_bytes == base

    # after everything the flagged handle predicts what the plain one does, and the last stage [T] is that sum
    f.set_stages([T])
    last = f.predict_staged(x)
    raw = f.predict_raw(x)
    assert np.array_equal(bits(raw), bits(last[:, 0])) and np.array_equal(bits(raw), bits(plain.predict_raw(x)))
    assert np.array_equal(bits(raw), bits(run[:, -1]))
    f.check()
    f.close()
    plain.close()


@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_a_forest_without_trees_has_no_valid_stage(env, kind):
    ta, torch = env
    forest = vr.make([], np.zeros((2, 3), np.float32), 3, 5) if kind == "vector" else obr.make_forest([], 5, 3, seed=1)
    f = handle(ta, forest, staged=True)
    with pytest.raises(ta.TahoeError) as e:
        f.set_stages([1])
    assert e.value.status == INVALID_ARG and "rounds[0] = 1 is outside [1, 0]" in str(e.value), str(e.value)
    f.set_stages(None)  # (NULL, 0) is fine
    f.set_stages([])
    assert f.staged_strategy(ROWS) == 0
    x = torch.zeros((ROWS, 5), device="cuda")
    with pytest.raises(ta.TahoeError) as e:
        f.predict_staged(x)
    assert e.value.status == UNSUPPORTED and "no stages are set" in str(e.value)
    assert not bits(f.predict_raw(x)).any()
    f.close()


@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_auto_is_direct_when_the_tile_cannot_fit(env, kind):
    ta, torch = env
    lds = C.c_int(0)
    assert ta.lib.tahoe_device_lds_bytes(C.byref(lds)) == 0
    cols = lds.value // 256 + 1  # one 64-row float32 tile is 256 bytes per column
    rows, k = 4, 3
    if kind == "vector":
        forest = vr.make_named(KINDS, cols, k, seed=91)
        data = vr.make_data(rows, cols, seed=92)
        per_tree = vector_leaf_vectors(forest, vr.vector_ref(forest, data)[1])
    else:
        forest = obr.make_forest(DEPTHS, cols, k, seed=91)
        data = obr.make_data(rows, cols, seed=92)
        per_tree = oblivious_leaf_vectors(forest, obr.ref_of(forest, data)[1])
    rounds = STAGE_SETS[0]
    f = handle(ta, forest, staged=True)
    f.set_stages(rounds)
    assert f.staged_strategy(rows) == ta.STRATEGY_DIRECT and f.get_strategy(rows) == ta.STRATEGY_DIRECT
    out = f.predict_staged(torch.from_numpy(data.copy()).cuda())
    assert np.array_equal(bits(out), bits(want_of(running_sums(per_tree), rounds, k)))
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------ 7: capture
def test_staged_predict_is_capturable(env):
    """After set_stages the call allocates nothing: it can be captured into a HIP graph and replayed."""
    ta, torch = env
    k = 9
    forest, data, _ = case("oblivious", 8, k)
    rounds = STAGE_SETS[0]
    f = handle(ta, forest, staged=True, output=ta.OUT_AVG)  # (with the epilogue kernel in the graph)
    f.set_stages(rounds)
    x = torch.from_numpy(data.copy()).cuda()
    out = torch.zeros((ROWS, len(rounds), k), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = f.predict_staged(x).clone()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f.predict_staged(x, out=out)
    g.replay()
    torch.cuda.synchronize()
    f.check()
    assert np.array_equal(bits(out), bits(eager))
    f.close()
