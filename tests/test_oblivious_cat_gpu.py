"""Category-set splits on oblivious handles (tahoe_oblivious_forest_create_cat) on the GPU.  Needs an MI355X.

Sums and leaf indices against the numpy rule of tests/oblivious_cat_ref.py under DIRECT, ROWTILE and AUTO, and against the
library's own categorical SparseForest on the expansion into complete trees.  The two identities of DESIGN.md section 31 (members
right: x >= k <=> x in {c : k <= c < 32 W} below 32 W; members left: x >= k <=> x not in {c : c < k} for x >= 0) make the numeric
oblivious handle the reference of all calls, bit for bit, with W = 1 (sets in the split record) and W = 3 (sets in the pool).
Genuine sets go through the four explanation calls at the bars their numeric tests hold: TreeSHAP |phi - phi64| <= (N + 4 (D + 2))
2^-24 A against poly and the bits of emulate (tests/test_oblivious_shap_gpu.py, test_oblivious_edges_gpu.py), Saabas and the bias
column bit for bit, interaction values the bits of emulate and (N + 6 (D + 2)) 2^-24 A off the diagonal
(tests/test_oblivious_inter_gpu.py), interventional values (N + 8) 2^-24 A (tests/test_oblivious_iv_gpu.py) -- the restatements fed
the sets through oblivious_cat_ref.seam.  The bars depend on the trees' shape, covers and leaves only, which the sets leave alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interventional_ref as ivr  # noqa: E402
import oblivious_cat_ref as ocr  # noqa: E402
import oblivious_inter_ref as oir  # noqa: E402
import oblivious_iv_ref as oiv  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = obr.MISSING
UNSUPPORTED = 7
U = 2.0 ** -24
ROWS = 130
BATCHES = (1, 63, 64, 65, 130)
MIXED = [0, 1, 2, 6, 3, 6, 4]  # depths of the explanation cases; on 5 columns the features repeat within a tree
_cache = {}

# name -> (depths, num_cols, K): tree counts that are no multiple of 4; 40 columns take the 16-byte staging reads, 5 and 7 do not
FORESTS = {
    "mixed_k1": ([0, 1, 2, 6, 16], 5, 1),
    "mixed_k3": ([0, 1, 2, 6, 16], 5, 3),
    "mid_k3": ([0, 1, 2, 6, 9], 5, 3),
    "seven_k1": ([2, 6, 0, 1, 6, 1, 2], 7, 1),
    "nine_k9": ([6, 2, 1, 0, 1, 6, 2, 1, 0], 40, 9),
}


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


def shaped(sums, k):
    return sums[:, 0] if k == 1 else sums


def handle(ta, forest, covers=None, **kw):
    """The forest on an oblivious handle: through tahoe_oblivious_forest_create_cat when it has sets"""
    if forest.get("cats"):
        kw.update(ocr.handle_args(forest))
    return ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], forest["cols"],
                              leaf_dim=forest["k"], missing=MISSING, leaf_covers=covers, **kw)


def sparse_handle(ta, forest, covers=None, **kw):
    """The expansion into complete trees on the library's categorical sparse handle"""
    nodes, trees, categories, members_left, cv = ocr.expand_to_sparse(forest, covers)
    return ta.capi.SparseForest(nodes, trees, forest["cols"], missing=MISSING, covers=cv, num_classes=forest["k"],
                           categories=categories, members_left=members_left, **kw)


def covered(forest):
    """What the issue asks of the sets of a test forest"""
    cats, ml = forest["cats"], forest["ml"]
    d = np.asarray(forest["depths"], np.int64)
    off = np.concatenate([[0], np.cumsum(d)])
    nw = {s: ocr.nwords_of(c) for s, c in cats.items()}
    sizes = {len(c) for c in cats.values()}
    assert {0, 1} <= sizes and 0 in nw.values() and 1 in nw.values() and 2 in nw.values() and 3 in nw.values()
    assert any(max(c) == 30 for c in cats.values() if c) and any(max(c) == 31 for c in cats.values() if c)  # 31 and 32 categories
    assert any(max(c) == 32 for c in cats.values() if c)  # ... and the first pooled width
    assert any(s in ml for s in cats) and any(s not in ml for s in cats)
    assert 0 in cats and int(off[-1]) - 1 in cats  # level 0 of the first tree, the last level of the last
    deepest = int(np.argmax(d))
    assert all(s in cats for s in range(off[deepest], off[deepest + 1]))  # every level of a tree
    two_sets = both = False
    for t in range(d.size):
        levels = range(int(off[t]), int(off[t + 1]))
        cat_f = [int(forest["fids"][s]) for s in levels if s in cats]
        num_f = {int(forest["fids"][s]) for s in levels if s not in cats}
        two_sets |= len(cat_f) != len(set(cat_f))
        both |= bool(set(cat_f) & num_f)
    assert two_sets and both  # one feature in two sets of a tree; one feature numeric and categorical in a tree
    return forest


def covered_forest(depths, cols, k, seed):
    """sets_forest of the first seed from `seed` on whose forest has every kind of set asked for"""
    for s in range(seed, seed + 100):
        try:
            return covered(ocr.sets_forest(depths, cols, k, seed=s))
        except AssertionError:
            continue
    raise AssertionError("no seed gives a forest with every kind of set")


def case(name):
    """(forest with sets, data [ROWS, cols], reference sums [ROWS, K], reference leaves [ROWS, T]), computed once and read-only"""
    if name not in _cache:
        depths, cols, k = FORESTS[name]
        # (on 40 columns a feature rarely repeats within a tree: nine_k9 is taken as it comes)
        forest = ocr.sets_forest(depths, cols, k, seed=1009) if name == "nine_k9" else covered_forest(depths, cols, k, 1000 + 100 * len(name))
        data = ocr.sets_data(ROWS, cols, seed=7 + cols)
        sums, leaf = ocr.cat_ref(forest, data)
        for a in (data, sums, leaf):
            a.setflags(write=False)
        _cache[name] = (forest, data, sums, leaf)
    return _cache[name]


# ------------------------------------------------------------------------------------------------ 1: against the rule
@pytest.mark.parametrize("name", list(FORESTS))
def test_sums_and_leaves_match_the_rule(env, name):
    ta, torch = env
    forest, data, want, want_leaf = case(name)
    k = forest["k"]
    f = handle(ta, forest)
    assert f.num_classes == k
    x = dev(env, data)
    perm = np.random.default_rng(5).permutation(ROWS)
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
        for r in (0, 64, ROWS - 1):  # a row alone and inside a batch
            assert np.array_equal(bits(f.predict_raw(x[r:r + 1].clone())), bits(shaped(want[r:r + 1], k))), (strat, r)
        leaf, sums = f.predict_leaf_idx(x[torch.from_numpy(perm).cuda()].contiguous())  # permuted rows, permuted results
        assert np.array_equal(bits(sums), bits(shaped(want[perm], k))) and np.array_equal(bits(leaf), want_leaf[perm].view(np.uint32))
        got[strat] = bits(f.predict_raw(x))
    assert np.array_equal(got["DIRECT"], got["ROWTILE"]) and np.array_equal(got["AUTO"], got["ROWTILE"])
    f.check()
    f.close()


def test_a_tile_that_cannot_fit_lds_runs_direct(env):
    ta, torch = env
    lds = C.c_int()
    assert ta.lib.tahoe_device_lds_bytes(C.byref(lds)) == 0
    cols = lds.value // 256 + 1  # one 64-row float32 tile is 256 bytes per column
    forest = ocr.sets_forest([2, 6, 1], cols, 1, seed=77, share=0.7)
    forest["fids"][:2] = (cols - 1, 0)
    assert any(ocr.nwords_of(c) >= 2 for c in forest["cats"].values())
    data = ocr.sets_data(65, cols, seed=78)
    want, want_leaf = ocr.cat_ref(forest, data)
    f = handle(ta, forest)
    assert f.kernel_form(65) == "oblivious_direct" and f.get_strategy(65) == ta.STRATEGY_DIRECT
    with pytest.raises(ta.TahoeError) as e:
        f.set_strategy(ta.STRATEGY_ROWTILE)
    assert e.value.status == UNSUPPORTED
    leaf, sums = f.predict_leaf_idx(dev(env, data))
    assert np.array_equal(bits(sums), bits(want[:, 0])) and np.array_equal(bits(leaf), want_leaf.view(np.uint32))
    f.check()
    f.close()


def cut(forest, lo, hi):
    """Trees lo .. hi - 1 of a forest with sets"""
    d = forest["depths"].astype(np.int64)
    s = np.concatenate([[0], np.cumsum(d)])
    v = np.concatenate([[0], np.cumsum(1 << d)]) * forest["k"]
    part = dict(forest, depths=forest["depths"][lo:hi], fids=forest["fids"][s[lo]:s[hi]], thr=forest["thr"][s[lo]:s[hi]],
                def_left=forest["def_left"][s[lo]:s[hi]], leaves=forest["leaves"][v[lo]:v[hi]])
    part["cats"] = {q - int(s[lo]): c for q, c in forest["cats"].items() if s[lo] <= q < s[hi]}
    part["ml"] = frozenset(q - int(s[lo]) for q in forest["ml"] if s[lo] <= q < s[hi])
    return part


@pytest.mark.parametrize("strat", ["DIRECT", "ROWTILE"])
def test_accumulate_continues_the_sum(env, strat):
    ta, torch = env
    forest, data, want, _ = case("seven_k1")
    x = dev(env, data)
    first, second = handle(ta, cut(forest, 0, 3)), handle(ta, cut(forest, 3, 7))
    for h in (first, second):
        h.set_strategy(getattr(ta, "STRATEGY_" + strat))
    sums = first.predict_raw(x)
    assert not np.array_equal(bits(sums), bits(want[:, 0]))
    second.predict_accumulate(x, sums)
    assert np.array_equal(bits(sums), bits(want[:, 0]))
    first.close()
    second.close()


# ------------------------------------------------------------------------------------------------ 2: the sparse expansion
# (the expansion of a tree of depth 16 is 2^17 sparse nodes per output: the forests of depth <= 9 go through it)
OUTPUTS = [(name, output, bias) for name, (depths, _, k) in FORESTS.items() if max(depths) <= 9
           for output, bias in [("RAW", 0.0), ("AVG", 0.25), ("SIGMOID", -0.5), ("SOFTMAX", 0.125)] if output != "SOFTMAX" or k > 1]


@pytest.mark.parametrize("name,output,bias", OUTPUTS)
def test_predictions_equal_the_categorical_sparse_expansion(env, name, output, bias):
    ta, torch = env
    forest, data, want, want_leaf = case(name)
    k = forest["k"]
    kw = dict(output=getattr(ta, "OUT_" + output) if output != "RAW" else 0, global_bias=bias)
    f, g = handle(ta, forest, **kw), sparse_handle(ta, forest, **kw)
    x = dev(env, data)
    a, b = f.predict(x), g.predict(x)
    assert np.array_equal(bits(a), bits(b)), (name, output)
    if output == "RAW":
        assert np.array_equal(bits(a), bits(shaped(want, k)))
        leaf, _ = g.predict_leaf_idx(x)
        assert np.array_equal(ocr.sparse_leaf_to_oblivious(leaf.cpu().numpy(), forest), want_leaf)
    else:
        assert not np.array_equal(bits(a), bits(shaped(want, k)))  # the transform ran
    f.check()
    f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ 3: the two identities
FLAGS = dict(contribs=True, approx_contribs=True, interactions=True, interventional=True)


def every_call(env, f, x, bg):
    """name -> bits of every call the handle serves"""
    ta, torch = env
    out = {}
    for strat in ("DIRECT", "ROWTILE", "AUTO"):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        out["predict " + strat] = bits(f.predict(x))
        out["predict_raw " + strat] = bits(f.predict_raw(x))
        leaf, sums = f.predict_leaf_idx(x)
        out["leaf " + strat], out["leaf sums " + strat] = bits(leaf), bits(sums)
    out["contribs"] = bits(f.predict_contribs(x))
    out["approx"] = bits(f.predict_contribs_approx(x))
    out["interactions"] = bits(f.predict_interactions(x))
    f.set_background(bg)
    out["interventional"] = bits(f.predict_contribs_interventional(x))  # bias column included
    f.check()
    return out


@pytest.mark.parametrize("left", [False, True], ids=["members_right", "members_left"])
@pytest.mark.parametrize("W", [1, 3], ids=["inline", "pooled"])
@pytest.mark.parametrize("k", [1, 3])
def test_identities_make_the_numeric_handle_the_reference_of_every_call(env, unforced, W, left, k):
    ta, torch = env
    numeric = ocr.integer_thresholds(obr.make_forest(MIXED, 5, k, seed=40 + k), W, seed=41)
    cat = (ocr.members_left_of if left else ocr.members_right)(numeric, W, every=1 if W == 1 else 2)  # W = 3: numeric levels mixed in
    pooled = sum(ocr.nwords_of(c) >= 2 for c in cat["cats"].values())
    assert (pooled == 0) if W == 1 else (pooled > 0)
    covers = osr.make_covers(numeric, "half", seed=42)
    x = dev(env, ocr.identity_data(ROWS, 5, W, seed=43, left=left))
    bg = dev(env, ocr.identity_data(9, 5, W, seed=44, left=left))
    kw = dict(output=ta.OUT_AVG, global_bias=0.25, **FLAGS)
    f, g = handle(ta, numeric, covers, **kw), handle(ta, cat, covers, **kw)
    assert g.info().device_bytes == f.info().device_bytes + ocr.pool_bytes(cat)
    want, got = every_call(env, f, x, bg), every_call(env, g, x, bg)
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    unforced.setenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", "1")  # ... and in the in-place form of the explanation kernels
    h = handle(ta, cat, covers, **kw)
    unforced.delenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", raising=False)
    forced = every_call(env, h, x, bg)
    for name in ("contribs", "approx", "interactions", "interventional"):
        assert np.array_equal(forced[name], want[name]), name
    for q in (f, g, h):
        q.close()


# ------------------------------------------------------------------------------------------------ 4: genuine sets, explanations
def shap_case(k, kind, avg=False, bias=0.0):
    """(forest with sets, covers, data, background, references), computed once and read-only; the restatements see the sets"""
    name = f"shap_k{k}_{kind}_{avg}"
    if name not in _cache:
        forest = covered_forest(MIXED, 5, k, 2000 + 100 * k)
        covers = osr.make_covers(forest, kind, seed=31 + k)
        data, bg = ocr.sets_data(ROWS, 5, seed=14), ocr.sets_data(7, 5, seed=15)
        with ocr.seam():
            ref = dict(poly=osr.poly(forest, covers, data, avg=avg, global_bias=bias),
                       emulate=osr.emulate(forest, covers, data, avg=avg, global_bias=bias),
                       saabas=osr.saabas(forest, covers, data, avg=avg, global_bias=bias),
                       inter_poly=oir.poly(forest, covers, data, avg=avg, global_bias=bias),
                       inter_emulate=oir.emulate(forest, covers, data, avg=avg, global_bias=bias),
                       iv=oiv.paths(forest, data, bg, MISSING, avg=avg, global_bias=bias),
                       iv_bias=oiv.bias(forest, bg, MISSING, avg, bias))
        _cache[name] = (forest, covers, data, bg, ref)
    return _cache[name]


def explain(env, f, call, x, dims=1):
    rows, k, F1 = x.shape[0], f.num_classes, f.num_cols + 1
    return getattr(f, call)(x).cpu().numpy().reshape((rows, k) + (F1,) * dims)


SHAP_CASES = [(1, "int", False, 0.0), (3, "half", True, -0.375), (9, "most", False, 0.0)]


@pytest.mark.parametrize("k,kind,avg,bias", SHAP_CASES)
def test_treeshap_and_saabas_follow_the_sets(env, unforced, k, kind, avg, bias):
    ta, torch = env
    forest, covers, data, _, ref = shap_case(k, kind, avg, bias)
    D = int(max(forest["depths"]))
    f = handle(ta, forest, covers, contribs=True, approx_contribs=True, output=ta.OUT_AVG if avg else 0, global_bias=bias)
    x = dev(env, data)
    got32 = explain(env, f, "predict_contribs", x)
    want, A, N = ref["poly"]
    err, bound = np.abs(got32.astype(np.float64) - want)[:, :, :-1], ((N + 4 * (D + 2)) * U * A)[:, :, :-1]
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"k{k} {kind}: max err / bound = {worst:.3f}")
    assert np.all(err <= bound), f"bound exceeded {worst:.3f}x at {np.argwhere(err > bound)[:5]}"
    assert np.array_equal(bits(got32), bits(ref["emulate"]))
    b = osr.bias_f32(forest, covers, avg, bias)
    assert np.array_equal(bits(got32[:, :, -1]), bits(np.broadcast_to(b, got32[:, :, -1].shape)))
    saabas = explain(env, f, "predict_contribs_approx", x)
    assert np.array_equal(bits(saabas), bits(ref["saabas"]))
    for r in BATCHES[:-1]:
        xr = x[:r].contiguous()
        assert np.array_equal(bits(explain(env, f, "predict_contribs", xr)), bits(got32[:r])), r
        assert np.array_equal(bits(explain(env, f, "predict_contribs_approx", xr)), bits(saabas[:r])), r
    perm = np.random.default_rng(5).permutation(ROWS)
    xp = x[torch.from_numpy(perm).cuda()].contiguous()
    assert np.array_equal(bits(explain(env, f, "predict_contribs", xp)), bits(got32[perm]))
    f.check()
    f.close()


@pytest.mark.parametrize("k,kind,avg,bias", SHAP_CASES)
def test_interaction_values_follow_the_sets(env, unforced, k, kind, avg, bias):
    ta, torch = env
    forest, covers, data, _, ref = shap_case(k, kind, avg, bias)
    D, F = int(max(forest["depths"])), forest["cols"]
    kw = dict(output=ta.OUT_AVG if avg else 0, global_bias=bias)
    f = handle(ta, forest, covers, interactions=True, contribs=True, **kw)
    x = dev(env, data)
    got = explain(env, f, "predict_interactions", x, dims=2)
    off = ~np.eye(F + 1, dtype=bool)
    want, A, N = ref["inter_poly"]
    err, bound = np.abs(got.astype(np.float64) - want)[..., off], ((N + 6 * (D + 2)) * U * A)[..., off]
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"k{k} {kind}: max err / bound = {worst:.3f}")
    assert np.all(err <= bound), f"bound exceeded {worst:.3f}x"
    assert np.array_equal(bits(got), bits(ref["inter_emulate"]))
    assert np.array_equal(bits(got), bits(got.swapaxes(-1, -2)))
    phi = explain(env, f, "predict_contribs", x)  # the diagonal: phi_i minus the float32 sum of the row's off-diagonals
    diag = np.zeros(got.shape[:2] + (F,), np.float32)
    for i in np.unique(forest["fids"]):
        s = np.zeros(got.shape[:2], np.float32)
        for j in range(F):
            if j != i:
                s = s + got[:, :, i, j]
        diag[:, :, i] = phi[:, :, i] - s
    idx = np.arange(F)
    assert np.array_equal(bits(got[:, :, idx, idx]), bits(diag))
    assert np.array_equal(bits(explain(env, f, "predict_interactions", x[:65].contiguous(), dims=2)), bits(got[:65]))
    f.check()
    f.close()


@pytest.mark.parametrize("k,kind,avg,bias", SHAP_CASES)
def test_interventional_values_follow_the_sets(env, unforced, k, kind, avg, bias):
    ta, torch = env
    forest, _, data, bg, ref = shap_case(k, kind, avg, bias)
    F, T, B = forest["cols"], len(forest["depths"]), bg.shape[0]
    f = handle(ta, forest, interventional=True, output=ta.OUT_AVG if avg else 0, global_bias=bias)
    x, bgd = dev(env, data), dev(env, bg)
    f.set_background(bgd)
    got = explain(env, f, "predict_contribs_interventional", x)
    want, A, N = ref["iv"]
    err, bound = np.abs(got.astype(np.float64) - want)[:, :, :F], ((N + 8) * U * A)[:, :, :F]
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"k{k} {kind}: max err / bound = {worst:.3f}")
    assert np.all(err <= bound), f"bound exceeded {worst:.3f}x"
    raw = f.predict_raw(bgd).cpu().numpy().reshape(B, k)  # the bias column: the host formula on the handle's own raw sums
    want_bias = np.array([ivr.bias_from_raw(raw[:, c], T, avg, bias) for c in range(k)]).astype(np.float32)
    assert np.array_equal(bits(got[:, :, F]), bits(np.broadcast_to(want_bias, got[:, :, F].shape)))
    assert np.array_equal(bits(want_bias), bits(ref["iv_bias"]))
    for r in (1, 65):
        assert np.array_equal(bits(explain(env, f, "predict_contribs_interventional", x[:r].contiguous())), bits(got[:r])), r
    f.check()
    f.close()


@pytest.mark.parametrize("avg", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_saabas_and_bias_equal_the_categorical_sparse_expansion_bit_for_bit(env, unforced, k, avg):
    """Integer covers: the node sums are exact in float32, so the expansion's float32 covers are the oblivious handle's float64
    ones.  The sparse handle follows the sets through TAHOE_CREATE_CAT_CONTRIBS, which SparseForest sets with categories."""
    ta, torch = env
    forest, covers, data, _, ref = shap_case(k, "int")
    kw = dict(output=ta.OUT_AVG if avg else 0, global_bias=0.25)
    f = handle(ta, forest, covers, contribs=True, approx_contribs=True, **kw)
    g = sparse_handle(ta, forest, covers, contribs=True, approx_contribs=True, **kw)
    x = dev(env, data)
    mine, theirs = explain(env, f, "predict_contribs_approx", x), explain(env, g, "predict_contribs_approx", x)
    assert np.array_equal(bits(mine), bits(theirs))
    with ocr.seam():
        assert np.array_equal(bits(mine), bits(osr.saabas(forest, covers, data, avg=avg, global_bias=0.25)))
    shap = explain(env, f, "predict_contribs", x)
    assert np.array_equal(bits(shap[:, :, -1]), bits(mine[:, :, -1]))  # one bias for both calls ...
    assert np.array_equal(bits(shap[:, :, -1]), bits(explain(env, g, "predict_contribs", x)[:, :, -1]))  # ... and the expansion's
    f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ 5: the handle
def create_cat(ta, forest, cats, flags=0, covers=None):
    """tahoe_oblivious_forest_create_cat itself; cats: None (NULL) or a tahoe_categorical_splits -> (status, handle)"""
    depths = np.ascontiguousarray(forest["depths"], np.int32)
    n = len(forest["fids"])
    splits = np.zeros(max(n, 1), ta.capi.OBLIVIOUS_SPLIT_DTYPE)
    splits["thr"][:n] = forest["thr"]
    splits["bits"][:n] = np.asarray(forest["fids"], np.int64) | (np.asarray(forest["def_left"]).astype(np.int64) << 30)
    leaves = np.ascontiguousarray(forest["leaves"], np.float32)
    cv = None if covers is None else np.ascontiguousarray(covers, np.float32)
    params = ta.ForestParams(0, 0, len(depths), forest["cols"], 0, 0, 0.5, 0.0, 0, MISSING)
    h = C.c_void_p()
    st = ta.lib.tahoe_oblivious_forest_create_cat(C.byref(h), depths.ctypes.data, splits.ctypes.data, leaves.ctypes.data,
                                                  None if cv is None else cv.ctypes.data, C.byref(params), forest["k"], flags,
                                                  None if cats is None else C.byref(cats))
    return st, h


def info_bytes(ta, h):
    info = ta.capi.ForestInfo()
    assert ta.lib.tahoe_forest_get_info(h, C.byref(info)) == 0
    return info.device_bytes


def test_no_sets_give_the_handle_of_create_ex(env):
    ta, torch = env
    forest, data, _, _ = case("mixed_k3")
    plain = ocr.numeric_part(forest)
    plain["thr"] = np.nan_to_num(plain["thr"], nan=0.5)
    covers = osr.make_covers(plain, "int", seed=3)
    flags = ta.capi.CREATE_CONTRIBS | ta.capi.CREATE_APPROX_CONTRIBS | ta.capi.CREATE_INTERACTIONS | ta.capi.CREATE_OBLIVIOUS_INTERVENTIONAL
    ref = handle(ta, plain, covers, **FLAGS)
    x = dev(env, data)
    want = bits(ref.predict_raw(x)), bits(ref.predict_leaf_idx(x)[0]), bits(ref.predict_contribs(x))
    empty, _keep = ta.capi.pack_categorical({})
    for cats in (None, empty):
        st, h = create_cat(ta, plain, cats, flags, covers)
        assert st == 0 and info_bytes(ta, h) == ref.info().device_bytes
        twin = ta.ObliviousForest.__new__(ta.ObliviousForest)  # the Python methods on the handle made above
        twin.__dict__.update(ref.__dict__)
        twin._h = h
        got = bits(twin.predict_raw(x)), bits(twin.predict_leaf_idx(x)[0]), bits(twin.predict_contribs(x))
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert twin.kernel_form(ROWS) == ref.kernel_form(ROWS)
        twin.close()
    ref.close()


@pytest.mark.parametrize("flags", [{}, FLAGS])
def test_device_bytes_grow_by_the_pool_alone(env, flags):
    """device_bytes(cats) = device_bytes(NULL) + 4 * sum over the sets of two words or more of (1 + nwords): a set of at most one
    word rides in its split record, and the explanation tables share the pool"""
    ta, _ = env
    for name in ("mixed_k3", "nine_k9"):
        forest = case(name)[0]
        covers = osr.make_covers(forest, "int", seed=3) if flags else None
        with_sets, without = handle(ta, forest, covers, **flags), handle(ta, ocr.numeric_part(forest), covers, **flags)
        assert ocr.pool_bytes(forest) > 0
        assert with_sets.info().device_bytes == without.info().device_bytes + ocr.pool_bytes(forest)
        with_sets.close()
        without.close()
    inline = ocr.with_sets(ocr.numeric_part(case("mixed_k3")[0]), {0: [31], 3: [], 5: [0, 7]}, ml=[5])
    a, b = handle(ta, inline), handle(ta, ocr.numeric_part(inline))
    assert a.info().device_bytes == b.info().device_bytes
    a.close()
    b.close()


def test_what_an_oblivious_handle_refuses_stays_refused(env):
    ta, torch = env
    forest, data, want, _ = case("mixed_k1")
    cols = forest["cols"]
    f = handle(ta, forest)
    x = dev(env, data)
    lib, h = ta.lib, f._h
    out = torch.full((ROWS * (cols + 1),), 7.0, device="cuda")
    indptr = torch.arange(0, ROWS + 1, dtype=torch.int64, device="cuda")
    indices = torch.zeros(ROWS, dtype=torch.int32, device="cuda")
    host_out = np.full(ROWS, 7.0, np.float32)
    rounds = np.array([1, 2], np.int32)
    calls = {
        "tahoe_forest_predict_csr": lambda: lib.tahoe_forest_predict_csr(h, out.data_ptr(), indptr.data_ptr(), indices.data_ptr(),
                                                                         x.data_ptr(), ROWS, ROWS, None),
        "tahoe_forest_predict_host": lambda: lib.tahoe_forest_predict_host(h, host_out.ctypes.data, data.ctypes.data, ROWS, 0),
        "tahoe_forest_set_stages": lambda: lib.tahoe_forest_set_stages(h, rounds.ctypes.data, 2),
        "tahoe_forest_predict_staged": lambda: lib.tahoe_forest_predict_staged(h, out.data_ptr(), x.data_ptr(), ROWS, None),
        "tahoe_forest_predict_contribs": lambda: lib.tahoe_forest_predict_contribs(h, out.data_ptr(), x.data_ptr(), ROWS, None),
    }
    for name, call in calls.items():
        assert call() == UNSUPPORTED, name
        msg = lib.tahoe_last_error().decode()
        assert "oblivious" in msg and name in msg, msg
    for strat in ("TILEBLOCK", "TILERING", "QRING"):
        with pytest.raises(ta.TahoeError) as e:
            f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert e.value.status == UNSUPPORTED and "oblivious" in str(e.value)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and (host_out == 7.0).all()
    f.reserve(1 << 20)  # served: nothing to size
    f.check()
    assert np.array_equal(bits(f.predict_raw(x)), bits(want[:, 0]))  # the handle is as it was
    f.close()


def test_predict_can_be_captured(env):
    ta, torch = env
    forest, data, want, _ = case("nine_k9")
    f = handle(ta, forest)
    x = dev(env, data)
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
