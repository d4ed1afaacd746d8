"""Vector-leaf handles at the edges, on the GPU: the walk (vector.hip, forms 27 and 28) and TreeSHAP (vector_contribs_kernel<KB> of
vector_shap.hip) on the cases of tests/vector_edges.py.  Needs an MI355X.

The walk: raw sums and leaf indices bit for bit tests/vector_ref.vector_ref and the expansion handle's, under AUTO, DIRECT and
ROWTILE, at every batch size, a row alone; where the reference is NaN (the IEEE leaf table) the output is NaN at the same
positions and every other element has equal bits.
TreeSHAP: (a) bit for bit the T x K-tree expansion on tahoe_sparse_forest_create_ex with tiled covers, under the automatic class
block and every forced one x {loop, grid}; (b) |phi - phi64| <= gamma x scale against vector_edges.poly, gamma = (paths +
4 (depth + 2)) 2^-24, scale = sparse_shap_ref.bound_scale on the expansion, / T with AVG -- the bar of
tests/test_vector_shap_gpu.py; (c) the bias column bit for bit vector_shap_ref.bias_column; (d) local accuracy against the
handle's own margins within that test's expression; (e) a row alone equals its row of the batch.
Refusals are status codes: 8193 columns, ROWTILE at 641 columns, a null data pointer.

Every accuracy test prints its largest error as a fraction of its bar, and its largest row-sum gap as a fraction of (d)'s
allowance.  Measured on an MI355X, the largest fractions per family, (b) / (d):
  tiles (every num_cols and K)            0.0099 / 0.0042      branch (every `missing`, K in {1, 3})   0.0096 / 0.0046
  covers (every mode)                     0.0028 / 0.0016      K in {1023, 1024}                       0.0001 / 0.0002
  one_col_rounds                          0.0071 / 0.0039
  vine31, vine40_on_31, mixed_len (three cover sets, K in {2, 9})                                       0.0016 / 0.0009

Before the unwound sum was solved from both ends of a path (unwind_split, contribs_internal.h) the long paths missed under the
`consistent` covers: vine31:k9 0.217 / 1.013, vine40_on_31:k9 0.966 / 5.283, vine40_on_31:k2 1.492 / 3.365, mixed_len:k9 0.467 /
2.013 -- with the expansion's bits, so contribs_kernel had the same error."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_shap_ref as ssr  # noqa: E402
import vector_edges as ve  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, UNSUPPORTED = 0, 1, 7
FORM_DIRECT, FORM_TILE = 27, 28
U = 2.0 ** -24
KNOBS = ("TAHOE_VECTOR_SHAP_KB", "TAHOE_VECTOR_SHAP_GRID")
WALK_BATCHES = (1, 63, 64, 65)


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


def assert_same(got, want, label, nan_ok=False):
    """Equal bits; with nan_ok a NaN of `want` asks for a NaN (of any sign and payload) at the same position"""
    g = np.ascontiguousarray(got.cpu().numpy() if hasattr(got, "cpu") else got, np.float32)
    w = np.ascontiguousarray(want.cpu().numpy() if hasattr(want, "cpu") else want, np.float32)
    assert g.shape == w.shape, (label, g.shape, w.shape)
    nan = np.isnan(w)
    if not nan_ok:
        assert not nan.any(), label
    assert np.array_equal(np.isnan(g), nan), label
    assert np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan]), label


def native(ta, c, label=None, contribs=False, **kw):
    forest = c["forest"]
    return ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=c["missing"],
                           covers=None if label is None else c["covers"][label], contribs=contribs, **kw)


def expansion(ta, c, label=None, contribs=False, **kw):
    """The T x K-tree expansion on tahoe_sparse_forest_create_ex(num_classes = K); every copy of tree t carries tree t's covers"""
    forest = c["forest"]
    nodes, trees = vr.expand(forest)
    kw.setdefault("threshold", 0.5)
    return ta.capi.SparseForest(nodes, trees, forest["cols"], missing=c["missing"], num_classes=forest["k"],
                                covers=None if label is None else vsr.tile_covers(forest, c["covers"][label]), contribs=contribs, **kw)


def shaped(a, k):
    return a[:, 0] if k == 1 else a


# ------------------------------------------------------------------------------------------------ 1: the walk
def check_walk(env, c, batches=WALK_BATCHES, nan_ok=False, tile=True, x=None):
    """Sums and leaf indices of the native handle under AUTO, DIRECT and (tile) ROWTILE against vector_ref and the expansion"""
    ta, torch = env
    forest, data = c["forest"], c["data"]
    k, T = forest["k"], forest["trees"].size
    with np.errstate(all="ignore"):
        want, want_leaf, _ = vr.vector_ref(forest, data, c["missing"])
    f, g = native(ta, c), expansion(ta, c)
    x = torch.from_numpy(data.copy()).cuda() if x is None else x
    assert f.kernel_form(data.shape[0]) == ("vector_tile" if tile else "vector_direct")  # AUTO
    got = {}
    for strat in ("AUTO", "DIRECT") + (("ROWTILE",) if tile else ()):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        for r in batches:
            xr = x[:r]
            leaf, sums = f.predict_leaf_idx(xr)
            raw = f.predict_raw(xr)
            for out in (sums, raw):
                assert_same(out, shaped(want[:r], k), (strat, r), nan_ok)
                assert_same(out, g.predict_raw(xr), (strat, r, "expansion"), nan_ok)
            assert np.array_equal(bits(leaf), want_leaf[:r].view(np.uint32)), (strat, r)
            eleaf, _ = g.predict_leaf_idx(xr)
            assert np.array_equal(bits(eleaf).reshape(r, T * k)[:, ::k], want_leaf[:r].view(np.uint32)), (strat, r)
        for i in (0, 1, data.shape[0] - 1):  # a row alone
            assert_same(f.predict_raw(x[i:i + 1].clone()), shaped(want[i:i + 1], k), (strat, "row", i), nan_ok)
        got[strat] = f.predict_raw(x)
    for strat in got:
        assert_same(got[strat], got["AUTO"].cpu().numpy(), strat, nan_ok)
        if nan_ok:  # DIRECT and ROWTILE agree in every bit, NaN included: the same adds in the same order
            assert np.array_equal(bits(got[strat]), bits(got["AUTO"])), strat
    f.check()
    f.close()
    g.close()
    return want


@pytest.mark.parametrize("cols", ve.WALK_COLS)
def test_walk_at_the_lds_limit_of_the_tile(env, cols):
    ta, torch = env
    c = ve.case(f"walk:{cols}")
    f = native(ta, c)
    fits = cols <= 640
    assert f.get_strategy(65) == (ta.STRATEGY_ROWTILE if fits else ta.STRATEGY_DIRECT)
    assert ta.lib.tahoe_forest_get_kernel_form(f._h, 65) == (FORM_TILE if fits else FORM_DIRECT)
    if not fits:
        with pytest.raises(ta.TahoeError) as e:
            f.set_strategy(ta.STRATEGY_ROWTILE)
        assert e.value.status == UNSUPPORTED and "vector-leaf" in str(e.value)
        assert f.get_strategy(65) == ta.STRATEGY_DIRECT
    f.close()
    check_walk(env, c, tile=fits)


def test_walk_at_640_columns_one_float_off_a_16_byte_boundary(env):
    """num_cols is a multiple of 4, but the batch starts one float past a 16-byte boundary: the scalar staging loop"""
    ta, torch = env
    c = ve.case("walk:640")
    rows, cols = c["data"].shape
    buf = torch.full((rows * cols + 4,), float("nan"), device="cuda")
    x = buf[1:1 + rows * cols].view(rows, cols)
    x.copy_(torch.from_numpy(c["data"].copy()))
    assert x.is_contiguous() and buf.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 4
    check_walk(env, c, x=x)


@pytest.mark.parametrize("name", ve.BRANCH_CASES + ["vine31:k9", "K:1023", "K:1024", ve.DEEP_CASE])
def test_walk_follows_the_branch_rule_bit_for_bit(env, name):
    check_walk(env, ve.case(name))


@pytest.mark.parametrize("name", ve.LEAF_CASES)
def test_walk_sums_ieee_leaves_in_tree_order(env, name):
    c = ve.case(name)
    want = check_walk(env, c, nan_ok=True)
    if name == "leaves:negzero":
        assert not want.view(np.uint32).any()  # +0.0 + -0.0 = +0.0 in every bit
    else:
        assert np.isnan(want).any() and np.isinf(want).any()


# ------------------------------------------------------------------------------------------------ 2: TreeSHAP
def scale_bar(c):
    """gamma x scale, [K]: the bar of tests/test_vector_shap_gpu.py, built the same way on the expansion"""
    sn, tr = vr.expand(c["forest"])
    scale, depth, paths = ssr.bound_scale(sn, tr, c["forest"]["k"])
    return (paths + 4 * (depth + 2)) * U * scale


def check_shap(env, name, batches, nan_ok=False, accuracy=True, labels=None):
    """(a), (c) and (e) at the row counts of `batches` -- none of them with batches=() -- and, with accuracy, (b) and (d)"""
    ta, torch = env
    c = ve.case(name)
    forest, data = c["forest"], c["data"]
    K, F, T = forest["k"], forest["cols"], forest["trees"].size
    rows = data.shape[0]
    x = torch.from_numpy(data.copy()).cuda()
    bar = scale_bar(c) if accuracy else None
    worst = 0.0
    for label in labels or c["covers"]:
        raw = ve.poly_raw(name, label)[0] if accuracy else None
        for avg, bias in ((False, 0.125), (True, -0.5)):
            kw = dict(output=ta.OUT_AVG if avg else 0, global_bias=bias)
            f = native(ta, c, label, True, **kw)
            phi = f.predict_contribs(x).cpu().numpy().reshape(rows, K, F + 1)
            if batches:
                g = expansion(ta, c, label, True, **kw)
                for r in batches:
                    xr = x[:r].contiguous()
                    a, b = f.predict_contribs(xr), g.predict_contribs(xr)
                    assert tuple(a.shape) == tuple(b.shape) == (r,) + ((K,) if K > 1 else ()) + (F + 1,)
                    assert_same(a, b, (name, label, avg, r), nan_ok)  # (a)
                g.close()
                for i in (0, rows - 1):  # (e)
                    alone = f.predict_contribs(x[i:i + 1].clone()).cpu().numpy().reshape(K, F + 1)
                    assert_same(alone, phi[i], (name, label, avg, "row", i), nan_ok)
                if not nan_ok:
                    assert np.isfinite(phi).all(), (name, label, avg)
                    bcol = vsr.bias_column(forest, c["covers"][label], avg, bias)
                    assert np.array_equal(bits(phi[:, :, F]), bits(np.broadcast_to(bcol, (rows, K)))), (name, label, avg)  # (c)
            if accuracy:
                tol = bar / (T if avg and T else 1)
                want = raw / (T if avg and T else 1)
                err = np.abs(phi[:, :, :F].astype(np.float64) - want[:, :, :F])
                frac = float((err / tol[None, :, None]).max()) if err.size else 0.0
                worst = max(worst, frac)
                print(f"{name} {label} avg={avg}: max err {err.max() if err.size else 0.0:.3e} = {frac:.4f} of the bar")
                m = native(ta, c, output=kw["output"], global_bias=bias)
                margin = m.predict(x).cpu().numpy().astype(np.float64).reshape(rows, K)
                m.close()
                gap = np.abs(phi.astype(np.float64).sum(-1) - margin)
                room = 2 * tol[None, :] + 1e-5 * np.abs(margin) + 1e-6
                print(f"{name} {label} avg={avg}: row sum against the margin, max gap {gap.max():.3e} = {(gap / room).max():.4f} of "
                      "its allowance")
                within, sums_up = bool(np.all(err <= tol[None, :, None])), bool(np.all(gap <= room))
                assert within, f"{name} {label} avg={avg}: {frac:.3f} of the bar"  # (b)
                assert sums_up, f"{name} {label} avg={avg}: {(gap / room).max():.3f} of the allowance"  # (d)
            f.check()
            f.close()
    if accuracy:
        print(f"{name}: largest fraction of the bar {worst:.4f}")


def check_forced(env, monkeypatch, name, kbs=(1, 2, 4, 8), nan_ok=False):
    """(a) under every forced class block, the blocks in a workgroup's loop and over gridDim.y"""
    ta, torch = env
    c = ve.case(name)
    label = next(iter(c["covers"]))
    cols, K = c["forest"]["cols"], c["forest"]["k"]
    x = torch.from_numpy(c["data"].copy()).cuda()
    kw = dict(output=ta.OUT_AVG, global_bias=-0.25)
    g = expansion(ta, c, label, True, **kw)
    want = g.predict_contribs(x).cpu().numpy()
    g.close()
    for kb in kbs:
        R = ve.tile_shape(cols, K, kb)[1]
        for grid in (0, 1):
            monkeypatch.setenv("TAHOE_VECTOR_SHAP_KB", str(kb))
            monkeypatch.setenv("TAHOE_VECTOR_SHAP_GRID", str(grid))
            f = native(ta, c, label, True, **kw)
            assert_same(f.predict_contribs(x), want, (name, kb, grid), nan_ok)
            for r in (R - 1, R + 1):
                if 1 <= r < x.shape[0]:
                    assert_same(f.predict_contribs(x[:r].contiguous()), want[:r], (name, kb, grid, r), nan_ok)
            f.check()
            f.close()


@pytest.mark.parametrize("name", ve.PATH_CASES)
def test_contribs_on_long_paths_and_full_bins_equal_the_expansion(env, name):
    check_shap(env, name, WALK_BATCHES, accuracy=False)


@pytest.mark.parametrize("label", ve.PATH_LABELS)
@pytest.mark.parametrize("name", ve.PATH_CASES)
def test_accuracy_on_long_paths_and_full_bins(env, name, label):
    """(b) and (d).  The `consistent` covers put a vine's chain-side zero fractions near 0.97: the case that needs the unwound sum
    solved from both ends (four of these cases missed the bar or the allowance before, by up to 1.5 x and 5.3 x)"""
    check_shap(env, name, (), labels=(label,))


@pytest.mark.parametrize("name", ["vine31:k9", "mixed_len:k9", "one_col_rounds"])
def test_forced_class_blocks_on_long_paths(env, monkeypatch, name):
    check_forced(env, monkeypatch, name)


@pytest.mark.parametrize("name", ve.TILE_CASES)
def test_contribs_on_both_sides_of_every_tile_step(env, name):
    c = ve.case(name)
    kb, R, lds = ve.tile_shape(c["forest"]["cols"], c["forest"]["k"])
    assert lds <= ve.LDS_DEVICE
    check_shap(env, name, ve.batches(R))


@pytest.mark.parametrize("cols", ve.TILE_FORCED)
def test_forced_class_blocks_at_the_tile_steps(env, monkeypatch, cols):
    check_forced(env, monkeypatch, f"tiles:{cols}")


def test_8193_columns_are_refused_at_create(env):
    ta, _ = env
    forest = ve.remap(ve.case("tiles:8:k9")["forest"], ve.tile_columns(ve.TILE_REFUSED), ve.TILE_REFUSED)
    c = dict(ve.case("tiles:8:k9"), forest=forest)
    with pytest.raises(ta.TahoeError) as e:
        native(ta, c, "consistent", True)
    assert e.value.status == UNSUPPORTED and "20 B of LDS per column" in str(e.value) and "8193" in str(e.value)
    f = native(ta, c)  # the walk takes them
    assert f.get_strategy(65) == ta.STRATEGY_DIRECT
    f.close()


@pytest.mark.parametrize("name", ve.BRANCH_CASES)
def test_contribs_follow_the_branch_rule(env, name):
    check_shap(env, name, WALK_BATCHES)


@pytest.mark.parametrize("name", ve.COVER_CASES)
def test_contribs_under_extreme_cover_pairs(env, name):
    check_shap(env, name, WALK_BATCHES)


@pytest.mark.parametrize("name", ve.K_CASES)
def test_contribs_of_the_most_outputs(env, name):
    check_shap(env, name, (1, 65))


def test_forced_class_blocks_at_1024_outputs(env, monkeypatch):
    check_forced(env, monkeypatch, "K:1024", kbs=(1, 8))


def test_contribs_of_ieee_leaves_equal_the_expansion(env, monkeypatch):
    """NaN where the expansion has NaN, equal bits elsewhere: terms tw * leaf that overflow, +-inf and NaN leaves, inf - inf"""
    check_shap(env, "leaves:ieee", WALK_BATCHES, nan_ok=True, accuracy=False)
    check_shap(env, "leaves:negzero", (65,), nan_ok=True, accuracy=False)
    check_forced(env, monkeypatch, "leaves:ieee", nan_ok=True)


# ------------------------------------------------------------------------------------------------ 3: no columns
@pytest.mark.parametrize("name", ve.NOCOLS_CASES)
def test_a_forest_without_columns(env, name):
    """num_cols = 0: every tree is a single leaf, the walk reads no feature and TreeSHAP has no bin and no LDS"""
    ta, torch = env
    c = ve.case(name)
    forest = c["forest"]
    K, T, rows = forest["k"], forest["trees"].size, ve.ROWS
    want, _, _ = vr.vector_ref(forest, c["data"])
    cv = c["covers"]["unrelated"]
    lib = ta.lib
    x = torch.full((4,), float("nan"), device="cuda")  # a [rows, 0] batch has no element; the pointer must not be null
    for avg, bias in ((False, 0.125), (True, -0.5)):
        out_bits = ta.OUT_AVG if avg else 0
        f = native(ta, c, "unrelated", True, output=out_bits, global_bias=bias)
        assert f.get_strategy(rows) == ta.STRATEGY_DIRECT
        sums = torch.full((rows, K), 7.0, device="cuda")
        leaf = torch.full((rows, T), -1, dtype=torch.int32, device="cuda")
        assert lib.tahoe_forest_predict_raw(f._h, sums.data_ptr(), x.data_ptr(), rows, None) == OK
        torch.cuda.synchronize()
        assert np.array_equal(bits(sums), want.view(np.uint32))
        sums.fill_(7.0)
        assert lib.tahoe_forest_predict_leaf_idx(f._h, leaf.data_ptr(), sums.data_ptr(), x.data_ptr(), rows, None) == OK
        torch.cuda.synchronize()
        assert np.array_equal(bits(sums), want.view(np.uint32)) and not leaf.cpu().numpy().any()
        preds = torch.full((rows, K), 7.0, device="cuda")
        assert lib.tahoe_forest_predict(f._h, preds.data_ptr(), x.data_ptr(), rows, None) == OK
        torch.cuda.synchronize()
        pw = want / np.float32(T) + np.float32(bias) if avg else want + np.float32(bias)
        assert np.array_equal(bits(preds), pw.view(np.uint32))
        phi = torch.full((rows, K, 1), 7.0, device="cuda")
        assert lib.tahoe_forest_predict_contribs(f._h, phi.data_ptr(), x.data_ptr(), rows, None) == OK
        torch.cuda.synchronize()
        bcol = vsr.bias_column(forest, cv, avg, bias)
        assert np.array_equal(bits(phi).reshape(rows, K), np.broadcast_to(bcol, (rows, K)).view(np.uint32))
        # a null data pointer is refused as on every handle, although no element would be read
        for call in (lambda: lib.tahoe_forest_predict_raw(f._h, sums.data_ptr(), None, rows, None),
                     lambda: lib.tahoe_forest_predict_contribs(f._h, phi.data_ptr(), None, rows, None)):
            assert call() == INVALID_ARG
            assert "null argument" in lib.tahoe_last_error().decode()
        f.check()
        f.close()
