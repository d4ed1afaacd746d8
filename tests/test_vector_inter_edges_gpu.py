"""SHAP interaction values on vector-leaf handles at the edges, on the GPU: vector_interactions_kernel<KB, form> of vector_inter.hip
on the cases of tests/vector_edges.py and tests/vector_inter_ref.py.  Needs an MI355X.

Every check is bit-equality with the T x K-tree expansion on tahoe_sparse_forest_create_ex(num_classes = K, TAHOE_CREATE_CONTRIBS)
whose copies of tree t carry tree t's covers; where the expansion is NaN (the IEEE leaf table) the output is NaN at the same
positions and every other element has equal bits.
  rule steps  the 3-tree K = 9 tile forest spread over num_cols on both sides of every step of the class-block / tile-row / form
              rule (vector_inter_ref.STEPS: 18 | 19, 25 | 26, 36 | 37, 51 | 52, 71 | 72) and at 2 and 1 columns (no pair), at 1,
              R - 1, R, R + 1 and 33 rows (slabs) or 1, 3, 4, 5 rows (in place), under the automatic block and every forced one
  K           4, 5, 7, 16 outputs at 8 columns; 1023 and 1024 outputs
  paths       vine31 (32-lane paths, the clamp at lane 63, the left neighbour two lanes down), mixed_len, one_col_rounds (no
              path with two features: the matrix is its diagonal), two_col_rounds (one pair adding in 21 rounds)
  bins        a forest of exactly one bin (three idle waves) and one of more than four
  branch, covers, leaves (IEEE values, -0.0), nocols (a 1 x 1 matrix holding the bias, no LDS)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vector_edges as ve  # noqa: E402
import vector_inter_ref as vir  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

pytestmark = pytest.mark.gpu

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


def assert_same(got, want, label, nan_ok=False):
    """Equal bits; with nan_ok a NaN of `want` asks for a NaN (of any sign and payload) at the same position"""
    g = np.ascontiguousarray(got.cpu().numpy(), np.float32)
    w = np.ascontiguousarray(want.cpu().numpy(), np.float32)
    assert g.shape == w.shape, (label, g.shape, w.shape)
    nan = np.isnan(w)
    if not nan_ok:
        assert not nan.any(), label
    assert np.array_equal(np.isnan(g), nan), label
    assert np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan]), label


def native(ta, c, label, **kw):
    forest = c["forest"]
    return ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=c["missing"],
                           covers=c["covers"][label], interactions=True, **kw)


def expansion(ta, c, label, **kw):
    forest = c["forest"]
    nodes, trees = vr.expand(forest)
    kw.setdefault("threshold", 0.5)
    return ta.capi.SparseForest(nodes, trees, forest["cols"], missing=c["missing"], num_classes=forest["k"],
                                covers=vsr.tile_covers(forest, c["covers"][label]), contribs=True, **kw)


def check(env, name, batches=None, nan_ok=False, labels=None, monkeypatch=None, forced=()):
    """The native handle against the expansion at the row counts of `batches` (default: around the handle's tile), RAW and AVG
    with a bias; with `forced` also under every (KB, grid) of it at the largest batch.  -> the last expansion output (numpy)"""
    ta, torch = env
    c = vir.case(name)
    forest, data = c["forest"], c["data"]
    batches = batches or vir.batches(forest["cols"], forest["k"])
    x = torch.from_numpy(data[:max(batches)].copy()).cuda()
    want = None
    for label in labels or c["covers"]:
        for avg, bias in ((False, 0.125), (True, -0.5)):
            kw = dict(output=ta.OUT_AVG if avg else 0, global_bias=bias)
            f, g = native(ta, c, label, **kw), expansion(ta, c, label, **kw)
            for r in batches:
                xr = x[:r].contiguous()
                want = g.predict_interactions(xr)
                assert_same(f.predict_interactions(xr), want, (name, label, avg, r), nan_ok)
            f.check()
            f.close()
            g.close()
            for kb, grid in forced if avg else ():
                monkeypatch.setenv("TAHOE_VECTOR_SHAP_KB", str(kb))
                monkeypatch.setenv("TAHOE_VECTOR_SHAP_GRID", str(grid))
                f = native(ta, c, label, **kw)
                assert_same(f.predict_interactions(x), want, (name, label, "forced", kb, grid), nan_ok)
                f.check()
                f.close()
                monkeypatch.delenv("TAHOE_VECTOR_SHAP_KB")
                monkeypatch.delenv("TAHOE_VECTOR_SHAP_GRID")
    return want.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the rule's steps
@pytest.mark.parametrize("cols", list(vir.STEPS))
def test_both_sides_of_every_step_of_the_rule(env, monkeypatch, cols):
    slabs, kb, R = vir.STEPS[cols]
    assert vir.shape(cols, 9)[:3] == (slabs, kb, R)
    batches = vir.batches(cols, 9)
    assert batches == ([1, 3, 4, 5] if not slabs else sorted({r for r in (1, R - 1, R, R + 1, 33) if r >= 1}))
    forced = [(b, g) for b in (1, 2, 4, 8) for g in (0, 1)]
    m = check(env, f"tiles:{cols}", batches, monkeypatch=monkeypatch, forced=forced)
    if cols == 1:  # no pair: the matrix is phi on the diagonal and the bias
        assert m.shape[-2:] == (2, 2) and not m[..., 0, 1].any() and not m[..., 1, 0].any()
    else:
        assert np.abs(m[..., :cols, :cols] - m[..., :cols, :cols] * np.eye(cols, dtype=np.float32)).max() > 0


@pytest.mark.parametrize("k", ve.TILE_KS)
def test_class_counts_around_the_blocks(env, monkeypatch, k):
    assert vir.shape(8, k)[1] == {4: 4, 5: 8, 7: 8, 16: 8}[k]
    check(env, f"tiles:8:k{k}", monkeypatch=monkeypatch, forced=[(b, g) for b in (2, 8) for g in (0, 1)])


@pytest.mark.parametrize("name", ve.K_CASES)
def test_a_thousand_outputs(env, monkeypatch, name):
    check(env, name, batches=[1, 33], monkeypatch=monkeypatch, forced=[(8, 0), (1, 1)])


# ------------------------------------------------------------------------------------------------ paths, rounds, bins
@pytest.mark.parametrize("name", ["vine31:k9", "vine31:k2", "mixed_len:k9"])
def test_long_paths(env, name):
    c = vir.case(name)
    longest = max(len(p) for p in vsr.paths(c["forest"]))
    assert longest == 31  # 32 lanes with the root element: two such paths fill a bin, the second one's reads clamp at lane 63
    check(env, name)


def test_no_path_with_two_features_gives_a_diagonal_matrix(env):
    c = vir.case("one_col_rounds")
    assert all(len(p) == 1 for p in vsr.paths(c["forest"]))
    m = check(env, "one_col_rounds")
    assert m.shape[-2:] == (2, 2) and not m[..., 0, 1].view(np.uint32).any() and not m[..., 1, 0].view(np.uint32).any()
    assert np.abs(m[..., 0, 0]).max() > 0


def test_one_pair_adds_in_21_rounds(env, monkeypatch):
    c = vir.case("two_col_rounds")
    assert [len(p) for p, _ in vsr.bins(c["forest"])] == [21] * 4
    m = check(env, "two_col_rounds", monkeypatch=monkeypatch, forced=[(1, 0), (2, 1)])
    assert np.abs(m[..., 0, 1]).max() > 0


def test_one_bin_and_more_than_four(env):
    """One bin: waves 1 to 3 have nothing to evaluate and their triangles stay zero; five and more: a wave takes a second bin"""
    ta, torch = env
    forest, data, covers = vsr.case("tiny_ratio_k3")
    assert len(vsr.bins(forest)) == 1 and max(len(p) for p in vsr.paths(forest)) == 2
    assert len(vsr.bins(vsr.case("five_k9")[0])) >= 5
    for name in ("tiny_ratio_k3", "five_k9"):
        forest, data, covers = vsr.case(name)
        c = dict(forest=forest, data=data, covers=covers, missing=vr.MISSING)
        x = torch.from_numpy(data[:33].copy()).cuda()
        for label in covers:
            f, g = native(ta, c, label), expansion(ta, c, label)
            want = g.predict_interactions(x)
            assert_same(f.predict_interactions(x), want, (name, label))
            assert want.abs().max().item() > 0
            f.close()
            g.close()


# ------------------------------------------------------------------------------------------------ branch rule, covers, leaves
@pytest.mark.parametrize("name", ve.BRANCH_CASES + ve.COVER_CASES)
def test_branch_rule_and_extreme_covers(env, name):
    check(env, name, batches=[1, 33])


@pytest.mark.parametrize("name", ve.LEAF_CASES)
def test_ieee_leaves(env, name):
    m = check(env, name, batches=[1, 33], nan_ok=True)
    if name == "leaves:ieee":
        assert np.isnan(m).any()
    else:
        assert np.isfinite(m).all()


@pytest.mark.parametrize("name", ve.NOCOLS_CASES)
def test_no_columns(env, name):
    """num_cols = 0: every tree is a single leaf; no bin, no LDS, and the matrix of a (row, k) is the bias alone"""
    ta, torch = env
    c = vir.case(name)
    K, label, lib = c["forest"]["k"], "unrelated", ta.lib
    x = torch.full((4,), float("nan"), device="cuda")  # a [rows, 0] batch has no element; the pointer must not be null
    for avg, bias in ((False, 0.125), (True, -0.5)):
        kw = dict(output=ta.OUT_AVG if avg else 0, global_bias=bias)
        f, g = native(ta, c, label, **kw), expansion(ta, c, label, **kw)
        want = vsr.bias_column(c["forest"], c["covers"][label], avg, bias)
        for rows in (1, 33):
            a, b = (torch.full((rows, K, 1, 1), 7.0, device="cuda") for _ in range(2))
            assert lib.tahoe_forest_predict_interactions(f._h, a.data_ptr(), x.data_ptr(), rows, None) == 0
            assert lib.tahoe_forest_predict_interactions(g._h, b.data_ptr(), x.data_ptr(), rows, None) == 0
            torch.cuda.synchronize()
            assert_same(a, b, (name, avg, rows))
            assert np.array_equal(a.cpu().numpy().reshape(rows, K).view(np.uint32), np.tile(want, (rows, 1)).view(np.uint32))
        assert lib.tahoe_forest_predict_interactions(f._h, a.data_ptr(), None, 1, None) == 1  # null data: refused as everywhere
        f.check()
        f.close()
        g.close()
