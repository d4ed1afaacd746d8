"""Partial dependence (tahoe_forest_predict_partial_dependence) on the GPU, bit for bit against the float32 restatement of
tests/pd_ref.py unless a test says otherwise.  Needs an MI355X.  Forests of at most 16 trees, grids of at most 200 points."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pd_cases  # noqa: E402
import pd_ref  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, 7
FN = "tahoe_forest_predict_partial_dependence"


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def handle(env, fo, pd=True, **kw):
    ta, _ = env
    return ta.capi.SparseForest(fo["nodes"], fo["trees"], fo["num_cols"], missing=fo["missing"], covers=fo["covers"],
                                num_classes=fo["num_classes"], categories=fo["categories"], members_left=fo["members_left"],
                                partial_dependence=pd, **kw)


def gpu_pd(env, f, feats, grid):
    """[G, C] float32 from the device."""
    _, torch = env
    grid = np.ascontiguousarray(grid, dtype=np.float32)
    assert grid.ndim == 2 and grid.shape[1] == len(feats)
    g = torch.from_numpy(grid).cuda()
    out = f.partial_dependence(feats, g)
    torch.cuda.synchronize()
    f.check()
    return out.cpu().numpy().reshape(g.shape[0], -1)


def want_pd(fo, feats, grid):
    return pd_ref.pd_f32(fo["nodes"], fo["trees"], fo["covers"], feats, grid, fo["missing"], fo["num_classes"], fo["cats"])


def assert_bits(got, want, label=""):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        g, c = bad[0]
        raise AssertionError(f"{label}: {len(bad)} of {got.size} values differ, first at point {g} class {c}: {got[g, c]!r} vs {want[g, c]!r}")


@pytest.fixture(scope="module")
def forests(env):
    """The three random forests with their handles, shared by the tests below."""
    out = {}
    for case in pd_cases.RANDOM_CASES:
        fo = pd_cases.random_forest(**case["forest"])
        out[case["id"]] = (fo, handle(env, fo), case["targets"])
    yield out
    for _, f, _ in out.values():
        f.close()


@pytest.mark.parametrize("which", ["one_class", "three_classes", "categorical"])
def test_one_two_and_more_targets(env, forests, which):
    """One, two and five targets (C = 1 and C = 3); a categorical target and a categorical non-target feature with members going
    left at some splits and right at others (C = 2)."""
    fo, f, target_sets = forests[which]
    if which == "categorical":
        ml = set(fo["members_left"])
        assert ml and ml != set(fo["categories"])  # both ways
    for feats in target_sets:
        grid = pd_cases.random_grid(fo, feats, 150, seed=20 + len(feats))
        assert_bits(gpu_pd(env, f, feats, grid), want_pd(fo, feats, grid), f"{which} targets {feats}")


@pytest.mark.parametrize("which", ["one_class", "three_classes", "categorical"])
def test_zero_targets(env, forests, which):
    fo, f, _ = forests[which]
    got = gpu_pd(env, f, [], np.zeros((70, 0), np.float32))
    want = want_pd(fo, [], np.zeros((70, 0), np.float32))
    assert_bits(got, want, which)
    assert (bits(got) == bits(got[:1])).all()  # every row the same value: the cover-weighted mean


@pytest.mark.parametrize("which", ["one_class", "three_classes", "categorical"])
def test_all_targets_is_predict_raw(env, forests, which):
    ta, torch = env
    fo, f, _ = forests[which]
    F = fo["num_cols"]
    rows = pd_cases.random_grid(fo, list(range(F)), 130, seed=5)
    raw = f.predict_raw(torch.from_numpy(rows).cuda())
    torch.cuda.synchronize()
    raw = raw.cpu().numpy().reshape(rows.shape[0], -1)
    perm = np.random.default_rng(4).permutation(F)
    assert_bits(gpu_pd(env, f, perm, rows[:, perm]), raw, which)


@pytest.mark.parametrize("G", [1, 63, 64, 65])
def test_grid_sizes_around_the_tile(env, forests, G):
    fo, f, target_sets = forests["three_classes"]
    feats = target_sets[1]
    grid = pd_cases.random_grid(fo, feats, G, seed=G)
    assert_bits(gpu_pd(env, f, feats, grid), want_pd(fo, feats, grid), f"G = {G}")


def test_chunks_positions_and_repeats(env, forests, monkeypatch):
    """G = 130 through chunks of 64 (two chunk boundaries); one grid point at three positions, two of them in other chunks;
    a second call; the same grid through the default chunk."""
    fo, whole, target_sets = forests["three_classes"]
    feats = target_sets[1]
    monkeypatch.setenv("TAHOE_PD_CHUNK_ROWS", "64")
    f = handle(env, fo)
    monkeypatch.delenv("TAHOE_PD_CHUNK_ROWS")
    T = len(fo["trees"])
    assert f.info().device_bytes + 4 * T * (whole_chunk(T) - 64) == whole.info().device_bytes  # the knob was read
    grid = pd_cases.random_grid(fo, feats, 130, seed=77)
    grid[70] = grid[129] = grid[3]
    got = gpu_pd(env, f, feats, grid)
    assert_bits(got, want_pd(fo, feats, grid), "chunks of 64")
    assert np.array_equal(bits(got[3]), bits(got[70])) and np.array_equal(bits(got[3]), bits(got[129]))
    assert_bits(gpu_pd(env, f, feats, grid), got, "second call")
    assert_bits(gpu_pd(env, whole, feats, grid), got, "default chunk")
    assert_bits(gpu_pd(env, f, feats, grid[3:4]), got[3:4], "alone")
    f.close()


def whole_chunk(T):
    """The default chunk: what keeps 4 T chunk near 32 MiB, in whole 64-point tiles."""
    return max((32 << 20) // (4 * T) // 64 * 64, 64)


def test_special_grid_values(env, forests):
    """The missing sentinel (and a value within its 1e-6), NaN, -0.0, +-inf and a value equal to a threshold, on each target."""
    fo, f, _ = forests["one_class"]
    inner = fo["nodes"][fo["nodes"]["bits"] >= 0]
    for fid in (2, 5):
        thr = inner["val"][(inner["bits"] & 0x3fffffff) == fid]
        assert thr.size
        vals = np.array(pd_cases.SPECIALS + [thr[0], np.nextafter(thr[0], np.float32(-np.inf)), thr[-1]], np.float32)
        other = 5 if fid == 2 else 2
        grid = np.stack([np.repeat(vals, vals.size), np.tile(vals, vals.size)], axis=1)  # every pair
        assert_bits(gpu_pd(env, f, [fid, other], grid), want_pd(fo, [fid, other], grid), f"specials on {fid}")
        one = gpu_pd(env, f, [fid], vals[:, None])
        assert_bits(one, want_pd(fo, [fid], vals[:, None]), f"specials on {fid} alone")
        assert not np.array_equal(bits(one[-3]), bits(one[-2]))  # on the threshold goes right, just below it goes left


def test_a_zero_cover_child_is_not_visited(env):
    """Root on x1 (not a target) with covers 0 / 5: the left child, a leaf of +inf, must not be visited (0 * inf would be NaN)."""
    sn = np.zeros(5, dtype=pd_cases.SPARSE_NODE_DTYPE)
    sn[0] = (0.0, 1, 1)
    sn[1] = (np.inf, pd_cases.LEAF, 0)
    sn[2] = (0.5, 0, 3)
    sn[3] = (2.0, pd_cases.LEAF, 0)
    sn[4] = (3.0, pd_cases.LEAF, 0)
    fo = dict(nodes=sn, trees=np.array([0], np.int32), covers=np.array([5, 0, 5, 2, 3], np.float32), num_cols=2, num_classes=1,
              missing=pd_cases.MISSING, cats=None, categories=None, members_left=())
    f = handle(env, fo)
    got = gpu_pd(env, f, [0], np.array([[0.0], [1.0]], np.float32))
    assert got[:, 0].tolist() == [2.0, 3.0]
    assert gpu_pd(env, f, [], np.zeros((1, 0), np.float32))[0, 0] == np.float32(np.float32(0.4) * np.float32(2.0)) + np.float32(0.6) * np.float32(3.0)
    assert np.isinf(gpu_pd(env, f, [1], np.array([[-1.0]], np.float32))[0, 0])  # as a target's branch the leaf is reached
    f.close()


def test_the_depth_32_chain(env):
    """32 pending right siblings per lane when no split is a target (the full stack); 32 targets when every split is one."""
    fo = pd_cases.chain(32)
    f = handle(env, fo)
    got = gpu_pd(env, f, [32], np.zeros((65, 1), np.float32))
    assert_bits(got, want_pd(fo, [32], np.zeros((65, 1), np.float32)), "no split a target")
    assert np.isfinite(got).all() and got[0, 0] != 0.0
    feats = list(range(32))
    grid = np.where(np.random.default_rng(8).random((100, 32)) < 0.9, -1.0, 1.0).astype(np.float32)  # mostly left: deep paths
    grid[0] = -1.0  # all the way down
    got = gpu_pd(env, f, feats, grid)
    assert_bits(got, want_pd(fo, feats, grid), "every split a target")
    assert got[0, 0] == np.float32(-7.5)
    half = feats[::2]  # every other level a target: the stack and the branches interleave
    assert_bits(gpu_pd(env, f, half, grid[:, ::2]), want_pd(fo, half, grid[:, ::2]), "every other split a target")
    f.close()


def test_a_dense_model_through_dense_to_sparse(env):
    ta, torch = env
    T, D, F = 12, 5, 10
    nodes = ta.synth_forest_hist(T, D, F, seed=51, feature_seed=52)
    sn, tr, cv = ta.capi.dense_to_sparse(nodes, T, D, covers=True)
    fo = dict(nodes=sn, trees=tr, covers=cv, num_cols=F, num_classes=1, missing=pd_cases.MISSING, cats=None, categories=None,
              members_left=(), cat_features=())
    f = handle(env, fo)
    x = ta.synth_data_hist(120, F, seed=53, feature_seed=52, missing_prob=0.05, missing=pd_cases.MISSING)
    for feats in ([3], [0, 7]):
        assert_bits(gpu_pd(env, f, feats, x[:, feats]), want_pd(fo, feats, x[:, feats]), f"dense model, targets {feats}")
    # all targets: the dense handle's own raw sums
    dense = ta.Forest(nodes, T, D, F, missing=pd_cases.MISSING)
    raw = dense.predict_raw(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert_bits(gpu_pd(env, f, list(range(F)), x), raw.cpu().numpy().reshape(-1, 1), "dense model, all targets")
    dense.close()
    f.close()


def test_with_treeshap_tables(env):
    """TAHOE_CREATE_PARTIAL_DEPENDENCE | TAHOE_CREATE_CONTRIBS: predict_contribs keeps its bits, and the zero-target value is the
    bias column less global_bias, within the rounding bound of the walk (the bias is a float64 sum rounded once)."""
    ta, torch = env
    fo = pd_cases.random_forest(**pd_cases.RANDOM_CASES[1]["forest"])
    both = handle(env, fo, contribs=True, global_bias=0.25)
    shap = handle(env, fo, pd=False, contribs=True, global_bias=0.25)
    x = torch.from_numpy(pd_cases.random_grid(fo, list(range(fo["num_cols"])), 100, seed=6)).cuda()
    a, b = both.predict_contribs(x), shap.predict_contribs(x)
    torch.cuda.synchronize()
    assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
    bias = a.cpu().numpy()[0, :, -1].astype(np.float64) - 0.25
    got = gpu_pd(env, both, [], np.zeros((1, 0), np.float32))[0].astype(np.float64)
    _, A = pd_ref.pd_f64(fo["nodes"], fo["trees"], fo["covers"], [], np.zeros((1, 0), np.float32), fo["missing"], fo["num_classes"])
    tol = pd_ref.bound(fo["nodes"], fo["trees"], A[0])
    print("zero-target value", got, "bias - global_bias", bias, "bound", tol)
    assert (A[0] >= 0.25).all()  # the bias column's own rounding, 2^-24 (|mean| + 0.25), is within the bound's 2^-23 A
    assert (np.abs(got - bias) <= tol).all()
    both.close()
    shap.close()


def test_device_bytes(env, forests):
    """At create: 8 bytes per node and the workspace; not by a call."""
    fo, f, target_sets = forests["one_class"]
    plain = handle(env, fo, pd=False)
    T, N = len(fo["trees"]), fo["nodes"].size
    assert f.info().device_bytes == plain.info().device_bytes + 8 * N + 4 * T * whole_chunk(T)
    before = f.info().device_bytes
    gpu_pd(env, f, target_sets[0], pd_cases.random_grid(fo, target_sets[0], 200, seed=1))
    assert f.info().device_bytes == before
    plain.close()


def _call(ta, h, out, targets, grid, rows, nt=None):
    t = np.ascontiguousarray(targets, dtype=np.int32) if targets is not None else None
    nt = (0 if t is None else t.size) if nt is None else nt
    st = ta.lib.tahoe_forest_predict_partial_dependence(h, out, t.ctypes.data if t is not None and t.size else None, nt, grid, rows, None)
    return st, ta.lib.tahoe_last_error().decode()


def test_refusals_on_a_device(env, forests):
    ta, torch = env
    fo, f, _ = forests["three_classes"]
    out = torch.zeros((8, 3), device="cuda")
    grid = torch.zeros((8, 2), device="cuda")
    o, g = out.data_ptr(), grid.data_ptr()
    # other handle kinds, and a sparse handle without the flag: before any argument is looked at
    plain = handle(env, fo, pd=False)
    st, msg = _call(ta, plain._h, None, [0, 0], None, 8)
    assert st == UNSUPPORTED and FN in msg and "TAHOE_CREATE_PARTIAL_DEPENDENCE" in msg
    plain.close()
    nodes = ta.synth_forest(4, 3, 6, seed=5)
    for kind, other in (("dense", ta.Forest(nodes, 4, 3, 6)), ("multi-class dense", ta.Forest(nodes, 4, 3, 6, num_classes=2)),
                        ("oblivious", ta.capi.ObliviousForest([1], [0], [0.5], [0], [1.0, 2.0], 2)),
                        ("vector-leaf", ta.capi.VectorForest(pd_cases.chain(1)["nodes"], [0], [[1.0], [2.0], [3.0]], 33))):
        st, msg = _call(ta, other._h, None, [0, 0], None, 8)
        assert st == UNSUPPORTED and FN in msg and f"{kind} handle" in msg, (kind, msg)
        other.close()
    # the targets, naming the index
    for targets, nt, word in (([0], 33, "num_targets 33"), ([0], -1, "num_targets -1"), (None, 2, "targets is NULL"),
                              ([1, 8], None, "targets[1] = 8"), ([-1], None, "targets[0] = -1"), ([2, 5, 2], None, "targets[2] = 2 repeats targets[0]")):
        st, msg = _call(ta, f._h, o, targets, g, 8, nt)
        assert st == INVALID_ARG and FN in msg and word in msg, (targets, msg)
    # bad targets come before grid_rows == 0, which comes before the null pointers
    assert _call(ta, f._h, None, [9], None, 0)[0] == INVALID_ARG
    assert _call(ta, f._h, None, [1, 2], None, 0)[0] == 0
    assert _call(ta, f._h, None, [1, 2], g, 8)[0] == INVALID_ARG
    assert _call(ta, f._h, o, [1, 2], None, 8)[0] == INVALID_ARG
    assert _call(ta, f._h, o, [], None, 8)[0] == 0  # no targets: the grid is not read
    torch.cuda.synchronize()
    want = want_pd(fo, [], np.zeros((8, 0), np.float32))
    assert_bits(out.cpu().numpy(), want, "no targets, NULL grid")
    out.zero_()
    st, msg = _call(ta, f._h, o, [1, 2], g, (1 << 64) // 8)
    assert st == INVALID_ARG and "overflow" in msg
    torch.cuda.synchronize()
    assert not out.any().item()  # nothing launched


def test_python_axes_form(env, forests):
    ta, torch = env
    fo, f, _ = forests["three_classes"]
    a0 = np.linspace(-2, 2, 7).astype(np.float32)
    a1 = np.array([-0.25, 0.0, 0.25, np.nan, pd_cases.MISSING], np.float32)
    out = f.partial_dependence([4, 1], [a0, torch.from_numpy(a1).cuda()])
    torch.cuda.synchronize()
    assert tuple(out.shape) == (7, 5, 3)
    grid = np.stack([np.repeat(a0, 5), np.tile(a1, 7)], axis=1)  # first axis slowest
    assert_bits(out.cpu().numpy().reshape(35, 3), want_pd(fo, [4, 1], grid), "axes")
    fo1, f1, _ = forests["one_class"]
    out = f1.partial_dependence([3], [a0])
    torch.cuda.synchronize()
    assert tuple(out.shape) == (7,)
    assert_bits(out.cpu().numpy().reshape(7, 1), want_pd(fo1, [3], a0[:, None]), "one axis")
    flat = f1.partial_dependence([3], torch.from_numpy(a0[:, None]).cuda())
    assert tuple(flat.shape) == (7,)
