"""Partial dependence at the edges, on the GPU (tests/pd_edges.py holds the cases and says why each is there): bit for bit against
the float32 restatement of tests/pd_ref.py -- a NaN for a NaN where a case can hold one (pd_edges.same) -- and, where the values
are finite, within pd_ref.bound of the float64 evaluation.  Tree-order sums through pd_sum_kernel's blocks of 16 and its tail with
the walk's last workgroup partly filled; IEEE values in the walk's arithmetic; forests without trees, of root leaves, with nodes
before the first root, with an unreachable internal node, with a 30-bit feature id; 3, 7 and 31 targets; other missing
sentinels; the header's promises on output settings, strategies, streams, graph capture and allocation.
Needs an MI355X.  Forests of at most 100 trees of depth <= 3 (or the 32-chain), grids of at most 256 points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pd_cases  # noqa: E402
import pd_edges as pe  # noqa: E402
from test_pd_gpu import _call, assert_bits, bits, env, gpu_pd, handle, want_pd, whole_chunk  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F32 = np.float32


def assert_within_bound(got, fo, feats, grid, label):
    want, tol = pe.want_f64(fo, feats, grid)
    err = np.abs(got.astype(np.float64) - want)
    print(f"{label}: max error {err.max():.3g}, bound there {tol.reshape(err.shape).flat[err.argmax()]:.3g}")
    assert (err <= tol).all(), label


def predict_raw(env, f, fo, feats, grid):
    """[G, C] float32: tahoe_forest_predict_raw of rows that hold the grid in the columns `feats` and 0 elsewhere."""
    _, torch = env
    rows = np.zeros((grid.shape[0], fo["num_cols"]), F32)
    rows[:, feats] = grid
    raw = f.predict_raw(torch.from_numpy(rows).cuda())
    torch.cuda.synchronize()
    f.check()
    return raw.cpu().numpy().reshape(grid.shape[0], -1)


# ---- tree-order sums ----
@pytest.fixture(scope="module")
def order_refs():
    """(case, float32 reference) per (T, C, G), computed once."""
    cache = {}

    def get(T, C, G=pe.ORDER_G):
        if (T, C, G) not in cache:
            fo = pe.order_case(T, C, G)
            cache[T, C, G] = fo, want_pd(fo, fo["targets"], fo["grid"])
        return cache[T, C, G]

    return get


@pytest.mark.parametrize("T,C", pe.ORDER_CASES)
def test_tree_order_sums(env, order_refs, T, C):
    """class_trees = T / C on both sides of 16, 32 and 48, T % 4 = 0 .. 3 with three tiles: the blocks of 16 and the tail of
    pd_sum_kernel in the specified order (tests/test_pd_edges_ref.py: any other order changes at least a quarter of the bits)."""
    fo, want = order_refs(T, C)
    f = handle(env, fo)
    got = gpu_pd(env, f, fo["targets"], fo["grid"])
    f.close()
    assert_bits(got, want, f"T = {T}, C = {C}")
    assert_within_bound(got, fo, fo["targets"], fo["grid"], f"T = {T}, C = {C}")


def test_tree_order_sums_with_a_workspace_stride_of_64(env, order_refs, monkeypatch):
    """(33, 1) under TAHOE_PD_CHUNK_ROWS=64: ws rows 64 floats apart, 130 points in chunks of 64, 64 and 2."""
    fo, want = order_refs(33, 1)
    whole = handle(env, fo)
    monkeypatch.setenv("TAHOE_PD_CHUNK_ROWS", "64")
    f = handle(env, fo)
    monkeypatch.delenv("TAHOE_PD_CHUNK_ROWS")
    assert f.info().device_bytes + 4 * 33 * (whole_chunk(33) - 64) == whole.info().device_bytes  # the knob was read
    assert_bits(gpu_pd(env, f, fo["targets"], fo["grid"]), want, "chunks of 64")
    assert_bits(gpu_pd(env, whole, fo["targets"], fo["grid"]), want, "default chunk")
    f.close()
    whole.close()


def test_tree_order_sums_with_a_rounded_chunk(env, order_refs, monkeypatch):
    """(99, 3) under TAHOE_PD_CHUNK_ROWS=100, rounded up to 128: exactly one chunk, one point more, two chunks."""
    fo, _ = order_refs(99, 3)
    whole = handle(env, fo)
    monkeypatch.setenv("TAHOE_PD_CHUNK_ROWS", "100")
    f = handle(env, fo)
    monkeypatch.delenv("TAHOE_PD_CHUNK_ROWS")
    assert f.info().device_bytes + 4 * 99 * (whole_chunk(99) - 128) == whole.info().device_bytes  # 100 became 128
    whole.close()
    for G in (128, 129, 256):
        fo_g, want = order_refs(99, 3, G)
        assert np.array_equal(fo_g["nodes"], fo["nodes"])  # the same forest, another grid
        assert_bits(gpu_pd(env, f, fo_g["targets"], fo_g["grid"]), want, f"G = {G}")
    f.close()


# ---- IEEE values ----
@pytest.mark.parametrize("name", list(pe.IEEE_CASES))
def test_ieee_values(env, name):
    """No targets, the listed targets, every split feature a target: the restatement's bits (a NaN for a NaN), the hand-derived
    bits where the case has them, and with every split a target predict_raw's bits where the value is not NaN."""
    case = pe.IEEE_CASES[name]()
    f = handle(env, case)
    for run, feats, grid in pe.runs(case):
        want = want_pd(case, feats, grid)
        got = gpu_pd(env, f, feats, grid)
        print(name, run, "got", bits(got).ravel()[:6], "want", bits(want).ravel()[:6])
        assert pe.same(got, want), (name, run, got.ravel()[:8], want.ravel()[:8])
        if run in case["expect"]:
            assert (bits(got) == case["expect"][run]).all(), (name, run, bits(got).ravel()[:8])
        if run == "all":
            raw = predict_raw(env, f, case, feats, grid)
            ok = ~np.isnan(want)
            assert np.array_equal(bits(got)[ok], bits(raw)[ok]), (name, "predict_raw", got[ok][:8], raw[ok][:8])
    f.close()


def test_weight_underflow_and_infinities_by_hand(env):
    """The specified arithmetic's NaN below an underflowed weight, +inf down the spine; NaN and +inf where infinite trees meet."""
    case = pe.weight_underflow()
    f = handle(env, case)
    assert np.isnan(gpu_pd(env, f, [32], case["grid"])).all()
    assert np.isnan(gpu_pd(env, f, [], np.zeros((3, 0), F32))).all()
    got = gpu_pd(env, f, list(range(32)), case["grid_all"])
    assert bits(got)[0, 0] == bits(F32(np.inf)) and np.isfinite(got[1:]).any()
    f.close()
    case = pe.inf_trees()
    f = handle(env, case)
    got = gpu_pd(env, f, [0], case["grid"])
    assert np.isnan(got[:, 0]).all() and (bits(got[:, 1]) == bits(F32(np.inf))).all()
    f.close()


# ---- structure ----
@pytest.mark.parametrize("name", list(pe.STRUCTURE_CASES))
def test_structure(env, name):
    case = pe.STRUCTURE_CASES[name]()
    f = handle(env, case)
    twin = pe.TWINS[name]() if name in pe.TWINS else None
    for run, feats, grid in list(pe.runs(case))[:2]:  # no targets, the listed ones
        got = gpu_pd(env, f, feats, grid)
        assert_bits(got, want_pd(case, feats, grid), f"{name}, {run}")
        assert_within_bound(got, case, feats, grid, f"{name}, {run}")
        if twin is not None:
            assert_bits(got, want_pd(twin, feats, grid), f"{name}, {run}, the plain twin")
    f.close()


def test_a_feature_id_with_bit_29_set(env):
    """No category sets on the handle: the feature id is 30 bits wide, and feature 1 is another feature."""
    case = pe.high_fid()
    f = handle(env, case)
    for feats in case["target_lists"]:
        got = gpu_pd(env, f, feats, case["grid"])
        assert_bits(got, want_pd(case, feats, case["grid"]), f"high fid, targets {feats}")
        assert np.array_equal(bits(got)[:, 0], case["expect"][tuple(feats)])
    f.close()


@pytest.mark.parametrize("C", [1, 3])
def test_no_trees(env, C):
    """A handle without trees creates, and the call writes +0.0f to every entry (the sum from +0.0f over no trees)."""
    ta, torch = env
    case = pe.no_trees(C)
    f = handle(env, case)
    grid = torch.from_numpy(case["grid"]).cuda()
    for targets in ([], case["targets"]):
        out = torch.full((70, C), 7.0, device="cuda")
        st, msg = _call(ta, f._h, out.data_ptr(), targets, grid.data_ptr() if targets else None, 70)
        assert st == 0, (st, msg)
        torch.cuda.synchronize()
        f.check()
        got = out.cpu().numpy()
        assert not bits(got).any(), got.ravel()[:8]
        assert_bits(got, want_pd(case, targets, case["grid"][:, :len(targets)]), f"no trees, targets {targets}")
    f.close()


# ---- targets ----
@pytest.fixture(scope="module")
def one_class(env):
    """pd_cases' one_class forest: as it is (8 columns), and with 33 columns (25 of them split on by no tree)."""
    fo = pd_cases.random_forest(**pd_cases.RANDOM_CASES[0]["forest"])
    wide = dict(fo, num_cols=33)
    f, fw = handle(env, fo), handle(env, wide)
    yield fo, f, wide, fw
    f.close()
    fw.close()


@pytest.mark.parametrize("nt", [3, 7, 31])
def test_three_seven_and_thirty_one_targets(env, one_class, nt):
    fo, f, wide, fw = one_class
    if nt == 31:
        fo, f = wide, fw
        feats = [int(x) for x in np.random.default_rng(31).permutation(33)[:31]]
        assert len(set(feats) & set(pe.split_features(fo))) >= 6
    else:
        feats = [int(x) for x in np.random.default_rng(nt).permutation(8)[:nt]]
    grid = pd_cases.random_grid(fo, feats, 65, seed=nt)
    assert_bits(gpu_pd(env, f, feats, grid), want_pd(fo, feats, grid), f"{nt} targets")


def test_a_target_no_tree_splits_on(env, one_class):
    _, _, wide, fw = one_class
    assert 20 not in pe.split_features(wide) and 2 in pe.split_features(wide)
    grid = pd_cases.random_grid(wide, [20, 2], 65, seed=4)
    alone = gpu_pd(env, fw, [20], grid[:, :1])
    assert_bits(alone, want_pd(wide, [20], grid[:, :1]), "unused target alone")
    mean = gpu_pd(env, fw, [], np.zeros((65, 0), F32))
    assert_bits(alone, mean, "unused target alone = no targets")
    assert_bits(gpu_pd(env, fw, [20, 2], grid), want_pd(wide, [20, 2], grid), "unused target beside a used one")
    assert_bits(gpu_pd(env, fw, [2], grid[:, 1:]), gpu_pd(env, fw, [20, 2], grid), "the unused target changes nothing")


# ---- the missing sentinel ----
@pytest.mark.parametrize("missing", [0.5, np.nan, np.inf], ids=["0.5", "nan", "inf"])
def test_other_missing_sentinels(env, missing):
    """The sentinel, its float32 neighbours and the special values on one and on two targets (every pair)."""
    fo = dict(pd_cases.random_forest(**pd_cases.RANDOM_CASES[0]["forest"]), missing=missing)
    f = handle(env, fo)
    m = F32(missing)
    vals = np.array([m, np.nextafter(m, F32(np.inf)), np.nextafter(m, F32(-np.inf)), m + F32(5e-7)] + pd_cases.SPECIALS, F32)
    for fid, other in ((2, 5), (5, 2)):
        one = gpu_pd(env, f, [fid], vals[:, None])
        assert_bits(one, want_pd(fo, [fid], vals[:, None]), f"missing {missing} on {fid}")
        grid = np.stack([np.repeat(vals, vals.size), np.tile(vals, vals.size)], axis=1)
        assert_bits(gpu_pd(env, f, [fid, other], grid), want_pd(fo, [fid, other], grid), f"missing {missing} on {fid} and {other}")
    f.close()


# ---- the header's promises ----
@pytest.mark.parametrize("which", ["one_class", "three_classes"])
def test_output_settings_and_strategies_change_no_bit(env, which):
    """No AVG division, no global_bias, no output transform; the predict strategy is not this call's."""
    ta, _ = env
    case = next(c for c in pd_cases.RANDOM_CASES if c["id"] == which)
    fo = pd_cases.random_forest(**case["forest"])
    feats = case["targets"][1]
    grid = pd_cases.random_grid(fo, feats, 130, seed=15)
    want = want_pd(fo, feats, grid)
    plain = handle(env, fo)
    assert_bits(gpu_pd(env, plain, feats, grid), want, which)
    output = ta.capi.OUT_AVG | (ta.capi.OUT_SIGMOID if fo["num_classes"] == 1 else ta.capi.OUT_SOFTMAX)
    dressed = handle(env, fo, output=output, global_bias=0.375)
    assert dressed.info().device_bytes == plain.info().device_bytes
    assert_bits(gpu_pd(env, dressed, feats, grid), want, f"{which}, output 0x{output:x}, global_bias 0.375")
    before = plain.info().device_bytes
    accepted = []
    for strategy in range(ta.capi.STRATEGY_QRING + 1):
        try:
            plain.set_strategy(strategy)
        except ta.TahoeError:
            continue
        accepted.append(strategy)
        assert_bits(gpu_pd(env, plain, feats, grid), want, f"{which}, strategy {strategy}")
    assert ta.capi.STRATEGY_AUTO in accepted and len(accepted) >= 2, accepted
    assert plain.info().device_bytes == before
    plain.close()
    dressed.close()


def test_streams_and_graph_capture(env):
    """Asynchronous on the caller's stream, nothing allocated: a side stream, and one captured call replayed twice."""
    _, torch = env
    fo = pe.order_case(51, 3)
    feats = fo["targets"]
    f = handle(env, fo)
    want = gpu_pd(env, f, feats, fo["grid"])
    assert_bits(want, want_pd(fo, feats, fo["grid"]), "default stream")
    before = f.info().device_bytes
    grid = torch.from_numpy(fo["grid"]).cuda()
    out = torch.zeros((130, 3), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    f.partial_dependence(feats, grid, out=out, stream=side)
    side.synchronize()
    f.check(side)
    assert_bits(out.cpu().numpy(), want, "side stream")
    out.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        f.partial_dependence(feats, grid, out=out, stream=side)
    for replay in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        f.check()
        assert_bits(out.cpu().numpy(), want, f"replay {replay}")
    assert f.info().device_bytes == before
    del g
    f.close()
