"""Staged prediction on the GPU (tahoe_forest_set_stages / tahoe_forest_predict_staged): every stage bit for bit
  - raw sums: the CPU oracle's sequential float32 sum on the forest cut to the stage's trees;
  - transformed outputs: tahoe_forest_predict of a GPU handle created from the cut forest under the same strategy
    (expf on the CPU need not match the GPU's);
never the staged call against itself.  Shapes are the smallest at which the stage cursor can go wrong: tree counts that are no
multiple of ROWTILE's four waves or of the sparse consumer's batch of 4, more trees than the 32 ring entries, class ends inside
a round, stages inside / at the end of / across a round, rows around the 64-row tile and the 16-rows-per-wave owner mapping.
Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
UNSUPPORTED = 7
_cache = {}


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta
    from oracle import oracle

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch, oracle


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def strategy(ta, name):
    return getattr(ta, "STRATEGY_" + name)


def rows_data(ta, rows, cols, seed):
    """Rows with the missing sentinel and NaN among them."""
    return ta.synth_data(rows, cols, seed=seed, missing_prob=0.08, missing=MISSING, nan_prob=0.04)


# ---------------------------------------------------------------------------------------------------------------- dense
D1 = dict(T=13, depth=4, cols=9, stages=[1, 2, 3, 4, 5, 8, 13], rows=130)


def dense_c1(ta, oracle):
    """13 trees of depth 4 (tree 2's root is a leaf), 130 rows, and the oracle's raw sums of every stage, computed once."""
    if "d1" not in _cache:
        T, depth, cols = D1["T"], D1["depth"], D1["cols"]
        nodes = ta.synth_forest(T, depth, cols, seed=101, leaf_prob=0.15)
        per = ta.capi.tree_num_nodes(depth)
        nodes["bits"][2 * per] = nodes["bits"][2 * per] | np.int32(-2 ** 31)
        nodes["val"][2 * per] = 0.625
        data = rows_data(ta, D1["rows"], cols, seed=102)
        want = np.stack([oracle.predict(nodes[: n * per], n, depth, data, MISSING)[0] for n in D1["stages"]], axis=1)
        want.setflags(write=False)
        _cache["d1"] = (nodes, data, want)
    return _cache["d1"]


@pytest.mark.parametrize("name", ["DIRECT", "ROWTILE", "AUTO"])
def test_dense_raw_stages_match_the_oracle(env, name):
    ta, torch, oracle = env
    nodes, data, want = dense_c1(ta, oracle)
    f = ta.Forest(nodes, D1["T"], D1["depth"], D1["cols"], missing=MISSING)
    f.set_strategy(strategy(ta, name))
    f.set_stages(D1["stages"])
    assert f.staged_strategy(130) == (ta.STRATEGY_ROWTILE if name == "AUTO" else strategy(ta, name))
    x = torch.from_numpy(data).cuda()
    for rows in (1, 63, 64, 65, 130):
        got = f.predict_staged(x[:rows].contiguous())
        f.check()
        assert tuple(got.shape) == (rows, len(D1["stages"]))
        assert np.array_equal(bits(got), bits(want[:rows])), (name, rows)
    f.close()


@pytest.mark.parametrize("name", ["DIRECT", "ROWTILE"])
@pytest.mark.parametrize("out_name", ["AVG", "AVG_SIGMOID", "SIGMOID_THRESHOLD", "AVG_THRESHOLD_BIAS", "RAW_BIAS"])
def test_dense_outputs_match_a_truncated_handle(env, name, out_name):
    ta, torch, oracle = env
    nodes, data, _ = dense_c1(ta, oracle)
    output, thr, bias = {"AVG": (ta.OUT_AVG, 0.0, 0.0), "AVG_SIGMOID": (ta.OUT_AVG | ta.OUT_SIGMOID, 0.0, 0.25),
                         "SIGMOID_THRESHOLD": (ta.OUT_SIGMOID | ta.OUT_THRESHOLD, 0.5, 0.0),
                         "AVG_THRESHOLD_BIAS": (ta.OUT_AVG | ta.OUT_THRESHOLD, 0.01, -0.125),
                         "RAW_BIAS": (ta.OUT_RAW, 0.0, 0.5)}[out_name]
    T, depth, cols = D1["T"], D1["depth"], D1["cols"]
    per = ta.capi.tree_num_nodes(depth)
    x = torch.from_numpy(data).cuda()
    f = ta.Forest(nodes, T, depth, cols, missing=MISSING, output=output, threshold=thr, global_bias=bias)
    f.set_strategy(strategy(ta, name))
    f.set_stages(D1["stages"])
    got = f.predict_staged(x)
    for s, n in enumerate(D1["stages"]):
        cut = ta.Forest(nodes[: n * per], n, depth, cols, missing=MISSING, output=output, threshold=thr, global_bias=bias)
        cut.set_strategy(strategy(ta, name))
        assert np.array_equal(bits(got[:, s]), bits(cut.predict(x))), (name, out_name, n)
        cut.close()
    f.close()


# ---------------------------------------------------------------------------------------------------------- multi-class
MC = dict(C=3, Tc=5, depth=4, cols=7, rows=130)


def dense_mc(ta, oracle):
    """15 trees, class = tree % 3, and per class the oracle's raw sums after 1 .. 5 rounds: want[rows][5][3]."""
    if "mc" not in _cache:
        C, Tc, depth, cols = MC["C"], MC["Tc"], MC["depth"], MC["cols"]
        nodes = ta.synth_forest(C * Tc, depth, cols, seed=111, leaf_prob=0.2)
        per = ta.capi.tree_num_nodes(depth)
        data = rows_data(ta, MC["rows"], cols, seed=112)
        trees = nodes.reshape(C * Tc, per)
        want = np.empty((MC["rows"], Tc, C), np.float32)
        for c in range(C):
            for n in range(1, Tc + 1):
                want[:, n - 1, c] = oracle.predict(np.ascontiguousarray(trees[c::C][:n]).ravel(), n, depth, data, MISSING)[0]
        want.setflags(write=False)
        _cache["mc"] = (nodes, data, want)
    return _cache["mc"]


@pytest.mark.parametrize("name", ["DIRECT", "ROWTILE", "AUTO"])
@pytest.mark.parametrize("stages", [[1, 2, 5], [5]])
def test_multiclass_raw_stages_match_the_oracle(env, name, stages):
    ta, torch, oracle = env
    nodes, data, want = dense_mc(ta, oracle)
    C, Tc = MC["C"], MC["Tc"]
    f = ta.Forest(nodes, C * Tc, MC["depth"], MC["cols"], missing=MISSING, num_classes=C)
    f.set_strategy(strategy(ta, name))
    f.set_stages(stages)
    x = torch.from_numpy(data).cuda()
    for rows in (1, 65, 130):
        got = f.predict_staged(x[:rows].contiguous())
        assert tuple(got.shape) == (rows, len(stages), C)
        assert np.array_equal(bits(got), bits(want[:rows, [n - 1 for n in stages], :])), (name, stages, rows)
    f.close()


@pytest.mark.parametrize("name", ["DIRECT", "ROWTILE"])
@pytest.mark.parametrize("out_name", ["RAW", "AVG", "AVG_SIGMOID", "SOFTMAX", "AVG_SOFTMAX_BIAS"])
def test_multiclass_outputs_match_a_truncated_handle(env, name, out_name):
    ta, torch, oracle = env
    nodes, data, want = dense_mc(ta, oracle)
    output, bias = {"RAW": (ta.OUT_RAW, 0.0), "AVG": (ta.OUT_AVG, 0.0), "AVG_SIGMOID": (ta.OUT_AVG | ta.OUT_SIGMOID, 0.0),
                    "SOFTMAX": (ta.OUT_SOFTMAX, 0.0), "AVG_SOFTMAX_BIAS": (ta.OUT_AVG | ta.OUT_SOFTMAX, 0.5)}[out_name]
    C, Tc, depth, cols = MC["C"], MC["Tc"], MC["depth"], MC["cols"]
    per = ta.capi.tree_num_nodes(depth)
    x = torch.from_numpy(data).cuda()
    f = ta.Forest(nodes, C * Tc, depth, cols, missing=MISSING, output=output, global_bias=bias, num_classes=C)
    f.set_strategy(strategy(ta, name))
    for stages in ([1, 2, 5], [5]):
        f.set_stages(stages)
        got = f.predict_staged(x)
        for s, n in enumerate(stages):
            cut = ta.Forest(nodes[: n * C * per], n * C, depth, cols, missing=MISSING, output=output, global_bias=bias, num_classes=C)
            cut.set_strategy(strategy(ta, name))
            assert np.array_equal(bits(got[:, s, :]), bits(cut.predict(x))), (name, out_name, stages, n)
            cut.close()
        if out_name == "RAW":
            assert np.array_equal(bits(got), bits(want[:, [n - 1 for n in stages], :]))
    f.close()


# --------------------------------------------------------------------------------------------------------------- sparse
SP = dict(T=37, cols=20, rows=130, stages=[1, 3, 4, 5, 32, 33, 37], stages2=[1, 4, 17, 18])


def sparse_forest(ta, oracle):
    """37 irregular trees; the oracle's raw sums of every stage, and of the first 36 trees as two classes."""
    if "sp" not in _cache:
        sn, tr = ta.capi.synth_sparse_forest(SP["T"], SP["cols"], 3, 12, 0.3, 65535, 121)
        data = rows_data(ta, SP["rows"], SP["cols"], seed=122)
        want = np.stack([oracle.sparse_predict(sn, tr[:n], data, MISSING)[0] for n in SP["stages"]], axis=1)
        want2 = np.empty((SP["rows"], len(SP["stages2"]), 2), np.float32)
        for c in range(2):
            for s, n in enumerate(SP["stages2"]):
                want2[:, s, c] = oracle.sparse_predict(sn, np.ascontiguousarray(tr[:36][c::2][:n]), data, MISSING)[0]
        want.setflags(write=False)
        want2.setflags(write=False)
        _cache["sp"] = (sn, tr, data, want, want2)
    return _cache["sp"]


@pytest.mark.parametrize("name", ["DIRECT", "ROWTILE", "TILEBLOCK", "AUTO"])
def test_sparse_raw_stages_match_the_oracle(env, name):
    ta, torch, oracle = env
    sn, tr, data, want, _ = sparse_forest(ta, oracle)
    f = ta.capi.SparseForest(sn, tr, SP["cols"], missing=MISSING)
    f.set_strategy(strategy(ta, name))
    f.set_stages(SP["stages"])
    assert f.staged_strategy(130) == (ta.STRATEGY_TILEBLOCK if name == "AUTO" else strategy(ta, name))
    x = torch.from_numpy(data).cuda()
    for rows in (1, 64, 130):
        got = f.predict_staged(x[:rows].contiguous())
        f.check()  # TAHOE_OK after every call: no ring wait of the TILEBLOCK kernel timed out
        assert np.array_equal(bits(got), bits(want[:rows])), (name, rows)
    f.close()


@pytest.mark.parametrize("name", ["DIRECT", "ROWTILE", "TILEBLOCK"])
def test_sparse_multiclass_stages(env, name):
    ta, torch, oracle = env
    sn, tr, data, _, want2 = sparse_forest(ta, oracle)
    sn36, tr36 = sn[: tr[36]], tr[:36]
    x = torch.from_numpy(data).cuda()
    f = ta.capi.SparseForest(sn36, tr36, SP["cols"], missing=MISSING, num_classes=2)
    f.set_strategy(strategy(ta, name))
    f.set_stages(SP["stages2"])
    for rows in (1, 64, 130):
        got = f.predict_staged(x[:rows].contiguous())
        f.check()
        assert tuple(got.shape) == (rows, 4, 2)
        assert np.array_equal(bits(got), bits(want2[:rows])), (name, rows)
    f.close()
    # output bits: AVG | SOFTMAX with a bias against truncated handles
    kw = dict(missing=MISSING, num_classes=2, output=ta.OUT_AVG | ta.OUT_SOFTMAX, global_bias=0.25)
    f = ta.capi.SparseForest(sn36, tr36, SP["cols"], **kw)
    f.set_strategy(strategy(ta, name))
    f.set_stages(SP["stages2"])
    got = f.predict_staged(x)
    f.check()
    for s, n in enumerate(SP["stages2"]):
        cut = ta.capi.SparseForest(sn[: tr[2 * n]], tr[: 2 * n], SP["cols"], **kw)
        cut.set_strategy(strategy(ta, name))
        assert np.array_equal(bits(got[:, s, :]), bits(cut.predict(x))), (name, n)
        cut.close()
    f.close()


# ---------------------------------------------------------------------------------------------------------- categorical
def cat_forest(ta, T, cols, cat_feats, seed, universe=200):
    """synth_sparse_forest with every inner node on a feature of cat_feats made a categorical split."""
    sn, tr = ta.capi.synth_sparse_forest(T, cols, 3, 10, 0.3, 65535, seed)
    rng = np.random.default_rng(seed)
    b = sn["bits"].view(np.uint32)
    inner = np.flatnonzero((b >> 31) == 0)
    chosen = inner[np.isin(b[inner] & ((1 << 30) - 1), cat_feats)]
    cats = {int(i): rng.choice(universe, size=int(rng.integers(1, 60)), replace=False) for i in chosen}
    ml = {int(i) for i in chosen if rng.random() < 1 / 3}
    return sn, tr, cats, ml


@pytest.mark.parametrize("name", ["DIRECT", "ROWTILE", "TILEBLOCK"])
def test_categorical_stages(env, name):
    ta, torch, oracle = env
    cols, feats, T, stages, rows = 12, [1, 5, 9], 9, [2, 9], 130
    sn, tr, cats, ml = cat_forest(ta, T, cols, feats, seed=131)
    assert len(cats) > 20 and 0 < len(ml) < len(cats)
    data = rows_data(ta, rows, cols, seed=132)
    rng = np.random.default_rng(133)
    for fid in feats:  # categories, non-integers, negatives, NaN and the sentinel
        v = rng.integers(0, 220, rows).astype(np.float32)
        u = rng.random(rows)
        v = np.where(u < 0.1, v + np.float32(0.5), v)
        v = np.where((u >= 0.1) & (u < 0.2), np.float32(-1.0), v)
        v = np.where((u >= 0.2) & (u < 0.27), np.float32(np.nan), v)
        v = np.where((u >= 0.27) & (u < 0.34), np.float32(MISSING), v)
        data[:, fid] = v
    data = np.ascontiguousarray(data, dtype=np.float32)
    _, (node, offset, words, mla) = ta.capi.pack_categorical(cats, ml)
    x = torch.from_numpy(data).cuda()
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, categories=cats, members_left=ml)
    f.set_strategy(strategy(ta, name))
    f.set_stages(stages)
    got = f.predict_staged(x)
    f.check()
    for s, n in enumerate(stages):
        want = categorical_ref.predict(sn, tr[:n], data, MISSING, node, offset, words, mla)[0]
        assert np.array_equal(bits(got[:, s]), bits(want)), (name, n)
    f.close()


# -------------------------------------------------------------------------------------------- whole forest, bookkeeping
@pytest.mark.parametrize("kind", ["dense", "multiclass", "sparse"])
def test_the_stage_of_the_whole_forest_is_predict(env, kind):
    ta, torch, oracle = env
    if kind == "dense":
        nodes, data, _ = dense_c1(ta, oracle)
        f = ta.Forest(nodes, D1["T"], D1["depth"], D1["cols"], missing=MISSING, output=ta.OUT_AVG | ta.OUT_SIGMOID, global_bias=0.1)
        names, Tc = ("DIRECT", "ROWTILE"), D1["T"]
    elif kind == "multiclass":
        nodes, data, _ = dense_mc(ta, oracle)
        f = ta.Forest(nodes, 15, MC["depth"], MC["cols"], missing=MISSING, output=ta.OUT_SOFTMAX, num_classes=3)
        names, Tc = ("DIRECT", "ROWTILE"), 5
    else:
        sn, tr, data, _, _ = sparse_forest(ta, oracle)
        f = ta.capi.SparseForest(sn, tr, SP["cols"], missing=MISSING, output=ta.OUT_SIGMOID)
        names, Tc = ("DIRECT", "ROWTILE", "TILEBLOCK"), SP["T"]
    x = torch.from_numpy(data).cuda()
    f.set_stages([Tc])
    for name in names:
        f.set_strategy(strategy(ta, name))
        got = f.predict_staged(x)
        want = f.predict(x)
        f.check()
        assert np.array_equal(bits(got[:, 0]), bits(want)), (kind, name)
    f.close()


def test_stage_bookkeeping(env):
    ta, torch, oracle = env
    nodes, data, want = dense_c1(ta, oracle)
    T, depth, cols, stages = D1["T"], D1["depth"], D1["cols"], D1["stages"]
    x = torch.from_numpy(data).cuda()
    f = ta.Forest(nodes, T, depth, cols, missing=MISSING)
    before = bits(f.predict(x))
    bytes0 = f.info().device_bytes
    # no stages yet
    assert f.staged_strategy(130) == 0
    with pytest.raises(ta.TahoeError) as e:
        f.predict_staged(x)
    assert e.value.status == UNSUPPORTED and "no stages" in str(e.value)
    # refusals name the index and keep what was set
    f.set_stages([2, 5])
    assert f.info().device_bytes == bytes0 + 8
    for bad, word in (([0, 1], "rounds[0]"), ([1, 14], "rounds[1]"), ([1, 3, 3], "rounds[2]"), ([4, 2], "rounds[1]")):
        with pytest.raises(ta.TahoeError) as e:
            f.set_stages(bad)
        assert e.value.status == 1 and word in str(e.value), bad
    assert np.array_equal(bits(f.predict_staged(x)), bits(want[:, [1, 4]]))
    # a second call replaces the first
    f.set_stages([1, 8, 13])
    assert f.info().device_bytes == bytes0 + 12
    whole = f.predict_staged(x)
    assert np.array_equal(bits(whole), bits(want[:, [0, 5, 6]]))
    # one call and two halves: the same bits
    halves = torch.cat([f.predict_staged(x[:57].contiguous()), f.predict_staged(x[57:].contiguous())])
    assert np.array_equal(bits(halves), bits(whole))
    # a forced strategy without a staged form
    f.set_strategy(ta.STRATEGY_QRING)
    assert f.staged_strategy(130) == 0
    with pytest.raises(ta.TahoeError) as e:
        f.predict_staged(x)
    assert e.value.status == UNSUPPORTED and "staged form" in str(e.value)
    f.set_strategy(ta.STRATEGY_AUTO)
    # rows == 0 and NULL pointers
    assert ta.lib.tahoe_forest_predict_staged(f._h, None, None, 0, None) == 0
    assert ta.lib.tahoe_forest_predict_staged(f._h, None, x.data_ptr(), 10, None) == 1
    # cleared
    f.set_stages(None)
    assert f.info().device_bytes == bytes0 and f.staged_strategy(130) == 0
    with pytest.raises(ta.TahoeError) as e:
        f.predict_staged(x)
    assert e.value.status == UNSUPPORTED
    # the plain predict is what it was
    assert np.array_equal(bits(f.predict(x)), before)
    f.check()
    f.close()


def test_staged_predict_is_capturable(env):
    """After set_stages the call allocates nothing: it can be captured into a HIP graph and replayed."""
    ta, torch, oracle = env
    sn, tr, data, want, _ = sparse_forest(ta, oracle)
    f = ta.capi.SparseForest(sn, tr, SP["cols"], missing=MISSING)
    f.set_stages(SP["stages"])
    x = torch.from_numpy(data).cuda()
    out = torch.zeros((SP["rows"], len(SP["stages"])), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f.predict_staged(x, out=out)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f.predict_staged(x, out=out)
    g.replay()
    torch.cuda.synchronize()
    f.check()
    assert np.array_equal(bits(out), bits(want))
    f.close()
