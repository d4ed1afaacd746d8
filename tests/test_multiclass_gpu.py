"""Multi-class forests (tahoe_forest_create_multiclass) on the GPU against the CPU oracle.  Needs an MI355X.

Tree t belongs to class t % C.  Bars: the margins of class c are bit for bit oracle.predict on the sub-forest of trees
c, c + C, ... (raw, and the sums of the leaf pass); leaf indices are bit for bit the oracle's on the whole forest; AVG and
bias bit for bit numpy float32; sigmoid within 1e-6 relative; softmax within 1e-6 + 1e-5 p of the float64 softmax of the
float32 values after AVG and bias.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MISSING = -999.0
FORMS = set()  # kernel forms the predicts of this file ran (test_every_form_was_exercised)
KNOBS = ("TAHOE_QRING_CHAINS", "TAHOE_QRING_CODE8", "TAHOE_QRING_REGIONS", "TAHOE_QRING_SLICES", "TAHOE_QRING_WIDE",
         "TAHOE_QRING_GROUPS")


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta
    from oracle import oracle

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, oracle, torch


@pytest.fixture
def knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def num_cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def forest_nodes(ta, gen, T, D, cols, seed):
    if gen == "hist":
        return ta.synth_forest_hist(T, D, cols, seed=seed, feature_seed=seed + 1, max_bins=200, scale_decades=2.0)
    return ta.synth_forest(T, D, cols, seed=seed, leaf_prob=0.05)


def batch(ta, gen, rows, cols, seed):
    if gen == "hist":
        x = ta.synth_data_hist(rows, cols, seed=seed, feature_seed=seed - 1, scale_decades=2.0, missing_prob=0.03, missing=MISSING)
        rng = np.random.default_rng(seed)
        x[rng.random(x.shape) < 0.01] = np.nan
        return x
    return ta.synth_data(rows, cols, seed=seed, missing_prob=0.03, missing=MISSING, nan_prob=0.01)


def expected(oracle, nodes, C, T, D, data):
    """-> (margins [rows, C] float32, leaf [rows, T] uint32)."""
    per = nodes.size // T
    by_tree = nodes.reshape(T, per)
    margins = np.stack([oracle.predict(np.ascontiguousarray(by_tree[c::C]).reshape(-1), T // C, D, data, MISSING, threads=8)[0]
                        for c in range(C)], axis=1)
    leaf = oracle.predict(nodes, T, D, data, MISSING, want_leaf=True, threads=8)[1]
    return margins, leaf


def check_outputs(env, nodes, C, T, D, cols, x, margins, bias=0.25):
    """AVG + bias (bit-exact), + SIGMOID (1e-6 relative), + SOFTMAX (float64 reference) on AUTO."""
    ta, oracle, torch = env
    Tc = T // C
    z = margins / np.float32(Tc) + np.float32(bias)
    for output in (ta.OUT_AVG, ta.OUT_AVG | ta.OUT_SIGMOID, ta.OUT_AVG | ta.OUT_SOFTMAX, ta.OUT_SOFTMAX):
        f = ta.Forest(nodes, T, D, cols, missing=MISSING, output=output, global_bias=bias, num_classes=C)
        got = f.predict(x).cpu().numpy()
        f.check()
        f.close()
        assert got.shape == (x.shape[0], C)
        zz = z if output & ta.OUT_AVG else margins + np.float32(bias)
        if output == ta.OUT_AVG:
            assert np.array_equal(bits(got), bits(zz))
        elif output & ta.OUT_SIGMOID:
            want = 1.0 / (1.0 + np.exp(-zz.astype(np.float64)))
            assert np.allclose(got, want, rtol=1e-6, atol=0)
        else:
            e = np.exp(zz.astype(np.float64) - zz.max(axis=1, keepdims=True))
            p = e / e.sum(axis=1, keepdims=True)
            assert np.all(np.abs(got - p) <= 1e-6 + 1e-5 * p), np.abs(got - p).max()


def run_mc(env, nodes, C, T, D, cols, data, rows_list, strategies=None, outputs=True, want_form=None, relayout=False):
    ta, oracle, torch = env
    margins, leaf_want = expected(oracle, nodes, C, T, D, data)
    f = ta.Forest(nodes, T, D, cols, missing=MISSING, num_classes=C, relayout=relayout)
    assert f.num_classes == C and ta.lib.tahoe_forest_num_classes(f._h) == C
    info = f.info()
    if strategies is None:
        strategies = [ta.STRATEGY_DIRECT] + ([ta.STRATEGY_ROWTILE] if info.lds_bytes_per_block > 0 else []) + (
            [ta.STRATEGY_QRING] if info.qring_walkers > 0 else []) + [ta.STRATEGY_AUTO]
    xall = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    for s in strategies:
        f.set_strategy(s)
        for R in rows_list:
            x = xall[:R].contiguous()
            form = f.kernel_form(R)
            FORMS.add(form)
            leaf, sums = f.predict_leaf_idx(x)
            raw = f.predict_raw(x)
            f.check()
            assert raw.shape == (R, C) and sums.shape == (R, C) and leaf.shape == (R, T)
            tag = f"strategy {s}, rows {R}, form {form}"
            assert np.array_equal(bits(raw.cpu().numpy()), bits(margins[:R])), "margins: " + tag
            assert np.array_equal(bits(sums.cpu().numpy()), bits(margins[:R])), "leaf-pass sums: " + tag
            assert np.array_equal(bits(leaf.cpu().numpy()), leaf_want[:R]), "leaf indices: " + tag
    if want_form is not None:
        f.set_strategy(ta.STRATEGY_AUTO)
        assert f.kernel_form(rows_list[-1]) == want_form
    f.close()
    if outputs:
        check_outputs(env, nodes, C, T, D, cols, xall, margins)
    return margins


# C, Tc, depth, cols, generator, create-time knobs, rows (+ "wave": whole waves of the large tile plus a remainder), AUTO's form
CASES = [
    ("degenerate", 2, 1, 0, 1, "uniform", {}, [1, 63], None),
    ("small", 3, 5, 3, 18, "uniform", {}, [1, 65, 129], None),
    ("region8", 7, 20, 6, 54, "hist", {}, [193, 385, "wave384"], "qring_region8"),
    ("region6", 10, 30, 8, 100, "uniform", {}, [577, "wave384"], "qring_region6"),
    ("region3", 4, 100, 10, 200, "uniform", {"TAHOE_QRING_CODE8": "0", "TAHOE_QRING_CHAINS": "3"}, [63, 20_000], "qring_region3"),
    ("region2", 4, 100, 10, 200, "uniform", {"TAHOE_QRING_CODE8": "0", "TAHOE_QRING_CHAINS": "2"}, [129, 20_000], "qring_region2"),
    ("mixed", 4, 100, 10, 200, "uniform", {"TAHOE_QRING_CODE8": "0"}, [385, "wave192"], "qring_region_mixed"),
    ("split", 26, 8, 6, 16, "uniform", {}, [1000], "qring_split"),
    ("columns", 10, 30, 8, 100, "uniform", {"TAHOE_QRING_REGIONS": "0"}, [65, 577], "qring_columns"),
    ("qwide", 10, 30, 6, 784, "uniform", {}, [1, 193, 2000], "qring_wide"),
    ("gx", 10, 30, 6, 784, "uniform", {"TAHOE_QRING_WIDE": "0"}, [63, 700], "qring_gx"),
    ("shallow", 5, 40, 3, 32, "uniform", {}, [1, 129, 5000], "rowtile"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_margins_leaves_and_outputs(env, knobs, case):
    ta, oracle, torch = env
    name, C, Tc, D, cols, gen, env_knobs, rows_list, form = case
    for k, v in env_knobs.items():
        knobs.setenv(k, v)
    cus = num_cus(torch)
    rows_list = [cus * 384 + 321 if r == "wave384" else cus * 192 + 777 if r == "wave192" else r for r in rows_list]
    T = C * Tc
    nodes = forest_nodes(ta, gen, T, D, cols, seed=100 + len(name) + cols)
    data = batch(ta, gen, max(rows_list), cols, seed=200 + cols)
    run_mc(env, nodes, C, T, D, cols, data, rows_list, want_form=form, outputs=name not in ("region2", "gx", "columns"))


def test_tree_groups_with_a_boundary_inside_a_class(env, knobs):
    """Forests with more than 32767 thresholds on a feature are quantised in groups of consecutive (internal) trees; a group
    that begins inside a class continues that class's running sum.  Tree slices (small batch) and plain tiles."""
    ta, oracle, torch = env
    C, Tc, D, cols = 7, 100, 8, 4
    T = C * Tc
    nodes = ta.synth_forest(T, D, cols, seed=43)
    f = ta.Forest(nodes, T, D, cols, missing=MISSING, num_classes=C)
    G = f.info().qring_groups
    assert G >= 2 and f.get_strategy(500) == ta.STRATEGY_QRING
    assert any((T * k // G) % Tc != 0 for k in range(1, G))  # a group boundary inside a class
    f.close()
    data = ta.synth_data(20_000, cols, seed=44, missing_prob=0.05, missing=MISSING, nan_prob=0.01)
    run_mc(env, nodes, C, T, D, cols, data, [1, 500, 20_000], strategies=[ta.STRATEGY_QRING, ta.STRATEGY_DIRECT])


def test_one_class_equals_an_ordinary_handle(env, knobs):
    ta, oracle, torch = env
    T, D, cols, R = 60, 7, 40, 3000
    nodes = ta.synth_forest(T, D, cols, seed=71, leaf_prob=0.05)
    x = torch.from_numpy(ta.synth_data(R, cols, seed=72, missing_prob=0.03, missing=MISSING, nan_prob=0.01)).cuda()
    out = ta.OUT_AVG | ta.OUT_SIGMOID
    params = ta.ForestParams(0, D, T, cols, 0, out, 0.0, 0.5, 0, MISSING)
    h = ctypes.c_void_p()
    assert ta.lib.tahoe_forest_create_multiclass(ctypes.byref(h), nodes.ctypes.data, ctypes.byref(params), 1, 0) == 0
    one = ta.Forest.__new__(ta.Forest)
    one.params, one._h, one.num_trees, one.depth, one.num_cols = params, h, T, D, cols
    one.num_classes = ta.lib.tahoe_forest_num_classes(h)
    assert one.num_classes == 1
    plain = ta.Forest(nodes, T, D, cols, missing=MISSING, output=out, global_bias=0.5)
    for s in (ta.STRATEGY_AUTO, ta.STRATEGY_DIRECT, ta.STRATEGY_ROWTILE, ta.STRATEGY_TILEBLOCK, ta.STRATEGY_TILERING, ta.STRATEGY_QRING):
        one.set_strategy(s)
        plain.set_strategy(s)
        assert one.kernel_form(R) == plain.kernel_form(R)
        for fn in ("predict", "predict_raw"):
            a, b = getattr(one, fn)(x), getattr(plain, fn)(x)
            assert a.shape == (R,) and np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), (s, fn)
        la, sa = one.predict_leaf_idx(x)
        lb, sb = plain.predict_leaf_idx(x)
        assert np.array_equal(la.cpu().numpy(), lb.cpu().numpy()) and np.array_equal(bits(sa.cpu().numpy()), bits(sb.cpu().numpy()))
    one.check()
    one.close()
    plain.close()


def test_each_column_equals_the_handle_of_its_class(env, knobs):
    ta, oracle, torch = env
    C, Tc, D, cols, R = 6, 25, 8, 64, 4000
    T = C * Tc
    nodes = ta.synth_forest(T, D, cols, seed=81, leaf_prob=0.05)
    x = torch.from_numpy(ta.synth_data(R, cols, seed=82, missing_prob=0.03, missing=MISSING, nan_prob=0.01)).cuda()
    mc = ta.Forest(nodes, T, D, cols, missing=MISSING, num_classes=C)
    got = mc.predict_raw(x).cpu().numpy()
    by_tree = nodes.reshape(T, -1)
    for c in range(C):
        one = ta.Forest(np.ascontiguousarray(by_tree[c::C]).reshape(-1), Tc, D, cols, missing=MISSING)
        assert np.array_equal(bits(got[:, c]), bits(one.predict_raw(x).cpu().numpy())), c
        one.close()
    mc.close()


def test_probability_relayout_changes_nothing(env, knobs):
    ta, oracle, torch = env
    C, Tc, D, cols = 5, 12, 7, 48
    T = C * Tc
    nodes = ta.capi.set_probability_weights(ta.synth_forest(T, D, cols, seed=91, leaf_prob=0.05), T, D)
    data = ta.synth_data(2000, cols, seed=92, missing_prob=0.03, missing=MISSING, nan_prob=0.01)
    f = ta.Forest(nodes, T, D, cols, missing=MISSING, num_classes=C, relayout=True)
    assert f.info().relayout == 1 and f.info().relayout_swaps > 0
    FORMS.add(f.kernel_form(2000))
    f.close()
    run_mc(env, nodes, C, T, D, cols, data, [65, 2000], relayout=True, outputs=False)


def test_refusals(env, knobs):
    ta, oracle, torch = env
    C, Tc, D, cols, R = 4, 10, 6, 32, 500
    T = C * Tc
    nodes = ta.synth_forest(T, D, cols, seed=95)
    f = ta.Forest(nodes, T, D, cols, missing=MISSING, num_classes=C)
    for s in (ta.STRATEGY_TILEBLOCK, ta.STRATEGY_TILERING):
        with pytest.raises(ta.TahoeError) as e:
            f.set_strategy(s)
        assert e.value.status == 7
    assert f.get_strategy(R) in (ta.STRATEGY_ROWTILE, ta.STRATEGY_QRING, ta.STRATEGY_DIRECT)
    data = ta.synth_data(R, cols, seed=96)
    x = torch.from_numpy(data).cuda()
    sums = torch.full((R,), 7.0, device="cuda")
    with pytest.raises(ta.TahoeError) as e:
        f.predict_accumulate(x, sums)
    assert e.value.status == 7
    with pytest.raises(ta.TahoeError) as e:
        f.predict_host(data)
    assert e.value.status == 7
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all())  # nothing was launched
    f.check()
    f.close()


def test_reserved_multiclass_predict_is_capturable_in_a_hip_graph(env, knobs):
    ta, oracle, torch = env
    C, Tc, D, cols, R = 10, 20, 8, 100, 20_000
    T = C * Tc
    nodes = ta.synth_forest(T, D, cols, seed=97, leaf_prob=0.05)
    f = ta.Forest(nodes, T, D, cols, missing=MISSING, output=ta.OUT_AVG | ta.OUT_SOFTMAX, global_bias=0.1, num_classes=C)
    f.reserve(R)
    x = torch.empty((R, cols), dtype=torch.float32, device="cuda")
    out = torch.zeros((R, C), dtype=torch.float32, device="cuda")
    x.copy_(torch.from_numpy(ta.synth_data(R, cols, seed=98)))
    f.predict(x, out)  # eager first launch of this handle's kernels
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        f.predict(x, out, stream=torch.cuda.current_stream())
    for seed in (99, 100):
        x.copy_(torch.from_numpy(ta.synth_data(R, cols, seed=seed, missing_prob=0.05, missing=MISSING)))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        f.check()
        eager = f.predict(x).cpu().numpy()
        assert np.array_equal(bits(out.cpu().numpy()), bits(eager)), seed
        assert np.allclose(eager.sum(axis=1), 1.0, atol=1e-5)
    f.close()


def test_every_form_was_exercised():
    """The predicts of this file (run in file order) went through every consumer that has a multi-class form."""
    want = {"direct", "rowtile", "qring_region3", "qring_region2", "qring_region_mixed", "qring_region8", "qring_region6",
            "qring_split", "qring_columns", "qring_gx", "qring_wide"}
    assert want <= FORMS, sorted(want - FORMS)
