"""NaN as a missing value (TAHOE_CREATE_NAN_MISSING) on the GPU.  Needs an MI355X.

Every comparison is on float32 bits, against the existing CPU references on the batch with its NaNs replaced by the sentinel
(tests/nan_missing_cases.py says why that is the reference, and checks on the CPU that each test is not vacuous: the forests have
def_left = 0 nodes on the columns that hold NaNs, so "NaN is missing" and "NaN goes left" give other bits).  The plan (strategy,
kernel form, chunk rows) is asserted wherever a test is about one path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nan_missing_cases as nm  # noqa: E402
import test_columns_gpu as tcg  # noqa: E402  (the column layouts)
import test_multiclass_gpu as mcg  # noqa: E402  (CASES, forest_nodes, batch: the smallest shapes that reach each QRING form)
from guarded import Guarded, guarded_input  # noqa: E402
from nan_missing_cases import S, bits, sub  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 127, 129, 193, 385, 1000)
DENSE = ("AUTO", "DIRECT", "ROWTILE", "QRING")  # what a flagged dense or multi-class handle serves
DENSE_UNSERVED = ("TILEBLOCK", "TILERING")
SPARSE = ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK", "QRING")
CAT = ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK")
KNOBS = tcg.KNOBS + ("TAHOE_QUANT_BUCKETS", "TAHOE_QUANT_MULTI", "TAHOE_CSR_FUSED", "TAHOE_SPARSE_QRING")


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


def strat(ta, name):
    return getattr(ta, "STRATEGY_" + name)


def dev(torch, x):
    return torch.from_numpy(np.array(x, order="C")).cuda()  # (a copy: the shared batches are read-only)


def accepted(ta, f, served, unserved=()):
    """Every strategy of `served` is accepted; each of `unserved` fails with status 7 and a message naming the flag"""
    for name in served:
        f.set_strategy(strat(ta, name))
    for name in unserved:
        with pytest.raises(ta.TahoeError) as e:
            f.set_strategy(strat(ta, name))
        assert e.value.status == 7 and "TAHOE_CREATE_NAN_MISSING" in str(e.value), (name, str(e.value))
    f.set_strategy(ta.STRATEGY_AUTO)


def check_rows_and_columns(env, f, x, want, names, layouts=("stride=rows+3", "ptrs"), label=""):
    """predict_raw on the rows and predict_columns in the layouts, under each named strategy, against the reference's bits"""
    ta, _, torch = env
    xd = dev(torch, x)
    for name in names:
        f.set_strategy(strat(ta, name))
        got = f.predict_raw(xd)
        f.check()
        assert np.array_equal(bits(got), bits(want)), (label, name, "rows", x.shape)
        for layout in layouts:
            got = f.predict_columns(tcg.as_layout(torch, x, layout))
            f.check()
            assert np.array_equal(bits(got), bits(want)), (label, name, layout, f.columns_plan(x.shape[0]), x.shape)


# ------------------------------------------------------------------------------------------- the handle kinds, built once
_kinds = {}


def kind(env, name):
    """name -> dict(make(nan_missing, **kw) -> handle, x [1000, cols], want, left, served, unserved): the forests of
    test_columns_gpu.py -- K1-like 500 x depth 8 on 18 features, 120 sparse trees on 64, 60 categorical trees on 32 -- with NaN
    at 1 % beside the sentinel at 3 %, and the references on 1000 rows, computed once and read-only"""
    ta, oracle, _ = env
    if name in _kinds:
        return _kinds[name]
    if name in ("dense", "dense4"):
        T, D, cols, C = 500, 8, 18, 4 if name == "dense4" else 1
        nodes = ta.synth_forest(T, D, cols, seed=11, leaf_prob=0.05)
        x = ta.synth_data(1000, cols, seed=12, missing_prob=0.03, missing=S, nan_prob=0.01)
        want, left, leaf = nm.dense_refs(oracle, nodes, T, D, x, C, leaf=True)
        k = dict(make=lambda nan_missing=True, missing=S, **kw: ta.Forest(nodes, T, D, cols, missing=missing, num_classes=C,
                                                                          nan_missing=nan_missing, **kw),
                 served=DENSE, unserved=DENSE_UNSERVED, nodes=nodes, T=T, D=D, C=C,
                 ref=lambda data, **kw: nm.dense_refs(oracle, nodes, T, D, data, C, **kw))
    elif name in ("sparse", "sparse4"):
        T, cols, C = 120, 64, 4 if name == "sparse4" else 1
        sn, tr = ta.capi.synth_sparse_forest(T, cols, 4, 24, 0.32, 65535, 44)
        x = ta.synth_data(1000, cols, seed=13, missing_prob=0.03, missing=S, nan_prob=0.01)
        want, left, leaf = nm.sparse_refs(oracle, sn, tr, x, C, leaf=True)
        k = dict(make=lambda nan_missing=True, missing=S, **kw: ta.capi.SparseForest(sn, tr, cols, missing=missing, num_classes=C,
                                                                                     nan_missing=nan_missing, **kw),
                 served=SPARSE, unserved=(), sn=sn, tr=tr, T=T, C=C,
                 ref=lambda data, **kw: nm.sparse_refs(oracle, sn, tr, data, C, **kw))
    else:
        assert name == "cat"
        cf = nm.cat_forest(ta)
        cols, T, C = cf["cols"], len(cf["tr"]), 1
        x = nm.cat_batch(ta, cf, 1000, seed=12)
        want, left, leaf = nm.cat_refs(cf, x, leaf=True)
        k = dict(make=lambda nan_missing=True, missing=S, **kw: ta.capi.SparseForest(cf["sn"], cf["tr"], cols, missing=missing,
                                                                                     categories=cf["cats"], members_left=cf["ml"],
                                                                                     nan_missing=nan_missing, **kw),
                 served=CAT, unserved=("QRING",), cf=cf, T=T, C=C, ref=lambda data, **kw: nm.cat_refs(cf, data, **kw))
    nm.first_row_differs(x, want, left, leaf)  # a batch of one row shows the rule too
    for a in (x, want, left, leaf):
        a.setflags(write=False)
    k.update(name=name, cols=cols, x=x, want=want, left=left, leaf=leaf)
    _kinds[name] = k
    return k


KINDS = ("dense", "dense4", "sparse", "sparse4", "cat")


# ----------------------------------------------------------------------------------------------- row counts and strategies
@pytest.mark.parametrize("name", KINDS)
def test_row_counts_every_served_strategy(env, knobs, name):
    ta, oracle, torch = env
    k = kind(env, name)
    nm.not_vacuous(k["want"], k["left"], k["x"], name)
    assert nm.nan_rows(k["x"])[0] and (bits(k["want"][:1]) != bits(k["left"][:1])).any()  # ... in a batch of one row as well
    f = k["make"]()
    if name == "cat":  # QRING is refused on every categorical handle, with its own message
        accepted(ta, f, k["served"])
        with pytest.raises(ta.TahoeError) as e:
            f.set_strategy(ta.STRATEGY_QRING)
        assert e.value.status == 7
    else:
        accepted(ta, f, k["served"], k["unserved"])
    for rows in ROWS:
        f.set_strategy(ta.STRATEGY_AUTO)
        assert f.get_strategy(rows) in [strat(ta, n) for n in k["served"] if n != "AUTO"]  # AUTO plans a served strategy
        check_rows_and_columns(env, f, k["x"][:rows], k["want"][:rows], k["served"], label=f"{name}, rows {rows}")
    f.close()


@pytest.mark.parametrize("name", KINDS)
def test_a_handle_without_the_flag_is_untouched(env, knobs, name):
    """The same forest and batch: NaN goes left, under every strategy the handle has ever served"""
    ta, oracle, torch = env
    k = kind(env, name)
    f = k["make"](nan_missing=False)
    names = tcg.strategies(ta, f)
    assert set(names) >= set(k["served"]) and (name != "dense" or set(names) == set(tcg.ALL))
    for rows in (1, 65, 385, 1000):
        check_rows_and_columns(env, f, k["x"][:rows], k["left"][:rows], names, layouts=("ptrs",), label=f"{name} without the flag")
    f.close()


def test_a_nan_sentinel_without_the_flag_never_takes_a_default_branch(env, knobs):
    ta, oracle, torch = env
    k = kind(env, "dense")
    x = k["x"][:385]
    never = oracle.predict(k["nodes"], k["T"], k["D"], x, float("nan"), threads=4)[0]  # no value is missing, NaN goes left
    nan_only = oracle.predict(k["nodes"], k["T"], k["D"], sub(x, -777.0), -777.0, threads=4)[0]  # the sentinel -999 is a number
    assert (bits(never) != bits(nan_only)).any() and (bits(never) != bits(k["left"][:385])).any()
    f = k["make"](nan_missing=False, missing=float("nan"))
    check_rows_and_columns(env, f, x, never, tcg.strategies(ta, f), layouts=("ptrs",), label="missing = NaN, no flag")
    f.close()
    f = k["make"](nan_missing=True, missing=float("nan"))  # with the flag: "NaN only"
    check_rows_and_columns(env, f, x, nan_only, DENSE, layouts=("ptrs",), label="missing = NaN, flag")
    f.close()


# -------------------------------------------------------------------------------------------------------------- QRING forms
QRING_CASES = [c for c in mcg.CASES if c[8] is not None and c[8].startswith("qring")]


@pytest.mark.parametrize("case", QRING_CASES, ids=[c[0] for c in QRING_CASES])
def test_every_qring_form(env, knobs, case):
    """test_multiclass_gpu.py's table (the smallest shape that reaches each form), as one class, on a flagged handle: the plan
    asserted, rows straddling the form's tile, from rows and from columns"""
    ta, oracle, torch = env
    name, C, Tc, D, cols, gen, env_knobs, _, form = case
    for key, v in env_knobs.items():
        knobs.setenv(key, v)
    if form not in ("qring_split", "qring_region_mixed"):
        knobs.setenv("TAHOE_QRING_SLICES", "1")  # small batches stay in the form's own tiles
    T = C * Tc
    nodes = mcg.forest_nodes(ta, gen, T, D, cols, seed=100 + len(name) + cols)
    f = ta.Forest(nodes, T, D, cols, missing=S, nan_missing=True)
    f.set_strategy(ta.STRATEGY_QRING)
    t = f.info().qring_tile_rows
    t = t if t >= 2 else 128
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if form == "qring_region_mixed":  # by definition whole waves of 192-row tiles plus a remainder of 128-row tiles
        counts = [cus * 192 + e for e in (127, 129)]
    else:
        counts = sorted({t - 1, t + 1, 127, 129, 2 * t + 1})
    data = mcg.batch(ta, gen, max(counts), cols, seed=200 + cols)
    want, left = nm.dense_refs(oracle, nodes, T, D, data)
    for rows in counts:
        nm.not_vacuous(want[:rows], left[:rows], data[:rows], f"{form}, rows {rows}")
        assert f.kernel_form(rows) == form and f.columns_plan(rows) == (form, 0), (rows, f.kernel_form(rows), f.columns_plan(rows))
        check_rows_and_columns(env, f, data[:rows], want[:rows], ("QRING",), label=f"{form}, rows {rows}")
    f.close()


# ----------------------------------------------------------------------------------------------------- the quantise kernels
# (name, num_cols, knobs): which of the six kernels quantize_build_tables / quantize_launch pick for small tables --
# 16 features per workgroup where num_cols % 16 == 0, 8 where % 8 == 0, else the bucketed pair kernel on an even num_cols, the
# search-tree pair kernel without buckets, one feature per workgroup on an odd num_cols
QUANT = [("multi16", 16, {}), ("multi8", 24, {}), ("bucket_pair", 18, {}), ("pair", 18, {"TAHOE_QUANT_BUCKETS": "0"}),
         ("pair_of_16", 16, {"TAHOE_QUANT_BUCKETS": "0", "TAHOE_QUANT_MULTI": "0"}), ("single", 17, {})]


@pytest.mark.parametrize("case", QUANT, ids=[c[0] for c in QUANT])
def test_nan_in_every_feature_slot_of_the_quantise_kernels(env, knobs, case):
    """NaNs only in odd columns, only in even columns, then in one column at a time; no sentinel anywhere, so the NaNs are the
    only missing values: a kernel that tests one of its features only, or codes the NaN without raising the chunk's flag, gives
    other bits.  Trees c and c + cols split on column c at their roots, with def_left = 0 and 1: every column's NaNs move
    rows, and a NaN's code read as a number would go the wrong way in the second."""
    ta, oracle, torch = env
    name, cols, env_knobs = case
    for key, v in env_knobs.items():
        knobs.setenv(key, v)
    T, D, rows = 2 * cols, 4, 700  # (two quantise chunks of 512 rows)
    nodes = nm.hand_forest(ta, T, D, cols, seed=cols)
    f = ta.Forest(nodes, T, D, cols, missing=S, nan_missing=True)
    f.set_strategy(ta.STRATEGY_QRING)
    rng = np.random.default_rng(cols)
    base = rng.uniform(-1, 1, (rows, cols)).astype(np.float32)
    patterns = [("odd", list(range(1, cols, 2))), ("even", list(range(0, cols, 2)))] + [(f"column {c}", [c]) for c in range(cols)]
    for label, where in patterns:
        x = base.copy()
        mask = np.zeros(x.shape, bool)
        mask[:, where] = rng.random((rows, len(where))) < 0.05
        x[mask] = np.nan
        x = nm.with_nan_patterns(x)
        want, left = nm.dense_refs(oracle, nodes, T, D, x, threads=1)
        differ = nm.not_vacuous(want, left, x, f"{name}, {label}")
        assert np.array_equal(differ, nm.nan_rows(x)), (name, label)  # every row with a NaN shows it
        check_rows_and_columns(env, f, x, want, ("QRING",), layouts=("ptrs",), label=f"{name}, NaN in {label}")
    f.close()


def test_chunk_flag_raised_by_a_single_nan(env, knobs):
    """test_missing_flag_of_the_right_quantise_chunk's construction: every root splits on the last column, with def_left = 0 in
    the even trees (there the test is not vacuous) and 1 in the odd ones (there the missing code as a number goes wrong); the
    only missing value of the batch is one NaN -- at row 511, at row 512 column 0, at row 1023 of 2100 rows -- and no sentinel
    appears.  TAHOE_QRING_TOP24 at its default: a quantise pass that codes the NaN but leaves the chunk's flag down sends the
    tile through a form without the missing rule, where the code 0xFFFF is the largest number."""
    ta, oracle, torch = env
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tahoe_amd", "csrc", "qring_internal.h")).read()
    assert "constexpr int kQuantMinRowsPerBlock = 512;" in src
    assert "TAHOE_QRING_TOP24" not in os.environ
    T, D, cols, rows = 24, 4, 8, 1100
    nodes = nm.hand_forest(ta, T, D, cols, seed=5, root_col=cols - 1)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (rows, cols)).astype(np.float32)
    f = ta.Forest(nodes, T, D, cols, missing=S, nan_missing=True)
    f.set_strategy(ta.STRATEGY_QRING)
    assert f.columns_plan(rows)[1] == 0

    def run(batch, at):
        assert int(np.isnan(batch).sum()) == 1 and not (batch == np.float32(S)).any()
        want, left = nm.dense_refs(oracle, nodes, T, D, batch, threads=1)
        assert np.array_equal(np.flatnonzero(bits(want) != bits(left)), [at])  # the rule matters, there only
        check_rows_and_columns(env, f, batch, want, ("QRING",), label=f"one NaN in row {at}")

    x1 = x.copy()
    x1[511, cols - 1] = np.nan
    run(x1, 511)
    x2 = x.copy()
    x2[512, 0] = np.nan  # the first row of the second chunk, first column: some tree splits on column 0 below its root
    want, left = nm.dense_refs(oracle, nodes, T, D, x2, threads=1)
    assert np.array_equal(np.flatnonzero(bits(want) != bits(left)), [512])
    check_rows_and_columns(env, f, x2, want, ("QRING",), label="one NaN in row 512")
    x3 = np.concatenate([x, x])[:2100]  # (2100 rows of 8 columns: two 1024-row chunks and a tail)
    x3[1023, cols - 1] = np.nan
    run(x3, 1023)
    f.close()


# ---------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("m", [-999.0, 0.5, 0.0, float("nan"), float("inf"), float("-inf")], ids=lambda m: f"missing={m}")
def test_the_definition(env, knobs, m):
    """missing <=> isnan(x) || fabsf(x - m) <= 1e-6f on +-0, +-inf, subnormals, both sides of the band's edges and four NaN bit
    patterns, for finite, NaN and infinite sentinels, on a dense handle and on the sparse handle converted from it"""
    ta, oracle, torch = env
    T, D, cols = 40, 5, 8
    nodes = nm.hand_forest(ta, T, D, cols, seed=21, thr=(-1.0, 1.0))
    half = nodes.reshape(T, -1)[::2]
    half["bits"] |= np.int32(1 << 30)  # def_left = 1 in every second tree: both defaults are walked
    x = nm.definition_batch(m, cols)
    want, flagless = nm.definition_refs(oracle, nodes, T, D, x, m)
    nm.not_vacuous(want, flagless, x, f"missing = {m}")
    if np.isinf(m):  # an infinite x under an infinite sentinel is an ordinary value: the reference does not treat it as missing
        row = np.zeros((1, cols), np.float32)
        row[0, :] = np.float32(m)
        big = np.full((1, cols), np.float32(3e38) * np.sign(np.float32(m)), np.float32)
        r_inf = nm.definition_refs(oracle, nodes, T, D, row, m)[0]
        assert np.array_equal(bits(r_inf), bits(oracle.predict(nodes, T, D, big, -777.0)[0]))  # as the largest number
        assert not np.array_equal(bits(r_inf), bits(oracle.predict(nodes, T, D, np.full((1, cols), -777.0, np.float32), -777.0)[0]))
        x = np.concatenate([x, row])
        want = np.concatenate([want, r_inf])
    f = ta.Forest(nodes, T, D, cols, missing=m, nan_missing=True)
    accepted(ta, f, DENSE, DENSE_UNSERVED)
    check_rows_and_columns(env, f, x, want, DENSE, label=f"dense, missing = {m}")
    f.close()
    sn, tr = ta.capi.dense_to_sparse(nodes, T, D)  # the converted forest, created with the flag, gives the dense handle's bits
    f = ta.capi.SparseForest(sn, tr, cols, missing=m, nan_missing=True)
    accepted(ta, f, SPARSE)
    check_rows_and_columns(env, f, x, want, SPARSE, label=f"converted to sparse, missing = {m}")
    f.close()


def test_nan_thresholds_in_the_model(env, knobs):
    """x >= NaN is never true, and a missing x still takes the default branch there -- a NaN x now included"""
    ta, oracle, torch = env
    T, D, cols = 30, 5, 8
    nodes = nm.hand_forest(ta, T, D, cols, seed=31)
    inner = np.flatnonzero(nodes["bits"] >= 0)
    nodes["val"][inner[::5]] = np.nan
    x = nm.definition_batch(S, cols, rows=300, seed=32)
    want, left = nm.dense_refs(oracle, nodes, T, D, x)
    nm.not_vacuous(want, left, x, "NaN thresholds")
    f = ta.Forest(nodes, T, D, cols, missing=S, nan_missing=True)
    check_rows_and_columns(env, f, x, want, DENSE, label="NaN thresholds")
    f.close()


def test_a_forest_without_trees_and_a_depth_0_forest(env, knobs):
    ta, oracle, torch = env
    x = nm.definition_batch(S, 4, rows=70, seed=33)
    f = ta.Forest(np.empty(0, dtype=ta.NODE_DTYPE), 0, 3, 4, missing=S, nan_missing=True, output=ta.OUT_SIGMOID, global_bias=0.5)
    plain = ta.Forest(np.empty(0, dtype=ta.NODE_DTYPE), 0, 3, 4, missing=S, output=ta.OUT_SIGMOID, global_bias=0.5)
    names = tcg.strategies(ta, f)
    assert "DIRECT" in names and "AUTO" in names and not set(names) & set(DENSE_UNSERVED)
    for name in names:
        f.set_strategy(strat(ta, name))
        assert np.array_equal(bits(f.predict(dev(torch, x))), bits(plain.predict(dev(torch, x))))
        assert np.array_equal(bits(f.predict_raw(dev(torch, x))), bits(np.zeros(70, np.float32)))
    f.close()
    plain.close()
    T = 7
    leaves = ta.capi.encode_nodes(np.zeros(T), np.arange(T) + 0.25, np.zeros(T), np.ones(T), np.ones(T))
    want = oracle.predict(leaves, T, 0, sub(x), S)[0]
    f = ta.Forest(leaves, T, 0, 4, missing=S, nan_missing=True)
    names = tcg.strategies(ta, f)
    assert "DIRECT" in names and "AUTO" in names and not set(names) & set(DENSE_UNSERVED)
    check_rows_and_columns(env, f, x, want, names, label="depth 0")
    f.close()


# ------------------------------------------------------------------------------------------------------------- categorical
def test_nan_at_a_categorical_split_takes_the_default_branch(env, knobs):
    """Four stumps whose roots are category sets on column 0, one per (def_left, members_left) pair; the rows hold a NaN, the
    sentinel, a member and a non-member.  With the flag the NaN goes where the sentinel goes; without it, it is a non-member."""
    ta, oracle, torch = env
    import categorical_ref

    sn = np.zeros(12, ta.capi.SPARSE_NODE_DTYPE)
    tr = np.arange(0, 12, 3).astype(np.int32)
    cats, ml = {}, set()
    for t, (def_left, members_left) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        sn["bits"][3 * t] = (def_left << 30)  # fid 0
        sn["left_idx"][3 * t] = 1
        sn["bits"][[3 * t + 1, 3 * t + 2]] = np.int32(-(1 << 31))
        sn["val"][[3 * t + 1, 3 * t + 2]] = [10.0 ** t, -(10.0 ** t) / 4]  # left leaf, right leaf: every path has its own sum
        cats[3 * t] = [2, 5]
        if members_left:
            ml.add(3 * t)
    x = np.array([[np.nan, 0.0], [S, 0.0], [5.0, 0.0], [3.0, 0.0], [-np.nan, 1.0]], np.float32)
    _, (node, offset, words, mla) = ta.capi.pack_categorical(cats, ml)
    want = np.ascontiguousarray(categorical_ref.predict(sn, tr, sub(x), S, node, offset, words, mla)[0], np.float32)
    non_member = np.ascontiguousarray(categorical_ref.predict(sn, tr, x, S, node, offset, words, mla)[0], np.float32)
    # on the CPU: the NaN rows of the reference are the sentinel's row, which takes each stump's default branch ...
    default = np.float32(0)
    for t, def_left in enumerate((0, 0, 1, 1)):
        default = np.float32(default + np.float32(10.0 ** t if def_left else -(10.0 ** t) / 4))
    assert want[0] == want[1] == want[4] == default
    # ... and as a non-member it goes left where members go right, right where members go left
    assert non_member[0] == non_member[3] and non_member[0] != want[0] and non_member[1] == want[1]
    for nan_missing, ref in ((True, want), (False, non_member)):
        f = ta.capi.SparseForest(sn, tr, 2, missing=S, categories=cats, members_left=ml, nan_missing=nan_missing)
        check_rows_and_columns(env, f, x, ref, CAT, label=f"nan_missing={nan_missing}")
        f.close()


# --------------------------------------------------------------------------------------- every other call, per handle kind
@pytest.mark.parametrize("name", ["dense", "dense4", "sparse", "cat"])
def test_leaf_indices_accumulate_host_and_staged(env, knobs, name):
    ta, oracle, torch = env
    k = kind(env, name)
    rows = 385
    x, want, leaf_want = k["x"][:rows], k["want"][:rows], k["leaf"][:rows]
    xd = dev(torch, x)
    f = k["make"]()
    stages = (3, 40, k["T"] // k["C"])
    for sname in k["served"]:
        f.set_strategy(strat(ta, sname))
        leaf, sums = f.predict_leaf_idx(xd)
        f.check()
        assert np.array_equal(bits(leaf), leaf_want) and np.array_equal(bits(sums), bits(want)), (name, sname, "leaf_idx")
        assert np.array_equal(bits(f.predict(xd)), bits(want)), (name, sname, "predict")
        if k["C"] == 1:
            start = np.linspace(-3, 3, rows).astype(np.float32)
            if name == "dense":
                cont = oracle.predict_continue(k["nodes"], k["T"], k["D"], sub(x), S, start.copy())
            elif name == "sparse":
                import categorical_ref

                cont = categorical_ref.predict(k["sn"], k["tr"], sub(x), S, init=start)[0]
            else:
                cont = nm.cat_refs(k["cf"], x, init=start)[0]
            got = f.predict_accumulate(xd, dev(torch, start))
            f.check()
            assert np.array_equal(bits(got), bits(cont)), (name, sname, "accumulate")
            assert np.array_equal(bits(f.predict_host(np.ascontiguousarray(x))), bits(want)), (name, sname, "host")
    # three stages, each against the truncated forest's reference; every strategy that has a staged form
    f.set_stages(stages)
    for sname in k["served"]:
        f.set_strategy(strat(ta, sname))
        if f.staged_strategy(rows) == 0:
            assert sname == "QRING"
            continue
        got = f.predict_staged(xd).cpu().numpy()
        f.check()
        for s, n in enumerate(stages):
            if name.startswith("dense"):
                per = k["nodes"].size // k["T"]
                ref = nm.dense_refs(oracle, k["nodes"][: n * k["C"] * per], n * k["C"], k["D"], x, k["C"])[0]
            elif name == "sparse":
                ref = nm.sparse_refs(oracle, k["sn"], k["tr"][:n], x)[0]
            else:
                ref = nm.cat_refs(k["cf"], x, trees=k["cf"]["tr"][:n])[0]
            assert np.array_equal(bits(got[:, s]), bits(ref)), (name, sname, "stage", s)
    f.close()


def csr_of(x, seed):
    """(indptr, indices, values, the dense matrix they stand for): half of the entries absent; the stored ones keep their NaNs
    and sentinels"""
    keep = np.random.default_rng(seed).random(x.shape) < 0.5
    indptr = np.zeros(x.shape[0] + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    dense = np.where(keep, x, np.float32(S)).astype(np.float32)
    values = x[keep]
    assert np.isnan(values).any() and (values == np.float32(S)).any()
    return indptr, np.nonzero(keep)[1].astype(np.int32), values, dense


@pytest.mark.parametrize("name", ["dense", "dense4", "sparse", "cat"])
def test_predict_csr_fused_and_chunked(env, knobs, name):
    """Stored NaNs, stored sentinels and absent entries are all missing"""
    ta, oracle, torch = env
    k = kind(env, name)
    rows = 385
    indptr, indices, values, dense = csr_of(k["x"][:rows], seed=5)
    want, left = k["ref"](dense)
    nm.not_vacuous(want, left, dense, name + " from CSR")
    args = (dev(torch, indptr), dev(torch, indices), dev(torch, values))
    f = k["make"]()
    fused = [n for n in ("ROWTILE", "TILEBLOCK") if n in k["served"]]
    for sname in fused:
        f.set_strategy(strat(ta, sname))
        form, chunk = f.csr_plan(rows, values.size)
        assert chunk == 0 and form.startswith("csr_"), (name, sname, form, chunk)
        assert np.array_equal(bits(f.predict_csr(*args)), bits(want)), (name, sname)
        f.check()
    f.close()
    knobs.setenv("TAHOE_CSR_CHUNK_MB", "1")  # read at create; with 64 columns or fewer: chunks of at least 4096 rows
    knobs.setenv("TAHOE_CSR_FUSED", "0")
    f = k["make"]()
    for sname in [n for n in k["served"] if n not in fused]:
        f.set_strategy(strat(ta, sname))
        form, chunk = f.csr_plan(rows, values.size)
        assert chunk > 0 and not form.startswith("csr_"), (name, sname, form, chunk)
        assert np.array_equal(bits(f.predict_csr(*args)), bits(want)), (name, sname, form)
        f.check()
    f.close()


def test_predict_csr_in_several_chunks(env, knobs):
    """TAHOE_CSR_CHUNK_MB=1 on 300 columns: 768 rows per chunk; the chunked paths of CSR and column input land on served forms"""
    ta, oracle, torch = env
    T, D, cols, rows = 30, 6, 300, 2 * 768 + 5
    nodes = nm.hand_forest(ta, T, D, cols, seed=8)
    x = ta.synth_data(rows, cols, seed=9, missing_prob=0.03, missing=S, nan_prob=0.01)
    indptr, indices, values, dense = csr_of(x, seed=6)
    want, left = nm.dense_refs(oracle, nodes, T, D, dense)
    nm.not_vacuous(want, left, dense, "chunks")
    knobs.setenv("TAHOE_CSR_CHUNK_MB", "1")
    knobs.setenv("TAHOE_CSR_FUSED", "0")
    knobs.setenv("TAHOE_COLUMNS_FUSED", "0")
    f = ta.Forest(nodes, T, D, cols, missing=S, nan_missing=True)
    accepted(ta, f, DENSE, DENSE_UNSERVED)
    for sname in ("AUTO", "DIRECT", "QRING"):
        f.set_strategy(strat(ta, sname))
        form, chunk = f.csr_plan(rows, values.size)
        assert chunk == 768 and (form.startswith("qring") or form in ("direct", "rowtile")), (sname, form, chunk)
        assert np.array_equal(bits(f.predict_csr(dev(torch, indptr), dev(torch, indices), dev(torch, values))), bits(want)), sname
        f.check()
    f.set_strategy(ta.STRATEGY_AUTO)
    form, chunk = f.columns_plan(rows)
    assert chunk == 768 and (form.startswith("qring") or form in ("direct", "rowtile")), (form, chunk)
    assert np.array_equal(bits(f.predict_columns(tcg.as_layout(torch, dense, "ptrs"))), bits(want))
    f.close()


@pytest.mark.parametrize("name", ["dense", "sparse", "cat"])
def test_predict_columns_paths(env, knobs, name):
    """The fused quantise pass, the fused tile loaders and the chunks, in the strided and the pointer-table layout"""
    ta, oracle, torch = env
    k = kind(env, name)
    rows = 385
    x, want = k["x"][:rows], k["want"][:rows]
    f = k["make"]()
    plans = {}
    for sname in k["served"]:
        f.set_strategy(strat(ta, sname))
        plans[sname] = f.columns_plan(rows)
    assert plans["ROWTILE"] == ("columns_rowtile" if name == "dense" else "columns_sparse_rowtile", 0), plans
    assert plans["DIRECT"][1] > 0 and plans["DIRECT"][0] in ("direct", "sparse_direct"), plans
    if "QRING" in plans:
        assert plans["QRING"][1] == 0 and "qring" in plans["QRING"][0], plans
    if "TILEBLOCK" in plans:
        assert plans["TILEBLOCK"] == ("columns_sparse_top", 0), plans
    check_rows_and_columns(env, f, x, want, k["served"], layouts=tcg.LAYOUTS, label=name)
    f.close()


def test_probability_relayout_beside_the_flag(env, knobs):
    ta, oracle, torch = env
    k = kind(env, "dense")
    nodes = ta.capi.set_probability_weights(k["nodes"].copy(), k["T"], k["D"])
    f = ta.Forest(nodes, k["T"], k["D"], k["cols"], missing=S, nan_missing=True, relayout=True)
    assert f.info().relayout == 1 and f.info().relayout_swaps > 0
    accepted(ta, f, DENSE, DENSE_UNSERVED)
    xd = dev(torch, k["x"])
    for sname in DENSE:
        f.set_strategy(strat(ta, sname))
        leaf, sums = f.predict_leaf_idx(xd)
        assert np.array_equal(bits(sums), bits(k["want"])) and np.array_equal(bits(leaf), k["leaf"]), sname
        assert np.array_equal(bits(f.predict_raw(xd)), bits(k["want"])), sname
    f.close()


@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_a_captured_call_replays_on_inputs_rewritten_in_place(env, knobs, name):
    """The rule allocates nothing: after reserve a call is captured, and replays on batches whose NaNs sit elsewhere"""
    ta, oracle, torch = env
    k = kind(env, name)
    rows = 1000
    x1 = np.ascontiguousarray(k["x"])
    x2 = np.ascontiguousarray(k["x"][::-1])
    w1, w2 = k["want"], np.ascontiguousarray(k["want"][::-1])
    f = k["make"]()
    for sname in k["served"]:
        f.set_strategy(strat(ta, sname))
        f.reserve(rows)
        xd = dev(torch, x1)
        out = torch.zeros(f._out_shape(rows), dtype=torch.float32, device="cuda")
        f.predict_raw(xd, out)  # eager first launch of this form's kernels
        torch.cuda.synchronize()
        before = f.info().device_bytes
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        with torch.cuda.graph(g, stream=side):
            f.predict_raw(xd, out, stream=side)
        for src, w in ((x2, w2), (x1, w1)):
            xd.copy_(torch.from_numpy(src))
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            f.check()
            assert np.array_equal(bits(out), bits(w)), (name, sname)
        assert f.info().device_bytes == before, (name, sname)
    f.close()


# ------------------------------------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_guard_bands_around_every_entry_point(env, knobs, name):
    """One flagged call per entry point with its outputs and inputs inside tests/guarded.py buffers"""
    ta, oracle, torch = env
    k = kind(env, name)
    rows, T = 193, k["T"]
    x, want, leaf_want = k["x"][:rows], k["want"][:rows], k["leaf"][:rows]
    f = k["make"]()
    xin = guarded_input(torch, x, torch.float32, device="cuda")

    def out_buf(shape=(rows,), dtype=None):
        return Guarded(torch, shape, dtype or torch.float32, device="cuda")

    o = out_buf()
    f.predict(xin.view, o.view)
    assert np.array_equal(bits(o.check("predict")), bits(want))
    o = out_buf()
    f.predict_raw(xin.view, o.view)
    assert np.array_equal(bits(o.check("predict_raw")), bits(want))
    lo, so = out_buf((rows, T), torch.int32), out_buf()
    f.predict_leaf_idx(xin.view, leaf=lo.view, sums=so.view)
    assert np.array_equal(bits(lo.check("leaf")), leaf_want) and np.array_equal(bits(so.check("leaf sums")), bits(want))
    acc = out_buf().load(np.zeros(rows, np.float32))
    f.predict_accumulate(xin.view, acc.view)
    assert np.array_equal(bits(acc.check("accumulate")), bits(want))
    f.set_stages((2, T))
    st = out_buf((rows, 2))
    f.predict_staged(xin.view, st.view)
    assert np.array_equal(bits(st.check("staged")[:, 1]), bits(want))
    f.check()
    xin.check_unchanged("the row-major batch")
    # columns: one guarded buffer per column
    cols_in = [guarded_input(torch, np.ascontiguousarray(x[:, c]), torch.float32, device="cuda") for c in range(k["cols"])]
    o = out_buf()
    f.predict_columns([c.view for c in cols_in], out=o.view)
    assert np.array_equal(bits(o.check("predict_columns")), bits(want))
    for c in cols_in:
        c.check_unchanged("a column")
    # CSR: stored NaNs and sentinels, half of the entries absent
    indptr, indices, values, dense = csr_of(x, seed=7)
    ip, ix, vals = (guarded_input(torch, a, t, device="cuda") for a, t in ((indptr, torch.int64), (indices, torch.int32),
                                                                          (values, torch.float32)))
    o = out_buf()
    f.predict_csr(ip.view, ix.view, vals.view, out=o.view)
    f.check()
    assert np.array_equal(bits(o.check("predict_csr")), bits(k["ref"](dense)[0]))
    for g, what in ((ip, "indptr"), (ix, "indices"), (vals, "values")):
        g.check_unchanged(what)
    # the host call: numpy buffers
    hin = guarded_input(np, x, "float32")
    ho = Guarded(np, (rows,), "float32")
    f.predict_host(hin.view, ho.view)
    assert np.array_equal(bits(ho.check("predict_host")), bits(want))
    hin.check_unchanged("the host batch")
    f.close()
