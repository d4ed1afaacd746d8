"""Column-major batches on the GPU (predict_columns: tahoe_forest_predict_columns and tahoe_forest_predict_column_ptrs; DESIGN.md
section 37).  Every comparison is torch.equal-strength on the float32 bits, against predict of the same handle on the row-major
matrix of the same values, and once per handle kind against a reference that is not the library (the CPU oracle, categorical_ref,
the numpy walks of the native handles).  The plan (kernel form, rows per chunk) is asserted wherever a test is about one path,
so a shape that stops reaching its path fails.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import test_multiclass_gpu as mcg  # noqa: E402  (CASES, KNOBS, forest_nodes, batch: the smallest shapes that reach each QRING form)
import vector_ref as vr  # noqa: E402
from guarded import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
ALL = ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK", "TILERING", "QRING")
SPARSE = ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK", "QRING")
TILE_FORMS = ("columns_rowtile", "columns_sparse_rowtile", "columns_sparse_top")
LAYOUTS = ("stride=rows", "stride=rows+3", "stride=round4", "ptrs")
KNOBS = mcg.KNOBS + ("TAHOE_QRING_NARROW128", "TAHOE_QRING_TOP24", "TAHOE_COLUMNS_FUSED", "TAHOE_CSR_CHUNK_MB")


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


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t).view(np.uint32)


def strided(torch, x, stride, gap=np.float32(12345.0), offset=1):
    """x [rows, cols] as a column-major view into one flat buffer with that column stride; the gaps hold `gap`.  The buffer
    starts `offset` floats into its allocation, so with an odd stride no column is 16-byte aligned."""
    rows, cols = x.shape
    assert stride >= rows
    flat = np.full(offset + max(cols * stride, 1), gap, dtype=np.float32)
    for c in range(cols):
        flat[offset + c * stride: offset + c * stride + rows] = x[:, c]
    dev = torch.from_numpy(flat).cuda()
    return torch.as_strided(dev, (rows, cols), (1, stride), storage_offset=offset)


def column_list(torch, x, seed=0):
    """One allocation per column, made in shuffled order, each with its own odd slack in front"""
    rows, cols = x.shape
    out = [None] * cols
    for c in np.random.default_rng(seed).permutation(cols):
        pad = 1 + 2 * int(c % 3)
        buf = torch.empty(rows + pad, dtype=torch.float32, device="cuda")
        buf[pad:] = torch.from_numpy(np.ascontiguousarray(x[:, c]))
        out[c] = buf[pad:]
    return out


def as_layout(torch, x, layout):
    rows = x.shape[0]
    if layout == "ptrs":
        return column_list(torch, x, seed=rows)
    stride = {"stride=rows": rows, "stride=rows+3": rows + 3, "stride=round4": (rows + 3) // 4 * 4}[layout]
    return strided(torch, x, stride, offset=1 if layout != "stride=round4" else 0)


def strategies(ta, f, names=ALL):
    ok = []
    for name in names:
        try:
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            ok.append(name)
        except ta.TahoeError as e:
            assert e.status == 7, str(e)
    return ok


def same_bits(env, f, x, names, layouts=LAYOUTS, label="", want_raw=None):
    """predict_columns in every layout against predict on the row-major matrix under each named strategy (and against
    want_raw, a reference's bits, where given); returns the plan per strategy."""
    ta, _, torch = env
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    plans = {}
    for name in names:
        f.set_strategy(getattr(ta, "STRATEGY_" + name))
        want = f.predict(xd)
        plans[name] = f.columns_plan(x.shape[0])
        if want_raw is not None:
            assert np.array_equal(bits(want), bits(want_raw)), (label, name, "predict != reference")
        for layout in layouts:
            got = f.predict_columns(as_layout(torch, x, layout))
            f.check()
            assert got.shape == want.shape and got.dtype == want.dtype
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (label, name, layout, plans[name], x.shape)
    return plans


# ------------------------------------------------------------------------------------------------------------ dense handles
_k1 = {}


def k1_like(env):
    """500 trees of depth 8 on 18 features, 1000 rows and the oracle's sums: computed once, read-only"""
    ta, oracle, _ = env
    if not _k1:
        T, D, cols = 500, 8, 18
        nodes = ta.synth_forest(T, D, cols, seed=11, leaf_prob=0.05)
        x = ta.synth_data(1000, cols, seed=12, missing_prob=0.03, missing=MISSING, nan_prob=0.01)
        _k1.update(T=T, D=D, cols=cols, nodes=nodes, x=x, want=oracle.predict(nodes, T, D, x, MISSING, threads=8)[0])
    return _k1


def check_dense_plans(plans):
    assert plans["ROWTILE"] == ("columns_rowtile", 0), plans
    assert plans["QRING"][0].startswith("qring_") and plans["QRING"][1] == 0, plans
    for name in ("DIRECT", "TILEBLOCK", "TILERING"):
        if name in plans:
            assert plans[name][1] > 0 and plans[name][0] not in TILE_FORMS, plans
    assert plans["DIRECT"][0] == "direct"


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 127, 129, 193, 385, 1000])
def test_row_counts_every_strategy_both_entry_points(env, knobs, rows):
    ta, _, torch = env
    k = k1_like(env)
    f = ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING)
    names = strategies(ta, f)
    assert set(names) == set(ALL), names
    plans = same_bits(env, f, k["x"][:rows], names, want_raw=k["want"][:rows])  # raw output: the oracle's bits too
    check_dense_plans(plans)
    auto = f.get_strategy(rows)
    assert plans["AUTO"] == plans[{ta.STRATEGY_QRING: "QRING", ta.STRATEGY_ROWTILE: "ROWTILE", ta.STRATEGY_TILERING: "TILERING",
                                   ta.STRATEGY_TILEBLOCK: "TILEBLOCK", ta.STRATEGY_DIRECT: "DIRECT"}[auto]]  # AUTO's own form, fed from columns
    f.close()


QRING_CASES = [c for c in mcg.CASES if c[8] is not None and c[8].startswith("qring")]


@pytest.mark.parametrize("case", QRING_CASES, ids=[c[0] for c in QRING_CASES])
def test_every_qring_form_reads_columns(env, knobs, case):
    """test_multiclass_gpu.py's table (the smallest shape that reaches each form), as one class; rows straddle the form's tile"""
    ta, oracle, torch = env
    name, C, Tc, D, cols, gen, env_knobs, _, form = case
    for key, v in env_knobs.items():
        knobs.setenv(key, v)
    if form not in ("qring_split", "qring_region_mixed"):
        knobs.setenv("TAHOE_QRING_SLICES", "1")  # small batches stay in the form's own tiles
    T = C * Tc
    nodes = mcg.forest_nodes(ta, gen, T, D, cols, seed=100 + len(name) + cols)
    f = ta.Forest(nodes, T, D, cols, missing=MISSING)
    f.set_strategy(ta.STRATEGY_QRING)
    t = f.info().qring_tile_rows
    t = t if t >= 2 else 128
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if form == "qring_region_mixed":  # by definition whole waves of 192-row tiles plus a remainder of 128-row tiles
        counts = [cus * 192 + e for e in (127, 129)]
    else:
        counts = sorted({t - 1, t + 1, 127, 129, 2 * t + 1})
    data = mcg.batch(ta, gen, max(counts), cols, seed=200 + cols)
    want = oracle.predict(nodes, T, D, data, MISSING, threads=8)[0] if form == "qring_region8" else None
    for rows in counts:
        assert f.columns_plan(rows) == (form, 0), (rows, f.columns_plan(rows))
        same_bits(env, f, data[:rows], ("QRING",), layouts=("stride=rows", "ptrs") if rows > 2000 else LAYOUTS,
                  label=f"{form}, rows {rows}", want_raw=None if want is None else want[:rows])
    f.close()


def test_missing_flag_of_the_right_quantise_chunk(env, knobs):
    """Small tables put a quantise workgroup on kQuantMinRowsPerBlock = 512 rows (quantize_launch; the constant is read from the
    source here, so a change of it fails this test instead of moving the case off the chunk edge).  The only missing value of
    the batch sits in the last row of the first chunk and the last column: the walk of that tile, and only it, must apply the
    rule.  A second batch puts it at row 1023 as well, the edge of a 1024-row chunk and of the second 512-row one."""
    ta, oracle, torch = env
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tahoe_amd", "csrc", "qring_internal.h")).read()
    assert "constexpr int kQuantMinRowsPerBlock = 512;" in src
    T, D, cols, rows = 24, 4, 8, 1100
    rng = np.random.default_rng(5)
    fid = np.tile(np.array([cols - 1] + list(rng.integers(0, cols, 2 ** D - 2)) + [0] * 2 ** D), T)  # every root splits on the last column
    per = 2 ** (D + 1) - 1
    is_leaf = np.tile(np.arange(per) >= 2 ** D - 1, T)
    val = np.where(is_leaf, rng.uniform(-1, 1, T * per), rng.uniform(-0.5, 0.5, T * per)).astype(np.float32)
    nodes = ta.capi.encode_nodes(fid, val, np.zeros(T * per), np.ones(T * per), is_leaf)  # missing goes right, -999 as a number left
    x = rng.uniform(-1, 1, (rows, cols)).astype(np.float32)
    x[511, cols - 1] = MISSING
    want = oracle.predict(nodes, T, D, x, MISSING, threads=1)[0]
    as_number = oracle.predict(nodes, T, D, x, 12345.0, threads=1)[0]
    assert want[511] != as_number[511] and np.array_equal(np.delete(want, 511), np.delete(as_number, 511))  # the rule matters, there only
    f = ta.Forest(nodes, T, D, cols, missing=MISSING)
    f.set_strategy(ta.STRATEGY_QRING)
    assert f.columns_plan(rows)[1] == 0
    same_bits(env, f, x, ("QRING",), want_raw=want)
    x2 = x.copy()
    x2[511, cols - 1], x2[512, 0] = 0.25, MISSING  # ... and the first row of the second chunk, first column
    same_bits(env, f, x2, ("QRING",), want_raw=oracle.predict(nodes, T, D, x2, MISSING, threads=1)[0])
    x3 = np.concatenate([x2, x2])[:2100]  # (2100 rows of 8 columns: two 1024-row chunks and a tail)
    x3[[512, 512 + rows], 0] = 0.25
    x3[1023, cols - 1] = MISSING
    assert int((x3 == np.float32(MISSING)).sum()) == 1
    same_bits(env, f, x3, ("QRING",), want_raw=oracle.predict(nodes, T, D, x3, MISSING, threads=1)[0])
    f.close()


@pytest.mark.parametrize("cols", [13, 30, 257, 300])
def test_widths_on_the_tile_loader(env, knobs, cols):
    """Not a multiple of 4, and tiles above the default 64 KiB of dynamic LDS (257 and 300 columns)"""
    ta, oracle, torch = env
    T, D = 60, 5
    nodes = ta.synth_forest(T, D, cols, seed=3)
    f = ta.Forest(nodes, T, D, cols, missing=MISSING)
    names = strategies(ta, f)
    for rows in (65, 193):
        x = ta.synth_data(rows, cols, seed=cols + rows, missing_prob=0.05, missing=MISSING, nan_prob=0.01)
        plans = same_bits(env, f, x, names, want_raw=oracle.predict(nodes, T, D, x, MISSING, threads=4)[0])
        assert plans["ROWTILE"] == ("columns_rowtile", 0)
    f.close()


def test_rows_too_wide_for_a_tile_take_chunks(env, knobs):
    ta, oracle, torch = env
    T, D, cols = 20, 5, 700
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=5), T, D, cols, missing=MISSING)
    names = strategies(ta, f)
    assert "ROWTILE" not in names and "AUTO" in names and "DIRECT" in names
    plans = same_bits(env, f, ta.synth_data(193, cols, seed=6, missing_prob=0.02, missing=MISSING), names)
    for name, (form, chunk) in plans.items():
        assert form not in TILE_FORMS and (chunk > 0) == (not form.startswith("qring")), plans
    assert plans["DIRECT"][1] > 0 and plans["TILERING"][1] > 0
    f.close()


def test_multiclass_avg_softmax_with_a_bias(env, knobs):
    ta, oracle, torch = env
    T, D, cols, nc = 90, 6, 40, 3
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=7, leaf_prob=0.05), T, D, cols, missing=MISSING, output=ta.OUT_SOFTMAX | ta.OUT_AVG,
                  global_bias=-0.5, num_classes=nc)
    names = strategies(ta, f)
    assert set(names) == {"AUTO", "DIRECT", "ROWTILE", "QRING"}
    for rows in (1, 65, 385):
        plans = same_bits(env, f, ta.synth_data(rows, cols, seed=rows, missing_prob=0.05, missing=MISSING, nan_prob=0.01), names)
        assert plans["ROWTILE"] == ("columns_rowtile", 0) and plans["QRING"][1] == 0 and plans["DIRECT"][1] > 0
    f.close()


# ----------------------------------------------------------------------------------------------------------- sparse handles
@pytest.mark.parametrize("num_classes", [1, 4])
def test_sparse_handle_all_five_strategies(env, knobs, num_classes):
    ta, oracle, torch = env
    T, cols = 120, 64
    sn, tr = ta.capi.synth_sparse_forest(T, cols, 4, 24, 0.32, 65535, 44)
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, num_classes=num_classes,
                             output=ta.OUT_SOFTMAX if num_classes > 1 else ta.OUT_RAW)
    names = strategies(ta, f, SPARSE)
    assert len(names) == 5, names
    for rows in (1, 64, 65, 127, 129, 191, 193, 383, 385):  # (sparse_qring: tiles of 384 rows as 128- and 192-row forms)
        x = ta.synth_data(rows, cols, seed=rows + 7, missing_prob=0.1, missing=MISSING, nan_prob=0.01)
        want = oracle.sparse_predict(sn, tr, x, MISSING, threads=4)[0] if num_classes == 1 else None
        plans = same_bits(env, f, x, names, want_raw=want)
        assert plans["ROWTILE"] == ("columns_sparse_rowtile", 0) and plans["TILEBLOCK"] == ("columns_sparse_top", 0)
        assert plans["QRING"] == ("sparse_qring", 0) and plans["DIRECT"][0] == "sparse_direct" and plans["DIRECT"][1] > 0
    f.close()


def test_categorical_handle_with_the_reference(env, knobs):
    ta, oracle, torch = env
    cols, feats, T = 32, [1, 5, 9, 17, 30], 60
    sn, tr = ta.capi.synth_sparse_forest(T, cols, 4, 16, 0.32, 65535, 11)
    rng = np.random.default_rng(11)
    b = sn["bits"].view(np.uint32)
    inner = np.flatnonzero((b >> 31) == 0)
    chosen = inner[np.isin(b[inner] & ((1 << 30) - 1), feats)]
    cats = {int(i): rng.choice(300, size=int(rng.integers(1, 200)), replace=False) for i in chosen}
    ml = {int(i) for i in chosen if rng.random() < 1 / 3}
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, categories=cats, members_left=ml)
    rows = 193
    x = ta.synth_data(rows, cols, seed=12, missing_prob=0.2, missing=MISSING, nan_prob=0.01)
    for c in feats:  # categories, non-integers, -0.0 and NaN in the categorical columns
        v = rng.integers(0, 320, rows).astype(np.float32)
        v[rng.random(rows) < 0.1] += np.float32(0.5)
        v[rng.random(rows) < 0.05] = np.float32(-0.0)
        v[rng.random(rows) < 0.05] = np.float32(np.nan)
        x[:, c] = np.where(x[:, c] == np.float32(MISSING), x[:, c], v)
    names = strategies(ta, f, ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK"))
    assert len(names) == 4
    _, (node, offset, words, mla) = ta.capi.pack_categorical(cats, ml)
    want, _ = categorical_ref.predict(sn, tr, x, MISSING, node, offset, words, mla)
    plans = same_bits(env, f, x, names, want_raw=np.ascontiguousarray(want, dtype=np.float32))
    assert plans["TILEBLOCK"] == ("columns_sparse_top", 0) and plans["ROWTILE"] == ("columns_sparse_rowtile", 0)
    f.close()


# ----------------------------------------------------------------------------------------------------------- native handles
@pytest.mark.parametrize("kind,k", [("oblivious", 1), ("oblivious", 8), ("vector", 1), ("vector", 10)])
def test_oblivious_and_vector_leaf_handles_take_chunks(env, knobs, kind, k):
    ta, oracle, torch = env
    cols = 7
    if kind == "vector":
        forest = vr.make_named(["leaf", 5, "stump", 8, 3, 6, "leaf", 8, 2, 7, 4], cols, k, 3700 + k)
        f = ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], cols, missing=MISSING)
        data = lambda rows: vr.make_data(rows, cols, seed=rows)  # noqa: E731
        ref = lambda x: vr.vector_ref(forest, x)[0]  # noqa: E731
    else:
        forest = obr.make_forest([0, 3, 6, 1, 2, 5, 4, 6, 3, 2, 0], cols, k, 3600 + k)
        f = ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], cols, leaf_dim=k,
                               missing=MISSING)
        data = lambda rows: obr.make_data(rows, cols, seed=rows)  # noqa: E731
        ref = lambda x: obr.ref_of(forest, x)[0]  # noqa: E731
    names = strategies(ta, f, ("AUTO", "DIRECT", "ROWTILE"))
    assert len(names) == 3
    for rows in (1, 65, 193):
        x = np.array(data(rows), np.float32)
        want = ref(x)
        plans = same_bits(env, f, x, names, want_raw=want[:, 0] if k == 1 else want)
        assert all(chunk > 0 and form.startswith(kind) for form, chunk in plans.values()), plans
    f.close()


# ------------------------------------------------------------------------------------------------------------ the table
def test_pointer_table_shuffled_allocations_and_a_column_named_twice(env, knobs):
    ta, oracle, torch = env
    k = k1_like(env)
    rows = 385
    x = k["x"][:rows].copy()
    f = ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING)
    dup = x.copy()
    dup[:, 5] = dup[:, 11]  # the matrix with that column duplicated
    xd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(dup).cuda()
    for name in strategies(ta, f):
        f.set_strategy(getattr(ta, "STRATEGY_" + name))
        for seed in (1, 2):
            cols = column_list(torch, x, seed=seed)
            assert len({c.data_ptr() for c in cols}) == len(cols)
            assert torch.equal(f.predict_columns(cols).view(torch.int32), f.predict(xd).view(torch.int32)), name
            cols[5] = cols[11]  # two entries of the table name one buffer
            assert torch.equal(f.predict_columns(cols).view(torch.int32), f.predict(dd).view(torch.int32)), name
        f.check()
    assert np.array_equal(bits(f.predict(dd)), bits(oracle.predict(k["nodes"], k["T"], k["D"], dup, MISSING, threads=4)[0]))
    f.close()


# ------------------------------------------------------------------------------------------------- reads, writes, values
def every_kind(env):
    """(label, handle, strategies, data(rows)) for one dense, one sparse and one oblivious handle"""
    ta, _, _ = env
    k = k1_like(env)
    yield "dense", ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING), ALL, lambda rows: k["x"][:rows]
    sn, tr = ta.capi.synth_sparse_forest(120, 64, 4, 24, 0.32, 65535, 44)
    yield ("sparse", ta.capi.SparseForest(sn, tr, 64, missing=MISSING), SPARSE,
           lambda rows: ta.synth_data(rows, 64, seed=rows, missing_prob=0.1, missing=MISSING, nan_prob=0.01))
    forest = obr.make_forest([0, 3, 6, 1, 2, 5, 4, 6, 3, 2, 0], 7, 3, 3603)
    yield ("oblivious", ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], 7,
                                           leaf_dim=3, missing=MISSING), ("AUTO", "DIRECT", "ROWTILE"),
           lambda rows: np.array(obr.make_data(rows, 7, seed=rows), np.float32))


@pytest.mark.parametrize("rows", [65, 193])
def test_reads_stay_inside_the_columns(env, knobs, rows):
    """col_stride = rows + 64; what lies between the columns is the sentinel once and +inf / NaN once.  A loader that read past
    a column's rows would put those values into a tile or a code and change the output; nothing here faults."""
    ta, oracle, torch = env
    for label, f, names, data in every_kind(env):
        x = np.ascontiguousarray(data(rows))
        views = []
        for gap in (np.float32(MISSING), np.float32(np.inf), np.float32(np.nan)):
            views.append(strided(torch, x, rows + 64, gap=gap, offset=64))  # (offset: the gap lies in front of column 0 too)
        xd = torch.from_numpy(x).cuda()
        for name in strategies(ta, f, names):
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            want = f.predict(xd).view(torch.int32)
            for v in views:
                assert torch.equal(f.predict_columns(v).view(torch.int32), want), (label, name)
                # the same columns through the table: pointers into the padded buffer
                assert torch.equal(f.predict_columns([v[:, c] for c in range(x.shape[1])]).view(torch.int32), want), (label, name)
            f.check()
        f.close()


@pytest.mark.parametrize("rows", [1, 65, 385])
def test_writes_stay_inside_the_output(env, knobs, rows):
    ta, oracle, torch = env
    for label, f, names, data in every_kind(env):
        x = np.ascontiguousarray(data(rows))
        xd = torch.from_numpy(x).cuda()
        for name in strategies(ta, f, names):
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            want = bits(f.predict(xd))
            for layout in ("stride=rows", "ptrs"):
                out = Guarded(torch, f._out_shape(rows), torch.float32, band_rows=384, device="cuda")
                f.predict_columns(as_layout(torch, x, layout), out=out.view)
                f.check()
                assert np.array_equal(bits(out.check(f"{label}, {name}, {layout}, rows {rows}")), want), (label, name, layout)
        f.close()


def test_special_values_in_the_corners(env, knobs):
    ta, oracle, torch = env
    k = k1_like(env)
    f = ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING)
    names = strategies(ta, f)
    special = np.array([MISSING, np.nan, np.inf, -np.inf, -0.0, 1e-45], np.float32)
    rows, cols = 129, k["cols"]
    for i, v in enumerate(special):
        x = k["x"][:rows].copy()
        for r, c in ((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)):
            x[r, c] = v
        x[(i + 1) % rows, 3] = special[(i + 1) % len(special)]
        same_bits(env, f, x, names, layouts=("stride=rows", "ptrs"), label=repr(v),
                  want_raw=oracle.predict(k["nodes"], k["T"], k["D"], x, MISSING, threads=4)[0])
    f.close()


# ------------------------------------------------------------------------------------------------------ chunks, allocation
def test_chunk_count_does_not_change_the_bits(env, knobs):
    ta, oracle, torch = env
    T, D, cols = 30, 6, 300
    nodes = ta.synth_forest(T, D, cols, seed=8)
    knobs.setenv("TAHOE_CSR_CHUNK_MB", "1")  # read when the handle is created: 768 rows of 300 columns
    f = ta.Forest(nodes, T, D, cols, missing=MISSING)
    f.set_strategy(ta.STRATEGY_DIRECT)
    form, chunk = f.columns_plan(2000)
    assert form == "direct" and chunk == 768
    x = ta.synth_data(2 * chunk + 5, cols, seed=9, missing_prob=0.03, missing=MISSING, nan_prob=0.01)
    want = oracle.predict(nodes, T, D, x, MISSING, threads=8)[0]
    for rows in (chunk - 1, chunk, chunk + 1, 2 * chunk + 5):  # 1, 1, 2 and 3 chunks
        assert -(-rows // f.columns_plan(rows)[1]) == {chunk - 1: 1, chunk: 1, chunk + 1: 2}.get(rows, 3)
        same_bits(env, f, x[:rows], ("DIRECT", "TILERING"), layouts=("stride=rows", "ptrs"), want_raw=want[:rows])
    assert f.info().device_bytes > 0
    f.close()


def test_reserve_columns_then_calls_allocate_nothing_and_can_be_captured(env, knobs):
    ta, oracle, torch = env
    k = k1_like(env)
    rows = 1000
    x = k["x"][:rows]
    x2 = np.ascontiguousarray(x[::-1])  # fresh inputs, written in place below
    sn, tr = ta.capi.synth_sparse_forest(120, 18, 4, 24, 0.32, 65535, 44)
    for f in (ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING), ta.capi.SparseForest(sn, tr, 18, missing=MISSING)):
        xd, xd2 = torch.from_numpy(x).cuda(), torch.from_numpy(x2).cuda()
        for name in strategies(ta, f):
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            f.reserve_columns(rows)
            f.reserve(rows)
            want, want2 = f.predict(xd).clone(), f.predict(xd2).clone()
            before = f.info().device_bytes
            xc = strided(torch, x, rows + 3)
            cols = column_list(torch, x)
            a = f.predict_columns(xc)
            b = f.predict_columns(strided(torch, x[:129], 129))  # a smaller batch
            c = f.predict_columns(cols)
            f.check()
            assert f.info().device_bytes == before, name
            assert torch.equal(a, want) and torch.equal(b, want[:129]) and torch.equal(c, want), name
            # a side stream gives the bits of the default stream
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                d = f.predict_columns(xc, stream=side)
                e = f.predict_columns(cols, stream=side)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            assert torch.equal(d.view(torch.int32), want.view(torch.int32)) and torch.equal(e.view(torch.int32), want.view(torch.int32)), name
            # one call captured on a side stream (a linear graph), replayed twice on inputs written in place
            out = torch.zeros_like(want)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                f.predict_columns(xc, out=out, stream=side)
            for src, w in ((x2, want2), (x, want)):
                xc.copy_(torch.from_numpy(src).cuda())
                out.zero_()
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(out.view(torch.int32), w.view(torch.int32)), name
            assert f.info().device_bytes == before, name
            f.check()
        f.close()


def test_knob_sends_auto_to_chunks(env, knobs):
    ta, oracle, torch = env
    k = k1_like(env)
    rows = 385
    f = ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING)
    fused = f.columns_plan(rows)
    assert fused[1] == 0
    f.close()
    knobs.setenv("TAHOE_COLUMNS_FUSED", "0")
    f = ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING)
    plans = same_bits(env, f, k["x"][:rows], ("AUTO", "ROWTILE"), want_raw=k["want"][:rows])
    assert plans["AUTO"] == (fused[0], plans["AUTO"][1]) and plans["AUTO"][1] > 0  # the same walk, on a row-major chunk
    assert plans["ROWTILE"] == ("columns_rowtile", 0)  # a forced strategy is not affected
    f.close()


def test_a_handle_without_trees_reads_no_column(env, knobs):
    """As tahoe_forest_predict on such a handle: the bias through the output transform, whatever the batch holds; no chunk is made"""
    ta, oracle, torch = env
    f = ta.Forest(np.empty(0, dtype=ta.NODE_DTYPE), 0, 3, 4, missing=MISSING, output=ta.OUT_SIGMOID, global_bias=0.5)
    before = f.info().device_bytes
    for rows in (1, 65):
        plans = same_bits(env, f, ta.synth_data(rows, 4, seed=rows), strategies(ta, f))
        assert all(chunk == 0 for _, chunk in plans.values()), plans
    assert f.info().device_bytes == before
    f.close()
