"""Typed, nullable tables on the GPU (Table, predict_table: tahoe_table_create, tahoe_forest_predict_table).
Every comparison is for equal float32 bits against predict of the same handle on table_ref.materialise(...) of the same buffers,
and once per handle kind against a reference that is not the library (the CPU oracle, categorical_ref, the numpy walks of the
native handles).  The plan (kernel form, rows per chunk) is asserted wherever a test is about one path.  cuDF and pyarrow are not
imported: Series below publishes what a cuDF column publishes.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import table_ref  # noqa: E402
import test_multiclass_gpu as mcg  # noqa: E402  (CASES, KNOBS, forest_nodes, batch: the smallest shapes that reach each QRING form)
import vector_ref as vr  # noqa: E402
from guarded import Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
ALL = ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK", "TILERING", "QRING")
SPARSE = ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK", "QRING")
KNOBS = mcg.KNOBS + ("TAHOE_QRING_NARROW128", "TAHOE_QRING_TOP24", "TAHOE_COLUMNS_FUSED", "TAHOE_TABLE_FUSED", "TAHOE_CSR_CHUNK_MB")
DTYPES = tuple(np.dtype(d) for d in table_ref.DTYPES)
OFFSETS = (0, 1, 7, 8, 13, 67)
TAIL = 5  # garbage elements behind every column's rows


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


class Series:
    """What a cuDF Series publishes: __cuda_array_interface__ over device bytes (a torch uint8 tensor), the validity bitmap as its
    `mask` entry"""

    def __init__(self, dev_bytes, dtype, n, mask=None):
        self.keep = dev_bytes
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": np.dtype(dtype).str, "data": (dev_bytes.data_ptr(), False),
                                         "version": 3, "strides": None}
        if mask is not None:
            self.__cuda_array_interface__["mask"] = mask


def typed(x, dtype, scale=3.0):
    """A float32 column as values of `dtype` that the same thresholds still split"""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return x.copy()
    if dtype == np.float64:
        return x.astype(np.float64) * (1.0 + 3e-8)  # (between two float32 values: the rounding is part of the test)
    if dtype == np.float16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16)
    info = np.iinfo(dtype)
    v = np.nan_to_num(np.rint(x.astype(np.float64) * scale), nan=0.0)
    return np.clip(np.abs(v) if info.min == 0 else v, info.min, info.max).astype(dtype)


def garbage_element(dtype, garbage):
    if dtype.kind == "f":
        return np.nan if garbage else (6.0e4 if dtype == np.float16 else 3.0e38)
    return np.iinfo(dtype).max if garbage else np.iinfo(dtype).min


def under_element(dtype, under):
    """What lies under a null: never looked at"""
    if dtype.kind == "f":
        return {"nan": np.nan, "inf": np.inf, "sentinel": MISSING, "large": 6.0e4 if dtype == np.float16 else 1.0e30}[under]
    info = np.iinfo(dtype)
    return {"nan": info.max, "inf": info.min, "sentinel": -999 if info.min <= -999 else 0, "large": info.max}[under]


class Built:
    """A Table over fresh device buffers and the matrix it stands for.  cols_np[c]: the column's values (rows of them); valid[c]:
    None or booleans; offsets[c]: elements (and bits) of garbage in front; behind the rows lie TAIL garbage elements and the
    garbage bits that fill the bitmap's last byte -- the bitmap has no byte more than offset + rows bits need.  Garbage bits are
    all `garbage`.  Even columns go in as torch tensors where torch has the dtype, the others as Series."""

    def __init__(self, env, cols_np, valid=None, offsets=None, garbage=0, under=None, order_seed=None, missing=MISSING):
        ta, _, torch = env
        n = len(cols_np)
        self.rows = len(cols_np[0]) if n else 0
        valid = [None] * n if valid is None else list(valid)
        self.offsets = [0] * n if offsets is None else list(offsets)
        self.host, self.host_validity, self.dev, self.vdev = [None] * n, [None] * n, [None] * n, [None] * n
        columns, validity = [None] * n, [None] * n
        torch_types = ta.capi._torch_col_types()
        order = range(n) if order_seed is None else np.random.default_rng(order_seed).permutation(n)
        for c in order:  # (allocation order)
            a, off = np.asarray(cols_np[c]), self.offsets[c]
            buf = np.full(off + self.rows + TAIL, garbage_element(a.dtype, garbage), dtype=a.dtype)
            buf[off: off + self.rows] = a
            if valid[c] is not None:
                if under is not None:
                    buf[off: off + self.rows][~np.asarray(valid[c], bool)] = under_element(a.dtype, under)
                self.host_validity[c] = table_ref.pack_validity(valid[c], off, before=garbage, after=garbage)
                self.vdev[c] = torch.from_numpy(self.host_validity[c].copy()).cuda()
            self.host[c] = buf[: off + self.rows]
            self.dev[c] = torch.from_numpy(buf.view(np.uint8).copy()).cuda()
            tdtype = {v: k for k, v in torch_types.items() if k != torch.bool}.get(ta.capi._COL_TYPESTR[a.dtype.str])
            if c % 2 == 0 and tdtype is not None:
                columns[c] = self.dev[c].view(tdtype)[: off + self.rows]
                validity[c] = self.vdev[c]
            else:
                mask = None if self.vdev[c] is None else Series(self.vdev[c], np.uint8, self.vdev[c].numel())
                columns[c] = Series(self.dev[c], a.dtype, off + self.rows, mask=mask)
        self.M = table_ref.materialise(self.host, self.host_validity, self.offsets, missing)
        self.table = ta.Table(columns, validity=validity, offsets=self.offsets)
        assert self.table.rows == self.rows and self.table.num_cols == n


def mixed(x, rng, dtypes=DTYPES, nulls=0.1, scale=3.0):
    """(typed columns, validity, offsets) for the float32 matrix x: the dtypes in turn, the six offsets in turn, and the validity
    kinds in turn -- none, all valid, random nulls, a null in row 0 only, in the last row only, every row null"""
    rows, cols = x.shape
    cols_np = [typed(x[:, c], dtypes[c % len(dtypes)], scale) for c in range(cols)]
    valid = []
    for c in range(cols):
        kind = c % 6 if c != cols - 2 else 5  # (one all-null column whatever the width)
        v = np.ones(rows, bool)
        if kind == 0:
            v = None
        elif kind == 2:
            v = rng.random(rows) >= nulls
        elif kind == 3:
            v[0] = False
        elif kind == 4:
            v[-1] = False
        elif kind == 5:
            v[:] = False
        valid.append(v)
    offsets = [OFFSETS[(c + c // 6) % 6] for c in range(cols)]
    return cols_np, valid, offsets


def strategies(ta, f, names=ALL):
    ok = []
    for name in names:
        try:
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            ok.append(name)
        except ta.TahoeError as e:
            assert e.status == 7, str(e)
    return ok


def same_bits(env, f, built, names, label="", want_raw=None):
    """predict_table against predict on the materialised matrix under each named strategy (and against want_raw, a reference's
    bits, where given); returns the plan per strategy."""
    ta, _, torch = env
    tables = built if isinstance(built, (list, tuple)) else [built]
    md = torch.from_numpy(np.ascontiguousarray(tables[0].M)).cuda()
    plans = {}
    for name in names:
        f.set_strategy(getattr(ta, "STRATEGY_" + name))
        want = f.predict(md)
        plans[name] = f.table_plan(tables[0].rows)
        if want_raw is not None:
            assert np.array_equal(bits(want), bits(want_raw)), (label, name, "predict != reference")
        for i, b in enumerate(tables):
            assert np.array_equal(bits(b.M), bits(tables[0].M)), "tables of one call stand for one matrix"
            got = f.predict_table(b.table)
            f.check()
            assert got.shape == want.shape and got.dtype == want.dtype
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (label, name, i, plans[name], b.M.shape)
    return plans


def check_dense_plans(plans):
    assert plans["QRING"][0].startswith("qring_") and plans["QRING"][1] == 0, plans
    for name in ("DIRECT", "ROWTILE", "TILEBLOCK", "TILERING"):
        if name in plans:
            assert plans[name][1] > 0 and not plans[name][0].startswith("columns_"), plans
    assert plans["DIRECT"][0] == "direct" and plans["ROWTILE"][0] == "rowtile"


# ------------------------------------------------------------------------------------------------------------ dense handles
_k1 = {}


def k1_like(env):
    """500 trees of depth 8 on 18 features and 1025 rows: made once, read-only"""
    ta, _, _ = env
    if not _k1:
        T, D, cols = 500, 8, 18
        _k1.update(T=T, D=D, cols=cols, nodes=ta.synth_forest(T, D, cols, seed=11, leaf_prob=0.05),
                   x=ta.synth_data(1025, cols, seed=12))
    return _k1


@pytest.mark.parametrize("rows", [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1000, 1025])
def test_row_counts_every_strategy(env, knobs, rows):
    """The byte edges of the bitmap, the edges of the 64-row transpose block and of the 512- and 1024-row quantise chunks; every
    dtype, offset and validity kind; garbage bits and elements around every column, all 0 once and all 1 once"""
    ta, oracle, torch = env
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tahoe_amd", "csrc", "qring_internal.h")).read()
    assert "constexpr int kQuantMinRowsPerBlock = 512;" in src
    k = k1_like(env)
    f = ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING)
    names = strategies(ta, f)
    assert set(names) == set(ALL), names
    cols_np, valid, offsets = mixed(k["x"][:rows], np.random.default_rng(rows))
    tables = [Built(env, cols_np, valid, offsets, garbage=g, under=u) for g, u in ((0, "nan"), (1, "large"))]
    assert np.any(tables[0].M == np.float32(MISSING)) and (rows < 8 or np.any(tables[0].M[:, 2] != np.float32(MISSING)))
    want = oracle.predict(k["nodes"], k["T"], k["D"], tables[0].M, MISSING, threads=8)[0]  # raw output: the oracle's bits too
    plans = same_bits(env, f, tables, names, want_raw=want)
    check_dense_plans(plans)
    auto = f.get_strategy(rows)
    assert plans["AUTO"] == plans[{ta.STRATEGY_QRING: "QRING", ta.STRATEGY_ROWTILE: "ROWTILE", ta.STRATEGY_TILERING: "TILERING",
                                   ta.STRATEGY_TILEBLOCK: "TILEBLOCK", ta.STRATEGY_DIRECT: "DIRECT"}[auto]]
    f.close()


def test_what_lies_under_a_null_is_never_looked_at(env, knobs):
    ta, oracle, torch = env
    k = k1_like(env)
    rows = 193
    f = ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING)
    cols_np, valid, offsets = mixed(k["x"][:rows], np.random.default_rng(3), nulls=0.3)
    tables = [Built(env, cols_np, valid, offsets, garbage=i % 2, under=u) for i, u in enumerate(("nan", "inf", "sentinel", "large"))]
    assert not np.array_equal(tables[0].host[2], tables[1].host[2], equal_nan=True)  # the buffers differ, the matrix does not
    same_bits(env, f, tables, strategies(ta, f),
              want_raw=oracle.predict(k["nodes"], k["T"], k["D"], tables[0].M, MISSING, threads=8)[0])
    f.close()


# The values of tests/test_table_ref.py, per dtype, and the float32 thresholds that tell their conversions apart
T24 = 2.0 ** 24
EDGE = {
    "float32": ([-0.0, 0.0, 1e-40, 1.0, -1.0, 3.0e38, np.inf, -np.inf, np.nan], [0.0, 1e-40, 1.0]),
    # 1 + 2^-23 is a float32; + 2^-25 rounds onto it (tie to even would go down: 2^-24 is the tie, so add a little more), - 2^-25
    # rounds to 1.0, just below it.  1e-40 and 0.99e-40 round to float32 subnormals on either side of the threshold 1e-40f.
    "float64": ([1.0 + 2.0 ** -23 + 2.0 ** -25, 1.0 + 2.0 ** -23 - 2.0 ** -25, 1.0 + 2.0 ** -24 + 2.0 ** -40, 1.0 + 2.0 ** -24, 1e300,
                 -1e300, np.nan, 1e-40, 0.99e-40, 1e-46, -0.0, T24 + 1, 3.4028235677973366e38],
                [1.0 + 2.0 ** -23, 1e-40, 0.0, T24, 3.0e38]),
    "float16": ([6e-8, 1.2e-7, -6e-8, -0.0, 65504.0, np.inf, np.nan, 1.0], [2.0 ** -24, 2.0 ** -23, 0.0, 65504.0]),
    "int8": ([-128, 127, 0, -1], [-128.0, 127.0, 0.0]),
    "int16": ([-32768, 32767, 0, -999], [-32768.0, 32767.0, -998.0]),
    "int32": ([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), -2 ** 31, 2 ** 31 - 1, 0, -999], [T24, T24 + 2, T24 + 4, -T24, 2.0 ** 31]),
    "int64": ([2 ** 24 + 1, 2 ** 24 + 3, -2 ** 63, 2 ** 63 - 1, 2 ** 32 + 1, 0, -999], [T24, T24 + 4, 2.0 ** 63, 2.0 ** 32, -2.0 ** 63]),
    "uint8": ([0, 1, 255], [1.0, 255.0]),
    "uint16": ([0, 65535, 32768], [65535.0, 32768.0]),
    "uint32": ([0, 2 ** 32 - 1, 2 ** 31, 2 ** 24 + 1], [2.0 ** 32, 2.0 ** 31, T24, T24 + 2]),
    "uint64": ([0, 2 ** 64 - 1, 2 ** 63, 2 ** 24 + 3], [2.0 ** 64, 2.0 ** 63, T24 + 4, T24 + 2]),
}


def edge_forest(ta, dtypes, T, D, seed):
    """Complete trees whose inner nodes split column c (of dtype dtypes[c]) on one of that dtype's edge thresholds; both default
    directions"""
    rng = np.random.default_rng(seed)
    per, inner = 2 ** (D + 1) - 1, 2 ** D - 1
    fid = rng.integers(0, len(dtypes), T * per)
    is_leaf = np.tile(np.arange(per) >= inner, T)
    thr = np.array([rng.choice(EDGE[dtypes[c]][1]) for c in fid], np.float32)
    val = np.where(is_leaf, rng.uniform(-1, 1, T * per), thr).astype(np.float32)
    return ta.capi.encode_nodes(np.where(is_leaf, 0, fid), val, rng.integers(0, 2, T * per), np.ones(T * per), is_leaf)


def edge_columns(dtypes, rows, seed):
    rng = np.random.default_rng(seed)
    cols = []
    for name in dtypes:
        with np.errstate(over="ignore", invalid="ignore"):
            pool = np.array(EDGE[name][0], dtype=name)
        cols.append(pool[rng.integers(0, len(pool), rows)])
    return cols


def test_every_type_in_one_table_at_the_edges_of_float32(env, knobs):
    """One column per dtype; the rows hold the extreme values of test_table_ref.py and the forest splits on the float32 values
    their conversions land on or beside: an INT64 taken through int32, a float64 truncated instead of rounded, or a flushed
    float32 subnormal would each take another branch somewhere."""
    ta, oracle, torch = env
    names = list(table_ref.DTYPES)
    T, D, rows = 60, 5, 257
    nodes = edge_forest(ta, names, T, D, seed=1)
    cols_np = edge_columns(names, rows, seed=2)
    valid = [None if c % 3 else np.random.default_rng(c).random(rows) >= 0.1 for c in range(len(names))]
    built = [Built(env, cols_np, valid, [OFFSETS[c % 6] for c in range(len(names))], garbage=g, under="nan") for g in (0, 1)]
    M = built[0].M
    sub = M[:, 1][(M[:, 1] > 0) & (M[:, 1] < np.finfo(np.float32).tiny)]
    assert sub.size and np.float32(1e-40) in sub  # the float64 column does hold values that round to float32 subnormals
    f = ta.Forest(nodes, T, D, len(names), missing=MISSING)
    plans = same_bits(env, f, built, strategies(ta, f), want_raw=oracle.predict(nodes, T, D, M, MISSING, threads=4)[0])
    assert plans["QRING"][1] == 0 and plans["DIRECT"][1] > 0
    f.close()


@pytest.mark.parametrize("name", table_ref.DTYPES)
def test_one_table_per_type(env, knobs, name):
    ta, oracle, torch = env
    T, D, rows, cols = 40, 4, 130, 4
    nodes = edge_forest(ta, [name] * cols, T, D, seed=5)
    cols_np = edge_columns([name] * cols, rows, seed=6)
    valid = [None, np.random.default_rng(7).random(rows) >= 0.2, np.ones(rows, bool), None]
    built = Built(env, cols_np, valid, [0, 13, 67, 1], garbage=1, under="large")
    f = ta.Forest(nodes, T, D, cols, missing=MISSING)
    same_bits(env, f, built, strategies(ta, f, ("AUTO", "DIRECT", "QRING")), label=name,
              want_raw=oracle.predict(nodes, T, D, built.M, MISSING, threads=2)[0])
    f.close()


QRING_CASES = [c for c in mcg.CASES if c[8] is not None and c[8].startswith("qring")]


@pytest.mark.parametrize("case", QRING_CASES, ids=[c[0] for c in QRING_CASES])
def test_every_qring_form_reads_the_table(env, knobs, case):
    """test_multiclass_gpu.py's table (the smallest shape that reaches each form), as one class; rows straddle the form's tile;
    every fourth column is float64, the others float32, and every tile has one null"""
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
        counts = [cus * 192 + 129]
    else:
        counts = sorted({t - 1, t + 1, 129, 2 * t + 1})
    data = mcg.batch(ta, gen, max(counts), cols, seed=200 + cols)
    for rows in counts:
        assert f.table_plan(rows) == (form, 0), (rows, f.table_plan(rows))
        x = data[:rows]
        cols_np = [typed(x[:, c], np.float64 if c % 4 == 3 else np.float32) for c in range(cols)]
        valid = [np.ones(rows, bool) for _ in range(cols)]
        for i, r in enumerate(range(0, rows, 64)):  # one null per 64 rows, hence per tile: in turn on every column
            valid[(i * 7 + 3) % cols][min(r + (i * 5) % 64, rows - 1)] = False
        built = Built(env, cols_np, valid, [OFFSETS[c % 6] for c in range(cols)], garbage=rows % 2, under="sentinel" if rows % 2 else "inf")
        want = oracle.predict(nodes, T, D, built.M, MISSING, threads=8)[0] if form == "qring_region8" else None
        same_bits(env, f, built, ("QRING",), label=f"{form}, rows {rows}", want_raw=want)
    f.close()


def test_a_null_raises_the_missing_flag_of_its_quantise_chunk(env, knobs):
    """test_missing_flag_of_the_right_quantise_chunk's forest (every root splits on the last column, missing goes right), and the
    same forest with def_left = 1 in the odd trees: a tile that walked without the missing rule reads the missing code as the
    largest number and goes right, which is where def_left = 0 sends a missing value anyway, so only the odd trees show it (DESIGN.md
    section 38).  The batch's only missing value is a null -- no sentinel, no NaN anywhere, -0.75 under the null -- in the last row
    of the first 512-row chunk and the last column, then in the first row of the second chunk and column 0, then in row 1023 of a
    2100-row batch.  A null that got the missing code without raising its chunk's flag fails here."""
    ta, oracle, torch = env
    assert "TAHOE_QRING_TOP24" not in os.environ
    T, D, cols, rows = 24, 4, 8, 1100
    rng = np.random.default_rng(5)
    fid = np.tile(np.array([cols - 1] + list(rng.integers(0, cols, 2 ** D - 2)) + [0] * 2 ** D), T)  # every root splits on the last column
    per = 2 ** (D + 1) - 1
    is_leaf = np.tile(np.arange(per) >= 2 ** D - 1, T)
    val = np.where(is_leaf, rng.uniform(-1, 1, T * per), rng.uniform(-0.5, 0.5, T * per)).astype(np.float32)
    x = rng.uniform(-1, 1, (2100, cols)).astype(np.float32)
    dtypes = (np.float32, np.float64, np.float32, np.float16)
    for def_left in (np.zeros(T * per), np.repeat(np.arange(T) % 2, per)):  # missing goes right; ... left in the odd trees
        nodes = ta.capi.encode_nodes(fid, val, def_left, np.ones(T * per), is_leaf)
        f = ta.Forest(nodes, T, D, cols, missing=MISSING)
        f.set_strategy(ta.STRATEGY_QRING)
        for n, r, c in ((rows, 511, cols - 1), (rows, 512, 0), (2100, 1023, cols - 1)):
            xx = x[:n].copy()
            xx[r, c] = -0.75  # what lies under the null: an ordinary value, left of every threshold
            cols_np = [typed(xx[:, j], dtypes[j % 4]) for j in range(cols)]
            valid = [np.ones(n, bool) if j % 2 == 0 or j == c else None for j in range(cols)]
            valid[c][r] = False
            built = Built(env, cols_np, valid, [OFFSETS[j % 6] for j in range(cols)], garbage=1)
            assert int((built.M == np.float32(MISSING)).sum()) == 1 and built.M[r, c] == np.float32(MISSING) and not np.isnan(built.M).any()
            want = oracle.predict(nodes, T, D, built.M, MISSING, threads=1)[0]
            as_number = built.M.copy()
            as_number[r, c] = -0.75
            other = oracle.predict(nodes, T, D, as_number, MISSING, threads=1)[0]
            assert want[r] != other[r] and np.array_equal(np.delete(want, r), np.delete(other, r))  # the rule matters, there only
            assert f.table_plan(n)[0].startswith("qring_") and f.table_plan(n)[1] == 0  # fused: the quantise pass reads the table
            same_bits(env, f, built, ("QRING",), label=f"null at ({r}, {c}) of {n}", want_raw=want)
        f.close()


def test_multiclass_avg_softmax_with_a_bias(env, knobs):
    ta, oracle, torch = env
    T, D, cols, nc = 90, 6, 40, 3
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=7, leaf_prob=0.05), T, D, cols, missing=MISSING, output=ta.OUT_SOFTMAX | ta.OUT_AVG,
                  global_bias=-0.5, num_classes=nc)
    names = strategies(ta, f)
    assert set(names) == {"AUTO", "DIRECT", "ROWTILE", "QRING"}
    for rows in (1, 65, 385):
        built = Built(env, *mixed(ta.synth_data(rows, cols, seed=rows), np.random.default_rng(rows)), garbage=rows % 2, under="nan")
        plans = same_bits(env, f, built, names)
        assert plans["QRING"][1] == 0 and plans["DIRECT"][1] > 0 and plans["ROWTILE"][1] > 0
    f.close()


def test_nan_missing_handles_nan_beside_nulls(env, knobs):
    """On a TAHOE_CREATE_NAN_MISSING handle a float64 or float16 NaN is missing like a null; without the flag it goes left"""
    ta, oracle, torch = env
    k = k1_like(env)
    rows, cols = 385, k["cols"]
    rng = np.random.default_rng(9)
    x = k["x"][:rows].copy()
    x[rng.random(x.shape) < 0.05] = np.nan
    cols_np, valid, offsets = mixed(x, rng, dtypes=(np.dtype(np.float64), np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.int16)))
    built = Built(env, cols_np, valid, offsets, garbage=1, under="large")
    assert np.isnan(built.M[:, 0]).any() and np.isnan(built.M[:, 1]).any()
    as_sentinel = np.where(np.isnan(built.M), np.float32(MISSING), built.M)
    f = ta.Forest(k["nodes"], k["T"], k["D"], cols, missing=MISSING, nan_missing=True)
    names = strategies(ta, f)
    assert set(names) == {"AUTO", "DIRECT", "ROWTILE", "QRING"}
    plans = same_bits(env, f, built, names, want_raw=oracle.predict(k["nodes"], k["T"], k["D"], as_sentinel, MISSING, threads=8)[0])
    assert plans["QRING"][1] == 0
    f.close()
    plain = ta.Forest(k["nodes"], k["T"], k["D"], cols, missing=MISSING)
    same_bits(env, plain, built, ("QRING", "DIRECT"), want_raw=oracle.predict(k["nodes"], k["T"], k["D"], built.M, MISSING, threads=8)[0])
    plain.close()
    sn, tr = ta.capi.synth_sparse_forest(120, cols, 4, 24, 0.32, 65535, 44)
    sf = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, nan_missing=True)
    names = strategies(ta, sf, SPARSE)
    assert len(names) == 5
    plans = same_bits(env, sf, built, names, want_raw=oracle.sparse_predict(sn, tr, as_sentinel, MISSING, threads=4)[0])
    assert plans["QRING"] == ("sparse_qring", 0)
    sf.close()


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
    for rows in (1, 65, 129, 193, 385):  # (sparse_qring: tiles of 384 rows as 128- and 192-row forms)
        built = Built(env, *mixed(ta.synth_data(rows, cols, seed=rows + 7), np.random.default_rng(rows)), garbage=rows % 2, under="inf")
        want = oracle.sparse_predict(sn, tr, built.M, MISSING, threads=4)[0] if num_classes == 1 else None
        plans = same_bits(env, f, built, names, want_raw=want)
        assert plans["QRING"] == ("sparse_qring", 0), plans
        for name in ("DIRECT", "ROWTILE", "TILEBLOCK"):
            assert plans[name][1] > 0 and plans[name][0].startswith("sparse_"), plans
    f.close()


def test_categorical_handle_a_null_takes_the_default_branch(env, knobs):
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
    x = ta.synth_data(rows, cols, seed=12)
    cols_np, valid, offsets = mixed(x, rng, nulls=0.2)
    for i, c in enumerate(feats):  # the categorical columns: category ids as integers of five dtypes, nulls among them
        cols_np[c] = rng.integers(0, 320, rows).astype((np.uint16, np.int32, np.int64, np.uint32, np.int16)[i])
        valid[c] = rng.random(rows) >= 0.2
    built = Built(env, cols_np, valid, offsets, garbage=1, under="large")
    names = strategies(ta, f, ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK"))
    assert len(names) == 4
    _, (node, offset, words, mla) = ta.capi.pack_categorical(cats, ml)
    want, _ = categorical_ref.predict(sn, tr, built.M, MISSING, node, offset, words, mla)
    plans = same_bits(env, f, built, names, want_raw=np.ascontiguousarray(want, dtype=np.float32))
    assert all(chunk > 0 for _, chunk in plans.values()), plans
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
        x = np.nan_to_num(np.array(data(rows), np.float32), nan=0.5)
        cols_np = [typed(x[:, c], (np.float32, np.float64, np.float16)[c % 3]) for c in range(cols)]
        valid = [None if c % 2 else np.random.default_rng(rows + c).random(rows) >= 0.15 for c in range(cols)]
        built = Built(env, cols_np, valid, [OFFSETS[c % 6] for c in range(cols)], garbage=rows % 2, under="nan")
        want = ref(built.M)
        plans = same_bits(env, f, built, names, want_raw=want[:, 0] if k == 1 else want)
        assert all(chunk > 0 and form.startswith(kind) for form, chunk in plans.values()), plans
    f.close()


# ------------------------------------------------------------------------------------------------- buffers, reads, writes
def every_kind(env):
    """(label, handle, strategies, width) for one dense, one sparse and one oblivious handle"""
    ta, _, _ = env
    k = k1_like(env)
    yield "dense", ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING), ALL, k["cols"]
    sn, tr = ta.capi.synth_sparse_forest(120, 64, 4, 24, 0.32, 65535, 44)
    yield "sparse", ta.capi.SparseForest(sn, tr, 64, missing=MISSING), SPARSE, 64
    forest = obr.make_forest([0, 3, 6, 1, 2, 5, 4, 6, 3, 2, 0], 7, 3, 3603)
    yield ("oblivious", ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], 7,
                                           leaf_dim=3, missing=MISSING), ("AUTO", "DIRECT", "ROWTILE"), 7)


def test_shuffled_allocations_and_one_buffer_named_by_two_descriptors(env, knobs):
    ta, oracle, torch = env
    k = k1_like(env)
    rows, cols = 385, k["cols"]
    cols_np, valid, offsets = mixed(k["x"][:rows], np.random.default_rng(2))
    f = ta.Forest(k["nodes"], k["T"], k["D"], cols, missing=MISSING)
    names = strategies(ta, f)
    built = [Built(env, cols_np, valid, offsets, garbage=1, under="nan", order_seed=s) for s in (None, 1, 2)]
    assert len({b.dev[3].data_ptr() - b.dev[2].data_ptr() for b in built}) > 1  # the allocations do lie in different orders
    same_bits(env, f, built, names)
    # column 5 named again as column 11, through the same data buffer: another offset (3 rows further, so 3 rows fewer are left)
    # and a bitmap of its own
    b0 = built[0]
    n = rows - 3
    data5, off5 = b0.dev[5], offsets[5]
    v11 = np.random.default_rng(4).random(n) >= 0.3
    vb = table_ref.pack_validity(v11, off5 + 3, before=1, after=1)
    vdev = torch.from_numpy(vb.copy()).cuda()
    columns, validity, offs, host, hostv = [], [], [], [], []
    for c in range(cols):
        a = b0.host[c].dtype
        src, o = (c, offsets[c]) if c != 11 else (5, off5 + 3)
        a = b0.host[src].dtype
        mask = b0.vdev[c] if c != 11 else vdev
        length = o + n
        columns.append(Series(b0.dev[src], a, length, mask=None if mask is None else Series(mask, np.uint8, mask.numel())))
        offs.append(o)
        host.append(np.concatenate([b0.host[src], np.zeros(TAIL, a)])[:length])
        hostv.append(b0.host_validity[c] if c != 11 else vb)
    table = ta.Table(columns, offsets=offs)
    M = table_ref.materialise(host, hostv, offs, MISSING)
    assert table.rows == n and np.array_equal(bits(M[:, 5]), bits(b0.M[:n, 5])) and not np.array_equal(bits(M[:, 11]), bits(b0.M[:n, 11]))
    md = torch.from_numpy(M).cuda()
    for name in names:
        f.set_strategy(getattr(ta, "STRATEGY_" + name))
        assert torch.equal(f.predict_table(table).view(torch.int32), f.predict(md).view(torch.int32)), name
    f.check()
    table.close()
    f.close()


@pytest.mark.parametrize("rows", [1, 65, 385])
def test_writes_stay_inside_the_output(env, knobs, rows):
    ta, oracle, torch = env
    for label, f, names, width in every_kind(env):
        built = Built(env, *mixed(ta.synth_data(rows, width, seed=rows), np.random.default_rng(rows)), garbage=1, under="nan")
        md = torch.from_numpy(built.M).cuda()
        for name in strategies(ta, f, names):
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            want = bits(f.predict(md))
            out = Guarded(torch, f._out_shape(rows), torch.float32, band_rows=384, device="cuda")
            f.predict_table(built.table, out=out.view)
            f.check()
            assert np.array_equal(bits(out.check(f"{label}, {name}, rows {rows}")), want), (label, name)
        f.close()


# ------------------------------------------------------------------------------------------------------ chunks, allocation
def test_chunk_count_does_not_change_the_bits(env, knobs):
    ta, oracle, torch = env
    T, D, cols = 30, 6, 300
    nodes = ta.synth_forest(T, D, cols, seed=8)
    knobs.setenv("TAHOE_CSR_CHUNK_MB", "1")  # read when the handle is created: 768 rows of 300 columns
    f = ta.Forest(nodes, T, D, cols, missing=MISSING)
    f.set_strategy(ta.STRATEGY_DIRECT)
    form, chunk = f.table_plan(2000)
    assert form == "direct" and chunk == 768
    x = ta.synth_data(2 * chunk + 5, cols, seed=9)
    for rows in (chunk - 1, chunk, chunk + 1, 2 * chunk + 5):  # 1, 1, 2 and 3 chunks
        assert -(-rows // f.table_plan(rows)[1]) == {chunk - 1: 1, chunk: 1, chunk + 1: 2}.get(rows, 3)
        built = Built(env, *mixed(x[:rows], np.random.default_rng(rows)), garbage=rows % 2, under="inf")
        same_bits(env, f, built, ("DIRECT", "TILERING"), want_raw=oracle.predict(nodes, T, D, built.M, MISSING, threads=8)[0])
    assert f.info().device_bytes > 0
    f.close()


def test_reserve_table_then_calls_allocate_nothing_and_can_be_captured(env, knobs):
    ta, oracle, torch = env
    k = k1_like(env)
    rows, cols = 1000, k["cols"]
    rng = np.random.default_rng(6)
    cols_np, valid, offsets = mixed(k["x"][:rows], rng)
    cols_np2, valid2, _ = mixed(np.ascontiguousarray(k["x"][:rows][::-1]), rng, nulls=0.25)  # fresh values and bitmaps, written in place below
    valid2 = [v2 if v is not None else None for v, v2 in zip(valid, valid2)]
    sn, tr = ta.capi.synth_sparse_forest(120, cols, 4, 24, 0.32, 65535, 44)
    for f in (ta.Forest(k["nodes"], k["T"], k["D"], cols, missing=MISSING), ta.capi.SparseForest(sn, tr, cols, missing=MISSING)):
        for name in strategies(ta, f):
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            a, b = Built(env, cols_np, valid, offsets, garbage=0, under="nan"), Built(env, cols_np2, valid2, offsets, garbage=1, under="large")
            small = Built(env, [c[:129] for c in cols_np], [None if v is None else v[:129] for v in valid], offsets)
            f.reserve_table(rows)
            f.reserve(rows)
            want_a = f.predict(torch.from_numpy(a.M).cuda()).clone()
            want_b = f.predict(torch.from_numpy(b.M).cuda()).clone()
            assert not torch.equal(want_a, want_b)
            before = f.info().device_bytes
            got, got_small = f.predict_table(a.table), f.predict_table(small.table)
            f.check()
            assert f.info().device_bytes == before, name
            assert torch.equal(got.view(torch.int32), want_a.view(torch.int32)), name
            assert torch.equal(got_small.view(torch.int32), want_a[:129].view(torch.int32)), name
            # a side stream gives the bits of the default stream
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                d = f.predict_table(a.table, stream=side)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            assert torch.equal(d.view(torch.int32), want_a.view(torch.int32)), name
            # one call captured on a side stream (a linear graph), replayed after data and bitmaps were rewritten in place
            out = torch.zeros_like(want_a)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                f.predict_table(a.table, out=out, stream=side)
            saved = [t.clone() for t in a.dev], [None if t is None else t.clone() for t in a.vdev]
            for src, srcv, w in ((b.dev, b.vdev, want_b), (saved[0], saved[1], want_a)):
                for c in range(cols):
                    a.dev[c].copy_(src[c])
                    if a.vdev[c] is not None:
                        a.vdev[c].copy_(srcv[c])
                out.zero_()
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(out.view(torch.int32), w.view(torch.int32)), name
            assert f.info().device_bytes == before, name
            f.check()
        f.close()


def test_knob_sends_auto_to_chunks(env, knobs):
    ta, oracle, torch = env
    T, D, cols, rows = 24, 4, 8, 1100  # (a forest whose AUTO is QRING at this size: asserted)
    k = k1_like(env)
    f = ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING)
    rows = next((r for r in (1025, 513, 385) if f.get_strategy(r) == ta.STRATEGY_QRING), None)
    assert rows is not None, "AUTO never picks QRING on this forest: the knob has nothing to switch"
    fused = f.table_plan(rows)
    assert fused[1] == 0 and fused[0].startswith("qring_")
    f.close()
    knobs.setenv("TAHOE_TABLE_FUSED", "0")
    f = ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING)
    built = Built(env, *mixed(k["x"][:rows], np.random.default_rng(1)), garbage=1, under="nan")
    plans = same_bits(env, f, built, ("AUTO", "QRING"), want_raw=oracle.predict(k["nodes"], k["T"], k["D"], built.M, MISSING, threads=8)[0])
    assert plans["AUTO"] == (fused[0], plans["AUTO"][1]) and plans["AUTO"][1] > 0  # the same walk, on a row-major chunk
    assert plans["QRING"] == fused  # a forced strategy is not affected
    f.close()


def test_a_handle_without_trees_reads_no_column(env, knobs):
    """As tahoe_forest_predict on such a handle: the bias through the output transform, whatever the table holds; no chunk is made"""
    ta, oracle, torch = env
    f = ta.Forest(np.empty(0, dtype=ta.NODE_DTYPE), 0, 3, 4, missing=MISSING, output=ta.OUT_SIGMOID, global_bias=0.5)
    before = f.info().device_bytes
    for rows in (1, 65):
        built = Built(env, *mixed(ta.synth_data(rows, 4, seed=rows), np.random.default_rng(rows)))
        plans = same_bits(env, f, built, strategies(ta, f))
        assert all(chunk == 0 for _, chunk in plans.values()), plans
    assert f.info().device_bytes == before
    f.close()


def test_no_rows_and_a_table_of_another_width(env, knobs):
    ta, oracle, torch = env
    k = k1_like(env)
    f = ta.Forest(k["nodes"], k["T"], k["D"], k["cols"], missing=MISSING)
    empty = ta.Table([torch.empty(0, dtype=torch.float64, device="cuda") for _ in range(k["cols"])])
    assert empty.rows == 0
    out = f.predict_table(empty)
    assert tuple(out.shape) == (0,)
    one = torch.full((1,), 7.0, device="cuda")  # the library's own rows == 0: TAHOE_OK, nothing written
    assert ta.lib.tahoe_forest_predict_table(f._h, one.data_ptr(), empty._h, None) == 0 and one.item() == 7.0
    # rows == 0 behind an offset: the buffers hold elements, the table none
    behind = ta.Table([torch.zeros(7, dtype=torch.int16, device="cuda") for _ in range(k["cols"])], offsets=[7] * k["cols"])
    assert behind.rows == 0 and tuple(f.predict_table(behind).shape) == (0,)
    narrow = ta.Table([torch.zeros(5, dtype=torch.float32, device="cuda") for _ in range(k["cols"] - 1)])
    with pytest.raises(ValueError, match="columns"):
        f.predict_table(narrow)
    out = torch.zeros(5, device="cuda")
    status = ta.lib.tahoe_forest_predict_table(f._h, out.data_ptr(), narrow._h, None)  # the library's own refusal
    assert status == 1 and "tahoe_forest_predict_table" in ta.lib.tahoe_last_error().decode() and "num_cols" in ta.lib.tahoe_last_error().decode()
    assert ta.lib.tahoe_forest_predict_table(f._h, None, narrow._h, None) == 1 and "preds_dev" in ta.lib.tahoe_last_error().decode()
    for t in (empty, behind, narrow):
        t.close()
        t.close()  # twice is fine
    f.close()
