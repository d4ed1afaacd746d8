"""Category-set splits at the edges, on the GPU: every walk that reads a set against the closed form of tests/cat_edges.py -- leaf
indices and float32 bits, nothing compared with the code under test.  Needs an MI355X.

a. Every float32 form.  The CAT = true instantiations sparse.hip launches, how each is reached and what kernel_form() says:
     sparse_kernel<TILE = false>  DIRECT     "sparse_direct"      sparse_kernel<TILE = true>  ROWTILE    "sparse_rowtile"
     sparse_top_kernel<NW = 16>   TILEBLOCK  "sparse_top"         sparse_top_kernel<NW = 8>   TILEBLOCK  "sparse_top", 450 columns
   each with WRITE_LEAF (predict_leaf_idx; with and without sums) and without (predict_raw, predict_accumulate), with MC (three
   classes) and without, and with NANM (section e).  CSR / COLS / STAGED: section d.  kernel_form() does not tell 16 walker waves
   from 8: the tile of 450 columns leaves LDS (160 KiB) room for 8 only -- 450 * 256 B + 15 * 4 KiB + the ring is past it,
   with 7 * 4 KiB it fits -- and the test asserts "sparse_top" there.  AUTO resolves to one of the three forms.
b. Depth.  sparse_top_kernel holds the first kSTop = 512 compact nodes of a tree in LDS, breadth first with the root at position 1:
   9 complete levels.  A node is read from LDS when its position is below 512, else from global memory.  In a complete pilot tree
   of L levels the categorical node sits at position 2^(L+1) - 1: L = 7 -> 255 (inside, its leaves inside), L = 8 -> 511 (the last
   position of the last level held; its leaves at 512 / 513 come from global memory), L = 9 -> 1023 (the first level below), L = 10
   beyond.  In a chain of d pilots it sits at 2 d + 1: d = 254 -> 509, 255 -> 511, 256 -> 513, and 0 is the root.
c. The compact-node cut.  16383, 16384 and 16385 columns: the compact copy (14-bit fid beside kSCCat) exists up to 2^14 columns, but
   no kernel can read it there -- its 64-row tile needs 256 B of LDS per column, 4 MiB -- so TILEBLOCK and ROWTILE are refused
   at all three widths and AUTO runs sparse_direct, whose bits must be the closed form.  fid 16383 beside the kSCCat bit is
   therefore not reachable on the device; what is reachable (the widest TILEBLOCK handle, 450 columns, section a) is tested.
d. predict_host, predict_csr (entries dropped where missing, and all entries stored), predict_columns (strided and pointer table),
   predict_staged, predict_table (uint8 / int16 / int32 / int64 / uint64 / float64 category columns with nulls).
e. TAHOE_CREATE_NAN_MISSING.  f. Oblivious handles: inline and pooled records on adjacent levels.
g. The four explanation calls on stumps (tests/test_cat_shap_gpu.py's _stump and bars) and on two-level oblivious trees.

Sentinels: -999, 5.0 (a member of every all-ones set: missing wins), 0.0 (category 0 is missing), NaN and +inf (nothing is missing:
inf - inf is NaN, which is not <= 1e-6)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cat_edges as ce  # noqa: E402
import cat_shap_ref as cref  # noqa: E402
import oblivious_cat_ref as ocr  # noqa: E402
import oblivious_inter_ref as oir  # noqa: E402
import oblivious_iv_ref as oiv  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402
import sparse_shap_ref as ref  # noqa: E402
import test_cat_shap_gpu as cs  # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED = 7
U = 2.0 ** -24
FORMS = {"DIRECT": "sparse_direct", "ROWTILE": "sparse_rowtile", "TILEBLOCK": "sparse_top"}
FLOAT_FORMS = ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK")
N_NEIGHBOUR, N_ENDS = 14, 6
DEPTH_CHAIN, DEPTH_FULL = (0, 1, 2, 254, 255, 256, 257, 300), (1, 7, 8, 9, 10)


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def all_forests():
    import tahoe_amd as ta

    dt = ta.capi.SPARSE_NODE_DTYPE
    fs = ce.neighbour_forests(dt) + ce.ends_forests(dt)
    assert len(fs) == N_NEIGHBOUR + N_ENDS
    return fs


@functools.lru_cache(maxsize=None)
def case(i, missing, nan_missing=False):
    """(forest, rows, branches by the closed form); computed once and read-only"""
    f = all_forests()[i] if isinstance(i, int) else i
    data = f.rows(missing)
    right = f.goes_right(data, missing, nan_missing=nan_missing)
    for a in (data, right):
        a.setflags(write=False)
    return f, data, right


def make_handle(ta, f, missing, nc=1, nan_missing=False):
    """tahoe_sparse_forest_create_cat on the forest's own split arrays: the sets keep the word counts they were given"""
    h = ta.capi.SparseForest.__new__(ta.capi.SparseForest)
    h.params = ta.ForestParams(int(f.sn.size), 0, int(f.tr.size), f.cols, 0, 0, 0.0, 0.0, 0, missing)
    h._h = C.c_void_p()
    cats = ta.capi.CategoricalSplits(f.T, f.node.ctypes.data, f.offset.ctypes.data, f.words.ctypes.data, f.ml.ctypes.data)
    st = ta.lib.tahoe_sparse_forest_create_cat(C.byref(h._h), f.tr.ctypes.data, f.sn.ctypes.data, None, C.byref(h.params), nc,
                                               ta.CREATE_NAN_MISSING if nan_missing else 0, C.byref(cats))
    assert st == 0, ta.lib.tahoe_last_error().decode()
    h.num_trees, h.depth, h.num_cols, h.num_classes = f.T, 0, f.cols, nc
    return h


def accepted(ta, h):
    ok = []
    for name in FLOAT_FORMS:
        try:
            h.set_strategy(getattr(ta, "STRATEGY_" + name))
            ok.append(name)
        except ta.TahoeError as e:
            assert e.status == UNSUPPORTED, name
    return ok


def check_forms(env, f, data, right, missing, nc=1, nan_missing=False, batches=()):
    """predict_raw, predict_leaf_idx with and without sums, predict_accumulate from a non-zero start (one class) under AUTO, DIRECT,
    ROWTILE and TILEBLOCK; the whole batch and its first r rows for r in batches"""
    ta, torch = env
    rows = data.shape[0]
    want_leaf = f.expected_leaf(right)
    want = f.expected_sums(right, nc)
    init = (np.arange(rows) % 5 - 7).astype(np.float32)
    want_acc = f.expected_sums(right, 1, init) if nc == 1 else None
    h = make_handle(ta, f, missing, nc, nan_missing)
    assert h.num_classes == nc
    x = torch.from_numpy(np.array(data)).cuda()
    assert accepted(ta, h) == list(FLOAT_FORMS)
    for name in FLOAT_FORMS:
        h.set_strategy(getattr(ta, "STRATEGY_" + name))
        form = h.kernel_form(rows)
        assert form == FORMS[name] if name != "AUTO" else form in FORMS.values(), (name, form)
        raw = h.predict_raw(x)
        leaf, sums = h.predict_leaf_idx(x)
        leaf2, none = h.predict_leaf_idx(x, want_sums=False)
        h.check()
        got_leaf = bits(leaf)
        assert np.array_equal(got_leaf, want_leaf), (name, ce.first_mismatch(f, data, want_leaf, got_leaf))
        assert none is None and np.array_equal(bits(leaf2), want_leaf), (name, ce.first_mismatch(f, data, want_leaf, bits(leaf2)))
        assert tuple(raw.shape) == ((rows, nc) if nc > 1 else (rows,))
        assert np.array_equal(bits(raw), bits(want)), (name, f, "predict_raw")
        assert np.array_equal(bits(sums), bits(want)), (name, f, "predict_leaf_idx sums")
        if nc == 1:
            acc = torch.from_numpy(init.copy()).cuda()
            h.predict_accumulate(x, acc)
            assert np.array_equal(bits(acc), bits(want_acc)), (name, f, "predict_accumulate")
        for r in batches:
            xr = x[:r].contiguous()
            leaf, sums = h.predict_leaf_idx(xr)
            assert np.array_equal(bits(leaf), want_leaf[:r]), (name, r, ce.first_mismatch(f, data[:r], want_leaf[:r], bits(leaf)))
            assert np.array_equal(bits(sums), bits(want[:r])) and np.array_equal(bits(h.predict_raw(xr)), bits(want[:r])), (name, r)
        h.check()
    h.close()


# ------------------------------------------------------------------------------------------------ a: every float32 form
@pytest.mark.parametrize("s", range(len(ce.SENTINELS)), ids=[str(v) for v in ce.SENTINELS])
@pytest.mark.parametrize("i", range(N_NEIGHBOUR + N_ENDS))
def test_every_form_one_class(env, i, s):
    """Every forest under every sentinel; the short batches under one sentinel per neighbour forest and under all on the pool ends"""
    missing = ce.SENTINELS[s]
    f, data, right = case(i, missing)
    check_forms(env, f, data, right, missing, batches=ce.BATCHES if s == i % 5 or i >= N_NEIGHBOUR else ())


@pytest.mark.parametrize("i", range(N_NEIGHBOUR + N_ENDS))
def test_every_form_three_classes(env, i):
    missing = ce.SENTINELS[(i + 1) % 3]  # -999, 5.0, 0.0 in turn
    f, data, right = case(i, missing)
    assert f.T % 3 == 0
    check_forms(env, f, data, right, missing, nc=3, batches=(1, 65))


@pytest.mark.parametrize("missing", (-999.0, 0.0), ids=str)
@pytest.mark.parametrize("nc", [1, 3])
def test_the_widest_set(env, nc, missing):
    """One set of 2^19 words (categories up to 2^24 - 1) between small ones: the one large allocation of this file, 2 MiB."""
    import tahoe_amd as ta

    f, data, right = case(wide_forest(ta), missing)
    check_forms(env, f, data, right, missing, nc=nc, batches=(1, 65))


@functools.lru_cache(maxsize=None)
def wide_forest(ta):
    return ce.widest_forest(ta.capi.SPARSE_NODE_DTYPE)


@functools.lru_cache(maxsize=None)
def wide_row_forests(ta):
    dt = ta.capi.SPARSE_NODE_DTYPE
    a = ce.ends_forest(dt, ce.single(63), ce.single(63), 1, cols=450, fid_base=450 - 6)
    b = ce.depth_forest(dt, (0, 255, 256), (8, 9), cols=450, fid_base=450 - 6)
    return a, b


@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("which", [0, 1])
def test_eight_walker_tops_on_450_columns(env, which, nc):
    ta, _ = env
    f, data, right = case(wide_row_forests(ta)[which], 5.0)
    assert f.cols == 450 and max(f.fid) == 449
    check_forms(env, f, data, right, 5.0, nc=nc, batches=(65,))


# ------------------------------------------------------------------------------------------------ b: depth
@functools.lru_cache(maxsize=None)
def deep_forest(ta):
    return ce.depth_forest(ta.capi.SPARSE_NODE_DTYPE, DEPTH_CHAIN, DEPTH_FULL)


@pytest.mark.parametrize("missing", (-999.0, 0.0, 5.0), ids=str)
@pytest.mark.parametrize("nc", [1, 3])
def test_depth_of_the_categorical_node(env, nc, missing):
    ta, _ = env
    f, data, right = case(deep_forest(ta), missing)
    pos = [2 * t.d + 1 if t.shape == "chain" else (2 << t.d) - 1 for t in f.trees]  # compact position of the categorical node
    assert {1, 509, 511, 513, 255, 1023} <= set(pos) and max(pos) > 2000
    check_forms(env, f, data, right, missing, nc=nc, batches=ce.BATCHES)


# ------------------------------------------------------------------------------------------------ c: the compact-node cut
@pytest.mark.parametrize("num_cols", [16383, 16384, 16385])
def test_compact_node_cut(env, num_cols):
    ta, torch = env
    for f in ce.cut_forests(ta.capi.SPARSE_NODE_DTYPE, num_cols):
        assert f.cols == num_cols and num_cols - 1 in f.fid + [f.pilot_fid] and 0x2000 in f.fid
        data = f.rows(-999.0, min_rows=64)
        right = f.goes_right(data, -999.0)
        want_leaf, want = f.expected_leaf(right), f.expected_sums(right)
        h = make_handle(ta, f, -999.0)
        ok = accepted(ta, h)
        assert ok == ["AUTO", "DIRECT"], ok  # no 64-row tile of this width fits LDS, compact copy or not
        x = torch.from_numpy(data).cuda()
        for name in ok:
            h.set_strategy(getattr(ta, "STRATEGY_" + name))
            assert h.kernel_form(data.shape[0]) == "sparse_direct" and h.get_strategy(data.shape[0]) == ta.STRATEGY_DIRECT
            leaf, sums = h.predict_leaf_idx(x)
            raw = h.predict_raw(x)
            h.check()
            assert np.array_equal(bits(leaf), want_leaf), (name, ce.first_mismatch(f, data, want_leaf, bits(leaf)))
            assert np.array_equal(bits(sums), bits(want)) and np.array_equal(bits(raw), bits(want)), (name, f)
        h.close()


# ------------------------------------------------------------------------------------------------ d: other entry points
ENTRY_FORESTS = (0, 5, 12, N_NEIGHBOUR, N_NEIGHBOUR + 3, N_NEIGHBOUR + 4)


def csr_of(data, keep):
    indptr = np.zeros(data.shape[0] + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    return indptr, np.nonzero(keep)[1].astype(np.int32), data[keep]


@pytest.mark.parametrize("missing", (-999.0, 5.0, 0.0), ids=str)
@pytest.mark.parametrize("i", ENTRY_FORESTS)
def test_host_csr_columns_and_staged(env, i, missing):
    ta, torch = env
    f, data, right = case(i, missing)
    nc = 3 if f.T % 3 == 0 and i % 2 else 1
    rows = data.shape[0]
    want = f.expected_sums(right, nc)
    stages = sorted({1, f.T // nc // 2, f.T // nc})
    want_staged = np.stack([f.expected_sums(right, nc, num_trees=n * nc) for n in stages], axis=1)
    h = make_handle(ta, f, missing, nc)
    h.set_stages(stages)
    x = torch.from_numpy(np.array(data)).cuda()
    xt = torch.from_numpy(np.ascontiguousarray(data.T)).cuda()  # [cols, rows]: its transpose is the column-major batch
    dropped = csr_of(data, ~ce.is_missing(data, missing))  # an absent entry takes the default side
    stored = csr_of(data, np.ones(data.shape, bool))         # a stored sentinel is missing all the same, a stored 0.0 is category 0
    assert dropped[2].size < stored[2].size and (stored[2] == 0).any()
    for name in FLOAT_FORMS:
        h.set_strategy(getattr(ta, "STRATEGY_" + name))
        if nc == 1:
            host = h.predict_host(np.array(data), np.full(rows, 7.0, np.float32), chunk_rows=128)
            assert np.array_equal(bits(host), bits(want)), (name, "predict_host")
        for what, (indptr, indices, values) in (("dropped", dropped), ("stored", stored)):
            got = h.predict_csr(torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(), torch.from_numpy(values).cuda())
            assert np.array_equal(bits(got), bits(want)), (name, "predict_csr", what, h.csr_plan(rows, values.size))
        assert np.array_equal(bits(h.predict_columns(xt.t())), bits(want)), (name, "predict_columns", h.columns_plan(rows))
        assert np.array_equal(bits(h.predict_columns([c.clone() for c in xt])), bits(want)), (name, "predict_columns, pointers")
        assert np.array_equal(bits(h.predict_staged(x)), bits(want_staged)), (name, "predict_staged", h.staged_strategy(rows))
        h.check()
    h.close()


class Series:
    """What a cuDF Series publishes: __cuda_array_interface__ over device bytes, the validity bitmap as its `mask` entry"""

    def __init__(self, dev_bytes, dtype, n, mask=None):
        self.keep = (dev_bytes, mask)
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": np.dtype(dtype).str, "data": (dev_bytes.data_ptr(), False),
                                         "version": 3, "strides": None}
        if mask is not None:
            self.__cuda_array_interface__["mask"] = mask


@pytest.mark.parametrize("missing", (-999.0, 5.0, 0.0), ids=str)
@pytest.mark.parametrize("i", ENTRY_FORESTS[::2])
def test_typed_nullable_columns(env, i, missing):
    """Tree k's column has type TABLE_TYPES[k % 6]; every third element is null, whatever lies under it.  The table stands for the
    float32 matrix of (float)element; the closed form takes the nulls as missing by their mask, not by a sentinel written there."""
    ta, torch = env
    f = all_forests()[i]
    cols_np = [ce.typed_values(t.cset, ce.TABLE_TYPES[k % 6], missing) for k, t in enumerate(f.trees)]
    rows = max(c.size for c in cols_np) | 1
    cols_np = [np.roll(np.resize(c, rows), 5 * k) for k, c in enumerate(cols_np)]
    null = np.zeros((rows, f.cols), bool)
    M = np.full((rows, f.cols), 0.5, np.float32)
    M[:, f.pilot_fid] = 0.0
    columns, seen = [None] * f.cols, set()
    for c in range(f.cols):
        if c not in f.fid:
            columns[c] = torch.from_numpy(M[:, c].copy()).cuda()
            continue
        k = f.fid.index(c)
        a = cols_np[k]
        with np.errstate(over="ignore", invalid="ignore"):
            M[:, c] = a.astype(np.float32)
        null[:, c] = (np.arange(rows) + k) % 3 == 0
        mask = Series(torch.from_numpy(np.packbits(~null[:, c], bitorder="little")).cuda(), np.uint8, (rows + 7) // 8)
        columns[c] = Series(torch.from_numpy(a.view(np.uint8).copy()).cuda(), a.dtype, rows, mask=mask)
        seen.add(a.dtype.name)
        if a.dtype.kind == "i":
            assert (a < 0).any()
        if a.dtype.itemsize == 8 and a.dtype.kind != "f":
            assert {2 ** 24, 2 ** 24 + 1, 2 ** 40} <= set(a.tolist())
    assert seen == set(ce.TABLE_TYPES)
    right = f.goes_right(M, missing, null=null)
    under = f.goes_right(M, missing)
    assert (right != under).any()  # a null over a member (or a non-member) that would have gone the other way
    nc = 1 if i == 0 else 3
    want = f.expected_sums(right, nc)
    table = ta.capi.Table(columns)
    h = make_handle(ta, f, missing, nc)
    for name in FLOAT_FORMS:
        h.set_strategy(getattr(ta, "STRATEGY_" + name))
        got = h.predict_table(table)
        h.check()
        assert np.array_equal(bits(got), bits(want)), (name, f, h.table_plan(rows))
    h.close()
    table.close()


# ------------------------------------------------------------------------------------------------ e: NaN as a missing value
@pytest.mark.parametrize("missing", (-999.0, 5.0, float("nan")), ids=str)
@pytest.mark.parametrize("i", (0, 1, 6, 13) + tuple(range(N_NEIGHBOUR, N_NEIGHBOUR + N_ENDS)))
def test_nan_takes_the_default_side_on_a_flagged_handle(env, i, missing):
    f, data, right = case(i, missing, True)
    plain = case(i, missing)[2]
    nan = np.isnan(data[:, f.fid])
    assert nan.any() and np.array_equal(right[~nan], plain[~nan])  # everything else keeps its branch
    assert np.array_equal(right[nan], np.broadcast_to([not t.dl for t in f.trees], right.shape)[nan])
    pairs = {(t.ml, t.dl) for k, t in enumerate(f.trees) if nan[:, k].any()}
    assert pairs == set(ce.PAIRS)
    check_forms(env, f, data, right, missing, nc=1 if i % 2 else 3, nan_missing=True, batches=(1, 65))


# ------------------------------------------------------------------------------------------------ f: oblivious handles
@pytest.mark.parametrize("missing", (-999.0, 5.0, 0.0), ids=str)
def test_oblivious_inline_and_pooled_records_side_by_side(env, missing):
    ta, torch = env
    d = ce.oblivious_decoder()
    data = d.rows(missing)
    rows = data.shape[0]
    want_leaf = d.expected_leaf(data, missing)
    want = d.expected_sums(want_leaf)
    init = (np.arange(rows) % 5 - 7).astype(np.float32)
    want_acc = d.expected_sums(want_leaf, init)
    f = ta.ObliviousForest(d.depths, d.fids, np.full(len(d.levels), np.nan, np.float32), d.def_left, d.leaves, d.cols, missing=missing,
                           categories=d.cats, members_left=d.members_left)
    x = torch.from_numpy(data).cuda()
    for strat in ("DIRECT", "ROWTILE", "AUTO"):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert f.kernel_form(rows) == ("oblivious_direct" if strat == "DIRECT" else "oblivious_tile")
        for r in (rows,) + ce.BATCHES:
            xr = x[:r].contiguous()
            leaf, sums = f.predict_leaf_idx(xr)
            assert np.array_equal(bits(leaf), want_leaf[:r]), (strat, r, np.argwhere(bits(leaf) != want_leaf[:r])[:4])
            assert np.array_equal(bits(sums), bits(want[:r])) and np.array_equal(bits(f.predict_raw(xr)), bits(want[:r])), (strat, r)
        acc = torch.from_numpy(init.copy()).cuda()
        f.predict_accumulate(x, acc)
        assert np.array_equal(bits(acc), bits(want_acc)), strat
        f.check()
    f.close()


# ------------------------------------------------------------------------------------------------ g: explanation calls
STUMP_SETS = {"empty": [], "bit31": [31], "bit0": [0], "bit32": [32], "bit63": [63], "31+32": [31, 32],
              "33words": [31, 32, 63, 1055]}
M = cs.MISSING
STUMP_X = np.array([[c, v] for c in (31, 32, 63, 64, 0, -0.0, 30, 33, 62, 31.5, 1055, 1056, 1024, 1087, M, np.nan, -1, 2.0 ** 24, 95)
                    for v in (0, 1, M)][:-1], np.float32)


def stumps(ta, id_lists):
    """test_cat_shap_gpu._stump once per id list, as one forest"""
    parts = [cs._stump(ta, ids) for ids in id_lists]
    sn = np.concatenate([p[0].sn for p in parts])
    tr = np.arange(len(parts), dtype=np.int32) * 5
    forest = cref.CatForest(sn, tr, {5 * k: ids for k, ids in enumerate(id_lists)})
    return forest, np.concatenate([p[1] for p in parts])


@pytest.mark.parametrize("name", list(STUMP_SETS) + ["mixed_wave"])
def test_explanations_on_stumps(env, name):
    """word0 path (sets of at most one word), gather path (two words and more), and a forest whose path elements hold both kinds
    in one wave.  The bars are test_cat_shap_gpu.test_pool_edges's: (paths + 4 (depth + 2)) u scale, twice that for interactions."""
    ta, torch = env
    lists = [STUMP_SETS[name]] if name != "mixed_wave" else [[31], [31, 32, 63, 1055], [], [63], [0]]
    forest, cv = stumps(ta, lists)
    F, x = 2, STUMP_X
    bg = x[::-1][:5].copy()
    f = cs.make(ta, forest.sn, forest.tr, F, cv, forest.cats)
    phi, inter, iv, sa, raw = cs.run_all(env, f, x, bg)
    scale, depth, paths = ref.bound_scale(forest.sn, forest.tr, 1)
    tol = (paths + 4 * (depth + 2)) * U * scale
    want = cref.contribs(forest, cv, x, F, M)
    assert np.all(np.abs(phi[:, :, :F] - want[:, :, :F]) <= tol[None, :, None])
    want_v = cref.interventional(forest, x, bg, F, M, bg_raw=raw[::-1][:5])
    assert np.all(np.abs(iv[:, :, :F] - want_v[:, :, :F]) <= tol[None, :, None])
    assert np.all(np.abs(inter[:, :, 0, 1] - cref.interactions(forest, cv, x, F, M)[:, :, 0, 1]) <= 2 * tol[None, :])
    assert np.array_equal(bits(sa), bits(cref.saabas(forest, cv, F, x, M)))
    # the margins of the same handle, by the closed form of a stump: member -> the numeric node on f1, else the -1 leaf
    member = np.array([[ce.is_member(float(v), set(ids)) for ids in lists] for v in x[:, 0]])
    miss0, miss1 = ce.is_missing(x[:, 0], M), ce.is_missing(x[:, 1], M)
    with np.errstate(invalid="ignore"):
        below = np.where(np.where(miss1, False, x[:, 1] >= np.float32(0.5)), np.float32(2.0), np.float32(0.25))  # def_left
    want_raw = np.zeros(x.shape[0], np.float32)
    for k in range(len(lists)):
        want_raw = want_raw + np.where(np.where(miss0, True, member[:, k]), below, np.float32(-1.0))  # default right at the root
    assert np.array_equal(bits(raw[:, 0]), bits(want_raw))
    f.close()


def test_explanations_on_two_level_oblivious_trees(env):
    """The oblivious equivalent: trees of two set levels -- inline beside pooled, a 33-word set, an empty one -- at the bars of
    tests/test_oblivious_cat_gpu.py: TreeSHAP and interactions the bits of emulate and (N + 4 (D + 2)) / (N + 6 (D + 2)) u A
    against poly, Saabas bit for bit, interventional values (N + 8) u A."""
    ta, torch = env
    wide = ce.CatSet(33, [31, 32, 63, 1055], "33words")
    d = ce.ObliviousDecoder([[(ce.single(31), False, True), (ce.single(32), True, False)],
                             [(wide, False, False), (ce.empty(0), True, True)],
                             [(ce.CatSet(2, [0, 32], "0+32"), True, True), (ce.ones(1), False, False)]], "oblivious stumps")
    forest = d.forest()
    forest["leaves"] = np.random.default_rng(5).uniform(-1, 1, d.leaves.size).astype(np.float32)
    covers = osr.make_covers(forest, "int", seed=6)
    data, bg = d.rows(ocr.MISSING)[:130], d.rows(ocr.MISSING)[40:47]
    x, bgd = torch.from_numpy(data.copy()).cuda(), torch.from_numpy(bg.copy()).cuda()
    D, F = 2, d.cols
    with ocr.seam():
        poly, emulate, saabas = osr.poly(forest, covers, data), osr.emulate(forest, covers, data), osr.saabas(forest, covers, data)
        ipoly, iemulate = oir.poly(forest, covers, data), oir.emulate(forest, covers, data)
        ivp = oiv.paths(forest, data, bg, ocr.MISSING)
    kw = dict(missing=ocr.MISSING, leaf_covers=covers, categories=d.cats, members_left=d.members_left)
    args = (d.depths, d.fids, forest["thr"], d.def_left, forest["leaves"], d.cols)
    f = ta.ObliviousForest(*args, contribs=True, approx_contribs=True, interactions=True, interventional=True, **kw)
    shape = (data.shape[0], 1, F + 1)
    got = f.predict_contribs(x).cpu().numpy().reshape(shape)
    want, A, N = poly
    assert np.all(np.abs(got.astype(np.float64) - want)[:, :, :-1] <= ((N + 4 * (D + 2)) * U * A)[:, :, :-1])
    assert np.array_equal(bits(got), bits(emulate))
    assert np.array_equal(bits(f.predict_contribs_approx(x).cpu().numpy().reshape(shape)), bits(saabas))
    goti = f.predict_interactions(x).cpu().numpy().reshape(shape + (F + 1,))
    want, A, N = ipoly
    off = ~np.eye(F + 1, dtype=bool)
    assert np.all(np.abs(goti.astype(np.float64) - want)[..., off] <= ((N + 6 * (D + 2)) * U * A)[..., off])
    assert np.array_equal(bits(goti), bits(iemulate))
    f.set_background(bgd)
    gotv = f.predict_contribs_interventional(x).cpu().numpy().reshape(shape)
    want, A, N = ivp
    assert np.all(np.abs(gotv.astype(np.float64) - want)[:, :, :F] <= ((N + 8) * U * A)[:, :, :F])
    f.check()
    f.close()
