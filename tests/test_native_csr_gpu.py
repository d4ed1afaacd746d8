"""CSR rows on oblivious and vector-leaf handles created with TAHOE_CREATE_CSR (tahoe_forest_predict_csr, _reserve_csr,
_get_csr_plan).  Every comparison is for equal bits:
  - predict_csr against predict on the densified matrix, on the same handle;
  - where the output is raw, also against numpy: the reference walk's float32 sums on the densified matrix;
  - the plan (kernel form, rows per chunk) of every call, and the guard bands around its output and its three CSR arrays.
Shapes are the smallest at which the one-wave loader, the plumbing or the chunking can go wrong: 11 trees with a depth-0 tree first
and last; rows around the 64-row tile, with and without empty rows at the end; K across the 8-class block (9 stages the tile
twice); rows of 8 and 9 entries (the 8-lane stride); num_cols above the default 64 KiB of dynamic LDS, the last that fits the
device's LDS and the first that does not; three chunks with a ragged last one.  Needs an MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oblivious_cat_ref as ocr  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402
from guarded import Guarded, guarded_input  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = obr.MISSING
INVALID_ARG, UNSUPPORTED = 1, 7
INT32_MAX = 2 ** 31 - 1
T = 11
DEPTHS = [0, 3, 6, 1, 2, 5, 4, 6, 3, 2, 0]  # a depth-0 tree first and last
CAT_DEPTHS = [2, 0, 6, 1, 3, 5, 4, 6, 3, 2, 0]
KINDS = ["leaf", 5, "stump", 8, 3, 6, "leaf", 8, 2, 7, 4]  # irregular trees of depth <= 8, two single leaves
ALL_KINDS = ("oblivious", "cat", "vector")
TILE = {"oblivious": "oblivious_tile", "cat": "oblivious_tile", "vector": "vector_tile"}
DIRECT = {"oblivious": "oblivious_direct", "cat": "oblivious_direct", "vector": "vector_direct"}
FUSED = {"oblivious": "oblivious_csr_tile", "cat": "oblivious_csr_tile", "vector": "vector_csr_tile"}
assert len(DEPTHS) == len(CAT_DEPTHS) == len(KINDS) == T


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


# ---- the forests, computed once and read-only ----
_forests = {}


def forest_of(kind, cols, k):
    key = (kind, cols, k)
    if key not in _forests:
        seed = 3600 + 10 * cols + k
        if kind == "vector":
            _forests[key] = vr.make_named(KINDS, cols, k, seed)
        elif kind == "cat":
            _forests[key] = ocr.sets_forest(CAT_DEPTHS, cols, k, seed)
        else:
            _forests[key] = obr.make_forest(DEPTHS, cols, k, seed)
    return _forests[key]


def base_data(kind, rows, cols, seed):
    if kind == "vector":
        return vr.make_data(rows, cols, seed=seed)
    if kind == "cat":
        return ocr.sets_data(rows, cols, seed=seed)
    return obr.make_data(rows, cols, seed=seed)


def sparse_rows(kind, rows, cols, density, seed, empty_tail=0):
    """Rows of the kind's own data (ties on the thresholds, NaN, +-inf, the sentinel's neighbour) with a share `density` of the
    entries kept and the others missing; the last empty_tail rows hold nothing"""
    x = np.array(base_data(kind, rows, cols, seed), np.float32)
    x[np.random.default_rng(seed + 7).random(x.shape) >= density] = MISSING
    if empty_tail:
        x[rows - empty_tail:] = MISSING
    return x


def densify(indptr, indices, values, cols):
    x = np.full((indptr.size - 1, cols), MISSING, dtype=np.float32)
    for r in range(indptr.size - 1):
        x[r, indices[indptr[r]:indptr[r + 1]]] = values[indptr[r]:indptr[r + 1]]
    return x


def reference(kind, forest, dense):
    """The numpy walk's raw sums in the handle's output shape"""
    sums = (vr.vector_ref(forest, dense)[0] if kind == "vector" else
            ocr.cat_ref(forest, dense)[0] if kind == "cat" else obr.ref_of(forest, dense)[0])
    return sums[:, 0] if forest["k"] == 1 else sums


def handle(ta, forest, **kw):
    if "nodes" in forest:
        return ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=MISSING, **kw)
    if forest.get("cats"):
        kw.update(ocr.handle_args(forest))
    return ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], forest["cols"],
                              leaf_dim=forest["k"], missing=MISSING, **kw)


def csr_call(env, f, csr, dense, plan, tag, want_raw=None, rows_ok=None):
    """predict_csr into a guarded output from guarded CSR arrays.  The plan must be (form, chunked?); the output equals
    predict(dense) on the same handle and, where given, the numpy sums, on the rows of rows_ok (default: all)."""
    ta, torch = env
    indptr, indices, values = csr
    rows = indptr.size - 1
    form, chunk = f.csr_plan(rows, values.size)
    assert (form, chunk > 0) == plan, (tag, form, chunk)
    ip = guarded_input(torch, indptr, torch.int64, device="cuda")
    ix = guarded_input(torch, indices, torch.int32, device="cuda")
    vals = guarded_input(torch, values, torch.float32, device="cuda")
    out = Guarded(torch, f._out_shape(rows), torch.float32, device="cuda")
    f.predict_csr(ip.view, ix.view, vals.view, out=out.view)
    torch.cuda.synchronize()
    got = bits(out.check("predict_csr: " + tag))
    for g, what in ((ip, "indptr"), (ix, "indices"), (vals, "values")):
        g.check_unchanged(f"{what}: {tag}")
    ok = slice(None) if rows_ok is None else rows_ok
    want = bits(f.predict(torch.from_numpy(np.ascontiguousarray(dense)).cuda()))
    assert np.array_equal(got[ok], want[ok]), "predict_csr != predict(densified): " + tag
    if want_raw is not None:
        assert np.array_equal(got[ok], bits(want_raw)[ok]), "predict_csr != numpy: " + tag
    return got, chunk


def every_strategy(env, f, kind, csr, dense, tag, want_raw=None):
    """Forced ROWTILE and AUTO take the fused form, forced DIRECT the direct kernel on chunks"""
    ta, _ = env
    for strat, plan in (("ROWTILE", (FUSED[kind], False)), ("AUTO", (FUSED[kind], False)), ("DIRECT", (DIRECT[kind], True))):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        csr_call(env, f, csr, dense, plan, f"{tag}, {strat}", want_raw)
    f.check()


# ------------------------------------------------------------------------------------------ kinds, K and columns
@pytest.mark.parametrize("k", [1, 3, 8, 9])
@pytest.mark.parametrize("cols", [1, 7, 8])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_kinds_classes_and_columns(env, kind, cols, k):
    ta, _ = env
    forest = forest_of(kind, cols, k)
    if kind == "cat":
        widths = [ocr.nwords_of(c) for c in forest["cats"].values()]
        assert any(w <= 1 for w in widths) and any(w >= 2 for w in widths)  # sets in their record and sets in the pool
    x = sparse_rows(kind, 130, cols, 0.3, seed=11)
    csr = ta.dense_to_csr(x, MISSING)
    dense = densify(*csr, cols)
    f = handle(ta, forest, csr=True)
    every_strategy(env, f, kind, csr, dense, f"{kind} cols {cols} K {k}", reference(kind, forest, dense))
    f.close()


# ------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_rows_around_the_tile_and_empty_rows_at_the_end(env, kind, rows):
    ta, _ = env
    cols, k = 7, 3
    forest = forest_of(kind, cols, k)
    f = handle(ta, forest, csr=True)
    for tail in sorted({0, min(3, rows - 1)}):  # ... and a batch whose last rows are empty
        x = sparse_rows(kind, rows, cols, 0.3, seed=20 + rows, empty_tail=tail)
        csr = ta.dense_to_csr(x, MISSING)
        if tail:
            assert (np.diff(csr[0])[-tail:] == 0).all()
        dense = densify(*csr, cols)
        every_strategy(env, f, kind, csr, dense, f"{kind} rows {rows}, {tail} empty at the end", reference(kind, forest, dense))
    f.close()


# ------------------------------------------------------------------------------------------ density
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_densities_and_the_edge_of_the_eight_lane_stride(env, kind):
    ta, _ = env
    cols, k, rows = 12, 3, 130
    forest = forest_of(kind, cols, k)
    f = handle(ta, forest, csr=True)
    for density in (0.0, 0.05, 0.3, 1.0):
        x = sparse_rows(kind, rows, cols, density, seed=31)
        csr = ta.dense_to_csr(x, MISSING)
        if density == 0.0:
            assert csr[1].size == 0 and csr[2].size == 0  # nnz == 0: indices_dev and values_dev go in as NULL
        dense = densify(*csr, cols)
        every_strategy(env, f, kind, csr, dense, f"{kind} density {density}", reference(kind, forest, dense))
    # a row of exactly 8 entries and one of 9, between rows of other lengths
    x = np.array(base_data(kind, rows, cols, 32), np.float32)
    x[np.abs(x - np.float32(MISSING)) <= 1e-6] = 0.5  # (every entry stored, so that the counts below are exact)
    x[5, 8:] = MISSING
    x[6, 9:] = MISSING
    x[70, :4] = MISSING
    x[71, 1:] = MISSING
    csr = ta.dense_to_csr(x, MISSING)
    assert list(np.diff(csr[0])[[5, 6, 70, 71]]) == [8, 9, 8, 1]
    dense = densify(*csr, cols)
    every_strategy(env, f, kind, csr, dense, f"{kind} rows of 8 and 9 entries", reference(kind, forest, dense))
    f.close()


# ------------------------------------------------------------------------------------------ AUTO with the fused path switched off
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_auto_without_the_fused_path_runs_the_tile_kernel_on_chunks(env, kind, monkeypatch):
    ta, _ = env
    cols, k = 8, 9
    monkeypatch.setenv("TAHOE_CSR_FUSED", "0")  # (read at create)
    forest = forest_of(kind, cols, k)
    f = handle(ta, forest, csr=True)
    x = sparse_rows(kind, 130, cols, 0.3, seed=41)
    csr = ta.dense_to_csr(x, MISSING)
    dense = densify(*csr, cols)
    csr_call(env, f, csr, dense, (TILE[kind], True), f"{kind} AUTO, TAHOE_CSR_FUSED=0", reference(kind, forest, dense))
    f.set_strategy(ta.STRATEGY_ROWTILE)  # a forced strategy is honoured whatever the knob says
    csr_call(env, f, csr, dense, (FUSED[kind], False), f"{kind} ROWTILE, TAHOE_CSR_FUSED=0", reference(kind, forest, dense))
    f.check()
    f.close()


@pytest.mark.parametrize("cols,k,fused", [(96, 3, True), (97, 3, False), (48, 9, True), (49, 9, False)])
@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_auto_leaves_rows_of_many_entries_to_the_chunks(env, kind, cols, k, fused):
    """AUTO's second rule: the fused form while nnz x (blocks of 8 classes) <= 96 x rows; a forced ROWTILE stays fused"""
    ta, _ = env
    forest = forest_of(kind, cols, k)
    f = handle(ta, forest, csr=True)
    x = np.array(base_data(kind, 65, cols, 45), np.float32)
    x[np.abs(x - np.float32(MISSING)) <= 1e-6] = 0.5  # every entry stored: cols entries per row
    csr = ta.dense_to_csr(x, MISSING)
    assert csr[2].size == 65 * cols
    dense = densify(*csr, cols)
    want = reference(kind, forest, dense)
    csr_call(env, f, csr, dense, (FUSED[kind], False) if fused else (TILE[kind], True), f"{kind} AUTO, {cols} entries per row, K {k}", want)
    f.set_strategy(ta.STRATEGY_ROWTILE)
    csr_call(env, f, csr, dense, (FUSED[kind], False), f"{kind} ROWTILE, {cols} entries per row, K {k}", want)
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------ tiles above 64 KiB, the LDS limit
def lds_cols(ta):
    lds = C.c_int(0)
    assert ta.lib.tahoe_device_lds_bytes(C.byref(lds)) == 0
    return lds.value // 256  # one 64-row float32 tile is 256 bytes per column: 640 columns on an MI355X


@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_a_tile_above_the_default_dynamic_lds(env, kind, k):
    """num_cols = 300: a tile of 76 800 B.  Every CSR instantiation (KB = 1 / 8, with and without sets, vector) needs the
    max-LDS attribute of its own, or its launch fails."""
    ta, _ = env
    cols = 300
    assert cols * 256 > 65536 and cols <= lds_cols(ta)
    forest = forest_of(kind, cols, k)
    f = handle(ta, forest, csr=True)
    f.set_strategy(ta.STRATEGY_ROWTILE)
    x = sparse_rows(kind, 65, cols, 0.05, seed=51)
    csr = ta.dense_to_csr(x, MISSING)
    dense = densify(*csr, cols)
    csr_call(env, f, csr, dense, (FUSED[kind], False), f"{kind} cols {cols} K {k}", reference(kind, forest, dense))
    f.check()
    f.close()


@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_the_last_tile_that_fits_and_the_first_that_does_not(env, kind):
    ta, _ = env
    k, fit = 3, lds_cols(ta)
    for cols, fits in ((fit, True), (fit + 1, False)):
        forest = forest_of(kind, cols, k)
        f = handle(ta, forest, csr=True)
        x = sparse_rows(kind, 65, cols, 0.05, seed=52)
        csr = ta.dense_to_csr(x, MISSING)
        dense = densify(*csr, cols)
        want = reference(kind, forest, dense)
        if fits:
            every_strategy(env, f, kind, csr, dense, f"{kind} cols {cols}", want)
        else:
            with pytest.raises(ta.TahoeError) as e:
                f.set_strategy(ta.STRATEGY_ROWTILE)
            assert e.value.status == UNSUPPORTED
            for strat in ("AUTO", "DIRECT"):
                f.set_strategy(getattr(ta, "STRATEGY_" + strat))
                csr_call(env, f, csr, dense, (DIRECT[kind], True), f"{kind} cols {cols}, {strat}", want)
            f.check()
        f.close()


# ------------------------------------------------------------------------------------------ chunking
@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_three_chunks_with_a_ragged_last_one(env, kind, k, monkeypatch):
    ta, _ = env
    cols = 640
    monkeypatch.setenv("TAHOE_CSR_CHUNK_MB", "1")  # (read at create)
    forest = forest_of(kind, cols, k)
    f = handle(ta, forest, csr=True)
    f.set_strategy(ta.STRATEGY_DIRECT)
    chunk = f.csr_plan(1 << 20, 0)[1]
    assert 64 <= chunk <= (1 << 20) // (4 * cols)
    rows = 2 * chunk + 65  # the output pointer moves by r0 x K
    x = sparse_rows(kind, rows, cols, 0.02, seed=61)
    csr = ta.dense_to_csr(x, MISSING)
    dense = densify(*csr, cols)
    before = f.info().device_bytes
    _, got_chunk = csr_call(env, f, csr, dense, (DIRECT[kind], True), f"{kind} K {k}, {rows} rows in chunks of {chunk}",
                            reference(kind, forest, dense))
    assert got_chunk == chunk and f.info().device_bytes == before + chunk * cols * 4  # the chunk buffer, and nothing else
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_stored_values_column_order_and_index_types(env, kind):
    ta, torch = env
    cols, k, rows = 8, 3, 70
    forest = forest_of(kind, cols, k)
    f = handle(ta, forest, csr=True)
    # every value stored: the sentinel (missing all the same), NaN (goes left) and -0.0 (stays -0.0) among them
    dense = np.array(base_data(kind, rows, cols, 71), np.float32)
    dense[0, :3] = [MISSING, np.nan, -0.0]
    dense[65, -3:] = [-0.0, MISSING, np.nan]
    assert (dense == np.float32(MISSING)).any() and np.isnan(dense).any() and (np.signbit(dense) & (dense == 0)).any()
    indptr = np.arange(0, rows * cols + 1, cols, dtype=np.int64)
    indices = np.tile(np.arange(cols, dtype=np.int32), rows)
    want = reference(kind, forest, dense)
    every_strategy(env, f, kind, (indptr, indices, dense.reshape(-1).copy()), dense, f"{kind} all stored", want)
    # column ids in descending order
    every_strategy(env, f, kind, (indptr, indices.reshape(rows, cols)[:, ::-1].reshape(-1).copy(),
                                  dense[:, ::-1].reshape(-1).copy()), dense, f"{kind} descending ids", want)
    # indptr as int32 and indices as int64 (predict_csr casts them), and a torch.sparse_csr_tensor
    x = sparse_rows(kind, rows, cols, 0.3, seed=72)
    ip, ix, vals = ta.dense_to_csr(x, MISSING)
    sparse_dense = densify(ip, ix, vals, cols)
    xd = torch.from_numpy(sparse_dense).cuda()
    ipd, ixd, vd = (torch.from_numpy(a).cuda() for a in (ip, ix, vals))
    for strat in ("ROWTILE", "DIRECT"):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        want_bits = bits(f.predict(xd))
        assert np.array_equal(want_bits, bits(reference(kind, forest, sparse_dense)))
        assert np.array_equal(bits(f.predict_csr(ipd.to(torch.int32), ixd.to(torch.int64), vd)), want_bits), strat
        t = torch.sparse_csr_tensor(ipd, ixd.to(torch.int64), vd, size=(rows, cols))
        assert np.array_equal(bits(f.predict_csr(t)), want_bits), strat
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------ containment
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_bad_column_ids_are_skipped_and_reported_once(env, kind):
    ta, torch = env
    cols, k, rows = 8, 9, 130
    forest = forest_of(kind, cols, k)
    f = handle(ta, forest, csr=True)
    x = sparse_rows(kind, rows, cols, 0.5, seed=81)
    x[[3, 64, 129]] = np.float32([0.25, -1.0, 2.0, 0.5, 1.0, -2.0, 0.0, -0.5])  # (the rows with a bad entry: every column stored)
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    dense = densify(indptr, indices, values, cols)
    bad, skipped = indices.copy(), dense.copy()
    for r, col in ((3, -1), (64, cols), (129, INT32_MAX)):
        lo = int(indptr[r])
        assert indptr[r + 1] - lo >= 2  # the row's other entries count
        skipped[r, indices[lo]] = MISSING  # the skipped entry's column reads the sentinel
        bad[lo] = col
    want = reference(kind, forest, skipped)
    for strat, plan in (("ROWTILE", (FUSED[kind], False)), ("DIRECT", (DIRECT[kind], True))):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        form, chunk = f.csr_plan(rows, values.size)
        assert (form, chunk > 0) == plan
        ip = guarded_input(torch, indptr, torch.int64, device="cuda")
        ix = guarded_input(torch, bad, torch.int32, device="cuda")
        vals = guarded_input(torch, values, torch.float32, device="cuda")
        out = Guarded(torch, f._out_shape(rows), torch.float32, device="cuda")
        f.predict_csr(ip.view, ix.view, vals.view, out=out.view)  # returns OK: the bad entries are predicated off
        with pytest.raises(ta.TahoeError) as e:
            f.check()
        assert e.value.status == INVALID_ARG and "column" in str(e.value), str(e.value)
        f.check()  # reported once
        got = bits(out.check(f"bad columns, {strat}"))
        assert np.array_equal(got, bits(want)), strat
        assert np.array_equal(got, bits(f.predict(torch.from_numpy(skipped).cuda()))), strat
        csr_call(env, f, (indptr, indices, values), dense, plan, f"{kind} clean call after bad columns, {strat}")
        f.check()  # a clean call checks OK again
    f.close()


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_indptr_is_clamped_to_nnz(env, kind):
    ta, _ = env
    cols, k, rows = 8, 3, 130
    forest = forest_of(kind, cols, k)
    f = handle(ta, forest, csr=True)
    x = sparse_rows(kind, rows, cols, 0.3, seed=91)
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    wild = indptr.copy()
    wild[70] = -5        # row 69 ends before it begins, row 70 starts at a negative offset: clamped to 0
    wild[-1] = 1 << 40   # the last row claims entries far past nnz: clamped to nnz
    ok = np.ones(rows, dtype=bool)
    ok[[69, 70]] = False
    dense = densify(indptr, indices, values, cols)
    want = reference(kind, forest, dense)
    for strat, plan in (("ROWTILE", (FUSED[kind], False)), ("DIRECT", (DIRECT[kind], True))):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        csr_call(env, f, (wild, indices, values), dense, plan, f"{kind} wild indptr, {strat}", want, rows_ok=ok)
        f.check()  # in-range columns only: nothing to report, nothing read or written out of bounds
    f.close()


# ------------------------------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_a_row_alone_and_inside_a_batch(env, kind):
    ta, torch = env
    cols, k, rows = 8, 9, 130
    forest = forest_of(kind, cols, k)
    f = handle(ta, forest, csr=True)
    x = sparse_rows(kind, rows, cols, 0.4, seed=101)
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    ip, ix, vals = (torch.from_numpy(a).cuda() for a in (indptr, indices, values))
    for strat in ("ROWTILE", "DIRECT"):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        batch = bits(f.predict_csr(ip, ix, vals))
        for r in (0, 63, 64, 129):
            lo, hi = int(indptr[r]), int(indptr[r + 1])
            one = torch.tensor([0, hi - lo], dtype=torch.int64, device="cuda")
            alone = bits(f.predict_csr(one, ix[lo:hi], vals[lo:hi]))
            assert np.array_equal(alone[0], batch[r]), (strat, r)
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------ reserve_csr
@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_reserve_csr_then_calls_allocate_nothing(env, kind):
    ta, torch = env
    cols, k, rows = 8, 3, 130
    forest = forest_of(kind, cols, k)
    x = sparse_rows(kind, rows, cols, 0.3, seed=111)
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    ip, ix, vals = (torch.from_numpy(a).cuda() for a in (indptr, indices, values))
    want = bits(reference(kind, forest, densify(indptr, indices, values, cols)))
    for strat in ("ROWTILE", "DIRECT"):
        f = handle(ta, forest, csr=True)
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        f.reserve(rows)  # (nothing to size)
        f.reserve_csr(rows, values.size)
        before = f.info().device_bytes
        a = f.predict_csr(ip, ix, vals)
        b = f.predict_csr(ip[:66], ix, vals)  # a smaller batch of the same arrays
        assert f.info().device_bytes == before, strat
        assert np.array_equal(bits(a), want) and np.array_equal(bits(b), want[:65]), strat
        f.check()
        f.close()
        g = handle(ta, forest, csr=True)  # without reserve_csr: the second of two equal calls allocates nothing
        g.set_strategy(getattr(ta, "STRATEGY_" + strat))
        a = g.predict_csr(ip, ix, vals)
        before = g.info().device_bytes
        b = g.predict_csr(ip, ix, vals)
        assert g.info().device_bytes == before, strat
        assert np.array_equal(bits(a), want) and np.array_equal(bits(b), want), strat
        g.check()
        g.close()


# ------------------------------------------------------------------------------------------ beside the other flags
def csr_refusals(ta, torch, f, rows, word):
    """The three CSR calls on a handle without the flag: today's codes and texts, nothing written"""
    ip = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    out = torch.full((rows * f.num_classes,), 7.0, device="cuda")
    form, chunk = C.c_int(-1), C.c_size_t(99)
    for name, call in (("tahoe_forest_predict_csr", lambda: ta.lib.tahoe_forest_predict_csr(f._h, out.data_ptr(), ip.data_ptr(), None, None, rows, 0, None)),
                       ("tahoe_forest_reserve_csr", lambda: ta.lib.tahoe_forest_reserve_csr(f._h, rows, 0)),
                       ("tahoe_forest_get_csr_plan", lambda: ta.lib.tahoe_forest_get_csr_plan(f._h, rows, 0, C.byref(form), C.byref(chunk)))):
        assert call() == UNSUPPORTED, name
        msg = ta.lib.tahoe_last_error().decode()
        assert msg.startswith(f"{name}: not served on a") and word in msg, msg
    assert form.value == 0 and chunk.value == 0  # TAHOE_FORM_NONE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_beside_staged_and_contribs(env, kind):
    ta, torch = env
    cols, k, rows = 8, 3, 130
    forest = forest_of(kind, cols, k)
    if kind == "vector":
        covers = dict(covers=vsr.consistent_covers(forest, 5))
    else:
        covers = dict(leaf_covers=np.random.default_rng(5).integers(0, 50, int((1 << np.asarray(DEPTHS, np.int64)).sum())).astype(np.float32))
    x = sparse_rows(kind, rows, cols, 0.3, seed=121)
    csr = ta.dense_to_csr(x, MISSING)
    dense = densify(*csr, cols)
    xd = torch.from_numpy(dense).cuda()
    rounds = [1, 4, 7, 11]
    for other in (dict(staged=True), dict(contribs=True, **covers), dict(staged=True, contribs=True, **covers)):
        both, without = handle(ta, forest, csr=True, **other), handle(ta, forest, **other)
        assert both.info().device_bytes == without.info().device_bytes  # the flag builds no table
        calls = [lambda f: f.predict(xd), lambda f: f.predict_raw(xd), lambda f: f.predict_leaf_idx(xd)[0],
                 lambda f: f.predict_leaf_idx(xd)[1]]
        if other.get("staged"):
            both.set_stages(rounds)
            without.set_stages(rounds)
            calls.append(lambda f: f.predict_staged(xd))
        if other.get("contribs"):
            calls.append(lambda f: f.predict_contribs(xd))
        for i, call in enumerate(calls):
            assert np.array_equal(bits(call(both)), bits(call(without))), (other.keys(), i)
        assert both.info().device_bytes == without.info().device_bytes  # ... and no call but a chunked CSR one allocates for it
        every_strategy(env, both, kind, csr, dense, f"{kind} beside {sorted(other)}", reference(kind, forest, dense))
        # a handle without the flag refuses the three calls as it always has, whatever else it carries
        csr_refusals(ta, torch, without, rows, "oblivious" if kind == "oblivious" else "vector-leaf")
        for f in (both, without):
            f.check()
            f.close()


# ------------------------------------------------------------------------------------------ output bits
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_output_bits(env, kind):
    ta, _ = env
    cols, rows = 8, 130
    for k, kw in ((1, dict(output=ta.OUT_AVG | ta.OUT_SIGMOID)),
                  (3, dict(output=ta.OUT_SOFTMAX | ta.OUT_AVG, global_bias=0.375))):
        forest = forest_of(kind, cols, k)
        f = handle(ta, forest, csr=True, **kw)
        x = sparse_rows(kind, rows, cols, 0.3, seed=131)
        csr = ta.dense_to_csr(x, MISSING)
        every_strategy(env, f, kind, csr, densify(*csr, cols), f"{kind} K {k} {kw}")
        f.close()
