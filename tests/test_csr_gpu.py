"""CSR rows on the GPU: Forest.predict_csr(csr) against Forest.predict(the densified rows) on the same handle, bit for bit --
no tolerance anywhere.  Dense, multi-class, sparse, multi-class sparse and categorical handles under every strategy their
set_strategy accepts, the fused tile kernels and the chunked fallback, edge rows, stored sentinel / NaN / -0.0, unsorted
column ids, chunk counts, bad column ids (contained, reported once), reserve_csr and batch independence.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
ALL = ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK", "TILERING", "QRING")
FUSED_FORMS = ("csr_rowtile", "csr_sparse_rowtile", "csr_sparse_top")
ROW_COUNTS = (1, 63, 64, 65, 3001)


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def densify(indptr, indices, values, cols):
    x = np.full((indptr.size - 1, cols), MISSING, dtype=np.float32)
    for r in range(indptr.size - 1):
        x[r, indices[indptr[r]:indptr[r + 1]]] = values[indptr[r]:indptr[r + 1]]
    return x


def sparse_rows(ta, rows, cols, density, seed):
    """synth_data (a few NaN) with a `density` share of the entries kept, the rest the sentinel."""
    x = ta.synth_data(rows, cols, seed=seed, nan_prob=0.01)
    if density < 1.0:
        x[np.random.default_rng(seed).random((rows, cols)) >= density] = MISSING
    return x


def to_dev(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def strategies(ta, f, names=ALL):
    """The strategies of `names` that this handle's set_strategy accepts (the handle is left on the last one)."""
    ok = []
    for name in names:
        try:
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            ok.append(name)
        except ta.TahoeError as e:
            assert e.status == 7, str(e)
    return ok


def same_bits(ta, torch, f, x, names, label=""):
    """predict_csr against predict on the densified rows under each named strategy; returns the CSR forms the calls took."""
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    dense = densify(indptr, indices, values, x.shape[1])
    xd, ip, ix, vals = to_dev(torch, dense, indptr, indices, values)
    forms = {}
    for name in names:
        f.set_strategy(getattr(ta, "STRATEGY_" + name))
        want = f.predict(xd)
        got = f.predict_csr(ip, ix, vals)
        f.check()
        forms[name] = f.csr_plan(x.shape[0], values.size)
        assert got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), (label, name, forms[name], x.shape)
    return forms


@pytest.mark.parametrize("shape", [(500, 8, 18), (200, 6, 500)], ids=["k1_like", "wide500"])
def test_dense_handle_every_strategy_density_and_row_count(env, shape):
    ta, torch = env
    T, D, cols = shape
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=11, leaf_prob=0.05), T, D, cols, missing=MISSING, output=ta.OUT_AVG | ta.OUT_SIGMOID,
                  global_bias=0.25)
    names = strategies(ta, f)
    assert "ROWTILE" in names and "QRING" in names and "DIRECT" in names, names  # (500 columns: the 64-row tile still fits LDS)
    for density in (0.0, 0.01, 0.3, 1.0):
        for rows in ROW_COUNTS:
            forms = same_bits(ta, torch, f, sparse_rows(ta, rows, cols, density, seed=rows + int(100 * density)), names,
                              label=f"density {density}")
            assert forms["ROWTILE"] == ("csr_rowtile", 0)          # forced tile strategy: the fused kernel
            assert forms["QRING"][1] > 0 and forms["DIRECT"][0] == "direct" and forms["DIRECT"][1] > 0  # the chunked fallback
    f.close()


@pytest.mark.parametrize("cols", [13, 30, 257])
def test_columns_not_a_multiple_of_four(env, cols):
    ta, torch = env
    T, D = 60, 5
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=3), T, D, cols, missing=MISSING)
    names = strategies(ta, f)
    for rows in (65, 1000):
        same_bits(ta, torch, f, sparse_rows(ta, rows, cols, 0.2, seed=cols + rows), names)
    f.close()


def test_columns_above_the_tile_limit_take_the_fallback(env):
    ta, torch = env
    T, D, cols = 20, 5, 3072
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=5), T, D, cols, missing=MISSING)
    with pytest.raises(ta.TahoeError):
        f.set_strategy(ta.STRATEGY_ROWTILE)
    names = strategies(ta, f)
    assert "ROWTILE" not in names and "AUTO" in names
    forms = same_bits(ta, torch, f, sparse_rows(ta, 700, cols, 0.02, seed=6), names)
    assert all(form not in FUSED_FORMS and chunk > 0 for form, chunk in forms.values()), forms
    f.close()


def test_multiclass_softmax(env):
    ta, torch = env
    T, D, cols, nc = 90, 6, 40, 3
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=7, leaf_prob=0.05), T, D, cols, missing=MISSING, output=ta.OUT_SOFTMAX | ta.OUT_AVG,
                  global_bias=-0.5, num_classes=nc)
    names = strategies(ta, f)
    assert set(names) == {"AUTO", "DIRECT", "ROWTILE", "QRING"}
    for rows in (1, 65, 2000):
        forms = same_bits(ta, torch, f, sparse_rows(ta, rows, cols, 0.1, seed=rows), names)
        assert forms["ROWTILE"] == ("csr_rowtile", 0)
    f.close()


@pytest.mark.parametrize("num_classes", [1, 4])
def test_sparse_handle_all_five_strategies(env, num_classes):
    ta, torch = env
    T, cols = 120, 64
    sn, tr = ta.capi.synth_sparse_forest(T, cols, 4, 24, 0.32, 65535, 44)
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, num_classes=num_classes,
                             output=ta.OUT_SOFTMAX if num_classes > 1 else ta.OUT_SIGMOID)
    names = strategies(ta, f, ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK", "QRING"))
    assert len(names) == 5, names
    for density in (0.0, 0.05, 1.0):
        for rows in (1, 64, 65, 2500):
            forms = same_bits(ta, torch, f, sparse_rows(ta, rows, cols, density, seed=rows + 7), names)
            assert forms["ROWTILE"] == ("csr_sparse_rowtile", 0) and forms["TILEBLOCK"] == ("csr_sparse_top", 0)
            assert forms["QRING"][1] > 0 and forms["DIRECT"][1] > 0
    f.close()


def test_categorical_handle_with_the_reference_on_a_slice(env):
    ta, torch = env
    cols, feats, T = 32, [1, 5, 9, 17, 30], 60
    sn, tr = ta.capi.synth_sparse_forest(T, cols, 4, 16, 0.32, 65535, 11)
    rng = np.random.default_rng(11)
    b = sn["bits"].view(np.uint32)
    inner = np.flatnonzero((b >> 31) == 0)
    chosen = inner[np.isin(b[inner] & ((1 << 30) - 1), feats)]
    cats = {int(i): rng.choice(300, size=int(rng.integers(1, 200)), replace=False) for i in chosen}
    ml = {int(i) for i in chosen if rng.random() < 1 / 3}
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, categories=cats, members_left=ml)
    rows = 1500
    x = sparse_rows(ta, rows, cols, 0.3, seed=12)
    for c in feats:  # categories, non-integers, -0.0 and NaN among the stored values of the categorical columns
        v = rng.integers(0, 320, rows).astype(np.float32)
        v[rng.random(rows) < 0.1] += np.float32(0.5)
        v[rng.random(rows) < 0.05] = np.float32(-0.0)
        v[rng.random(rows) < 0.05] = np.float32(np.nan)
        x[:, c] = np.where(x[:, c] == np.float32(MISSING), x[:, c], v)
    names = strategies(ta, f, ("AUTO", "DIRECT", "ROWTILE", "TILEBLOCK"))
    assert len(names) == 4
    forms = same_bits(ta, torch, f, x, names)
    assert forms["TILEBLOCK"] == ("csr_sparse_top", 0) and forms["ROWTILE"] == ("csr_sparse_rowtile", 0)
    # a second opinion on a slice: the numpy reference on the densified rows
    _, (node, offset, words, mla) = ta.capi.pack_categorical(cats, ml)
    indptr, indices, values = ta.dense_to_csr(x[:200], MISSING)
    want, _ = categorical_ref.predict(sn, tr, densify(indptr, indices, values, cols), MISSING, node, offset, words, mla)
    for name in names:
        f.set_strategy(getattr(ta, "STRATEGY_" + name))
        got = f.predict_csr(*to_dev(torch, indptr, indices, values))
        f.check()
        assert np.array_equal(bits(got), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)), name
    f.close()


def test_all_rows_empty_and_one_row_holding_every_column(env):
    ta, torch = env
    T, D, cols = 50, 6, 100
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=2), T, D, cols, missing=MISSING)
    names = strategies(ta, f)
    empty = np.full((130, cols), MISSING, dtype=np.float32)
    same_bits(ta, torch, f, empty, names, "all rows empty")
    one = empty.copy()
    one[77] = ta.synth_data(1, cols, seed=9)[0]
    assert ta.dense_to_csr(one, MISSING)[0][-1] == cols
    same_bits(ta, torch, f, one, names, "one full row")
    # nnz == 0 through the C ABI with NULL entry arrays
    ip = torch.zeros(131, dtype=torch.int64, device="cuda")
    f.set_strategy(ta.STRATEGY_AUTO)
    got = f.predict_csr(ip, torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.float32, device="cuda"))
    assert np.array_equal(bits(got), bits(f.predict(torch.from_numpy(empty).cuda())))
    f.close()


def test_unsorted_column_ids_and_other_index_types(env):
    ta, torch = env
    T, D, cols = 80, 6, 120
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=4), T, D, cols, missing=MISSING)
    x = sparse_rows(ta, 900, cols, 0.25, seed=5)
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    rng = np.random.default_rng(1)
    pi, pv = indices.copy(), values.copy()
    for r in range(x.shape[0]):  # a per-row permutation of the sorted CSR
        lo, hi = indptr[r], indptr[r + 1]
        p = rng.permutation(hi - lo)
        pi[lo:hi], pv[lo:hi] = indices[lo:hi][p], values[lo:hi][p]
    assert not np.array_equal(pi, indices)
    xd, ip, ix, vals, pix, pvals = to_dev(torch, x, indptr, indices, values, pi, pv)
    for name in strategies(ta, f):
        f.set_strategy(getattr(ta, "STRATEGY_" + name))
        want = bits(f.predict(xd))
        assert np.array_equal(bits(f.predict_csr(ip, pix, pvals)), want), name
        assert np.array_equal(bits(f.predict_csr(ip.to(torch.int32), ix.to(torch.int64), vals)), want), name  # cast where needed
        assert np.array_equal(bits(f.predict_csr(torch.sparse_csr_tensor(ip, ix.to(torch.int64), vals, size=x.shape))), want), name
        f.check()
    f.close()


def test_stored_sentinel_nan_and_negative_zero(env):
    ta, torch = env
    # one tree per feature: x_j >= 0.0 ? 2^j : 0, missing goes left for even j and right for odd j
    cols = 6
    nodes = np.concatenate([ta.capi.encode_nodes([j, 0, 0], [0.0, 0.0, float(1 << j)], [j % 2 == 0, 0, 0], [1, 1, 1], [0, 1, 1])
                            for j in range(cols)])
    f = ta.Forest(nodes, cols, 1, cols, missing=MISSING)
    vals_in = np.array([MISSING, np.nan, -0.0, 0.0, -1.0, 3.0], dtype=np.float32)
    rows = np.array([np.roll(vals_in, s) for s in range(cols)], dtype=np.float32)
    indptr = np.arange(0, cols * cols + 1, cols, dtype=np.int64)  # every value stored, the sentinel and NaN included
    indices = np.tile(np.arange(cols, dtype=np.int32), cols)
    xd, ip, ix, vals = to_dev(torch, rows, indptr, indices, rows.reshape(-1))
    # by hand: -0.0 >= 0.0 holds (right), NaN >= 0.0 does not (left), a stored sentinel takes the default branch
    want = np.zeros(cols, dtype=np.float32)
    for r in range(cols):
        for j in range(cols):
            v = rows[r, j]
            right = (j % 2 == 1) if v == np.float32(MISSING) else bool(v >= 0.0)
            want[r] += np.float32(1 << j) if right else np.float32(0.0)
    for name in strategies(ta, f):
        f.set_strategy(getattr(ta, "STRATEGY_" + name))
        got = f.predict_csr(ip, ix, vals)
        f.check()
        assert np.array_equal(bits(got), bits(f.predict(xd))), name
        assert np.array_equal(bits(got), want.view(np.uint32)), name
    f.close()


def test_chunk_count_does_not_change_the_bits(env, monkeypatch):
    ta, torch = env
    T, D, cols, rows = 30, 6, 3072, 64 * 6 + 10
    nodes = ta.synth_forest(T, D, cols, seed=8)
    x = sparse_rows(ta, rows, cols, 0.03, seed=9)
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    xd, ip, ix, vals = to_dev(torch, x, indptr, indices, values)
    seen = {}
    for mb, chunks in ((64, 1), (3, 2), (1, 7)):  # the knob is read when the handle is created
        monkeypatch.setenv("TAHOE_CSR_CHUNK_MB", str(mb))
        f = ta.Forest(nodes, T, D, cols, missing=MISSING)
        for name in strategies(ta, f):
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            form, chunk = f.csr_plan(rows, values.size)
            assert chunk > 0 and chunk % 64 == 0 and -(-rows // chunk) == chunks and (chunks == 1 or rows % chunk != 0)
            got = bits(f.predict_csr(ip, ix, vals))
            f.check()
            assert np.array_equal(got, bits(f.predict(xd))), (mb, name)
            assert np.array_equal(seen.setdefault(name, got), got), (mb, name)
        assert f.info().device_bytes > 0
        f.close()


def test_bad_column_ids_are_skipped_and_reported_once(env):
    ta, torch = env
    T, D, cols, rows = 60, 6, 50, 300
    x = sparse_rows(ta, rows, cols, 0.2, seed=21)
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    bad = indices.copy()
    k1, k2 = int(indptr[100]), int(indptr[200])  # the first entries of rows 100 and 200
    assert indptr[101] > k1 and indptr[201] > k2
    bad[k1], bad[k2] = cols, -1
    hit = np.zeros(rows, dtype=bool)
    hit[[100, 200]] = True
    xd, ip, ix, bx, vals = to_dev(torch, x, indptr, indices, bad, values)
    sn, tr = ta.capi.dense_to_sparse(ta.synth_forest(T, D, cols, seed=20, leaf_prob=0.1), T, D)
    handles = [ta.Forest(ta.synth_forest(T, D, cols, seed=20), T, D, cols, missing=MISSING),
               ta.capi.SparseForest(sn, tr, cols, missing=MISSING)]
    for f in handles:
        for name in strategies(ta, f):
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            want = bits(f.predict(xd))
            got = bits(f.predict_csr(ip, bx, vals))  # returns OK: the bad entries are predicated off
            with pytest.raises(ta.TahoeError) as e:
                f.check()
            assert e.value.status == 1 and "column" in str(e.value), str(e.value)
            assert np.array_equal(got[~hit], want[~hit]), name
            f.check()  # reported once
            assert np.array_equal(bits(f.predict_csr(ip, ix, vals)), want), name
            f.check()  # a clean call checks OK again
        f.close()


def test_indptr_is_clamped_to_nnz(env):
    ta, torch = env
    T, D, cols, rows = 40, 5, 24, 200
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=30), T, D, cols, missing=MISSING)
    x = sparse_rows(ta, rows, cols, 0.3, seed=31)
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    wild = indptr.copy()
    wild[150] = -5              # row 149 ends before it begins, row 150 starts at a negative offset: clamped to 0
    wild[-1] = 1 << 40          # the last row claims entries far past nnz: clamped to nnz
    ok = np.ones(rows, dtype=bool)
    ok[[149, 150]] = False
    xd, ip, wp, ix, vals = to_dev(torch, x, indptr, wild, indices, values)
    for name in strategies(ta, f):
        f.set_strategy(getattr(ta, "STRATEGY_" + name))
        got = bits(f.predict_csr(wp, ix, vals))
        f.check()  # in-range columns only: nothing to report, nothing read out of bounds
        assert np.array_equal(got[ok], bits(f.predict(xd))[ok]), name
    f.close()


def test_reserve_csr_then_calls_allocate_nothing(env):
    ta, torch = env
    rows, density = 5000, 0.05
    T, D, cols = 300, 8, 64
    sn, tr = ta.capi.synth_sparse_forest(100, cols, 4, 20, 0.32, 65535, 3)
    for f in (ta.Forest(ta.synth_forest(T, D, cols, seed=1), T, D, cols, missing=MISSING),
              ta.capi.SparseForest(sn, tr, cols, missing=MISSING)):
        x = sparse_rows(ta, rows, cols, density, seed=2)
        indptr, indices, values = ta.dense_to_csr(x, MISSING)
        xd, ip, ix, vals = to_dev(torch, x, indptr, indices, values)
        for name in strategies(ta, f):
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            f.reserve_csr(rows, values.size)
            before = f.info().device_bytes
            a = f.predict_csr(ip, ix, vals)
            b = f.predict_csr(ip[:1001], ix, vals)  # a smaller batch of the same arrays
            f.check()
            assert f.info().device_bytes == before, name
            want = bits(f.predict(xd))
            assert np.array_equal(bits(a), want) and np.array_equal(bits(b), want[:1000]), name
        f.close()


def test_a_row_alone_and_inside_a_batch(env):
    ta, torch = env
    T, D, cols = 100, 7, 90
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=40), T, D, cols, missing=MISSING)
    x = sparse_rows(ta, 700, cols, 0.15, seed=41)
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    ip, ix, vals = to_dev(torch, indptr, indices, values)
    for name in strategies(ta, f):
        f.set_strategy(getattr(ta, "STRATEGY_" + name))
        batch = bits(f.predict_csr(ip, ix, vals))
        for r in (0, 63, 64, 333, 699):
            lo, hi = int(indptr[r]), int(indptr[r + 1])
            one = torch.tensor([0, hi - lo], dtype=torch.int64, device="cuda")
            alone = bits(f.predict_csr(one, ix[lo:hi], vals[lo:hi]))
            assert alone[0] == batch[r], (name, r)
        f.check()
    f.close()


def test_auto_takes_the_fused_kernel_where_auto_runs_that_tile_kernel(env):
    ta, torch = env
    # a shallow forest resolves to ROWTILE under AUTO, a sparse handle of few trees to TILEBLOCK: the same kernels, fed from CSR
    T, D, cols = 60, 3, 40
    f = ta.Forest(ta.synth_forest(T, D, cols, seed=50), T, D, cols, missing=MISSING)
    assert f.get_strategy(10_000) == ta.STRATEGY_ROWTILE and f.csr_plan(10_000, 20_000) == ("csr_rowtile", 0)
    f.close()
    sn, tr = ta.capi.synth_sparse_forest(40, 300, 4, 16, 0.32, 65535, 51)
    s = ta.capi.SparseForest(sn, tr, 300, missing=MISSING)
    assert s.get_strategy(10_000) == ta.STRATEGY_TILEBLOCK and s.csr_plan(10_000, 20_000) == ("csr_sparse_top", 0)
    same_bits(ta, torch, s, sparse_rows(ta, 1000, 300, 0.02, seed=52), ("AUTO",))
    s.close()
