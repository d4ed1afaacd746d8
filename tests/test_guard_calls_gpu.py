"""Guard bands around the other prediction entry points: predict_csr (the three fused forms and the chunked fallback, whose
output pointer moves by chunk offset x classes on the host), predict_staged, predict_host and partial_dependence (whose output
pointer moves chunk by chunk too).  Outputs are interiors of tests/guarded.py buffers, inputs too (CSR arrays, the grid, host
data); bands and inputs are compared by bits, interiors against the oracle (tests/pd_ref.py for partial dependence, the numpy
restatements of the native handles' tests for staged prediction on those).  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_ref as er  # noqa: E402
import pd_cases  # noqa: E402
import pd_ref  # noqa: E402
import test_multiclass_gpu as mcg  # noqa: E402
import test_staged_gpu as stg  # noqa: E402
import test_staged_native_gpu as sng  # noqa: E402
from guarded import Guarded, guarded_input  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
STAGED_ROWS = (130, 65, 64, 63, 1)


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta
    from oracle import oracle

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, oracle, torch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def strat(ta, name):
    return getattr(ta, "STRATEGY_" + name)


# --------------------------------------------------------------------------------------------------------------- predict_csr
def sparse_rows(ta, rows, cols, density, seed, empty_tail=0):
    """synth_data (a few NaN) with a `density` share of the entries kept; the last empty_tail rows hold nothing."""
    x = ta.synth_data(rows, cols, seed=seed, nan_prob=0.01)
    x[np.random.default_rng(seed).random((rows, cols)) >= density] = MISSING
    if empty_tail:
        x[rows - empty_tail:] = MISSING
    return x


def csr_call(env, f, x, want, form, chunks, tag):
    """predict_csr of the rows x into a guarded output, from guarded CSR arrays; the plan must be `form` in `chunks` chunks
    (0: a fused form)."""
    ta, oracle, torch = env
    rows = x.shape[0]
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    got_form, chunk = f.csr_plan(rows, values.size)
    assert got_form == form or (form.endswith("*") and got_form.startswith(form[:-1])), (tag, got_form, chunk)
    if chunks == 0:
        assert chunk == 0, (tag, chunk)
    else:
        assert chunk > 0 and -(-rows // chunk) >= chunks and rows % chunk != 0, (tag, rows, chunk)  # a ragged last chunk
    ip = guarded_input(torch, indptr, torch.int64, device="cuda")
    ix = guarded_input(torch, indices, torch.int32, device="cuda")
    vals = guarded_input(torch, values, torch.float32, device="cuda")
    out = Guarded(torch, f._out_shape(rows), torch.float32, device="cuda")
    f.predict_csr(ip.view, ix.view, vals.view, out=out.view)
    f.check()
    assert np.array_equal(bits(out.check("predict_csr: " + tag)), bits(want)), "predict_csr: " + tag
    for g, what in ((ip, "indptr"), (ix, "indices"), (vals, "values")):
        g.check_unchanged(f"{what}: {tag}")


CSR_ROWS = (130, 65, 64, 63, 1)


def test_csr_fused_rowtile_on_a_dense_handle(env):
    ta, oracle, torch = env
    T, D, cols = 40, 6, 32  # smoke()'s forest
    nodes = ta.synth_forest(T, D, cols, seed=7, leaf_prob=0.1)
    f = ta.Forest(nodes, T, D, cols, missing=MISSING)
    f.set_strategy(ta.STRATEGY_ROWTILE)
    for rows in CSR_ROWS:
        for tail in (0, min(3, rows - 1)):  # ... and a batch whose last rows are empty
            x = sparse_rows(ta, rows, cols, 0.3, seed=rows, empty_tail=tail)
            want = oracle.predict(nodes, T, D, x, MISSING)[0]
            csr_call(env, f, x, want, "csr_rowtile", 0, f"rows {rows}, {tail} empty at the end")
    f.close()


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("name,form", [("ROWTILE", "csr_sparse_rowtile"), ("TILEBLOCK", "csr_sparse_top")])
def test_csr_fused_forms_on_a_sparse_handle(env, name, form, C):
    ta, oracle, torch = env
    cols = stg.SP["cols"]
    sn, tr = ta.capi.synth_sparse_forest(stg.SP["T"], cols, 3, 12, 0.3, 65535, 121)  # test_staged_gpu.py's 37 trees
    if C == 2:
        sn, tr = sn[: tr[36]], tr[:36]
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, num_classes=C)
    f.set_strategy(strat(ta, name))
    for rows in CSR_ROWS:
        for tail in (0, min(3, rows - 1)):
            x = sparse_rows(ta, rows, cols, 0.3, seed=rows + 1, empty_tail=tail)
            if C == 1:
                want = oracle.sparse_predict(sn, tr, x, MISSING)[0]
            else:
                want = np.stack([oracle.sparse_predict(sn, np.ascontiguousarray(tr[c::2]), x, MISSING)[0] for c in range(2)], axis=1)
            csr_call(env, f, x, want, form, 0, f"{form}, {C} class(es), rows {rows}, {tail} empty at the end")
    f.close()


@pytest.mark.parametrize("name,form", [("DIRECT", "direct"), ("QRING", "qring_*")])
def test_csr_chunked_fallback_on_wide_rows(env, monkeypatch, name, form):
    """TAHOE_CSR_CHUNK_MB=1 on 3072 columns (test_chunk_count_does_not_change_the_bits): chunks of 64 rows, a ragged last one;
    every chunk's output goes to out + r0."""
    ta, oracle, torch = env
    T, D, cols = 30, 6, 3072
    nodes = ta.synth_forest(T, D, cols, seed=8)
    monkeypatch.setenv("TAHOE_CSR_CHUNK_MB", "1")  # read when the handle is created
    f = ta.Forest(nodes, T, D, cols, missing=MISSING)
    f.set_strategy(strat(ta, name))
    for rows in (64 * 6 + 10, 65, 1):
        x = sparse_rows(ta, rows, cols, 0.03, seed=9, empty_tail=min(3, rows - 1))
        want = oracle.predict(nodes, T, D, x, MISSING)[0]
        csr_call(env, f, x, want, form, 3 if rows > 129 else 1 if rows == 1 else 2, f"{name}, rows {rows}")
    f.close()


def test_csr_chunked_fallback_on_a_multiclass_handle(env, monkeypatch):
    """Few columns, rows past one chunk: the output pointer moves by r0 x num_classes per chunk."""
    ta, oracle, torch = env
    C, Tc, D, cols = 3, 30, 6, 40  # test_multiclass_softmax's shape
    T = C * Tc
    nodes = ta.synth_forest(T, D, cols, seed=7, leaf_prob=0.05)
    monkeypatch.setenv("TAHOE_CSR_CHUNK_MB", "1")
    f = ta.Forest(nodes, T, D, cols, missing=MISSING, num_classes=C)
    f.set_strategy(ta.STRATEGY_DIRECT)
    chunk = f.csr_plan(100_000, 1)[1]
    assert 0 < chunk <= 8192, chunk  # 1 MiB of 40 float32 columns
    rows = 2 * chunk + 65
    x = sparse_rows(ta, rows, cols, 0.1, seed=3, empty_tail=3)
    want, _ = mcg.expected(oracle, nodes, C, T, D, x)
    csr_call(env, f, x, want, "direct", 3, f"multi-class, rows {rows}, chunk {chunk}")
    f.close()


# ------------------------------------------------------------------------------------------------------------ predict_staged
def staged_call(env, f, data, want, rows, tag):
    ta, oracle, torch = env
    x = guarded_input(torch, data[:rows], torch.float32, device="cuda")
    out = Guarded(torch, (rows,) + tuple(want.shape[1:]), torch.float32, device="cuda")
    f.predict_staged(x.view, out=out.view)
    f.check()
    got = out.check("predict_staged: " + tag)
    x.check_unchanged("data: " + tag)
    return got


@pytest.mark.parametrize("name", ["DIRECT", "ROWTILE"])
def test_staged_dense(env, name):
    """test_staged_gpu.py's 13 trees, every stage; then the same with OUT_AVG, so that transform_staged_kernel runs over the
    guarded buffer (stage s divides by its own tree count, exactly)."""
    ta, oracle, torch = env
    nodes, data, want = stg.dense_c1(ta, oracle)
    D1 = stg.D1
    for output in (ta.OUT_RAW, ta.OUT_AVG):
        f = ta.Forest(nodes, D1["T"], D1["depth"], D1["cols"], missing=MISSING, output=output)
        f.set_strategy(strat(ta, name))
        f.set_stages(D1["stages"])
        assert f.staged_strategy(130) == strat(ta, name)
        for rows in STAGED_ROWS:
            got = staged_call(env, f, data, want, rows, f"dense {name}, output {output}, rows {rows}")
            if output == ta.OUT_RAW:
                assert np.array_equal(bits(got), bits(want[:rows])), (name, rows)
            else:
                for s, n in enumerate(D1["stages"]):
                    er.check(got[:, s], er.epilogue(want[:rows, s], ta.OUT_AVG, divisor=n), f"AVG, stage {s}, rows {rows}")
        f.close()


@pytest.mark.parametrize("name", ["DIRECT", "ROWTILE"])
def test_staged_multiclass(env, name):
    ta, oracle, torch = env
    nodes, data, want = stg.dense_mc(ta, oracle)
    MC, stages = stg.MC, [1, 2, 5]
    f = ta.Forest(nodes, MC["C"] * MC["Tc"], MC["depth"], MC["cols"], missing=MISSING, num_classes=MC["C"])
    f.set_strategy(strat(ta, name))
    f.set_stages(stages)
    w = np.ascontiguousarray(want[:, [n - 1 for n in stages], :])
    for rows in STAGED_ROWS:
        got = staged_call(env, f, data, w, rows, f"multi-class {name}, rows {rows}")
        assert got.shape == (rows, 3, MC["C"]) and np.array_equal(bits(got), bits(w[:rows])), (name, rows)
    f.close()


@pytest.mark.parametrize("name", ["DIRECT", "ROWTILE", "TILEBLOCK"])
def test_staged_sparse(env, name):
    ta, oracle, torch = env
    sn, tr, data, want, _ = stg.sparse_forest(ta, oracle)
    f = ta.capi.SparseForest(sn, tr, stg.SP["cols"], missing=MISSING)
    f.set_strategy(strat(ta, name))
    f.set_stages(stg.SP["stages"])
    assert f.staged_strategy(130) == strat(ta, name)
    for rows in STAGED_ROWS:
        got = staged_call(env, f, data, want, rows, f"sparse {name}, rows {rows}")
        assert np.array_equal(bits(got), bits(want[:rows])), (name, rows)
    f.close()


@pytest.mark.parametrize("k", [1, 9])
@pytest.mark.parametrize("kind", ["oblivious", "vector"])
def test_staged_native_handles(env, kind, k):
    """ObliviousForest(staged=True) / VectorForest(staged=True), forests, stages and running sums of test_staged_native_gpu.py."""
    ta, oracle, torch = env
    forest, data, run = sng.case(kind, 7, k)
    rounds = list(sng.STAGE_SETS[0])
    want = np.ascontiguousarray(sng.want_of(run, rounds, k))
    f = sng.handle(ta, forest, staged=True)
    f.set_stages(rounds)
    for name in ("DIRECT", "ROWTILE"):
        f.set_strategy(strat(ta, name))
        assert f.staged_strategy(sng.ROWS) == strat(ta, name)
        for rows in STAGED_ROWS:
            got = staged_call(env, f, data, want, rows, f"{kind} K = {k} {name}, rows {rows}")
            assert np.array_equal(bits(got), bits(want[:rows])), (kind, k, name, rows)
    f.close()


# -------------------------------------------------------------------------------------------------------------- predict_host
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_batches(env, pinned):
    """preds_host is the interior of a guarded numpy buffer: chunk c is copied back to preds + c x chunk_rows.  Three chunks with
    a ragged last one; one row; 4097 rows at chunk_rows = 1024 (a last chunk of one row).  The pageable source is guarded too; a
    pinned one is the library's own allocation and is compared with what was put in."""
    ta, oracle, torch = env
    T, D, cols = 40, 6, 32  # smoke()'s forest
    nodes = ta.synth_forest(T, D, cols, seed=7, leaf_prob=0.1)
    data = ta.synth_data(4097, cols, seed=8, missing_prob=0.05, missing=MISSING, nan_prob=0.01)
    want = oracle.predict(nodes, T, D, data, MISSING, threads=8)[0]
    f = ta.Forest(nodes, T, D, cols, missing=MISSING)
    for rows, chunk_rows in ((2 * 1024 + 100, 1024), (4097, 1024), (1, 1024), (130, 64)):
        src = guarded_input(np, data[:rows], np.float32)
        pin = None
        if pinned:
            pin = ta.PinnedArray(rows, cols)
            pin.array[:] = data[:rows]
        out = Guarded(np, (rows,), np.float32)
        f.predict_host(pin.array if pinned else src.view, preds=out.view, chunk_rows=chunk_rows)
        f.check()
        tag = f"predict_host, rows {rows}, chunk_rows {chunk_rows}, {'pinned' if pinned else 'pageable'}"
        assert np.array_equal(bits(out.check(tag)), bits(want[:rows])), tag
        if pinned:
            assert np.array_equal(bits(pin.array), bits(data[:rows])), tag
            pin.close()
        else:
            src.check_unchanged("data: " + tag)
    f.close()


# -------------------------------------------------------------------------------------------------------- partial_dependence
@pytest.mark.parametrize("targets", [0, 1], ids=["one_target", "two_targets"])
@pytest.mark.parametrize("which", [0, 1], ids=["one_class", "three_classes"])
def test_partial_dependence(env, monkeypatch, which, targets):
    """A grid larger than the call's chunk runs chunk after chunk, the output pointer moving by row0 x classes
    (tahoe_forest_predict_partial_dependence's loop over pd->chunk, which pd_create in partial_dependence.hip sets to
    TAHOE_PD_CHUNK_ROWS rounded up to 64s, else to what keeps the workspace at 32 MiB: 699 040 points for these 12 trees).  With
    the knob at 64, 130 points are two chunks and a ragged third; 1, 63, 64 and 65 are the edges of the 64-point tile."""
    ta, oracle, torch = env
    case = pd_cases.RANDOM_CASES[which]
    fo = pd_cases.random_forest(**case["forest"])
    feats = case["targets"][targets]
    assert len(feats) == targets + 1 and fo["num_classes"] == (1, 3)[which]
    monkeypatch.setenv("TAHOE_PD_CHUNK_ROWS", "64")  # read when the handle is created
    f = ta.capi.SparseForest(fo["nodes"], fo["trees"], fo["num_cols"], missing=fo["missing"], covers=fo["covers"],
                             num_classes=fo["num_classes"], categories=fo["categories"], members_left=fo["members_left"],
                             partial_dependence=True)
    whole = pd_cases.random_grid(fo, feats, 130, seed=77)
    want = pd_ref.pd_f32(fo["nodes"], fo["trees"], fo["covers"], feats, whole, fo["missing"], fo["num_classes"], fo["cats"])
    for G in (130, 65, 64, 63, 1):
        grid = guarded_input(torch, whole[:G], torch.float32, device="cuda")
        out = Guarded(torch, f._out_shape(G), torch.float32, device="cuda")
        f.partial_dependence(feats, grid.view, out=out.view)
        f.check()
        tag = f"partial_dependence, {fo['num_classes']} class(es), targets {feats}, G = {G}"
        got = out.check(tag).reshape(G, -1)
        assert np.array_equal(bits(got), bits(np.ascontiguousarray(want[:G], dtype=np.float32))), tag  # (a grid point's value
        grid.check_unchanged("grid: " + tag)                                                        # does not depend on its batch)
    f.close()
