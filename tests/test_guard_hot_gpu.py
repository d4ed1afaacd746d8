"""Guard bands around the hot path, kernel form by kernel form: predict_raw, predict_leaf_idx (with and without sums),
predict_accumulate and predict with an epilogue write only their own rows, leave their input alone, and the rows they write are
the oracle's.  Needs an MI355X.

Every output is the interior of a tests/guarded.py buffer: 384 rows (the largest row tile of any form; raised where info() names
a larger one) of guard pattern in front of it and behind it, compared by bits after every call.  The data is guarded the same
way and must come back with the bits it went in with.

One case = one handle (plus one with an epilogue) and one reference, taken once at the case's largest row count; rows are
independent, so its first R rows serve every smaller batch.  Row counts: 1, t - 1, t, t + 1, 2t + 1 for the form's row tile t
(info().tile_rows / ring_rows / qring_tile_rows, 64 where info() does not say; 128 as well where the form also walks 128-row
tiles) and the counts of the table the shape was taken from -- largest first, so that the quantised workspace and the
leaf-value buffers hold plausible stale rows when the small batches run.  Every call asserts the kernel form the case is there
for; the last test asserts that the forms seen are all 19 library forms and the four native ones.

The shapes come from the tests that already reach each form (smoke(), test_gpu_parity.py, test_multiclass_gpu.py's CASES,
test_staged_gpu.py, test_oblivious_gpu.py, test_vector_gpu.py).  Two things are added to their knobs, both create-time knobs
those files already use: the region forms of QRING walk batches of fewer 128-row tiles than CUs in tree slices (qring_split), so
their handles are created with TAHOE_QRING_SLICES=1, which keeps small batches in plain tiles -- otherwise no region form could
be asked for 1 or t + 1 rows; and qring_region_mixed is by definition whole waves of 192-row tiles plus a remainder of 128-row
tiles, so its tile-edge counts are one wave plus 1, 127, 128, 129, 257 rows (its handle keeps the table's knobs as they are: the
planner takes the mixed plan for a remainder that small only with the remainder's tree slices priced in).

The stated hole: predict_accumulate adds onto what the buffer holds.  A tail lane that reads the guard, adds 0.0f and writes it
back leaves the guard's bits and is not caught here (tests/test_guarded_ref.py shows it); one that adds a leaf value is.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref  # noqa: E402
import epilogue_ref as er  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import test_multiclass_gpu as mcg  # noqa: E402  (CASES, forest_nodes, batch, expected)
import test_staged_gpu as stg  # noqa: E402  (SP, rows_data, cat_forest)
import vector_ref as vr  # noqa: E402
from guarded import BAND_ROWS, Guarded, guarded_input  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
FORMS = set()  # kernel forms the calls of this file ran (test_every_form_was_exercised)
NATIVE_FORMS = {"oblivious_direct", "oblivious_tile", "vector_direct", "vector_tile"}
KNOBS = mcg.KNOBS + ("TAHOE_WSTREAM", "TAHOE_WSTREAM_SLAB_MB", "TAHOE_QRING_NARROW128", "TAHOE_QRING_TOP24")
ALSO_128 = ("qring_region2", "qring_region3", "qring_region8", "qring_region6", "qring_split", "qring_columns", "qring_gx",
            "sparse_qring")  # forms whose remainders / slices / columns are 128-row tiles whatever qring_tile_rows says


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


def edges(t):
    return [r for r in (1, t - 1, t, t + 1, 2 * t + 1) if r >= 1]


class Case:
    """make(**kw) -> a handle (kw: output, global_bias); data [R, cols]; want [R] / [R, C] float32; want_leaf [R, T] uint32;
    cont(start [R]) -> the continued sums, or None where predict_accumulate is refused; divisor: what OUT_AVG divides by."""

    def __init__(self, make, data, want, want_leaf, strategy, form, rows, divisor, cont=None, more_rows=lambda f, cus: []):
        self.make, self.data, self.want, self.want_leaf = make, data, want, want_leaf
        self.strategy, self.form, self.rows, self.divisor, self.cont, self.more_rows = strategy, form, rows, divisor, cont, more_rows


def tile_of(f, form):
    """The form's row tile from info(); 64 where info() does not say (DIRECT, ROWTILE, the sparse float forms, native handles)."""
    try:
        info = f.info()
    except Exception:  # a native handle without tahoe_forest_get_info
        return 64, 0
    if form.startswith("qring") or form == "sparse_qring":
        t = info.qring_tile_rows
    elif form.startswith("tilering"):
        t = info.ring_rows
    elif form == "tileblock":
        t = info.tile_rows
    else:
        t = 0
    largest = max(info.tile_rows, info.ring_rows, info.qring_tile_rows)
    return (t if t >= 2 else 64), largest


def row_counts(c, f, torch, max_rows):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t, largest = tile_of(f, c.form)
    rows = set(c.rows) | set(c.more_rows(f, cus))
    if c.form != "qring_region_mixed":  # (its edges are in more_rows: a wave plus the edges of the 128-row remainder)
        rows |= set(edges(t)) | (set(edges(128)) if c.form in ALSO_128 else set()) | set(edges(64))
    rows = sorted((r for r in rows if r <= max_rows), reverse=True)  # largest first
    return rows, max(BAND_ROWS, largest)


def sweep(env, c):
    """Every call of the hot path at every row count of the case, each into guarded outputs."""
    ta, oracle, torch = env
    f = c.make()
    C, T = f.num_classes, f.num_trees
    if c.strategy is not None:
        f.set_strategy(c.strategy)
    out_e = (ta.OUT_AVG | ta.OUT_SOFTMAX) if C > 1 else (ta.OUT_AVG | ta.OUT_SIGMOID)
    bias = 0.25
    fe = c.make(output=out_e, global_bias=bias)
    if c.strategy is not None:
        fe.set_strategy(c.strategy)
    rows_list, band = row_counts(c, f, torch, c.data.shape[0])
    assert rows_list and rows_list[0] == c.data.shape[0], (rows_list[:3], c.data.shape)  # the reference's rows are all used
    rng = np.random.default_rng(len(rows_list) + T)
    start_all = rng.uniform(-2.0, 2.0, c.data.shape[0]).astype(np.float32)  # seeded running sums
    cont_all = c.cont(start_all) if c.cont is not None else None
    shape = (lambda R: (R, C)) if C > 1 else (lambda R: (R,))
    for R in rows_list:
        form = f.kernel_form(R)
        FORMS.add(form)
        tag = f"{c.form}, {C} class(es), rows {R}"
        assert form == c.form, f"{tag}: the shape reaches {form}"
        assert fe.kernel_form(R) == c.form, tag
        x = guarded_input(torch, c.data[:R], torch.float32, device="cuda")
        want = c.want[:R]
        # predict_raw
        out = Guarded(torch, shape(R), torch.float32, band_rows=band, device="cuda")
        f.predict_raw(x.view, out.view)
        f.check()
        assert np.array_equal(bits(out.check("predict_raw: " + tag)), bits(want)), "predict_raw: " + tag
        # predict_leaf_idx with sums
        leaf = Guarded(torch, (R, T), torch.int32, band_rows=band, device="cuda")
        sums = Guarded(torch, shape(R), torch.float32, band_rows=band, device="cuda")
        f.predict_leaf_idx(x.view, leaf=leaf.view, sums=sums.view)
        f.check()
        assert np.array_equal(bits(leaf.check("leaf indices: " + tag)), c.want_leaf[:R]), "leaf indices: " + tag
        assert np.array_equal(bits(sums.check("leaf-pass sums: " + tag)), bits(want)), "leaf-pass sums: " + tag
        # ... and without
        leaf = Guarded(torch, (R, T), torch.int32, band_rows=band, device="cuda")
        f.predict_leaf_idx(x.view, want_sums=False, leaf=leaf.view)
        f.check()
        assert np.array_equal(bits(leaf.check("leaf indices alone: " + tag)), c.want_leaf[:R]), "leaf indices alone: " + tag
        # predict_accumulate onto seeded running sums
        if cont_all is not None:
            acc = Guarded(torch, (R,), torch.float32, band_rows=band, device="cuda").load(start_all[:R])
            f.predict_accumulate(x.view, acc.view)
            f.check()
            assert np.array_equal(bits(acc.check("predict_accumulate: " + tag)), bits(cont_all[:R])), "predict_accumulate: " + tag
        # predict with an epilogue: the transform kernel runs over the same buffer
        out = Guarded(torch, shape(R), torch.float32, band_rows=band, device="cuda")
        fe.predict(x.view, out.view)
        fe.check()
        er.check(out.check("predict: " + tag), er.epilogue(want, out_e, 0.0, bias, c.divisor), "predict: " + tag)
        x.check_unchanged("data: " + tag)
    f.close()
    fe.close()


# ------------------------------------------------------------------------------------------------------------ dense cases
def dense_case(env, nodes, T, D, cols, C, data, strategy, form, rows, more_rows=lambda f, cus: [], relayout=False):
    ta, oracle, torch = env

    def make(**kw):
        return ta.Forest(nodes, T, D, cols, missing=MISSING, num_classes=C, **kw)

    if C == 1:
        want, want_leaf = oracle.predict(nodes, T, D, data, MISSING, want_leaf=True, threads=8)
        cont = lambda start: oracle.predict_continue(nodes, T, D, data, MISSING, start.copy(), threads=8)  # noqa: E731
    else:
        want, want_leaf = mcg.expected(oracle, nodes, C, T, D, data)
        cont = None  # refused on a multi-class handle
    return Case(make, data, want, want_leaf, strategy, form, rows, T // C, cont, more_rows)


SMOKE_FORMS = [("DIRECT", "direct"), ("ROWTILE", "rowtile"), ("TILEBLOCK", "tileblock"), ("TILERING", "tilering_tile")]


@pytest.mark.parametrize("strat,form", SMOKE_FORMS, ids=[s[1] for s in SMOKE_FORMS])
def test_float_forms_on_the_smoke_forest(env, knobs, strat, form):
    """smoke()'s forest (40 trees of depth 6, 32 columns), strategies forced."""
    ta, oracle, torch = env
    T, D, cols, R = 40, 6, 32, 1000
    nodes = ta.synth_forest(T, D, cols, seed=7, leaf_prob=0.1)
    data = ta.synth_data(R, cols, seed=8, missing_prob=0.05, missing=MISSING, nan_prob=0.01)
    sweep(env, dense_case(env, nodes, T, D, cols, 1, data, getattr(ta, "STRATEGY_" + strat), form, [R]))


WIDE = [
    # name, knobs, T, D, cols, own rows ("slabs": two full slabs and a ragged third), form; seeds as in test_gpu_parity.py
    ("wide_tile", {"TAHOE_WSTREAM": "0"}, 9, 3, 700, 64, "tilering_wide_tile", 900, 901),
    ("wide_stream", {"TAHOE_WSTREAM": "1"}, 9, 2, 700, 64, "tilering_wide_stream", 950, 951),
    ("wide_stream_slabs", {"TAHOE_WSTREAM": "1", "TAHOE_WSTREAM_SLAB_MB": "1"}, 40, 6, 640, "slabs", "tilering_wide_stream", None, None),
]


@pytest.mark.parametrize("case", WIDE, ids=[c[0] for c in WIDE])
def test_wide_row_forms_of_tilering(env, knobs, case):
    """test_wide_rows_float32_form / _streaming_form at their smallest parameter rows, and the streaming form walking a batch
    slab by slab (a slab is 64 rows per CU at TAHOE_WSTREAM_SLAB_MB=1): the slab's own edges are row counts too."""
    ta, oracle, torch = env
    name, env_knobs, T, D, cols, R, form, fseed, dseed = case
    for k, v in env_knobs.items():
        knobs.setenv(k, v)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    more = lambda f, cus: []  # noqa: E731
    if R == "slabs":
        nodes = ta.synth_forest(T, D, cols, seed=990, leaf_prob=0.1)
        S = cus * 64
        R = 2 * S + 777
        data = ta.synth_data(R, cols, seed=991, missing_prob=0.01, missing=MISSING)
        more = lambda f, cus: [S - 1, S, S + 1]  # noqa: E731
    else:
        nodes = ta.synth_forest(T, D, cols, seed=fseed + T, leaf_prob=0.1 if D > 4 else 0.0)
        mp = 0.05 if name == "wide_stream" else 0.0
        Rmax = 2 * 64 + 1  # 2t + 1 of the largest tile these forms have
        data = ta.synth_data(Rmax, cols, seed=dseed + R, missing_prob=mp, missing=MISSING, nan_prob=mp / 2)
        more = lambda f, cus, own=R: [own]  # noqa: E731
        R = Rmax
    c = dense_case(env, nodes, T, D, cols, 1, data, ta.STRATEGY_TILERING, form, [R], more)
    sweep(env, c)


QRING_CASES = [c for c in mcg.CASES if c[8] is not None and c[8].startswith("qring")]
assert [c[8] for c in QRING_CASES] == ["qring_region8", "qring_region6", "qring_region3", "qring_region2", "qring_region_mixed",
                                       "qring_split", "qring_columns", "qring_wide", "qring_gx"]


@pytest.mark.parametrize("classes", ["one_class", "own_classes"])
@pytest.mark.parametrize("case", QRING_CASES, ids=[c[0] for c in QRING_CASES])
def test_quantised_forms(env, knobs, case, classes):
    """The CASES table of test_multiclass_gpu.py with its knobs, the forest once as one class and once with its own C."""
    ta, oracle, torch = env
    name, C, Tc, D, cols, gen, env_knobs, rows_list, form = case
    for k, v in env_knobs.items():
        knobs.setenv(k, v)
    if form not in ("qring_split", "qring_region_mixed"):  # (mixed: the planner prices the remainder's tree slices in)
        knobs.setenv("TAHOE_QRING_SLICES", "1")  # small batches stay in the case's own tiles (module docstring)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows_list = [cus * 384 + 321 if r == "wave384" else cus * 192 + 777 if r == "wave192" else r for r in rows_list]
    more = lambda f, cus: []  # noqa: E731
    if form == "qring_region_mixed":
        rows_list = [max(rows_list)]  # (below a whole wave of 192-row tiles the same handle runs region2 / region3)
        more = lambda f, cus: [cus * 192 + e for e in edges(128)]  # noqa: E731
    T = C * Tc
    nodes = mcg.forest_nodes(ta, gen, T, D, cols, seed=100 + len(name) + cols)
    biggest = max(rows_list + [2 * 384 + 1])
    data = mcg.batch(ta, gen, biggest, cols, seed=200 + cols)
    c = dense_case(env, nodes, T, D, cols, C if classes == "own_classes" else 1, data, ta.STRATEGY_QRING, form, rows_list + [biggest], more)
    sweep(env, c)


# ----------------------------------------------------------------------------------------------------------- sparse cases
SPARSE_FORMS = [("DIRECT", "sparse_direct"), ("ROWTILE", "sparse_rowtile"), ("TILEBLOCK", "sparse_top"), ("QRING", "sparse_qring")]
_sparse = {}


def sparse_inputs(ta):
    """test_staged_gpu.py's 37 irregular trees on 20 columns, and rows for 2t + 1 of the 384-row tile of sparse_qring."""
    if not _sparse:
        sn, tr = ta.capi.synth_sparse_forest(stg.SP["T"], stg.SP["cols"], 3, 12, 0.3, 65535, 121)
        _sparse["f"] = (sn, tr, stg.rows_data(ta, 2 * 384 + 1, stg.SP["cols"], seed=122))
    return _sparse["f"]


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("strat,form", SPARSE_FORMS, ids=[s[1] for s in SPARSE_FORMS])
def test_sparse_forms(env, knobs, strat, form, C):
    ta, oracle, torch = env
    sn, tr, data = sparse_inputs(ta)
    cols = stg.SP["cols"]
    if C == 2:
        sn, tr = sn[: tr[36]], tr[:36]  # the first 36 trees as two classes, as test_sparse_multiclass_stages takes them
        want = np.stack([oracle.sparse_predict(sn, np.ascontiguousarray(tr[c::2]), data, MISSING, threads=8)[0] for c in range(2)], axis=1)
        cont = None
    else:
        want = oracle.sparse_predict(sn, tr, data, MISSING, threads=8)[0]
        # (the oracle continues dense forests only: tests/categorical_ref.py restates the sparse walk with a start, and the
        # restatement from 0.0f is held to the oracle's bits here)
        assert np.array_equal(bits(categorical_ref.predict(sn, tr, data, MISSING)[0]), bits(want))
        cont = lambda start: categorical_ref.predict(sn, tr, data, MISSING, init=start)[0]  # noqa: E731
    want_leaf = oracle.sparse_predict(sn, tr, data, MISSING, want_leaf=True, threads=8)[1]

    def make(**kw):
        return ta.capi.SparseForest(sn, tr, cols, missing=MISSING, num_classes=C, **kw)

    sweep(env, Case(make, data, want, want_leaf, getattr(ta, "STRATEGY_" + strat), form, [stg.SP["rows"], data.shape[0]], tr.size // C, cont))


@pytest.mark.parametrize("strat,form", SPARSE_FORMS[:3], ids=[s[1] for s in SPARSE_FORMS[:3]])
def test_sparse_float_forms_on_a_categorical_handle(env, knobs, strat, form):
    """test_categorical_stages' forest (cat_forest) and its data, against tests/categorical_ref.py."""
    ta, oracle, torch = env
    cols, feats, T, rows = 12, [1, 5, 9], 9, 130
    sn, tr, cats, ml = stg.cat_forest(ta, T, cols, feats, seed=131)
    data = stg.rows_data(ta, rows, cols, seed=132)
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
    want, want_leaf = categorical_ref.predict(sn, tr, data, MISSING, node, offset, words, mla)
    cont = lambda start: categorical_ref.predict(sn, tr, data, MISSING, node, offset, words, mla, init=start)[0]  # noqa: E731

    def make(**kw):
        return ta.capi.SparseForest(sn, tr, cols, missing=MISSING, categories=cats, members_left=ml, **kw)

    sweep(env, Case(make, data, want, want_leaf, getattr(ta, "STRATEGY_" + strat), form, [rows], T, cont))


# ----------------------------------------------------------------------------------------------------------- native handles
NATIVE = [("oblivious", "nine_k1"), ("oblivious", "five_k8"), ("oblivious", "nine_k9"),
          ("vector", "nine_k1"), ("vector", "four_k8"), ("vector", "five_k9")]


@pytest.mark.parametrize("strat", ["DIRECT", "ROWTILE"])
@pytest.mark.parametrize("kind,name", NATIVE, ids=[f"{k}-{n}" for k, n in NATIVE])
def test_native_handles_across_the_block_of_eight_outputs(env, knobs, kind, name, strat):
    """K = 1, 8 and 9 put outputs on both sides of the block of 8 the native kernels work in: `k0 + j < K` is the mask under test,
    beside the row mask.  Forests, data and references are those of test_oblivious_gpu.py / test_vector_gpu.py."""
    ta, oracle, torch = env
    if kind == "oblivious":
        import test_oblivious_gpu as og

        forest, data, want, want_leaf = og.case(name)
        k, T = forest["k"], len(forest["depths"])
        make = lambda **kw: og.handle(ta, forest, **kw)  # noqa: E731
        cont = (lambda start: obr.ref_of(forest, data, init=start)[0][:, 0]) if k == 1 else None
        form = "oblivious_direct" if strat == "DIRECT" else "oblivious_tile"
    else:
        forest, data, want, want_leaf, _ = vr.case(name)
        k, T = forest["k"], forest["trees"].size
        make = lambda **kw: ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], forest["cols"], missing=MISSING, **kw)  # noqa: E731
        cont = None  # refused on a vector-leaf handle
        form = "vector_direct" if strat == "DIRECT" else "vector_tile"
    want = want[:, 0] if k == 1 else want
    c = Case(make, np.ascontiguousarray(data), want, np.ascontiguousarray(want_leaf).view(np.uint32), getattr(ta, "STRATEGY_" + strat), form,
             [data.shape[0]], T, cont)
    sweep(env, c)


def test_every_form_was_exercised(env):
    """The calls of this file (run in file order) went through every form tahoe_kernel_form_name names for 1 .. 19, and the two
    oblivious and two vector forms."""
    ta = env[0]
    library = {ta.lib.tahoe_kernel_form_name(i).decode() for i in range(1, 20)}
    assert len(library) == 19 and "?" not in library
    assert FORMS == library | NATIVE_FORMS, (sorted((library | NATIVE_FORMS) - FORMS), sorted(FORMS - library - NATIVE_FORMS))
