"""The workgroup prologues that stage a walk tile and the quantiser's tables as one burst of loads (tahoe_amd/csrc/stage_burst.h),
bit for bit against the CPU oracle.  Needs an MI355X.

What can break.  A lane whose piece index lies past the end of a copy takes another piece instead: with 8 to 2048 16-byte pieces
per region for 960 or 1024 threads there are copies with fewer pieces than threads, with between one and two per thread, and
with 2048 = 2 x 960 + 128.  The regions of a partly filled last tile lie past the batch and may hold anything, also the codes
of an earlier, larger batch.  A walker's first top rides in the same burst, also for a walker that has no tree.  The bucket
quantiser reads each feature pair's tables as one 16-byte-aligned image whose parts are padded: threshold counts of every
residue mod 4 in either position, an empty table beside a crowded one, a pair so crowded that the bucket count drops, and a
pair that fits no bucket count (the search-tree kernels, whose tables are staged through the same helper: every table
starts 16-byte aligned, a table without thresholds is four NaN pads).  Half of the row values are thresholds of
their own feature, so a misplaced table entry changes a code.  Every case compares predict_raw and predict_leaf_idx bitwise
with the oracle, asserts the kernel form and checks the handle's error flag after each call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MISSING = -999.0
KNOBS = ("TAHOE_QUANT_MULTI", "TAHOE_QUANT_BUCKETS", "TAHOE_QRING_CHAINS", "TAHOE_QRING_REGIONS", "TAHOE_QRING_SLICES",
         "TAHOE_QRING_WIDE", "TAHOE_QRING_WIDE_CHAINS", "TAHOE_QRING_CODE8", "TAHOE_QRING_GROUPS", "TAHOE_QRING_TOP24",
         "TAHOE_QRING_NARROW128")
ROWS = (1, 64, 65, 191, 193, 385)
EVEN_COLS = (2, 18, 130, 254, 256)  # the bucket-pair quantiser
ODD_COLS = (1, 17, 255)             # the single-feature quantiser
T = 17


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta
    from oracle import oracle

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, oracle, torch


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def inner_of(nodes):
    return np.flatnonzero((nodes["bits"].view(np.uint32) >> 31) == 0)


def fids(nodes):
    return nodes["bits"].view(np.uint32) & np.uint32((1 << 30) - 1)


def set_fid(nodes, at, fid):
    b = nodes["bits"].view(np.uint32)
    b[at] = (b[at] & np.uint32(0xC0000000)) | np.asarray(fid, dtype=np.uint32)


_ROWS = {}


def rows_for(ta, nodes, rows, cols, missing, key):
    """`rows` rows for a forest (cached per `key`, left unchanged): synth_data, then half of the entries replaced by a threshold
    of their own feature (ties decide the code)."""
    k = (key, rows, cols, missing)
    if k not in _ROWS:
        d = (ta.synth_data(rows, cols, seed=100 + rows, missing_prob=0.05, missing=MISSING, nan_prob=0.01) if missing
             else ta.synth_data(rows, cols, seed=100 + rows))
        rng = np.random.default_rng(rows * 131 + cols)
        inner = inner_of(nodes)
        f, v = fids(nodes)[inner].astype(np.int64), nodes["val"][inner]
        keep = ~np.isnan(v)
        f, v = f[keep], v[keep]
        order = np.argsort(f, kind="stable")
        f, v = f[order], v[order]
        lo, hi = np.searchsorted(f, np.arange(cols)), np.searchsorted(f, np.arange(cols), side="right")
        tie = rng.random((rows, cols)) < 0.5
        if missing:
            tie &= d != np.float32(MISSING)
        for c in range(cols):
            if hi[c] > lo[c]:
                r = np.flatnonzero(tie[:, c])
                d[r, c] = v[rng.integers(lo[c], hi[c], size=r.size)]
        assert missing or not (d == np.float32(MISSING)).any()
        d.setflags(write=False)
        _ROWS[k] = d
    return _ROWS[k]


def run(env, handle, want_fn, batches, form):
    """Every batch, in the order given, through predict_raw and predict_leaf_idx of `handle` == the oracle."""
    ta, oracle, torch = env
    for data in batches:
        rows = data.shape[0]
        assert handle.kernel_form(rows) == form, (handle.kernel_form(rows), form, rows)
        want_sums, want_leaf = want_fn(data)
        x = torch.from_numpy(data.copy()).cuda()
        raw = handle.predict_raw(x)
        handle.check()
        leaf, sums = handle.predict_leaf_idx(x)
        handle.check()
        label = f"{form}, {data.shape[1]} features, {rows} rows"
        assert np.array_equal(bits(raw.cpu().numpy()), bits(want_sums)), f"{label}: predict_raw differs"
        assert np.array_equal(bits(sums.cpu().numpy()), bits(want_sums)), f"{label}: sums of the leaf pass differ"
        assert np.array_equal(bits(leaf.cpu().numpy()), want_leaf), f"{label}: leaf indices differ"


def check_dense(env, nodes, trees, D, cols, form, key, row_counts=ROWS, num_classes=1, want_fn=None):
    ta, oracle, torch = env
    batches = [rows_for(ta, nodes, r, cols, ms, key) for r in row_counts for ms in (False, True)]
    f = ta.Forest(nodes, trees, D, cols, missing=MISSING, num_classes=num_classes)
    f.set_strategy(ta.STRATEGY_QRING)
    try:
        run(env, f, want_fn or (lambda d: oracle.predict(nodes, trees, D, d, MISSING, want_leaf=True)), batches, form)
    finally:
        f.close()


# ------------------------------------------------------------------------------------------------ tile staging
FORMS = {
    # name: (knobs, form, column counts)
    "region3_top24": ({"TAHOE_QRING_CHAINS": "3", "TAHOE_QRING_CODE8": "0", "TAHOE_QRING_NARROW128": "0", "TAHOE_QRING_TOP24": "1"},
                      "qring_region3", EVEN_COLS + ODD_COLS),
    "region3_u32": ({"TAHOE_QRING_CHAINS": "3", "TAHOE_QRING_CODE8": "0", "TAHOE_QRING_NARROW128": "0", "TAHOE_QRING_TOP24": "0"},
                    "qring_region3", EVEN_COLS + ODD_COLS),
    "region2": ({"TAHOE_QRING_CHAINS": "2", "TAHOE_QRING_CODE8": "0", "TAHOE_QRING_NARROW128": "0"}, "qring_region2",
                EVEN_COLS + ODD_COLS),
    "split": ({"TAHOE_QRING_SLICES": "2", "TAHOE_QRING_CODE8": "0", "TAHOE_QRING_NARROW128": "0"}, "qring_split", EVEN_COLS + ODD_COLS),
    "region6": ({"TAHOE_QRING_CODE8": "0"}, "qring_region6", (2, 18, 128, 1, 17)),
    "columns": ({"TAHOE_QRING_REGIONS": "0", "TAHOE_QRING_CODE8": "0"}, "qring_columns", (2, 18, 130, 256, 17, 255)),
}


def plain_forest(ta, D, cols, seed):
    nodes = ta.synth_forest(T, D, cols, seed=seed)
    dl = (nodes["bits"].view(np.uint32)[inner_of(nodes)] >> 30) & 1
    assert dl.any() and not dl.all(), "def_left set and clear"
    return nodes


@pytest.mark.parametrize("D", [12, 3])
@pytest.mark.parametrize("name,cols", [(n, c) for n, (_, _, cs) in FORMS.items() for c in cs])
def test_tile_staging(env, monkeypatch, name, cols, D):
    """Every form of qring_kernel at every piece count, every row count, with and without missing values in the batch."""
    ta = env[0]
    knobs_, form, _ = FORMS[name]
    for k, v in knobs_.items():
        monkeypatch.setenv(k, v)
    nodes = plain_forest(ta, D, cols, seed=cols + D)
    check_dense(env, nodes, T, D, cols, form, key=("plain", D, cols))


@pytest.mark.parametrize("D", [12, 3])
@pytest.mark.parametrize("cols", EVEN_COLS + ODD_COLS)
def test_tile_staging_u8_regions(env, cols, D):
    """128-row regions of u8 codes: a forest with at most 254 thresholds per feature."""
    ta = env[0]
    nodes = ta.synth_forest_hist(T, D, cols, seed=cols + D, feature_seed=5, max_bins=254)
    check_dense(env, nodes, T, D, cols, "qring_region8", key=("hist", D, cols))


@pytest.mark.parametrize("D", [12, 3])
@pytest.mark.parametrize("cols", EVEN_COLS + ODD_COLS)
def test_tile_staging_multiclass(env, monkeypatch, cols, D):
    """Three classes on the multi-class instantiation of the 192-row tile (15 trees: five per class)."""
    ta, oracle, _ = env
    monkeypatch.setenv("TAHOE_QRING_CHAINS", "3")
    monkeypatch.setenv("TAHOE_QRING_CODE8", "0")
    monkeypatch.setenv("TAHOE_QRING_NARROW128", "0")
    trees, C = 15, 3
    nodes = ta.synth_forest(trees, D, cols, seed=cols + D)
    by_tree = nodes.reshape(trees, nodes.size // trees)

    def want(d):
        margins = np.stack([oracle.predict(np.ascontiguousarray(by_tree[c::C]).reshape(-1), trees // C, D, d, MISSING)[0] for c in range(C)],
                           axis=1)
        return margins, oracle.predict(nodes, trees, D, d, MISSING, want_leaf=True)[1]

    check_dense(env, nodes, trees, D, cols, "qring_region3", key=("mc", D, cols), num_classes=C, want_fn=want)


@pytest.mark.parametrize("D", [12, 3])
@pytest.mark.parametrize("cols", EVEN_COLS + ODD_COLS)
def test_tile_staging_sparse(env, cols, D):
    """sparse_q_kernel on a converted forest with early leaves."""
    ta, oracle, torch = env
    nodes = ta.synth_forest(T, D, cols, seed=cols + D, leaf_prob=0.1)
    sn, tr = ta.capi.dense_to_sparse(nodes, T, D)
    batches = [rows_for(ta, nodes, r, cols, ms, ("sparse", D, cols)) for r in ROWS for ms in (False, True)]
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING)
    f.set_strategy(ta.STRATEGY_QRING)
    try:
        run(env, f, lambda d: oracle.sparse_predict(sn, tr, d, MISSING, want_leaf=True), batches, "sparse_qring")
    finally:
        f.close()


@pytest.mark.parametrize("chains", [3, 2])
@pytest.mark.parametrize("cols", [18, 256, 255])
def test_regions_past_a_smaller_batch_hold_an_earlier_one(env, monkeypatch, chains, cols):
    """One handle predicts 385 rows and then 65: the regions past the second batch hold the first batch's codes."""
    ta = env[0]
    monkeypatch.setenv("TAHOE_QRING_CHAINS", str(chains))
    monkeypatch.setenv("TAHOE_QRING_CODE8", "0")
    monkeypatch.setenv("TAHOE_QRING_NARROW128", "0")
    nodes = plain_forest(ta, 12, cols, seed=9)
    check_dense(env, nodes, T, 12, cols, "qring_region%d" % chains, key=("plain9", cols), row_counts=(385, 65))


# ------------------------------------------------------------------------------------------------ table staging
def forest_with_tables(ta, trees, D, cols, counts, seed):
    """A forest of `trees` trees of depth D in which feature c has exactly counts[c] distinct thresholds."""
    nodes = ta.synth_forest(trees, D, cols, seed=seed)
    inner = inner_of(nodes)
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.sum() <= inner.size and (counts > 0).any()
    used = np.flatnonzero(counts > 0)
    order = rng.permutation(inner)
    # the first sum(counts) nodes carry each threshold once, the rest repeat thresholds of the used features
    fid = np.concatenate([np.repeat(np.arange(cols), counts), rng.choice(used, size=inner.size - counts.sum())])
    val = np.empty(inner.size, dtype=np.float32)
    tables = [np.unique(rng.uniform(-4.0, 4.0, size=2 * n + 8).astype(np.float32))[:n] for n in counts]
    assert all(t.size == n for t, n in zip(tables, counts))
    at = 0
    for c in range(cols):
        val[at:at + counts[c]] = tables[c]
        at += counts[c]
    rest = fid[at:]
    val[at:] = [tables[c][rng.integers(0, counts[c])] for c in rest]
    set_fid(nodes, order, fid)
    nodes["val"][order] = val
    got = [np.unique(nodes["val"][inner][fids(nodes)[inner] == c]).size for c in range(cols)]
    assert got == list(counts), (got, list(counts))
    return nodes


def check_tables(env, monkeypatch, nodes, trees, D, cols, key, knobs_=()):
    monkeypatch.setenv("TAHOE_QRING_CHAINS", "3")
    monkeypatch.setenv("TAHOE_QRING_CODE8", "0")
    monkeypatch.setenv("TAHOE_QRING_NARROW128", "0")
    for k, v in knobs_:
        monkeypatch.setenv(k, v)
    check_dense(env, nodes, trees, D, cols, "qring_region3", key=key, row_counts=(193, 385))


@pytest.mark.parametrize("buckets", ["1", "0"])
def test_threshold_counts_mod_four(env, monkeypatch, buckets):
    """Pairs (4, 5), (6, 7), (5, 4), (7, 6) and (40, 43), (42, 41): every residue in either position.  With the bucket form and,
    TAHOE_QUANT_BUCKETS=0, with the search trees."""
    ta = env[0]
    counts = [4, 5, 6, 7, 5, 4, 7, 6, 40, 43, 42, 41]
    nodes = forest_with_tables(ta, T, 6, len(counts), counts, seed=4)
    check_tables(env, monkeypatch, nodes, T, 6, len(counts), ("mod4", buckets), [("TAHOE_QUANT_BUCKETS", buckets)])


def test_empty_table_beside_a_crowded_one(env, monkeypatch):
    """No threshold on feature 0 beside 3000 on feature 1 (the first pair); 3000 on feature 6 beside none on feature 7 (the last)."""
    ta = env[0]
    counts = [0, 3000, 30, 31, 32, 33, 3000, 0]
    nodes = forest_with_tables(ta, 15, 12, 8, counts, seed=6)
    check_tables(env, monkeypatch, nodes, 15, 12, 8, "empty")


@pytest.mark.parametrize("n", [19000, 30000])
def test_crowded_pair(env, monkeypatch, n):
    """2 x 19 000 thresholds in one pair: the bucket count must drop below 4096 for the pair's image to fit LDS.  2 x 30 000: no
    bucket count fits, the two-pass search-tree kernel serves."""
    ta = env[0]
    counts = [7, 9, n, n, 11, 6]
    nodes = forest_with_tables(ta, 15, 12, 6, counts, seed=n)
    check_tables(env, monkeypatch, nodes, 15, 12, 6, ("crowded", n))


def test_small_tables_many_features_per_workgroup(env, monkeypatch):
    """TAHOE_QUANT_MULTI=1 on 32 features with a handful of thresholds each."""
    ta = env[0]
    counts = [1 + (c * 7) % 13 for c in range(32)]
    nodes = forest_with_tables(ta, T, 6, 32, counts, seed=12)
    check_tables(env, monkeypatch, nodes, T, 6, 32, "multi", [("TAHOE_QUANT_MULTI", "1")])
