"""The QRING walkers' tree loop at its edges, bit for bit against the CPU oracle.  Needs an MI355X.

A walker's loop issues the previous tree's bottom-block gathers at the head of an iteration, prefetches the next top (its own
again on its last tree), walks, finishes the previous tree and commits the prefetched top; the first iteration gathers block 0
of its own tree and finishes nothing, an epilogue gathers and finishes the last tree.  What can break is a walker's first and
last iteration, so the forests are tiny: walkers with zero, one and two trees for 14 and for 15 walkers, with no steady-state
iteration and with exactly one; partial chains, a tile boundary and two tiles of rows; short tops, the 10-level top and the
heap levels between top and blocks; u16 and u8 codes; rows with and without the missing value (both bodies of the loop); tree
slices, classes, a continued sum, leaf indices; and the same loop in the wide-row kernel.  Every case asserts the kernel form
it was written for, compares float32 sums and leaf indices bitwise, and checks the handle's error flag."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MISSING = -999.0
COLS = 130  # more than 128 features: u16 codes run the 192-row (three chains) and the 128-row (two chains) region tiles
KNOBS = ("TAHOE_QUANT_MULTI", "TAHOE_QUANT_BUCKETS", "TAHOE_QRING_CHAINS", "TAHOE_QRING_REGIONS", "TAHOE_QRING_SLICES",
         "TAHOE_QRING_WIDE", "TAHOE_QRING_WIDE_CHAINS")


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta
    from oracle import oracle

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, oracle, torch


@pytest.fixture(autouse=True)
def clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def internal_mask(nodes):
    return (nodes["bits"].view(np.uint32) >> 31) == 0


def most_distinct(nodes, cols):
    """Largest number of distinct thresholds on one feature: <= 254 is a u8 table."""
    n = nodes[internal_mask(nodes)]
    fid = (n["bits"].view(np.uint32) & ((1 << 30) - 1)).astype(np.int64)
    return max((np.unique(n["val"][fid == f]).size for f in range(cols) if (fid == f).any()), default=0)


def forest(ta, T, D, cols=COLS, seed=1, crowd=0):
    """T random trees of depth D; `crowd` inner nodes are moved to feature 0 so that its table needs u16 codes whatever T is."""
    nodes = ta.synth_forest(T, D, cols, seed=seed)
    inner = np.flatnonzero(internal_mask(nodes))
    if crowd:
        pick = np.random.default_rng(seed).choice(inner, size=min(crowd, inner.size), replace=False)
        b = nodes["bits"].view(np.uint32)
        b[pick] &= np.uint32(0xC0000000)  # fid 0, def_left and the leaf flag kept
    dl = (nodes["bits"].view(np.uint32)[inner] >> 30) & 1
    assert inner.size < 8 or (dl.any() and not dl.all()), "def_left set and clear"
    return nodes


def rows_of(ta, rows, cols, seed, missing=True):
    if missing:
        return ta.synth_data(rows, cols, seed=seed, missing_prob=0.05, missing=MISSING, nan_prob=0.01)
    return ta.synth_data(rows, cols, seed=seed)


_DATA = {}


def shared_rows(ta, rows, cols, missing):
    """The rows of a case, drawn once per (rows, cols, missing) and left unchanged."""
    key = (rows, cols, missing)
    if key not in _DATA:
        _DATA[key] = rows_of(ta, rows, cols, 100 + rows, missing)
        if missing:
            assert (_DATA[key] == np.float32(MISSING)).any()
        _DATA[key].setflags(write=False)
    return _DATA[key]


def check(env, nodes, T, D, cols, form, row_counts, monkeypatch=None, chains=None, missing=(True, False)):
    """predict_raw and predict_leaf_idx (sums and leaves) of a QRING handle == the oracle, for every batch size, on rows with
    the missing value (MS body) and without (plain body)."""
    ta, oracle, torch = env
    if chains is not None:
        monkeypatch.setenv("TAHOE_QRING_CHAINS", str(chains))
    f = ta.Forest(nodes, T, D, cols, missing=MISSING)
    f.set_strategy(ta.STRATEGY_QRING)
    try:
        for rows in row_counts:
            assert f.kernel_form(rows) == form, (f.kernel_form(rows), form, rows)
            for ms in missing:
                data = shared_rows(ta, rows, cols, ms)
                want, want_leaf = oracle.predict(nodes, T, D, data, MISSING, want_leaf=True)
                x = torch.from_numpy(data.copy()).cuda()
                raw = f.predict_raw(x)
                f.check()
                leaf, sums = f.predict_leaf_idx(x)
                f.check()
                label = f"{form}, {T} trees, depth {D}, {rows} rows, missing={ms}"
                assert np.array_equal(bits(raw.cpu().numpy()), bits(want)), f"{label}: predict_raw differs"
                assert np.array_equal(bits(sums.cpu().numpy()), bits(want)), f"{label}: sums of the leaf pass differ"
                assert np.array_equal(bits(leaf.cpu().numpy()), want_leaf), f"{label}: leaf indices differ"
    finally:
        f.close()


TREES = [1, 13, 14, 15, 16, 28, 29, 31]


@pytest.mark.parametrize("chains", [3, 2])
@pytest.mark.parametrize("T", TREES)
def test_trees_per_walker_u16(env, monkeypatch, T, chains):
    """Depth 12 on u16 codes, the kernels of the flagship workload: 14 walkers (three chains) and 15 (two chains) with zero, one
    and two trees each.  193 rows: two tiles in either form, the second nearly empty."""
    ta = env[0]
    nodes = forest(ta, T, 12, seed=T, crowd=3000)
    assert most_distinct(nodes, COLS) > 254
    check(env, nodes, T, 12, COLS, "qring_region%d" % chains, (193,), monkeypatch, chains)


@pytest.mark.parametrize("chains", [3, 2])
@pytest.mark.parametrize("T", [1, 14, 15, 29])
def test_trees_per_walker_u8(env, monkeypatch, T, chains):
    """The same edges on u8 codes (384-row tiles of six chains with 14 walkers, 128-row tiles with 15)."""
    ta = env[0]
    nodes = forest(ta, T, 9, seed=40 + T)
    assert most_distinct(nodes, COLS) <= 254
    check(env, nodes, T, 9, COLS, "qring_region8", (193,), monkeypatch, chains)


@pytest.mark.parametrize("chains", [3, 2])
def test_rows_u16(env, monkeypatch, chains):
    """Partial chains, a tile boundary, two tiles."""
    ta = env[0]
    nodes = forest(ta, 29, 12, seed=7, crowd=3000)
    assert most_distinct(nodes, COLS) > 254
    check(env, nodes, 29, 12, COLS, "qring_region%d" % chains, (1, 64, 191, 192, 193, 385), monkeypatch, chains)


@pytest.mark.parametrize("chains", [3, 2])
@pytest.mark.parametrize("D,T,crowd,form", [(2, 30, 0, "qring_region8"), (3, 30, 0, "qring_region8"),
                                            (12, 17, 3000, "qring_region%d"), (14, 17, 0, "qring_region%d")])
def test_depths(env, monkeypatch, D, T, crowd, form, chains):
    """Short tops (depth 2 and 3: a root, or a root pair, above the bottom blocks), the 10-level top of depth 12, and depth 14:
    two levels from the quantised heap in global memory between the top and the blocks, loads that sit between the head's
    gathers and finish()."""
    ta = env[0]
    nodes = forest(ta, T, D, seed=D, crowd=crowd)
    assert (most_distinct(nodes, COLS) > 254) == (D >= 12)
    check(env, nodes, T, D, COLS, form % chains if "%d" in form else form, (193,), monkeypatch, chains)


@pytest.mark.parametrize("chains", [3, 2])
def test_u16_codes_on_sixteen_kib_regions(env, monkeypatch, chains):
    """16 trees of depth 12 over 8 features: thousands of thresholds per feature, six u16 chains on 16 KiB regions."""
    ta = env[0]
    nodes = forest(ta, 16, 12, cols=8, seed=3)
    assert most_distinct(nodes, 8) > 254
    check(env, nodes, 16, 12, 8, "qring_region6", (193, 385), monkeypatch, chains)


def test_tree_slices(env):
    """130 trees x 200 rows: every tile by two workgroups of 65 trees each (first tree of a walker = t_begin + wave), leaf values
    to the leaf buffer, ordered sum."""
    ta = env[0]
    nodes = forest(ta, 130, 8, seed=11)
    check(env, nodes, 130, 8, COLS, "qring_split", (200,))


@pytest.mark.parametrize("T", [45, 48])
def test_multiclass(env, T):
    """Three classes of 15 / 16 trees: class ends fall inside a round of the walkers and inside a batch of the consumer."""
    ta, oracle, torch = env
    C, D = 3, 8
    nodes = forest(ta, T, D, seed=T)
    data = shared_rows(ta, 193, COLS, True)
    by_tree = nodes.reshape(T, nodes.size // T)
    want = np.stack([oracle.predict(np.ascontiguousarray(by_tree[c::C]).reshape(-1), T // C, D, data, MISSING)[0] for c in range(C)], axis=1)
    want_leaf = oracle.predict(nodes, T, D, data, MISSING, want_leaf=True)[1]
    f = ta.Forest(nodes, T, D, COLS, missing=MISSING, num_classes=C)
    f.set_strategy(ta.STRATEGY_QRING)
    try:
        assert f.kernel_form(193).startswith("qring_region"), f.kernel_form(193)
        x = torch.from_numpy(data.copy()).cuda()
        raw = f.predict_raw(x)
        f.check()
        leaf, sums = f.predict_leaf_idx(x)
        f.check()
        assert np.array_equal(bits(raw.cpu().numpy()), bits(want)), "margins differ"
        assert np.array_equal(bits(sums.cpu().numpy()), bits(want)), "margins of the leaf pass differ"
        assert np.array_equal(bits(leaf.cpu().numpy()), want_leaf), "leaf indices differ"
    finally:
        f.close()


@pytest.mark.parametrize("chains", [3, 2])
def test_continued_sums(env, monkeypatch, chains):
    """predict_accumulate: the consumer starts from the sums of the trees before this forest (sums_in)."""
    ta, oracle, torch = env
    T, D = 29, 12
    monkeypatch.setenv("TAHOE_QRING_CHAINS", str(chains))
    nodes = forest(ta, T, D, seed=21, crowd=3000)
    data = shared_rows(ta, 385, COLS, True)
    start = np.random.default_rng(5).standard_normal(385).astype(np.float32)
    want = oracle.predict_continue(nodes, T, D, data, MISSING, start.copy())
    f = ta.Forest(nodes, T, D, COLS, missing=MISSING)
    f.set_strategy(ta.STRATEGY_QRING)
    try:
        assert f.kernel_form(385) == "qring_region%d" % chains
        sums = torch.from_numpy(start.copy()).cuda()
        f.predict_accumulate(torch.from_numpy(data.copy()).cuda(), sums)
        f.check()
        assert np.array_equal(bits(sums.cpu().numpy()), bits(want)), "continued sums differ"
    finally:
        f.close()


@pytest.mark.parametrize("cols,D,T", [(700, 9, 1), (700, 9, 15), (700, 9, 16), (700, 9, 31), (700, 12, 46),
                                      (3072, 8, 1), (3072, 8, 61), (3072, 8, 180), (3072, 8, 181), (3072, 8, 367)])
def test_wide_rows(env, cols, D, T):
    """The wide-row kernel has the same loop: one, 15, 16 and 31 iterations' worth of trees at one tree per wave, and at several
    trees per wave and chain a last iteration that is partly filled, exactly 15 full iterations, and one more."""
    ta = env[0]
    nodes = forest(ta, T, D, cols=cols, seed=T)
    check(env, nodes, T, D, cols, "qring_wide", (70,))
