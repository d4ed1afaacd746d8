"""Packed tops of the 192-row QRING tile, bit for bit against the CPU oracle.  Needs an MI355X.

A handle whose large tile is the 192-row tile on u16 codes keeps every tree's top twice: as u32 node words, and packed to three
bytes per node without def_left.  A tile in whose quantise chunks no missing value was seen stages the packed top (three 16-byte
loads per lane) and expands it to node words on the way to LDS; a tile with a missing value stages the u32 top.  What can break
is the packing (every bit of the fid, the code bytes, the node a lane's twelve dwords put where), short tops whose chunk offsets
are clamped, the choice per tile, and the first and last tree of a walker.  Every case runs with the packed tops and with
TAHOE_QRING_TOP24=0, asserts the kernel form, compares float32 sums and leaf indices bitwise with the oracle and checks the
handle's error flag; the handle's device bytes prove that the packed tops were built."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MISSING = -999.0
COLS = 130  # just past the six-region form
KNOBS = ("TAHOE_QUANT_MULTI", "TAHOE_QUANT_BUCKETS", "TAHOE_QRING_CHAINS", "TAHOE_QRING_REGIONS", "TAHOE_QRING_SLICES",
         "TAHOE_QRING_WIDE", "TAHOE_QRING_WIDE_CHAINS", "TAHOE_QRING_CODE8", "TAHOE_QRING_GROUPS", "TAHOE_QRING_TOP24",
         "TAHOE_QRING_NARROW128")
FORM = "qring_region3"


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
    monkeypatch.setenv("TAHOE_QRING_CHAINS", "3")  # 192-row tiles from small batches
    monkeypatch.setenv("TAHOE_QRING_CODE8", "0")   # u16 codes whatever the tables' sizes


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def inner_of(nodes):
    return np.flatnonzero((nodes["bits"].view(np.uint32) >> 31) == 0)


def fids(nodes):
    return nodes["bits"].view(np.uint32) & np.uint32((1 << 30) - 1)


def forest(ta, T, D, cols=COLS, seed=1, crowd=0):
    """T random trees of depth D; `crowd` inner nodes are moved to feature 0 (a table of thousands of thresholds)."""
    nodes = ta.synth_forest(T, D, cols, seed=seed)
    inner = inner_of(nodes)
    if crowd:
        pick = np.random.default_rng(seed).choice(inner, size=min(crowd, inner.size), replace=False)
        nodes["bits"].view(np.uint32)[pick] &= np.uint32(0xC0000000)  # fid 0, def_left and the leaf flag kept
    return nodes


_DATA = {}


def shared_rows(ta, rows, cols, missing):
    """The rows of a case, drawn once per (rows, cols, missing) and left unchanged."""
    key = (rows, cols, missing)
    if key not in _DATA:
        d = (ta.synth_data(rows, cols, seed=100 + rows, missing_prob=0.05, missing=MISSING, nan_prob=0.01) if missing
             else ta.synth_data(rows, cols, seed=100 + rows))
        assert (d == np.float32(MISSING)).any() == missing
        d.setflags(write=False)
        _DATA[key] = d
    return _DATA[key]


def top24_bytes(T, top_levels):
    """Device bytes of the packed tops: per tree the 16-byte chunks the walkers' lanes load (groups of four nodes, 12 bytes each,
    lane l's groups l, 64 + l, ... in its chunks l, 64 + l, ...)."""
    n_groups = max(1, (1 << top_levels) // 4)
    chunks = n_groups if n_groups <= 64 else (n_groups // 64 * 3 + 3) // 4 * 64
    return T * chunks * 16


def check(env, monkeypatch, nodes, T, D, cols, batches, num_classes=1, want_fn=None):
    """Every batch through predict_raw and predict_leaf_idx of a QRING handle == the oracle, with the packed tops and without."""
    ta, oracle, torch = env
    want = [(want_fn or (lambda d: oracle.predict(nodes, T, D, d, MISSING, want_leaf=True)))(d) for d in batches]
    device_bytes = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("TAHOE_QRING_TOP24", knob)
        f = ta.Forest(nodes, T, D, cols, missing=MISSING, num_classes=num_classes)
        f.set_strategy(ta.STRATEGY_QRING)
        try:
            device_bytes[knob] = f.info().device_bytes
            top_levels = f.info().top_levels
            assert top_levels == min(D - 2, 10)
            for data, (want_sums, want_leaf) in zip(batches, want):
                rows = data.shape[0]
                assert f.kernel_form(rows) == FORM, (f.kernel_form(rows), rows)
                x = torch.from_numpy(data.copy()).cuda()
                raw = f.predict_raw(x)
                f.check()
                leaf, sums = f.predict_leaf_idx(x)
                f.check()
                label = f"TOP24={knob}, {T} trees, depth {D}, {cols} features, {rows} rows"
                assert np.array_equal(bits(raw.cpu().numpy()), bits(want_sums)), f"{label}: predict_raw differs"
                assert np.array_equal(bits(sums.cpu().numpy()), bits(want_sums)), f"{label}: sums of the leaf pass differ"
                assert np.array_equal(bits(leaf.cpu().numpy()), want_leaf), f"{label}: leaf indices differ"
        finally:
            f.close()
    assert device_bytes["1"] - device_bytes["0"] == top24_bytes(T, top_levels), "the packed tops' bytes (were they built?)"


@pytest.mark.parametrize("D", [12, 3, 4, 5, 6, 14])
def test_tops(env, monkeypatch, D):
    """The full 1023-node top (depth 12), one- to four-level tops whose chunk offsets are clamped (depths 3 to 6), and depth 14:
    heap levels between top and blocks.  17 trees: walkers with two trees and with one."""
    ta = env[0]
    nodes = forest(ta, 17, D, seed=D, crowd=3000 if D >= 12 else 0)
    check(env, monkeypatch, nodes, 17, D, COLS, [shared_rows(ta, 193, COLS, False), shared_rows(ta, 193, COLS, True)])


def test_every_bit_of_the_fid(env, monkeypatch):
    """256 features; a third of the inner nodes split on features 0, 127, 128 and 255 (the roots too)."""
    ta = env[0]
    T, D, cols = 17, 12, 256
    nodes = forest(ta, T, D, cols=cols, seed=31)
    inner = inner_of(nodes)
    rng = np.random.default_rng(31)
    pick = np.union1d(rng.choice(inner, size=inner.size // 3, replace=False), np.arange(T) * (nodes.size // T))
    b = nodes["bits"].view(np.uint32)
    b[pick] = (b[pick] & np.uint32(0xC0000000)) | rng.choice(np.array([0, 127, 128, 255], dtype=np.uint32), size=pick.size)
    assert set(np.unique(fids(nodes)[np.arange(T) * (nodes.size // T)])) <= {0, 127, 128, 255}
    assert {0, 127, 128, 255} <= set(np.unique(fids(nodes)[inner]))
    check(env, monkeypatch, nodes, T, D, cols, [shared_rows(ta, 193, cols, False), shared_rows(ta, 193, cols, True)])


def test_codes(env, monkeypatch):
    """Feature 0 with exactly 32 767 distinct thresholds: every code 0x0001 .. 0x7FFF is some node's, 0x00FF, 0x7F00 and 0x7FFF
    among them (a code's high byte is 0xFF only in 0xFFFF, the code of a NaN threshold: there are NaN thresholds, one at a
    root).  Row values equal to thresholds: ties."""
    ta = env[0]
    T, D = 29, 12
    nodes = forest(ta, T, D, seed=77)
    inner = inner_of(nodes)
    b = nodes["bits"].view(np.uint32)
    on0 = inner[fids(nodes)[inner] == 0]
    b[on0] |= np.uint32(1)  # feature 0 belongs to the crowd alone
    rng = np.random.default_rng(77)
    pick = rng.choice(inner[inner != 0], size=32767, replace=False)
    b[pick] &= np.uint32(0xC0000000)
    nodes["val"][pick] = rng.permutation(np.linspace(-3.0, 3.0, 32767).astype(np.float32))
    assert np.unique(nodes["val"][pick]).size == 32767
    per_tree = nodes.size // T
    nan_at = np.concatenate(([0], rng.choice(np.setdiff1d(inner, pick), size=40, replace=False)))
    nan_at = nan_at[np.isin(nan_at, inner)]
    nodes["val"][nan_at] = np.nan
    assert per_tree > 0 and np.isnan(nodes["val"][0])
    data = shared_rows(ta, 193, COLS, False).copy()
    some = rng.choice(inner, size=600, replace=False)  # ties: a row's value on a node's feature = that node's threshold
    some = some[~np.isnan(nodes["val"][some])]
    data[rng.integers(0, 193, size=some.size), fids(nodes)[some].astype(np.int64)] = nodes["val"][some]
    with_missing = shared_rows(ta, 193, COLS, True).copy()
    with_missing[:, 0] = data[:, 0]
    with_missing[5, 0] = MISSING
    check(env, monkeypatch, nodes, T, D, COLS, [data, with_missing])


@pytest.mark.parametrize("T", [1, 13, 14, 15, 28, 29, 43])
def test_trees_per_walker(env, monkeypatch, T):
    """14 walkers with zero, one, two and three trees each: no steady-state iteration, and exactly one."""
    ta = env[0]
    nodes = forest(ta, T, 12, seed=T, crowd=3000)
    check(env, monkeypatch, nodes, T, 12, COLS, [shared_rows(ta, 193, COLS, False), shared_rows(ta, 193, COLS, True)])


def test_rows(env, monkeypatch):
    """Partial chains, a tile boundary, two tiles and a ragged third."""
    ta = env[0]
    nodes = forest(ta, 29, 12, seed=7, crowd=3000)
    check(env, monkeypatch, nodes, 29, 12, COLS, [shared_rows(ta, r, COLS, False) for r in (1, 191, 192, 193, 2 * 192 + 17)])


def test_both_tops_in_one_launch(env, monkeypatch):
    """A launch whose tiles stage both kinds of top, whatever the quantise pass's chunk size.  The pass reports "missing seen" per
    chunk of 2^c rows, 512 <= 2^c <= 65 536 (kQuantMinRowsPerBlock, kQuantMaxShift; c depends on the tables' bytes and the batch),
    chunks starting at multiples of 2^c.  Three spans of 65 536 rows: none of the first and third span's rows has a missing value,
    every 512th row of the second has one.  For every possible c rows 65 536 and 131 072 are chunk boundaries, every chunk of
    the second span has the flag and no chunk outside it has.  Neither boundary is a multiple of 192 (65 536 = 341 x 192 + 64,
    131 072 = 682 x 192 + 128): tile 341 straddles an unflagged and a flagged chunk, tile 682 a flagged and an unflagged one,
    both stage the u32 top as tiles 342 .. 681 do, and tiles 0 .. 340 and 683 .. 1024 stage packed tops (the last one ragged)."""
    ta = env[0]
    T, span = 15, 65536
    rows = 3 * span + 17
    nodes = forest(ta, T, 12, seed=9, crowd=3000)
    data = shared_rows(ta, rows, COLS, False).copy()
    flagged = span + 7 + 512 * np.arange(span // 512)
    data[flagged, 3] = MISSING
    assert span % 192 == 64 and (2 * span) % 192 == 128 and flagged.min() >= span and flagged.max() < 2 * span
    assert all(np.unique(flagged >> c).size == span >> c for c in range(9, 17)), "every chunk of the second span, for every chunk size"
    assert not (data[:span] == np.float32(MISSING)).any() and not (data[2 * span:] == np.float32(MISSING)).any()
    check(env, monkeypatch, nodes, T, 12, COLS, [data])


def test_missing_in_one_row_none_and_everywhere(env, monkeypatch):
    """Eight tiles (1536 rows) with the missing value in one row of a middle tile, with none, and with missing values in every tile.
    A single missing value flags its whole quantise chunk, at least 512 rows and here most likely the whole batch: which tiles
    besides the one take the u32 top depends on the chunk size (test_both_tops_in_one_launch does not)."""
    ta = env[0]
    nodes = forest(ta, 29, 12, seed=9, crowd=3000)
    none = shared_rows(ta, 1536, COLS, False)
    one = none.copy()
    one[700, 3] = MISSING
    check(env, monkeypatch, nodes, 29, 12, COLS, [one, none, shared_rows(ta, 1536, COLS, True)])


def test_multiclass(env, monkeypatch):
    """Three classes of 15 trees on the multi-class instantiation."""
    ta, oracle, _ = env
    T, C, D = 45, 3, 12
    nodes = forest(ta, T, D, seed=45, crowd=3000)
    by_tree = nodes.reshape(T, nodes.size // T)

    def want(d):
        margins = np.stack([oracle.predict(np.ascontiguousarray(by_tree[c::C]).reshape(-1), T // C, D, d, MISSING)[0] for c in range(C)], axis=1)
        return margins, oracle.predict(nodes, T, D, d, MISSING, want_leaf=True)[1]

    check(env, monkeypatch, nodes, T, D, COLS, [shared_rows(ta, 193, COLS, False), shared_rows(ta, 193, COLS, True)], num_classes=C, want_fn=want)


def test_two_groups_continued_sum(env, monkeypatch):
    """TAHOE_QRING_GROUPS=2: two tree groups, each with its own packed tops, the second continuing the first's sums; the whole
    continuing a given start (predict_accumulate)."""
    ta, oracle, torch = env
    T, D = 29, 12
    monkeypatch.setenv("TAHOE_QRING_GROUPS", "2")
    nodes = forest(ta, T, D, seed=21, crowd=3000)
    start = np.random.default_rng(5).standard_normal(401).astype(np.float32)
    got = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("TAHOE_QRING_TOP24", knob)
        f = ta.Forest(nodes, T, D, COLS, missing=MISSING)
        f.set_strategy(ta.STRATEGY_QRING)
        try:
            assert f.info().qring_groups == 2 and f.kernel_form(401) == FORM
            got[knob] = f.info().device_bytes
            for ms in (False, True):
                data = shared_rows(ta, 401, COLS, ms)
                want = oracle.predict_continue(nodes, T, D, data, MISSING, start.copy())
                sums = torch.from_numpy(start.copy()).cuda()
                f.predict_accumulate(torch.from_numpy(data.copy()).cuda(), sums)
                f.check()
                assert np.array_equal(bits(sums.cpu().numpy()), bits(want)), f"TOP24={knob}, missing={ms}: continued sums differ"
        finally:
            f.close()
    assert got["1"] - got["0"] == top24_bytes(T, 10)
