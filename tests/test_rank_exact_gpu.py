"""Rank codes and 16-bit keys against a closed form.  Needs an MI355X.

The fast kernels do not compare floats: QRING walks on per-feature rank codes (quantize.hip), the row-streaming wide form on one
affine 16-bit key map with a float32 tie fallback (wkey.hip).  On the search-tree forests of tests/order_forests.py the leaf a
row ends in IS its rank, #{thresholds <= x}, and three rows per threshold put every tie and neighbouring compare on some
row's path -- so a wrong code, key or node compare is a wrong leaf index in a known column, reported as (feature, x, expected
rank, got rank).  Every case asserts the kernel form it was written for, compares leaf indices, sums and predict_raw with the
closed form bitwise (no tolerance, no skipped row), and runs DIRECT on the same handle as the float32 control.
tests/test_order_forests.py pins the closed form itself to the CPU oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import order_forests as O  # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ("TAHOE_QUANT_MULTI", "TAHOE_QUANT_BUCKETS", "TAHOE_QRING_CHAINS", "TAHOE_QRING_REGIONS", "TAHOE_WSTREAM")
REGION16 = ("qring_region2", "qring_region3", "qring_region_mixed")


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


@pytest.fixture(autouse=True)
def clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def quant_knobs(monkeypatch, form):
    """The quantise kernel a handle created next takes, given its column count: multi (16 / 8 features per workgroup),
    buckets (bucketed pair kernel), tree (search-tree pair kernel; odd num_cols: one feature per workgroup)."""
    monkeypatch.setenv("TAHOE_QUANT_MULTI", "1" if form == "multi" else "0")
    monkeypatch.setenv("TAHOE_QUANT_BUCKETS", "0" if form == "tree" else "1")


def region_form(of, chains=None, regions=True):
    """The QRING form of a narrow forest with too few trees for tree slices, from the rule of qring_build / qring_form."""
    if not regions:
        return ("qring_columns",), 128
    if of.most_distinct() <= 254:
        return ("qring_region8",), 384
    if of.cols <= 128:
        return ("qring_region6",), 384
    return (("qring_region%d" % chains,) if chains else REGION16), 192


class Expect:
    """Closed-form leaves and sums of one (forest, rows) pair, computed once and shared by the batches cut from it."""

    def __init__(self, of, data, missing, num_classes=1):
        self.of, self.data, self.missing, self.nc = of, data, missing, num_classes
        self.sparse = isinstance(of, O.SparseOrderForest)
        self.leaf = (O.sparse_expected_leaf if self.sparse else O.expected_leaf)(of, data, missing)
        self.sums = (O.sparse_expected_sums if self.sparse else O.expected_sums)(of, self.leaf, num_classes)

    def compare(self, f, x, idx, label, leaf_too=True):
        """predict_leaf_idx (leaves, sums) and predict_raw of handle f on device rows x == rows idx of the closed form."""
        want_leaf, want = self.leaf[idx], self.sums[idx]
        leaf, sums = f.predict_leaf_idx(x)
        raw = f.predict_raw(x)
        f.check()
        got_leaf = bits(leaf.cpu().numpy())
        report = O.sparse_first_mismatch if self.sparse else O.first_mismatch
        assert np.array_equal(got_leaf, want_leaf), f"{label}: " + report(self.of, self.data[idx], want_leaf, got_leaf)
        assert np.array_equal(bits(sums.cpu().numpy()), bits(want)), f"{label}: sums of the leaf pass differ"
        assert np.array_equal(bits(raw.cpu().numpy()), bits(want)), f"{label}: predict_raw differs"
        return raw


def check_case(env, case, forms, strategy=None, tile_rows=None, groups=None, counts=(None,), num_classes=1, stream=False):
    """Creates the handle (knobs are read here), asserts the kernel form of every batch, and compares every batch on `strategy`
    and on DIRECT with the closed form.  counts: batch sizes cut from the case's rows (None = all of them)."""
    ta, torch = env
    of, data, n_triples, missing = case
    exp = Expect(of, data, missing, num_classes)
    f = ta.Forest(of.nodes, of.T, of.D, of.cols, missing=missing, num_classes=num_classes)
    strategy = ta.STRATEGY_QRING if strategy is None else strategy
    info = f.info()
    if tile_rows == "wide":  # rows per tile of the wide form follow LDS and depth; GX has no tile
        assert (info.qring_tile_rows in (64, 32, 16)) == (forms == ("qring_wide",)) and (info.qring_tile_rows == 0) == (forms == ("qring_gx",))
    elif tile_rows is not None:
        assert info.qring_tile_rows == tile_rows, (info.qring_tile_rows, tile_rows)
    if groups is not None:
        assert info.qring_groups == groups, (info.qring_groups, groups)
    if stream:
        assert info.stream_slots >= 4, info.stream_slots
    for n in counts:
        idx = O.take_rows(data.shape[0], n_triples, data.shape[0] if n is None else n)
        x = torch.from_numpy(np.ascontiguousarray(data[idx])).cuda()
        for s in (strategy, ta.STRATEGY_DIRECT):
            f.set_strategy(s)
            form = f.kernel_form(idx.size)
            assert form in (forms if s == strategy else ("direct",)), (form, forms, idx.size)
            exp.compare(f, x, idx, f"{form}, {idx.size} rows")
    f.close()
    return exp


# ---- quantiser forms x code widths ----
QUANT_COLS = [(32, "multi"), (8, "multi"), (6, "buckets"), (6, "tree"), (7, "tree")]
# multi<4> | multi<2> | bucketed pair | search-tree pair | quantize_kernel<1> (odd num_cols)


@pytest.mark.parametrize("D", [7, 10])
@pytest.mark.parametrize("cols,quant", QUANT_COLS)
def test_quantiser_forms_and_code_widths(env, monkeypatch, cols, quant, D):
    """One search tree on every feature: 127 thresholds (u8 codes) and 1023 (u16), on each quantise kernel; batches of 1, 63, 511
    and 513 rows and three rows per threshold, so that 512-row chunks with and without a missing value both occur."""
    quant_knobs(monkeypatch, quant)
    case = O.quantiser_case(cols, D)
    forms, tile = region_form(case[0])
    assert forms == (("qring_region8",) if D == 7 else ("qring_region6",))
    check_case(env, case, forms, tile_rows=tile, groups=1, counts=(1, 63, 511, 513, None))


@pytest.mark.parametrize("cols,offset,D", [(32, 2, 10), (32, 1, 10), (6, 1, 10), (32, 2, 7), (6, 1, 7)])
def test_quantiser_forms_through_an_unaligned_pointer(env, cols, offset, D):
    """The batch 8 bytes into a buffer: no float4 loads, quantize_launch falls from the many-features kernel to the pair
    kernels; 4 bytes: to one feature per workgroup.  Same bits as the aligned call, which are the closed form's."""
    ta, torch = env
    of, data, n_triples, missing = O.quantiser_case(cols, D)
    exp = Expect(of, data, missing)
    idx = np.arange(data.shape[0])
    f = ta.Forest(of.nodes, of.T, of.D, cols, missing=missing)
    f.set_strategy(ta.STRATEGY_QRING)
    assert f.kernel_form(idx.size) in region_form(of)[0]
    x = torch.from_numpy(data).cuda()
    flat = torch.empty(data.size + offset, dtype=torch.float32, device="cuda")
    flat[offset:] = x.reshape(-1)
    shifted = flat[offset:].view(data.shape[0], cols)
    assert x.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 * offset
    aligned = exp.compare(f, x, idx, "aligned")
    moved = exp.compare(f, shifted, idx, f"{4 * offset} bytes into the buffer")
    assert np.array_equal(bits(moved.cpu().numpy()), bits(aligned.cpu().numpy()))
    f.close()


# ---- the u8 limit ----
@pytest.mark.parametrize("quant", ["buckets", "tree"])
def test_u8_limit_254_thresholds(env, monkeypatch, quant):
    """254 distinct thresholds on a feature are the last u8 table (code 255 = missing): a row above every threshold has rank
    254 and goes right everywhere, a missing row follows def_left.  One more distinct threshold and the handle leaves u8."""
    ta, torch = env
    quant_knobs(monkeypatch, quant)
    case = O.u8_limit_case(0)
    of, data = case[0], case[1]
    assert of.most_distinct() == 254 and (data[:, 0] == np.inf).any() and O.in_band(data[:, 0], case[3]).any()
    exp = check_case(env, case, ("qring_region8",), tile_rows=384, groups=1, counts=(None, 513))
    top = data[:, 0] == np.inf
    assert (exp.leaf[top, 0] == 254).all() and (exp.leaf[top, 1] == 254).all()  # 2^7 - 1 + 127 in both trees: code 254
    over = O.u8_limit_case(1)
    assert over[0].most_distinct() == 255
    check_case(env, over, ("qring_region6",), tile_rows=384, groups=1, counts=(None, 513))


# ---- table sizes around a power of two ----
@pytest.mark.parametrize("quant", ["buckets", "tree"])
@pytest.mark.parametrize("n", O.TABLE_SIZES)
def test_table_sizes_around_a_power_of_two(env, monkeypatch, n, quant):
    """Exactly n distinct thresholds on a feature (search trees of 2^p entries: n = 2^p - 1 fills one, n = 2^p needs the next),
    beside features with fewer: unequal pairs."""
    quant_knobs(monkeypatch, quant)
    case = O.table_size_case(n)
    forms, tile = region_form(case[0])
    assert forms == (("qring_region8",) if n <= 254 else ("qring_region6",))
    check_case(env, case, forms, tile_rows=tile, groups=1)


# ---- large tables ----
@pytest.mark.parametrize("quant", ["buckets", "tree"])
@pytest.mark.parametrize("kind,groups", [("pair", 1), ("together", 1), ("single", 1), ("groups", 2)])
def test_large_tables(env, monkeypatch, kind, groups, quant):
    """32767 distinct thresholds, the last u16 table.  pair: two such features do not fit LDS together (two passes of
    quantize_pair_kernel); together: a large and a small one do; single: num_cols = 1; groups: 65534 thresholds on one feature,
    two tree groups whose float32 sums chain.  Three rows per threshold."""
    quant_knobs(monkeypatch, quant)
    case = O.large_case(kind)
    assert case[0].most_distinct() == (65534 if kind == "groups" else 32767)
    check_case(env, case, ("qring_region6",), tile_rows=384, groups=groups)


# ---- threshold distributions aimed at the bucketed search ----
@pytest.mark.parametrize("quant", ["buckets", "tree"])
@pytest.mark.parametrize("kind", O.BUCKET_KINDS)
def test_bucketed_search_distributions(env, monkeypatch, kind, quant):
    """Thresholds on bucket edges, one very long run, all equal, only +-inf, denormals and both zeros, 80 decades, a range
    whose width overflows, the sentinel's band: every run boundary and the window padding, against the search-tree kernel."""
    quant_knobs(monkeypatch, quant)
    case = O.bucket_case(kind)
    forms, tile = region_form(case[0])
    check_case(env, case, forms, tile_rows=tile, groups=1)


# ---- levels ----
@pytest.mark.parametrize("setting", ["chains2", "chains3", "columns"])
@pytest.mark.parametrize("D", O.LEVEL_DEPTHS)
@pytest.mark.parametrize("cols", [256, 64])
def test_levels_of_the_walk(env, monkeypatch, cols, D, setting):
    """Depths around the 10-level LDS top: top only, heap levels in global memory, bottom blocks; on the u16 region forms with
    two and three chains, and on the 128-slot column layout."""
    if setting == "columns":
        monkeypatch.setenv("TAHOE_QRING_REGIONS", "0")
    else:
        monkeypatch.setenv("TAHOE_QRING_CHAINS", setting[-1])
    case = O.levels_case(cols, D)
    forms, tile = region_form(case[0], chains=int(setting[-1]) if setting != "columns" else None, regions=setting != "columns")
    check_case(env, case, forms, tile_rows=tile, groups=1)


# ---- tree slices ----
def test_tree_slices(env):
    """132 search trees of depth 8 on 18 features at 1000 rows: every tile by several workgroups, ordered sum kernel."""
    check_case(env, O.slices_case(), ("qring_split",), groups=1, counts=(1000,))


# ---- wide rows ----
@pytest.mark.parametrize("D", [9, 13])
@pytest.mark.parametrize("cols,form", [(700, "qring_wide"), (1200, "qring_wide"), (3072, "qring_wide"), (5000, "qring_gx")])
def test_wide_rows_on_rank_codes(env, cols, form, D):
    """The quantised wide forms and the GX form, levels past the LDS slots from the heap in global memory."""
    check_case(env, O.wide_case(cols, D), (form,), tile_rows="wide", groups=1)


@pytest.mark.parametrize("kind", O.STREAM_KINDS)
def test_row_streaming_keys_and_their_tie_fallback(env, monkeypatch, kind):
    """TAHOE_WSTREAM=1, num_cols = 1024: one affine 16-bit key map.  A fine grid where neighbouring thresholds share a key, a
    feature on a 1000 x larger scale, a constant feature: every threshold's tie and both neighbours decided on float32."""
    ta, torch = env
    monkeypatch.setenv("TAHOE_WSTREAM", "1")
    check_case(env, O.stream_case(kind), ("tilering_wide_stream",), strategy=ta.STRATEGY_TILERING, stream=True)


# ---- sparse handles ----
def check_sparse(env, sf, data, missing):
    ta, torch = env
    exp = Expect(sf, data, missing)
    idx = np.arange(data.shape[0])
    x = torch.from_numpy(data).cuda()
    f = ta.capi.SparseForest(sf.nodes, sf.roots, sf.cols, missing=missing)
    assert f.info().is_sparse == 1
    for s, form in ((ta.STRATEGY_QRING, "sparse_qring"), (ta.STRATEGY_TILEBLOCK, "sparse_top"),
                    (ta.STRATEGY_ROWTILE, "sparse_rowtile"), (ta.STRATEGY_DIRECT, "sparse_direct")):
        f.set_strategy(s)
        assert f.kernel_form(idx.size) == form
        exp.compare(f, x, idx, form)
    f.close()


@pytest.mark.parametrize("name,build,args", [("quantiser-6-10", O.quantiser_case, (6, 10)), ("quantiser-32-7", O.quantiser_case, (32, 7)),
                                             ("levels-64-12", O.levels_case, (64, 12)), ("table-257", O.table_size_case, (257,))])
def test_sparse_walk_on_converted_search_trees(env, name, build, args):
    """The balanced forests through dense_to_sparse: sparse_q_kernel and the float32 sparse kernels, leaf positions through the
    in-order leaf sequence."""
    ta, torch = env
    of, data, n_triples, missing = build(*args)
    sn, tr = ta.capi.dense_to_sparse(of.nodes, of.T, of.D)
    sf = O.sparse_from_dense(of, sn, tr)
    assert sf.nodes.tobytes() == sn.tobytes() and np.array_equal(sf.roots, tr)
    check_sparse(env, sf, data, missing)


@pytest.mark.parametrize("cols", [6, 255])
def test_sparse_walk_on_irregular_search_trees_and_vines(env, cols):
    """Unbalanced search trees and vines, 24 levels deep."""
    sf, data, n_triples, missing = O.irregular_case(cols)
    check_sparse(env, sf, data, missing)


# ---- multi-class ----
def test_multiclass_margins_are_per_class_closed_form_sums(env):
    """num_classes = 3: column c of the margins is the closed-form sum of the trees t % 3 == c, in tree order."""
    case = O.multiclass_case()
    check_case(env, case, ("qring_region8",), groups=1, num_classes=3, counts=(None, 513))
