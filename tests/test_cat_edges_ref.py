"""The decoder forests of tests/cat_edges.py without a GPU: the closed form against answers typed by hand, then against the two
restatements of the rule that the other categorical tests rest on -- tests/categorical_ref.py on every generated sparse forest
under every sentinel, leaf for leaf and bit for bit, and tests/oblivious_cat_ref.py on the oblivious decoder -- so that the three
and the documented rule agree on every edge before a kernel is judged by the closed form."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cat_edges as ce  # noqa: E402
import categorical_ref  # noqa: E402
import oblivious_cat_ref as ocr  # noqa: E402

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dtype():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd.capi.SPARSE_NODE_DTYPE


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def forests(dtype):
    return (ce.neighbour_forests(dtype) + ce.ends_forests(dtype)
            + [ce.depth_forest(dtype, (0, 1, 2, 254, 255, 256, 257, 300), (1, 7, 8, 9, 10))])


# ---- the closed form itself ----
def hand_forest(dtype):
    """Four stumps (the categorical node is the root, its leaves at 1 and 2) on columns 1..4:
    {31} members right, default right | {32} members LEFT, default right | {0..31} members right, def_left | {} members LEFT, def_left"""
    trees = [ce.Tree(ce.single(31), False, False), ce.Tree(ce.single(32), True, False), ce.Tree(ce.ones(1), False, True),
             ce.Tree(ce.empty(0), True, True)]
    return ce.DecoderForest(dtype, trees, name="hand")


TINY = 2.0 ** -149
HAND_ROWS = [  # (x1, x2, x3, x4) with the sentinel 5.0 -> leaf per tree, sum = 1 * b0 + 2 * b1 + 4 * b2 + 8 * b3
    ((31.0, 32.0, 5.0, 7.0), (2, 1, 1, 2), 9.0),            # members; tree 2: 5 is a member AND the sentinel: missing wins, def_left
    ((31.99999, 31.5, -0.0, NAN), (2, 2, 2, 2), 15.0),      # truncation; 31 is no member of {32}; -0.0 is category 0; NaN: no member
    ((32.0, 64.0, 32.0, 5.0), (1, 2, 1, 1), 2.0),           # 32 W is past the words; tree 3: the sentinel on an empty set, def_left
    ((-TINY, 2.0 ** 24 + 32, TINY, -1.0), (1, 2, 2, 2), 14.0),  # a negative denormal is no member, a positive one is category 0
    ((INF, 4.0, 2.0 ** 24, -INF), (1, 2, 1, 2), 10.0),      # infinities and 2^24 are no members
]


@pytest.mark.parametrize("nan_missing", [False, True])
def test_closed_form_against_answers_typed_by_hand(dtype, nan_missing):
    f = hand_forest(dtype)
    assert f.left_pos == [1, 1, 1, 1] and f.node.tolist() == [0, 3, 6, 9] and f.offset.tolist() == [0, 1, 3, 4, 4]
    assert f.words[:4].tolist() == [1 << 31, 0, 1, 0xffffffff] and f.ml.tolist() == [0, 1, 0, 1]
    data = np.full((len(HAND_ROWS), f.cols), 0.5, np.float32)
    data[:, 0] = 0.0
    data[:, 1:5] = np.array([r[0] for r in HAND_ROWS], np.float32)
    want_leaf = np.array([r[1] for r in HAND_ROWS], np.uint32)
    want_sum = np.array([r[2] for r in HAND_ROWS], np.float32)
    if nan_missing:  # row 1, tree 3: the NaN is missing and takes def_left
        want_leaf[1, 3], want_sum[1] = 1, 7.0
    right = f.goes_right(data, 5.0, nan_missing=nan_missing)
    assert np.array_equal(f.expected_leaf(right), want_leaf)
    assert np.array_equal(bits(f.expected_sums(right)), bits(want_sum))
    three = f.expected_sums(right, num_classes=3)  # trees 0 and 3 are class 0
    assert np.array_equal(three[0], np.float32([9.0, 0.0, 0.0])) and np.array_equal(three[3], np.float32([8.0, 2.0, 4.0]))


def test_missing_band_and_sentinels_by_hand():
    one = np.float32(1.0)
    x = np.array([0.0, -0.0, 1e-6, 2e-6, 5.0, np.nextafter(np.float32(5), np.float32(6)), NAN, INF, -INF, 3e38], np.float32)
    assert ce.is_missing(x, 0.0).tolist() == [True, True, True, False, False, False, False, False, False, False]
    assert ce.is_missing(x, 5.0).tolist() == [False, False, False, False, True, True, False, False, False, False]
    assert not ce.is_missing(x, NAN).any() and not ce.is_missing(x, INF).any()  # inf - inf is NaN: +inf is not in its own band
    assert ce.is_missing(x, NAN, nan_missing=True).tolist() == [False] * 6 + [True] + [False] * 3
    assert ce.is_missing(one * -999, -999.0) and not ce.is_missing(np.nextafter(np.float32(-999), np.float32(0)), -999.0)
    assert ce.is_member(0.0, {0}) and ce.is_member(-0.0, {0}) and ce.is_member(0.99, {0}) and not ce.is_member(-0.5, {0})
    assert ce.is_member(16777215.0, {(1 << 24) - 1}) and not ce.is_member(16777216.0, {1 << 24}) and not ce.is_member(NAN, {0})


def test_generators_cover_what_they_promise(dtype):
    xs = ce.sets_of_interest()
    assert {s.W for s in xs} == set(ce.WORDS)
    assert {min(s.members) for s in xs if len(s.members) == 1} >= {0, 1, 30, 31, 32, 33, 62, 63, 64, 95, 991, 1023, 1055}
    fs = ce.neighbour_forests(dtype)
    seen = {}
    for f in fs:
        assert f.T % 3 == 0 and f.T <= 24
        for k, t in enumerate(f.trees):
            if t.cset.name in {x.name for x in xs} and 0 < k < f.T - 1:
                nb = (f.trees[k - 1].cset.name, f.trees[k + 1].cset.name)
                seen.setdefault(t.cset.name, set()).add((nb, t.ml, t.dl))
    for x in xs:
        got = seen[x.name]
        assert {(ml, dl) for _, ml, dl in got} == set(ce.PAIRS), x
        assert {nb for nb, _, _ in got} >= {("ones/W3", "ones/W3"), ("empty/W2", "empty/W2")}, x
    ends = ce.ends_forests(dtype)
    assert [f.trees[-1].cset.W for f in ends] == [2, 2, 2, 0, 1, 33]
    assert all(f.node[0] == 0 and f.offset[0] == 0 for f in ends)
    data = fs[0].rows(5.0)
    assert data.shape[0] >= 257 and data.shape[0] % 64 and (data[:, 0] == 0).all()
    col = data[:, fs[0].fid[1]]  # bit0/W1
    for v in (0.0, 0.5, 31.0, 32.0, 33.0, 63.0, 64.0, 5.0, 2.0 ** 24):
        assert (col == np.float32(v)).any(), v
    assert np.isnan(col).any() and np.signbit(col[col == 0]).any()
    w = ce.widest_forest(dtype)
    assert w.words.size == (1 << 19) + 1 + 1 + 0 + 1 + 3 + 1 and w.words.nbytes <= 3 << 20


# ---- against the restatements ----
@pytest.mark.parametrize("missing", ce.SENTINELS, ids=str)
def test_closed_form_equals_categorical_ref(dtype, missing):
    for f in forests(dtype):
        data = f.rows(missing)
        assert data.shape[0] < 4000, f
        right = f.goes_right(data, missing)
        for nc in (1, 3):
            init = (np.arange(data.shape[0] * nc) % 5 - 7).astype(np.float32) if nc == 1 else None
            sums, leaf = categorical_ref.predict(f.sn, f.tr, data, missing, f.node, f.offset, f.words, f.ml, num_classes=nc, init=init)
            assert np.array_equal(leaf, f.expected_leaf(right)), ce.first_mismatch(f, data, f.expected_leaf(right), leaf)
            assert np.array_equal(bits(sums), bits(f.expected_sums(right, nc, init))), f


def test_closed_form_equals_categorical_ref_on_the_widest_set(dtype):
    f = ce.widest_forest(dtype)
    for missing in (-999.0, 0.0):
        data = f.rows(missing)
        right = f.goes_right(data, missing)
        sums, leaf = categorical_ref.predict(f.sn, f.tr, data, missing, f.node, f.offset, f.words, f.ml)
        assert np.array_equal(leaf, f.expected_leaf(right)), ce.first_mismatch(f, data, f.expected_leaf(right), leaf)
        assert np.array_equal(bits(sums), bits(f.expected_sums(right)))
    col = data[:, f.fid[1]]
    assert (col == np.float32(2 ** 24 - 1)).any() and (col == np.float32(2 ** 24 - 32)).any() and (col == np.float32(2 ** 24)).any()


def test_nan_missing_is_the_sentinel_in_place_of_every_nan(dtype):
    """categorical_ref knows no NaN flag; with a finite sentinel a NaN on a flagged handle is what the sentinel is on a plain one."""
    for f in ce.ends_forests(dtype) + ce.neighbour_forests(dtype)[:2]:
        data = f.rows(-999.0)
        assert np.isnan(data).any()
        right = f.goes_right(data, -999.0, nan_missing=True)
        _, leaf = categorical_ref.predict(f.sn, f.tr, np.where(np.isnan(data), np.float32(-999.0), data), -999.0, f.node, f.offset,
                                          f.words, f.ml)
        assert np.array_equal(leaf, f.expected_leaf(right))
        assert not np.array_equal(right, f.goes_right(data, -999.0))


@pytest.mark.parametrize("missing", (-999.0, 5.0, 0.0), ids=str)
def test_oblivious_decoder_equals_oblivious_cat_ref(missing):
    d = ce.oblivious_decoder()
    nw = [ocr.nwords_of(c) for c in d.cats.values()]
    kinds = "".join("p" if n >= 2 else "i" for n in nw)
    assert "pi" in kinds and "ip" in kinds and "pp" in kinds and "ii" in kinds  # inline and pooled records side by side
    assert {max(c) for c, n in zip(d.cats.values(), nw) if n == 1 and c} >= {0, 30, 31} and 32 in {max(c) for c in d.cats.values() if c}
    data = d.rows(missing)
    want_leaf = d.expected_leaf(data, missing)
    sums, leaf = ocr.cat_ref(d.forest(), data, missing)
    assert np.array_equal(leaf, want_leaf)
    assert np.array_equal(bits(sums[:, 0]), bits(d.expected_sums(want_leaf)))


def test_oblivious_decoder_by_hand():
    """Tree 0 of the decoder, levels 0..2: {32} pooled, members right, default right | {31} inline, members right, def_left |
    {0, 32} pooled, members LEFT, default right."""
    d = ce.oblivious_decoder()
    assert [sorted(c.members) for c, _, _ in d.trees[0][:3]] == [[32], [31], [0, 32]]
    assert [(ml, dl) for _, ml, dl in d.trees[0][:3]] == [(False, False), (False, True), (True, False)]
    x = np.full((4, d.cols), 0.5, np.float32)  # 0.5 is category 0: a member of {0, 32} only
    x[0, 1:4] = (32.0, 31.0, 32.5)    # right, right, member -> left
    x[1, 1:4] = (31.0, 32.0, 1.0)     # left, left, no member -> right
    x[2, 1:4] = (-999.0, -999.0, -999.0)  # default right, def_left, default right
    x[3, 1:4] = (64.0, 31.9, 64.0)    # past the words, category 31, past the words -> right
    leaf = d.expected_leaf(x, -999.0)
    assert (leaf[:, 0] & 7).tolist() == [0b011, 0b100, 0b101, 0b110]
