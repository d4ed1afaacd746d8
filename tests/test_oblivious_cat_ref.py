"""tests/oblivious_cat_ref.py against the independent restatement of the categorical sparse walk (tests/categorical_ref.py) on the
expansion, and the two identities that let a numeric oblivious handle stand in as the reference of a categorical one.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref  # noqa: E402
import oblivious_cat_ref as ocr  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402

MISSING = obr.MISSING
W = 3


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("depths", [[0, 1, 2, 6, 3], [4, 0, 5, 1, 2, 3, 2]])
def test_the_rule_equals_the_sparse_walk_on_the_expansion(depths, k):
    forest = ocr.sets_forest(depths, 6, k, seed=7 + k)
    assert any(ocr.nwords_of(c) >= 2 for c in forest["cats"].values()) and any(not c for c in forest["cats"].values())
    data = ocr.sets_data(200, 6, seed=3)
    sums, leaf = ocr.cat_ref(forest, data)
    nodes, trees, categories, members_left, _ = ocr.expand_to_sparse(forest)
    # the C struct's arrays of the expansion's splits
    keys = sorted(categories)
    nw = [ocr.nwords_of(categories[i]) for i in keys]
    offset = np.concatenate([[0], np.cumsum(nw)]).astype(np.int64)
    words = np.zeros(max(int(offset[-1]), 1), np.uint32)
    for i, node in enumerate(keys):
        for c in categories[node]:
            words[offset[i] + c // 32] |= np.uint32(1 << (c % 32))
    ml = np.array([node in set(members_left) for node in keys], np.uint8)
    want, want_leaf = categorical_ref.predict(nodes, trees, data, MISSING, keys, offset, words, ml, num_classes=k)
    assert same_bits(sums, np.asarray(want).reshape(sums.shape))
    assert np.array_equal(ocr.sparse_leaf_to_oblivious(want_leaf, forest), leaf)
    for c in range(1, k):  # every output's tree takes the same path
        assert np.array_equal(want_leaf[:, c::k], want_leaf[:, ::k])


def test_without_sets_the_rule_is_the_numeric_one():
    forest = obr.make_forest([0, 3, 5, 1], 4, 2, seed=5)
    data = obr.make_data(150, 4, seed=6)
    a, b = ocr.cat_ref(forest, data), obr.ref_of(forest, data)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_seam_feeds_the_sets_to_the_restatements_and_comes_off_again():
    forest = ocr.sets_forest([3, 2], 3, 1, seed=1)
    data = ocr.sets_data(40, 3, seed=2)
    before = osr._bits, obr.ref_of
    with ocr.seam():
        assert np.array_equal(obr.ref_of(forest, data)[1], ocr.cat_ref(forest, data)[1])
        assert np.array_equal(osr._bits(forest, slice(0, 3), data, MISSING), ocr.cat_bits(forest, slice(0, 3), data, MISSING))
        plain = ocr.numeric_part(forest)
        assert np.array_equal(obr.ref_of(plain, data)[1], before[1](plain, data)[1])
    assert (osr._bits, obr.ref_of) == before


def one_level(k, left):
    """One tree of one level on feature 0 with the integer threshold k, and its categorical twin"""
    forest = dict(depths=np.array([1], np.int32), fids=np.array([0]), thr=np.array([k], np.float32), def_left=np.array([k % 2 == 0]),
                  leaves=np.array([1.0, 2.0], np.float32), k=1, cols=1)
    return forest, (ocr.members_left_of if left else ocr.members_right)(forest, W)


BELOW = np.array([-np.inf, -1e30, -2.7, -1.0, -0.5, -0.0, 0.0, 0.5, 2.7, np.nan, MISSING,
                  np.nextafter(np.float32(MISSING), np.float32(0))] + [c + d for c in range(32 * W) for d in (0.0, 0.5)], np.float32)
BELOW = BELOW[~(BELOW >= 32 * W)]
NONNEG = np.array([0.0, -0.0, 0.5, 2.7, 32.0 * W, 32.0 * W + 0.5, 1e6, 2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 32, 3e38, np.inf,
                   MISSING] + [c + d for c in range(32 * W) for d in (0.0, 0.5)], np.float32)


def test_identity_members_right_for_every_threshold():
    """x >= k <=> member of {c : k <= c < 32 W}, for every x below 32 W: negatives, +-0.0, non-integers, -inf, NaN, the sentinel"""
    data = BELOW.reshape(-1, 1)
    for k in range(1, 32 * W):
        numeric, cat = one_level(k, left=False)
        assert np.array_equal(ocr.cat_ref(cat, data)[1], obr.ref_of(numeric, data)[1]), k


def test_identity_members_left_for_every_threshold():
    """x >= k <=> not member of {c : c < k} (members_left), for x >= 0, values past the words, >= 2^24, +inf and the sentinel"""
    data = NONNEG.reshape(-1, 1)
    for k in range(1, 32 * W):
        numeric, cat = one_level(k, left=True)
        assert np.array_equal(ocr.cat_ref(cat, data)[1], obr.ref_of(numeric, data)[1]), k


def test_what_the_identities_exclude_does_differ():
    numeric, cat = one_level(5, left=False)
    x = np.array([[32.0 * W]], np.float32)  # past the words: never a member, but >= 5
    assert ocr.cat_ref(cat, x)[1][0, 0] == 0 and obr.ref_of(numeric, x)[1][0, 0] == 1
    numeric, cat = one_level(5, left=True)
    for v in (-1.0, np.nan, np.nextafter(np.float32(MISSING), np.float32(0))):  # no member goes right, but is not >= 5
        x = np.array([[v]], np.float32)
        assert ocr.cat_ref(cat, x)[1][0, 0] == 1 and obr.ref_of(numeric, x)[1][0, 0] == 0, v


def test_identity_data_stays_inside_what_each_identity_allows():
    for w in (1, 3):
        a = ocr.identity_data(130, 4, w, seed=1, left=False)
        assert not (a >= 32 * w).any() and np.isnan(a).any() and (a < 0).any()
        b = ocr.identity_data(130, 4, w, seed=2, left=True)
        ok = (b >= 0) | (np.abs(b - np.float32(MISSING)) <= np.float32(1e-6))
        assert ok.all() and (b >= 2.0 ** 24).any() and (b == 32 * w).any()
