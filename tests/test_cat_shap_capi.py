"""TAHOE_CREATE_CAT_CONTRIBS without a GPU: which creates take the flag, every refusal before a device is touched, the set algebra
of one path element checked edge by edge, and the float64 references of tests/cat_shap_ref.py against each other on the inputs
the GPU tests use."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cat_shap_cases as cases  # noqa: E402
import cat_shap_ref as cref  # noqa: E402
import categorical_ref  # noqa: E402

OK, INVALID_ARG, NO_DEVICE, INVALID_FOREST, UNSUPPORTED = 0, 1, 4, 6, 7
LEAF = np.int32(-(1 << 31))
MISSING = cases.MISSING


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def _has_gpu(ta):
    n = C.c_int(0)
    return ta.lib.tahoe_device_count(C.byref(n)) == 0 and n.value > 0


def _error(ta):
    return ta.lib.tahoe_last_error().decode()


def _create_cat(ta, sn, tr, cols, categories, left=(), flags=0, covers=None, num_classes=1, with_cats=True):
    """Status of tahoe_sparse_forest_create_cat; a created handle is destroyed."""
    sn = np.ascontiguousarray(sn, dtype=ta.capi.SPARSE_NODE_DTYPE)
    tr = np.ascontiguousarray(tr, dtype=np.int32)
    params = ta.ForestParams(int(sn.size), 0, int(tr.size), cols, 0, 0, 0.0, 0.0, 0, MISSING)
    cats, _keep = ta.capi.pack_categorical(categories, left)
    cv = None if covers is None else np.ascontiguousarray(covers, dtype=np.float32)
    h = C.c_void_p()
    st = ta.lib.tahoe_sparse_forest_create_cat(C.byref(h), tr.ctypes.data, sn.ctypes.data, cv.ctypes.data if cv is not None else None,
                                               C.byref(params), num_classes, flags, C.byref(cats) if with_cats else None)
    if st == OK:
        ta.lib.tahoe_forest_destroy(h)
    return st


def _stump(ta):
    sn = np.zeros(3, dtype=ta.capi.SPARSE_NODE_DTYPE)
    sn[0] = (0.5, 0, 1)
    sn[1] = (-1.0, LEAF, 0)
    sn[2] = (1.0, LEAF, 0)
    return sn, np.zeros(1, np.int32)


@pytest.mark.parametrize("with_cats", [True, False])
def test_the_flag_alone_is_refused_by_name(ta, with_cats):
    sn, tr = _stump(ta)
    assert ta.CREATE_CAT_CONTRIBS == 0x20
    st = _create_cat(ta, sn, tr, 2, {0: [1, 2]}, flags=ta.CREATE_CAT_CONTRIBS, covers=np.ones(3, np.float32), with_cats=with_cats)
    assert st == INVALID_ARG
    assert "TAHOE_CREATE_CAT_CONTRIBS" in _error(ta)


def test_every_other_create_refuses_the_flag(ta):
    sn, tr = _stump(ta)
    cv = np.ones(3, np.float32)
    params = ta.ForestParams(3, 0, 1, 2, 0, 0, 0.0, 0.0, 0, MISSING)
    h = C.c_void_p()
    for flags in (ta.CREATE_CAT_CONTRIBS, ta.CREATE_CAT_CONTRIBS | ta.CREATE_CONTRIBS):
        assert ta.lib.tahoe_sparse_forest_create_ex(C.byref(h), tr.ctypes.data, sn.ctypes.data, cv.ctypes.data, C.byref(params), 1,
                                                    flags) == INVALID_ARG
        assert not h.value
    nodes = ta.synth_forest(3, 2, 2, seed=1)
    dp = ta.ForestParams(0, 2, 3, 2, 0, 0, 0.0, 0.0, 0, MISSING)
    for flags in (ta.CREATE_CAT_CONTRIBS, ta.CREATE_CAT_CONTRIBS | ta.CREATE_CONTRIBS):
        assert ta.lib.tahoe_forest_create_ex(C.byref(h), nodes.ctypes.data, C.byref(dp), flags) == INVALID_ARG
        assert ta.lib.tahoe_forest_create_multiclass(C.byref(h), nodes.ctypes.data, C.byref(dp), 3, flags) == INVALID_ARG
        assert not h.value


@pytest.mark.parametrize("flags", ["contribs", "approx", "both"])
def test_splits_without_the_flag_stay_unsupported(ta, flags):
    sn, tr = _stump(ta)
    fl = {"contribs": ta.CREATE_CONTRIBS, "approx": ta.CREATE_APPROX_CONTRIBS,
          "both": ta.CREATE_CONTRIBS | ta.CREATE_APPROX_CONTRIBS}[flags]
    assert _create_cat(ta, sn, tr, 2, {0: [1, 2]}, flags=fl, covers=np.ones(3, np.float32)) == UNSUPPORTED


@pytest.mark.parametrize("flags", ["contribs", "approx"])
def test_bad_covers_are_refused_before_a_device(ta, flags):
    sn, tr = _stump(ta)
    fl = (ta.CREATE_CONTRIBS if flags == "contribs" else ta.CREATE_APPROX_CONTRIBS) | ta.CREATE_CAT_CONTRIBS
    for bad in (np.array([1, 0, 0], np.float32), np.array([1, -1, 2], np.float32), np.array([1, np.nan, 1], np.float32)):
        assert _create_cat(ta, sn, tr, 2, {0: [1, 2]}, flags=fl, covers=bad) == INVALID_FOREST
        assert "tree 0 node 0" in _error(ta)
    assert _create_cat(ta, sn, tr, 2, {0: [1, 2]}, flags=fl, covers=None) == INVALID_ARG


def _vine(ta, depth):
    """A vine of `depth` categorical nodes on features 0 .. depth - 1."""
    sn = np.zeros(2 * depth + 1, dtype=ta.capi.SPARSE_NODE_DTYPE)
    for k in range(depth):
        sn[2 * k] = (0.0, k, 2 * k + 1)
        sn[2 * k + 1] = (float(k), LEAF, 0)
    sn[2 * depth] = (-1.0, LEAF, 0)
    # node 2k's children are 2k + 1 (a leaf) and 2k + 2 (the next node)
    return sn, np.zeros(1, np.int32), {2 * k: [k % 7] for k in range(depth)}


def test_a_path_of_32_distinct_features_is_unsupported(ta):
    sn, tr, cats = _vine(ta, 32)
    cv = np.ones(sn.size, np.float32)
    assert _create_cat(ta, sn, tr, 40, cats, flags=ta.CREATE_CONTRIBS | ta.CREATE_CAT_CONTRIBS, covers=cv) == UNSUPPORTED
    assert "31" in _error(ta)
    # the Saabas tables alone have no path limit; 31 features fit the path bins
    want = OK if _has_gpu(ta) else NO_DEVICE
    assert _create_cat(ta, sn, tr, 40, cats, flags=ta.CREATE_APPROX_CONTRIBS | ta.CREATE_CAT_CONTRIBS, covers=cv) == want
    sn, tr, cats = _vine(ta, 31)
    assert _create_cat(ta, sn, tr, 40, cats, flags=ta.CREATE_CONTRIBS | ta.CREATE_CAT_CONTRIBS,
                       covers=np.ones(sn.size, np.float32)) == want


@pytest.mark.parametrize("flags", ["contribs", "approx", "both"])
def test_a_valid_request_reaches_the_device(ta, flags):
    """On the parent this is TAHOE_ERR_UNSUPPORTED."""
    forest, covers = cases.mixed(ta, 5, 3)
    fl = {"contribs": ta.CREATE_CONTRIBS, "approx": ta.CREATE_APPROX_CONTRIBS,
          "both": ta.CREATE_CONTRIBS | ta.CREATE_APPROX_CONTRIBS}[flags] | ta.CREATE_CAT_CONTRIBS
    st = _create_cat(ta, forest.sn, forest.tr, 5, forest.cats, forest.left, flags=fl, covers=covers)
    assert st == (OK if _has_gpu(ta) else NO_DEVICE), _error(ta)
    # no splits, or no cats at all: tahoe_sparse_forest_create_ex with the remaining flags
    assert _create_cat(ta, forest.sn, forest.tr, 5, {}, flags=fl, covers=covers) == (OK if _has_gpu(ta) else NO_DEVICE)
    assert _create_cat(ta, forest.sn, forest.tr, 5, {}, flags=fl, covers=covers, with_cats=False) == (OK if _has_gpu(ta) else NO_DEVICE)


def test_python_sets_the_flag_itself(ta):
    forest, covers = cases.mixed(ta, 5, 3)
    try:
        f = ta.capi.SparseForest(forest.sn, forest.tr, 5, missing=MISSING, covers=covers, contribs=True, categories=forest.cats,
                                 members_left=forest.left)
    except ta.capi.TahoeError as e:  # without the flag the refusal would be TAHOE_ERR_UNSUPPORTED
        assert not _has_gpu(ta) and e.status == NO_DEVICE
    else:
        f.close()


@pytest.mark.parametrize("seed", range(40))
def test_set_folding_against_the_edges_one_by_one(seed):
    """The allowed set + outside_ok of random edge lists answers every value as the conjunction of the edges does."""
    rng = np.random.default_rng(seed)
    edges = []
    for _ in range(int(rng.integers(1, 5))):
        nw = int(rng.choice([0, 1, 2, 5]))
        ids = np.nonzero(rng.random(32 * nw) < rng.choice([0.1, 0.5, 0.9]))[0]
        edges.append((ids, nw, bool(rng.integers(2))))
    if seed == 0:  # two need = 1 edges with disjoint sets: nothing follows
        edges = [([1, 2, 3], 1, True), ([40, 41], 2, True)]
    allowed, W, outside_ok = cref.fold(edges)
    x = np.concatenate([np.arange(32 * W + 40), [-1.0, np.nan, 2.0 ** 24], np.arange(32 * W + 40) + 0.7, [-0.0]]).astype(np.float32)
    want = np.ones(x.size, bool)
    for ids, nw, need in edges:
        want &= cref.member(ids, nw, x) == need
    got = cref.element_follows(allowed, W, outside_ok, x)
    assert np.array_equal(got, want)
    if seed == 0:
        assert not got.any() and not outside_ok


def test_the_rule_of_the_reference_is_categorical_ref(ta):
    forest, _ = cases.mixed(ta, 8, 5)
    x = cases.mixed_rows(64, 8, 6)
    node, offset, words, ml = forest.arrays()
    sums, leaf = categorical_ref.predict(forest.sn, forest.tr, x, MISSING, node, offset, words, ml)
    for t in range(forest.tr.size):
        root = int(forest.tr[t])
        for r in range(x.shape[0]):
            i = 0
            while forest.sn["bits"][root + i] >= 0:
                fid = int(forest.sn["bits"][root + i]) & 0x3FFFFFFF
                i = int(forest.sn["left_idx"][root + i]) + int(cref.go_right(forest, root + i, x[r:r + 1, fid], MISSING)[0])
            assert i == leaf[r, t]


@pytest.mark.parametrize("F,seed", [(5, 3), (8, 5)])
def test_the_float64_references_agree_among_themselves(ta, F, seed):
    """sum phi + bias = margin to 1e-12, for the conditional and the interventional game and the interaction rows."""
    forest, covers = cases.mixed(ta, F, seed)
    x, bg = cases.mixed_rows(9, F, seed + 1), cases.mixed_rows(6, F, seed + 2)
    margin = cref.predict64(forest, x, MISSING, 1)[:, 0]
    phi = cref.contribs(forest, covers, x, F, MISSING)[:, 0]
    assert np.all(np.abs(phi.sum(-1) - margin) <= 1e-12 * max(1.0, np.abs(margin).max()))
    iv = cref.interventional(forest, x, bg, F, MISSING, bg_raw=cref.predict64(forest, bg, MISSING, 1))[:, 0]
    assert np.all(np.abs(iv.sum(-1) - margin) <= 1e-6)  # the bias column is rounded to float32 once
    inter = cref.interactions(forest, covers, x, F, MISSING)[:, 0]
    assert np.array_equal(inter, inter.transpose(0, 2, 1))
    # the hand tree's dead path: no row reaches its leaf
    node, offset, words, ml = forest.arrays()
    _, leaf = categorical_ref.predict(forest.sn, forest.tr, np.concatenate([x, bg, cases.mixed_rows(500, F, 9)]), MISSING, node,
                                      offset, words, ml)
    assert not np.isin(leaf[:, -1], [5, 7, 8]).any()
