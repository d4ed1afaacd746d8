"""Categorical splits on sparse handles (tahoe_sparse_forest_create_cat) without a GPU: the new symbol, every refusal in the
documented order (all before a device is touched), NULL / empty splits accepted exactly where tahoe_sparse_forest_create_ex
accepts, the Python packer, and known answers written by hand for tests/categorical_ref.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref  # noqa: E402

OK, INVALID_ARG, NO_DEVICE, INVALID_FOREST, UNSUPPORTED = 0, 1, 4, 6, 7
LEAF = np.int32(-(1 << 31))
DEF_LEFT = 1 << 30
MISSING = -999.0


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


def _cats(ta, ns, node=None, offset=None, words=None, ml=None):
    """CategoricalSplits over the given arrays (None: a NULL pointer); the arrays ride along on the struct."""
    arrs = [None if a is None else np.ascontiguousarray(a, dt)
            for a, dt in ((node, np.int32), (offset, np.int32), (words, np.uint32), (ml, np.uint8))]
    s = ta.capi.CategoricalSplits(ns, *[a.ctypes.data if a is not None else None for a in arrs])
    s._keep = arrs
    return s


def _create_cat(ta, sn, tr, cols, cats, num_classes=1, output=0, flags=0, covers=None):
    """Status of tahoe_sparse_forest_create_cat (cats None: a NULL pointer); a created handle is destroyed."""
    sn = np.ascontiguousarray(sn)
    tr = np.ascontiguousarray(tr, dtype=np.int32)
    params = ta.ForestParams(int(sn.size), 0, int(tr.size), cols, 0, output, 0.0, 0.0, 0, MISSING)
    h = C.c_void_p()
    cv = None if covers is None else np.ascontiguousarray(covers, dtype=np.float32)
    st = ta.lib.tahoe_sparse_forest_create_cat(C.byref(h), tr.ctypes.data if tr.size else None,
                                               sn.ctypes.data if sn.size else None, cv.ctypes.data if cv is not None else None,
                                               C.byref(params), num_classes, flags, C.byref(cats) if cats is not None else None)
    if st != OK:
        assert not h.value
    if h.value:
        ta.lib.tahoe_forest_destroy(h)
    return st


def _create_ex(ta, sn, tr, cols, num_classes=1, output=0, flags=0, covers=None):
    sn = np.ascontiguousarray(sn)
    tr = np.ascontiguousarray(tr, dtype=np.int32)
    params = ta.ForestParams(int(sn.size), 0, int(tr.size), cols, 0, output, 0.0, 0.0, 0, MISSING)
    h = C.c_void_p()
    cv = None if covers is None else np.ascontiguousarray(covers, dtype=np.float32)
    st = ta.lib.tahoe_sparse_forest_create_ex(C.byref(h), tr.ctypes.data if tr.size else None,
                                              sn.ctypes.data if sn.size else None, cv.ctypes.data if cv is not None else None,
                                              C.byref(params), num_classes, flags)
    if h.value:
        ta.lib.tahoe_forest_destroy(h)
    return st


def three_trees(ta):
    """The hand-made forest of the known answers (missing = -999, features x0, x1):
    tree 0 (nodes 0-2):  node 0 categorical on x0, set {2, 33} (2 words), members right, def_left -> leaves 1.0 / 2.0
    tree 1 (nodes 3-5):  node 0 categorical on x1, set {0, 5} (1 word), members LEFT, default right -> leaves 10.0 / 20.0
    tree 2 (nodes 6-10): node 0 numeric x0 >= 2.5, def_left -> leaf 100.0 / node 2; node 2 categorical on x1, the EMPTY set
                         (0 words), members right, default right -> leaves 300.0 / 400.0"""
    sn = np.zeros(11, dtype=ta.capi.SPARSE_NODE_DTYPE)
    sn[0] = (0.0, 0 | DEF_LEFT, 1)
    sn[1] = (1.0, LEAF, 0)
    sn[2] = (2.0, LEAF, 0)
    sn[3] = (0.0, 1, 1)
    sn[4] = (10.0, LEAF, 0)
    sn[5] = (20.0, LEAF, 0)
    sn[6] = (2.5, 0 | DEF_LEFT, 1)
    sn[7] = (100.0, LEAF, 0)
    sn[8] = (0.0, 1, 3)
    sn[9] = (300.0, LEAF, 0)
    sn[10] = (400.0, LEAF, 0)
    tr = np.array([0, 3, 6], np.int32)
    node = np.array([0, 3, 8], np.int32)
    offset = np.array([0, 2, 3, 3], np.int32)
    words = np.array([1 << 2, 1 << 1, (1 << 0) | (1 << 5)], np.uint32)
    ml = np.array([0, 1, 0], np.uint8)
    return sn, tr, node, offset, words, ml


NAN = np.float32(np.nan)
# (x0, x1) -> leaf per tree with members_left as given, and with members_left NULL (tree 1's members then go right)
KNOWN = [
    ((2.0, 5.0), (2, 1, 1), (2, 2, 1)),        # member (x0 = 2); member of tree 1 (goes left, or right with NULL)
    ((2.7, 4.0), (2, 2, 3), (2, 1, 3)),        # 2.7 is category 2; 4 is no member; tree 2: empty set -> left
    ((3.0, -0.0), (1, 1, 3), (1, 2, 3)),       # 3 no member; -0.0 is category 0, a member of tree 1
    ((NAN, NAN), (1, 2, 1), (1, 1, 1)),        # NaN is never a member; x0 >= 2.5 is false for NaN
    ((-1.0, -0.5), (1, 2, 1), (1, 1, 1)),      # negatives are never members (LightGBM would read -0.5 as 0)
    ((64.0, 32.0), (1, 2, 3), (1, 1, 3)),      # x == 32 * nwords is past the bitset
    ((33.5, MISSING), (2, 2, 4), (2, 2, 4)),   # category 33 (second word); the sentinel takes the default: right
    ((MISSING, 0.0), (1, 1, 1), (1, 2, 1)),    # the sentinel with def_left: left
    ((63.9, 1.0), (1, 2, 3), (1, 1, 3)),       # category 63: last bit of the second word, not set
]
VALUES = [(None, 1.0, 2.0), (None, 10.0, 20.0), (None, 100.0, None, 300.0, 400.0)]  # by leaf index


def _want(leaves):
    v = [VALUES[t][leaves[t]] for t in range(3)]
    return np.float32(np.float32(np.float32(0.0) + np.float32(v[0])) + np.float32(v[1])) + np.float32(v[2])


def test_symbol_is_exported_and_bound(ta):
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    assert "tahoe_sparse_forest_create_cat" in ta.capi.EXPORTED_SYMBOLS
    assert hasattr(ta.lib, "tahoe_sparse_forest_create_cat")
    assert " tahoe_sparse_forest_create_cat" in syms
    assert ta.lib.tahoe_abi_version() == 2


@pytest.mark.parametrize("members_left", [True, False])
def test_known_answers_of_the_reference(ta, members_left):
    sn, tr, node, offset, words, ml = three_trees(ta)
    data = np.array([k[0] for k in KNOWN], np.float32)
    sums, leaf = categorical_ref.predict(sn, tr, data, MISSING, node, offset, words, ml if members_left else None)
    want_leaf = np.array([k[1] if members_left else k[2] for k in KNOWN], np.uint32)
    assert np.array_equal(leaf, want_leaf)
    want = np.array([_want(k[1] if members_left else k[2]) for k in KNOWN], np.float32)
    assert np.array_equal(sums.view(np.uint32), want.view(np.uint32))


def test_reference_classes_and_init(ta):
    sn, tr, node, offset, words, ml = three_trees(ta)
    data = np.array([k[0] for k in KNOWN], np.float32)
    one, leaf1 = categorical_ref.predict(sn, tr, data, MISSING, node, offset, words, ml)
    three, leaf3 = categorical_ref.predict(sn, tr, data, MISSING, node, offset, words, ml, num_classes=3)
    assert np.array_equal(leaf1, leaf3)
    vals = np.array([[VALUES[t][k[1][t]] for t in range(3)] for k in KNOWN], np.float32)
    assert np.array_equal(three, vals)  # one tree per class
    init = np.full(len(KNOWN), 0.5, np.float32)
    acc, _ = categorical_ref.predict(sn, tr, data, MISSING, node, offset, words, ml, init=init)
    want = ((init + vals[:, 0]) + vals[:, 1]) + vals[:, 2]
    assert np.array_equal(acc, want) and not np.array_equal(acc, one)


def test_packer(ta):
    cats, (node, offset, words, ml) = ta.capi.pack_categorical({8: [], 0: [33, 2, 2], 3: (5, 0)}, members_left={3})
    assert cats.num_splits == 3
    assert node.tolist() == [0, 3, 8] and offset.tolist() == [0, 2, 3, 3]
    assert words[:3].tolist() == [1 << 2, 1 << 1, (1 << 0) | (1 << 5)]
    assert ml.tolist() == [0, 1, 0]
    _, (_, _, _, ml2) = ta.capi.pack_categorical({1: [0]})
    assert ml2 is None
    with pytest.raises(ValueError):
        ta.capi.pack_categorical({1: [-1]})
    with pytest.raises(ValueError):
        ta.capi.pack_categorical({1: [1 << 24]})
    with pytest.raises(ValueError):
        ta.capi.pack_categorical({1: [0]}, members_left={2})


def _valid(ta):
    sn, tr, node, offset, words, ml = three_trees(ta)
    return sn, tr, node, offset, words, ml


@pytest.mark.parametrize("case", ["neg", "too_many", "null_node", "null_offset", "null_words", "not_ascending", "duplicate",
                                  "node_negative", "node_past_end", "offset0", "offset_decreases", "too_wide"])
def test_argument_refusals(ta, case):
    sn, tr, node, offset, words, ml = _valid(ta)
    n = sn.size
    args = dict(node=node, offset=offset, words=words, ml=ml)
    ns = 3
    if case == "neg":
        ns = -1
    elif case == "too_many":
        ns = n + 1
    elif case.startswith("null_"):
        args[case[5:]] = None
    elif case == "not_ascending":
        args["node"] = np.array([0, 8, 3], np.int32)
    elif case == "duplicate":
        args["node"] = np.array([0, 3, 3], np.int32)
    elif case == "node_negative":
        args["node"] = np.array([-1, 3, 8], np.int32)
    elif case == "node_past_end":
        args["node"] = np.array([0, 3, n], np.int32)
    elif case == "offset0":
        args["offset"] = np.array([1, 2, 3, 3], np.int32)
    elif case == "offset_decreases":
        args["offset"] = np.array([0, 2, 1, 3], np.int32)
    elif case == "too_wide":
        args["offset"] = np.array([0, 2, 2 + (1 << 19) + 1, 2 + (1 << 19) + 1], np.int32)
    assert _create_cat(ta, sn, tr, 2, _cats(ta, ns, **args)) == INVALID_ARG
    assert "categorical" in _error(ta)


def test_widest_split_is_accepted(ta):
    sn, tr, node, offset, words, ml = _valid(ta)
    wide = np.zeros(1 << 19, np.uint32)
    want = OK if _has_gpu(ta) else NO_DEVICE
    assert _create_cat(ta, sn, tr, 2, _cats(ta, 1, node=[0], offset=[0, 1 << 19], words=wide)) == want


def test_a_leaf_is_named_by_tree_and_node(ta):
    sn, tr, node, offset, words, ml = _valid(ta)
    assert _create_cat(ta, sn, tr, 2, _cats(ta, 3, node=[0, 3, 9], offset=offset, words=words, ml=ml)) == INVALID_FOREST
    msg = _error(ta)
    assert "tree 2 node 3:" in msg and "leaf" in msg
    # the same leaf in a three-class handle: still the caller's numbering
    assert _create_cat(ta, sn, tr, 2, _cats(ta, 3, node=[0, 3, 9], offset=offset, words=words, ml=ml), num_classes=3) == INVALID_FOREST
    assert "tree 2 node 3:" in _error(ta)


def test_refusal_order(ta):
    sn, tr, node, offset, words, ml = _valid(ta)
    covers = np.ones(sn.size, np.float32)
    bad_args = _cats(ta, 3, node=[0, 3, 3], offset=offset, words=words)
    leaf_listed = _cats(ta, 3, node=[0, 3, 9], offset=offset, words=words)
    good = _cats(ta, 3, node=node, offset=offset, words=words, ml=ml)
    broken = sn.copy()
    broken["left_idx"][3] = 0  # tree 1's root points at itself
    # _ex's own checks come first: classes, then flags
    assert _create_cat(ta, sn, tr, 2, bad_args, num_classes=2) == INVALID_ARG and "multiple" in _error(ta)
    assert _create_cat(ta, sn, tr, 2, bad_args, flags=0x1) == INVALID_ARG and "flags" in _error(ta)
    # then the splits' arguments, before the forest's structure
    assert _create_cat(ta, broken, tr, 2, bad_args) == INVALID_ARG and "categorical" in _error(ta)
    # then the structure, before a listed leaf
    assert _create_cat(ta, broken, tr, 2, leaf_listed) == INVALID_FOREST and "children" in _error(ta)
    # a listed leaf before the SHAP refusal
    assert _create_cat(ta, sn, tr, 2, leaf_listed, flags=ta.CREATE_CONTRIBS, covers=covers) == INVALID_FOREST
    assert "leaf" in _error(ta)


@pytest.mark.parametrize("flags", ["contribs", "approx", "both"])
def test_shap_and_saabas_are_refused(ta, flags):
    sn, tr, node, offset, words, ml = _valid(ta)
    fl = {"contribs": ta.CREATE_CONTRIBS, "approx": ta.CREATE_APPROX_CONTRIBS,
          "both": ta.CREATE_CONTRIBS | ta.CREATE_APPROX_CONTRIBS}[flags]
    covers = np.ones(sn.size, np.float32)
    assert _create_cat(ta, sn, tr, 2, _cats(ta, 3, node=node, offset=offset, words=words, ml=ml), flags=fl, covers=covers) == UNSUPPORTED
    assert "interval" in _error(ta)


def test_num_cols_past_2_29_is_refused(ta):
    sn, tr, node, offset, words, ml = _valid(ta)
    assert _create_cat(ta, sn, tr, (1 << 29) + 1, _cats(ta, 3, node=node, offset=offset, words=words, ml=ml)) == UNSUPPORTED
    assert "2^29" in _error(ta)
    want = OK if _has_gpu(ta) else NO_DEVICE
    assert _create_cat(ta, sn, tr, (1 << 29) + 1, None) == want  # without splits nothing changes


def _ex_cases(ta):
    sn, tr = ta.capi.synth_sparse_forest(6, 8, min_depth=2, max_depth=6, leaf_prob=0.3, max_tree_nodes=200, seed=5)
    covers = np.ones(sn.size, np.float32)
    broken = sn.copy()
    inner = np.flatnonzero((broken["bits"].view(np.uint32) >> 31) == 0)
    broken["left_idx"][inner[0]] = 0
    return [
        dict(sn=sn, tr=tr, cols=8),
        dict(sn=sn, tr=tr, cols=8, num_classes=2),
        dict(sn=sn, tr=tr, cols=8, num_classes=3, output=ta.OUT_SOFTMAX),
        dict(sn=sn, tr=tr, cols=8, num_classes=4),
        dict(sn=sn, tr=tr, cols=8, num_classes=0),
        dict(sn=sn, tr=tr, cols=8, output=ta.OUT_SOFTMAX),
        dict(sn=sn, tr=tr, cols=8, flags=ta.CREATE_CONTRIBS, covers=covers),
        dict(sn=sn, tr=tr, cols=8, flags=ta.CREATE_APPROX_CONTRIBS, covers=covers),
        dict(sn=sn, tr=tr, cols=8, flags=ta.CREATE_CONTRIBS),
        dict(sn=sn, tr=tr, cols=8, flags=0x1, covers=covers),
        dict(sn=broken, tr=tr, cols=8),
        dict(sn=sn, tr=tr, cols=3),
    ]


@pytest.mark.parametrize("empty", ["null", "zero", "zero_null_arrays"])
def test_no_splits_is_accepted_exactly_where_ex_accepts(ta, empty):
    for i, c in enumerate(_ex_cases(ta)):
        kw = {k: v for k, v in c.items() if k not in ("sn", "tr", "cols")}
        want = _create_ex(ta, c["sn"], c["tr"], c["cols"], **kw)
        want_msg = _error(ta)
        if empty == "null":
            cats = None
        elif empty == "zero":
            cats = _cats(ta, 0, node=[5], offset=[0], words=[0])
        else:
            cats = _cats(ta, 0)
        assert _create_cat(ta, c["sn"], c["tr"], c["cols"], cats, **kw) == want, i
        if want != OK:
            assert _error(ta) == want_msg, i
