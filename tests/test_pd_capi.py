"""Partial dependence (TAHOE_CREATE_PARTIAL_DEPENDENCE, tahoe_forest_predict_partial_dependence) without a GPU: the symbol, the
create-time refusals with their statuses and texts (all before a device is touched), the depth limit from both sides, the flag
on the creates that do not take it, and the call's refusal that needs no handle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pd_cases  # noqa: E402

OK, INVALID_ARG, NO_DEVICE, INVALID_FOREST, UNSUPPORTED = 0, 1, 4, 6, 7
PD = 0x800


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


def _created(ta):
    return OK if _has_gpu(ta) else NO_DEVICE


def _error(ta):
    return ta.lib.tahoe_last_error().decode()


def _create(ta, fo, flags=PD, covers="own", cats=None, num_classes=None):
    """Status of tahoe_sparse_forest_create_ex (or _cat with cats); a created handle is destroyed."""
    sn = np.ascontiguousarray(fo["nodes"])
    tr = np.ascontiguousarray(fo["trees"], dtype=np.int32)
    cv = None if covers is None else np.ascontiguousarray(fo["covers"] if isinstance(covers, str) else covers, dtype=np.float32)
    params = ta.ForestParams(int(sn.size), 0, int(tr.size), fo["num_cols"], 0, 0, 0.0, 0.0, 0, fo["missing"])
    h = C.c_void_p()
    nc = fo["num_classes"] if num_classes is None else num_classes
    args = [C.byref(h), tr.ctypes.data, sn.ctypes.data, cv.ctypes.data if cv is not None else None, C.byref(params), nc, flags]
    if cats is not None:
        packed, _keep = ta.capi.pack_categorical(*cats)
        st = ta.lib.tahoe_sparse_forest_create_cat(*args, C.byref(packed))
    else:
        st = ta.lib.tahoe_sparse_forest_create_ex(*args)
    if st != OK:
        assert not h.value
    if h.value:
        ta.lib.tahoe_forest_destroy(h)
    return st


def _small():
    return pd_cases.random_forest(seed=3, num_trees=4, num_cols=5, max_depth=4, leaf_prob=0.3)


def test_symbol_is_exported_bound_and_declared(ta):
    name = "tahoe_forest_predict_partial_dependence"
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    assert name in ta.capi.EXPORTED_SYMBOLS and hasattr(ta.lib, name) and f" {name}" in syms
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert f"tahoe_status {name}(" in header and "#define TAHOE_CREATE_PARTIAL_DEPENDENCE 0x800u" in header
    assert ta.CREATE_PARTIAL_DEPENDENCE == PD == ta.capi.CREATE_PARTIAL_DEPENDENCE
    assert ta.lib.tahoe_abi_version() == 2


def test_the_flag_is_accepted_alone_and_with_the_others(ta):
    fo = _small()
    for flags in (PD, PD | ta.CREATE_CONTRIBS, PD | ta.CREATE_APPROX_CONTRIBS, PD | ta.CREATE_CONTRIBS | ta.CREATE_APPROX_CONTRIBS):
        assert _create(ta, fo, flags=flags) == _created(ta), hex(flags)
    assert _create(ta, fo, flags=PD | 0x1) == INVALID_ARG and "unknown create flags 0x801" in _error(ta)


def test_the_flag_goes_with_categorical_splits_without_cat_contribs(ta):
    fo = pd_cases.random_forest(**pd_cases.RANDOM_CASES[2]["forest"])
    cats = (fo["categories"], fo["members_left"])
    assert _create(ta, fo, flags=PD, cats=cats) == _created(ta)
    # TAHOE_CREATE_CAT_CONTRIBS still needs one of its two flags
    assert _create(ta, fo, flags=PD | ta.CREATE_CAT_CONTRIBS, cats=cats) == INVALID_ARG and "TAHOE_CREATE_CAT_CONTRIBS" in _error(ta)


def test_null_covers_are_refused(ta):
    fo = _small()
    assert _create(ta, fo, covers=None) == INVALID_ARG
    assert "TAHOE_CREATE_PARTIAL_DEPENDENCE needs covers" in _error(ta)
    assert _create(ta, fo, covers=None, cats=({}, ())) == INVALID_ARG
    assert "TAHOE_CREATE_PARTIAL_DEPENDENCE needs covers" in _error(ta)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -1.0])
def test_the_cover_check_of_the_other_flags_holds(ta, bad):
    fo = _small()
    inner = int(np.flatnonzero(fo["nodes"]["bits"][:fo["trees"][1]] >= 0)[1])  # tree 0, its second internal node
    cv = fo["covers"].copy()
    cv[fo["nodes"]["left_idx"][inner]] = bad
    assert _create(ta, fo, covers=cv) == INVALID_FOREST
    msg = _error(ta)
    assert f"tree 0 node {inner}:" in msg and "TAHOE_CREATE_PARTIAL_DEPENDENCE" in msg and "covers" in msg


def test_both_covers_zero_is_refused(ta):
    fo = _small()
    cv = fo["covers"].copy()
    l = fo["nodes"]["left_idx"][0]
    cv[l] = cv[l + 1] = 0.0
    assert _create(ta, fo, covers=cv) == INVALID_FOREST and "tree 0 node 0:" in _error(ta) and "positive sum" in _error(ta)


def test_an_infinite_float32_cover_sum_is_refused(ta):
    fo = _small()
    root1 = int(fo["trees"][1])
    assert fo["nodes"]["bits"][root1] >= 0
    cv = fo["covers"].copy()
    l = root1 + fo["nodes"]["left_idx"][root1]
    cv[l] = cv[l + 1] = np.float32(3.0e38)  # each finite, their float32 sum is not
    assert _create(ta, fo, covers=cv) == INVALID_FOREST
    msg = _error(ta)
    assert "tree 1 node 0:" in msg and "float32 sum" in msg and "not finite" in msg
    cv[l + 1] = np.float32(3.0e37)  # a finite sum passes
    assert _create(ta, fo, covers=cv) == _created(ta)


def test_a_leaf_33_edges_deep_is_refused_and_32_is_not(ta):
    assert _create(ta, pd_cases.chain(33)) == UNSUPPORTED
    msg = _error(ta)
    assert "tree 0" in msg and "32 edges" in msg and "TAHOE_CREATE_PARTIAL_DEPENDENCE" in msg
    assert _create(ta, pd_cases.chain(32)) == _created(ta)
    # without the flag the depth is nobody's business
    assert _create(ta, pd_cases.chain(33), flags=0) == _created(ta)


def test_no_limit_on_the_features_of_a_path(ta):
    """A path of 40 distinct features (depth 32 allows 32; TreeSHAP's 31 is not checked): the depth-32 chain on 32 features."""
    fo = pd_cases.chain(32)
    assert len(set((fo["nodes"]["bits"][fo["nodes"]["bits"] >= 0] & 0x3fffffff).tolist())) == 32
    assert _create(ta, fo) == _created(ta)
    assert _create(ta, fo, flags=PD | ta.CREATE_CONTRIBS) == UNSUPPORTED and "31" in _error(ta)  # that flag's own limit stays


def test_refusal_order_classes_flags_covers_structure(ta):
    fo = _small()
    broken = dict(fo, nodes=fo["nodes"].copy())
    broken["nodes"]["left_idx"][0] = 0
    assert _create(ta, fo, num_classes=3) == INVALID_ARG and "multiple" in _error(ta)
    assert _create(ta, broken, flags=PD | 0x2, covers=None) == INVALID_ARG and "flags" in _error(ta)
    assert _create(ta, broken, covers=None) == INVALID_ARG and "covers" in _error(ta)
    assert _create(ta, broken) == INVALID_FOREST and "children" in _error(ta)


def test_other_creates_keep_their_unknown_flag_refusal(ta):
    lib = ta.lib
    h = C.c_void_p()
    # dense, and multi-class dense
    nodes = ta.synth_forest(4, 2, 4, seed=5)
    params = ta.ForestParams(0, 2, 4, 4, 0, 0, 0.0, 0.0, 0, -999.0)
    assert lib.tahoe_forest_create_ex(C.byref(h), nodes.ctypes.data, C.byref(params), PD) == INVALID_ARG
    assert "unknown create flags 0x800" in _error(ta) and not h.value
    assert lib.tahoe_forest_create_ex(C.byref(h), nodes.ctypes.data, C.byref(params), PD | ta.CREATE_CONTRIBS) == INVALID_ARG
    assert "unknown create flags 0x804" in _error(ta) and not h.value
    assert lib.tahoe_forest_create_multiclass(C.byref(h), nodes.ctypes.data, C.byref(params), 2, PD) == INVALID_ARG
    assert "flags" in _error(ta) and not h.value
    # oblivious: one tree of depth 1
    depths = np.array([1], np.int32)
    splits = np.zeros(1, ta.capi.OBLIVIOUS_SPLIT_DTYPE)
    leaves = np.array([1.0, 2.0], np.float32)
    covers = np.ones(2, np.float32)
    op = ta.ForestParams(0, 0, 1, 2, 0, 0, 0.5, 0.0, 0, -999.0)
    assert lib.tahoe_oblivious_forest_create_ex(C.byref(h), depths.ctypes.data, splits.ctypes.data, leaves.ctypes.data,
                                                covers.ctypes.data, C.byref(op), 1, PD) == INVALID_ARG
    assert "flag" in _error(ta) and "0x800" in _error(ta) and not h.value
    # vector-leaf: a stump
    sn = np.zeros(3, ta.capi.SPARSE_NODE_DTYPE)
    sn[0] = (0.5, 0, 1)
    sn[1] = (0.0, pd_cases.LEAF, 0)
    sn[2] = (0.0, pd_cases.LEAF, 1)
    tr = np.array([0], np.int32)
    lv = np.array([1.0, 2.0], np.float32)
    cv = np.array([2.0, 1.0, 1.0], np.float32)
    vp = ta.ForestParams(3, 0, 1, 2, 0, 0, 0.5, 0.0, 0, -999.0)
    assert lib.tahoe_vector_forest_create_ex(C.byref(h), tr.ctypes.data, sn.ctypes.data, lv.ctypes.data, 2, cv.ctypes.data,
                                             C.byref(vp), 1, PD) == INVALID_ARG
    assert "unknown create flags 0x800" in _error(ta) and not h.value


def test_a_null_handle_is_refused_first(ta):
    targets = np.array([0, 0], np.int32)  # repeated targets, a null output: the handle is still what the refusal names
    st = ta.lib.tahoe_forest_predict_partial_dependence(None, None, targets.ctypes.data, 40, None, 5, None)
    assert st == INVALID_ARG and "tahoe_forest_predict_partial_dependence" in _error(ta) and "null forest" in _error(ta)


def test_python_sets_the_flag_only_when_asked(ta):
    """SparseForest(partial_dependence=True) without covers reaches the library's refusal (no device needed)."""
    fo = _small()
    with pytest.raises(ta.capi.TahoeError) as e:
        ta.capi.SparseForest(fo["nodes"], fo["trees"], fo["num_cols"], missing=fo["missing"], partial_dependence=True)
    assert "needs covers" in str(e.value)
