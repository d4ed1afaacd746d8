"""Multi-class and TreeSHAP sparse handles through the C ABI without a GPU: the new symbols, the argument, cover and path-length
checks of tahoe_sparse_forest_create_ex (all before a device is touched), and tahoe_dense_to_sparse_ex."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE, INVALID_FOREST, UNSUPPORTED = 0, 1, 4, 6, 7
LEAF = np.int32(-(1 << 31))


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    import sys

    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def _has_gpu(ta):
    n = C.c_int(0)
    return ta.lib.tahoe_device_count(C.byref(n)) == 0 and n.value > 0


def _create(ta, sn, tr, cols, num_classes=1, output=0, flags=0, covers=None, keep=False):
    """Status of tahoe_sparse_forest_create_ex; a refused call creates nothing.  keep: destroy a created handle."""
    sn = np.ascontiguousarray(sn)
    tr = np.ascontiguousarray(tr, dtype=np.int32)
    params = ta.ForestParams(int(sn.size), 0, int(tr.size), cols, 0, output, 0.0, 0.0, 0, -999.0)
    h = C.c_void_p()
    cv = None if covers is None else np.ascontiguousarray(covers, dtype=np.float32)
    st = ta.lib.tahoe_sparse_forest_create_ex(C.byref(h), tr.ctypes.data if tr.size else None,
                                              sn.ctypes.data if sn.size else None, cv.ctypes.data if cv is not None else None,
                                              C.byref(params), num_classes, flags)
    if st != OK:
        assert not h.value
    if h.value:
        ta.lib.tahoe_forest_destroy(h)
    return st


def _error(ta):
    return ta.lib.tahoe_last_error().decode()


def _forest(ta, T=6, cols=8):
    sn, tr = ta.capi.synth_sparse_forest(T, cols, min_depth=2, max_depth=6, leaf_prob=0.3, max_tree_nodes=200, seed=5)
    return sn, tr


def _vine(ta, fids):
    """One tree: inner node k (at 2k) on feature fids[k], its left child a leaf (2k + 1), its right child the next inner node
    (2k + 2) or, after the last one, a leaf."""
    sn = np.zeros(2 * len(fids) + 1, dtype=ta.capi.SPARSE_NODE_DTYPE)
    for k, fid in enumerate(fids):
        sn[2 * k] = (0.5, int(fid), 2 * k + 1)
        sn[2 * k + 1] = (float(k), LEAF, 0)
    sn[-1] = (-1.0, LEAF, 0)
    return sn, np.zeros(1, np.int32)


def test_symbols_are_exported_and_bound(ta):
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    for name in ("tahoe_sparse_forest_create_ex", "tahoe_dense_to_sparse_ex"):
        assert name in ta.capi.EXPORTED_SYMBOLS
        assert hasattr(ta.lib, name)
        assert " " + name in syms
    assert ta.lib.tahoe_abi_version() == 2


@pytest.mark.parametrize("num_classes", [0, -1, 1025])
def test_num_classes_out_of_range(ta, num_classes):
    sn, tr = _forest(ta)
    assert _create(ta, sn, tr, 8, num_classes) == INVALID_ARG
    assert "num_classes" in _error(ta)


def test_trees_not_a_multiple_of_classes(ta):
    sn, tr = _forest(ta, T=7)
    assert _create(ta, sn, tr, 8, 3) == INVALID_ARG
    assert "multiple" in _error(ta)
    sn, tr = _forest(ta, T=10)
    assert _create(ta, sn, tr, 8, 4) == INVALID_ARG


def test_output_rules(ta):
    sn, tr = _forest(ta)
    assert _create(ta, sn, tr, 8, 1, output=ta.OUT_SOFTMAX) == INVALID_ARG
    assert "SOFTMAX" in _error(ta)
    assert _create(ta, sn, tr, 8, 3, output=ta.OUT_THRESHOLD) == INVALID_ARG
    assert "THRESHOLD" in _error(ta)
    assert _create(ta, sn, tr, 8, 3, output=ta.OUT_SOFTMAX | ta.OUT_SIGMOID) == INVALID_ARG
    # the old entry point still refuses SOFTMAX
    params = ta.ForestParams(int(sn.size), 0, int(tr.size), 8, 0, ta.OUT_SOFTMAX, 0.0, 0.0, 0, -999.0)
    h = C.c_void_p()
    assert ta.lib.tahoe_sparse_forest_create(C.byref(h), tr.ctypes.data, sn.ctypes.data, C.byref(params)) == INVALID_ARG


@pytest.mark.parametrize("flags", [0x1, 0x2, 0x8, 0x80000000, 0x4 | 0x1])
def test_unknown_flags_and_prob_relayout(ta, flags):
    sn, tr = _forest(ta)
    covers = np.ones(sn.size, np.float32)
    assert _create(ta, sn, tr, 8, 1, flags=flags, covers=covers) == INVALID_ARG
    assert "flags" in _error(ta)


def test_contribs_needs_covers(ta):
    sn, tr = _forest(ta)
    assert _create(ta, sn, tr, 8, 1, flags=ta.CREATE_CONTRIBS, covers=None) == INVALID_ARG
    assert "covers" in _error(ta)


def test_structure_is_still_checked_first(ta):
    sn, tr = _forest(ta)
    bad = sn.copy()
    inner = np.flatnonzero((bad["bits"].view(np.uint32) >> 31) == 0)
    bad["left_idx"][inner[0]] = 0
    assert _create(ta, bad, tr, 8, 2, flags=ta.CREATE_CONTRIBS, covers=np.ones(sn.size, np.float32)) == INVALID_FOREST


@pytest.mark.parametrize("pair", [(0.0, 0.0), (-1.0, 2.0), (np.nan, 1.0), (1.0, np.inf), (-np.inf, 1.0)])
def test_bad_covers_name_the_tree_and_the_node(ta, pair):
    sn, tr = _forest(ta, T=4)
    covers = np.ones(sn.size, np.float32)
    # tree 2: its second reachable internal node (breadth-first is fine: any internal node the walk reaches)
    lo = int(tr[2])
    bits = sn["bits"].view(np.uint32)
    inner = [i for i in range(lo, int(tr[3])) if (bits[i] >> 31) == 0]
    node = inner[1] - lo
    left = lo + int(sn["left_idx"][inner[1]])
    covers[left], covers[left + 1] = pair
    assert _create(ta, sn, tr, 8, 2, flags=ta.CREATE_CONTRIBS, covers=covers) == INVALID_FOREST
    msg = _error(ta)
    assert f"tree 2 node {node}:" in msg and "cover" in msg


def test_covers_ignored_without_the_flag(ta):
    sn, tr = _forest(ta)
    covers = np.full(sn.size, np.nan, np.float32)
    want = OK if _has_gpu(ta) else NO_DEVICE
    assert _create(ta, sn, tr, 8, 2, covers=covers) == want
    assert _create(ta, sn, tr, 8, 3, covers=None) == want


def test_unreachable_covers_are_not_checked(ta):
    sn, tr = _forest(ta, T=2)
    covers = np.ones(sn.size, np.float32)
    extra = np.zeros(2, sn.dtype)
    extra["bits"] = LEAF
    sn2 = np.concatenate([sn, extra])  # two unreachable leaves at the end of tree 1
    covers2 = np.concatenate([covers, np.array([np.nan, -1.0], np.float32)])
    want = OK if _has_gpu(ta) else NO_DEVICE
    assert _create(ta, sn2, tr, 8, 1, flags=ta.CREATE_CONTRIBS, covers=covers2) == want


def test_path_feature_limit(ta):
    want = OK if _has_gpu(ta) else NO_DEVICE
    sn, tr = _vine(ta, range(32))
    assert _create(ta, sn, tr, 40, 1, flags=ta.CREATE_CONTRIBS, covers=np.ones(sn.size, np.float32)) == UNSUPPORTED
    msg = _error(ta)
    assert "tree 0" in msg and "31" in msg
    # the same vine as the second tree of two classes: named as tree 1
    s1, t1 = _vine(ta, [0])
    both = np.concatenate([s1, sn])
    roots = np.array([0, s1.size], np.int32)
    assert _create(ta, both, roots, 40, 2, flags=ta.CREATE_CONTRIBS, covers=np.ones(both.size, np.float32)) == UNSUPPORTED
    assert "tree 1" in _error(ta)
    # 31 distinct features pass every check; without the flag the limit does not apply
    sn, tr = _vine(ta, range(31))
    assert _create(ta, sn, tr, 40, 1, flags=ta.CREATE_CONTRIBS, covers=np.ones(sn.size, np.float32)) == want
    sn, tr = _vine(ta, range(32))
    assert _create(ta, sn, tr, 40, 1) == want


def test_deep_path_that_repeats_features(ta):
    want = OK if _has_gpu(ta) else NO_DEVICE
    sn, tr = _vine(ta, [k % 8 for k in range(40)])
    assert _create(ta, sn, tr, 8, 1, flags=ta.CREATE_CONTRIBS, covers=np.ones(sn.size, np.float32)) == want
    sn, tr = _vine(ta, [k % 31 for k in range(40)])
    assert _create(ta, sn, tr, 31, 1, flags=ta.CREATE_CONTRIBS, covers=np.ones(sn.size, np.float32)) == want


def _walk_pairs(dense, per, sn, root):
    """(dense index, sparse index) of every reachable node of one tree, by a parallel walk."""
    out, stack = [], [(0, root)]
    while stack:
        d, s = stack.pop()
        out.append((d, s))
        if not (int(dense["bits"].view(np.uint32)[d]) >> 31):
            li = root + int(sn["left_idx"][s])
            stack.append((2 * d + 2, li + 1))
            stack.append((2 * d + 1, li))
    return out


@pytest.mark.parametrize("T,D,seed", [(9, 6, 3), (4, 1, 5), (5, 0, 6), (3, 12, 7)])
def test_dense_to_sparse_ex(ta, T, D, seed):
    nodes = ta.synth_forest(T, D, 11, seed=seed, leaf_prob=0.25)
    per = ta.capi.tree_num_nodes(D)
    rng = np.random.default_rng(seed)
    nodes["weight"] = rng.uniform(0.1, 10.0, nodes.size).astype(np.float32)
    sn, tr = ta.capi.dense_to_sparse(nodes, T, D)
    sn2, tr2, cv = ta.capi.dense_to_sparse(nodes, T, D, covers=True)
    assert sn.tobytes() == sn2.tobytes() and tr.tobytes() == tr2.tobytes()
    assert cv.dtype == np.float32 and cv.shape == (sn.size,)
    seen = 0
    for t in range(T):
        tree = nodes[t * per:(t + 1) * per]
        for d, s in _walk_pairs(tree, per, sn, int(tr[t])):
            assert cv[s].view(np.uint32) == tree["weight"][d].view(np.uint32), (t, d, s)
            seen += 1
    assert seen == sn.size  # the converter emits only reachable nodes


def test_dense_to_sparse_ex_needs_covers_out(ta):
    nodes = ta.synth_forest(2, 3, 4, seed=1)
    pn, pt, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert ta.lib.tahoe_dense_to_sparse_ex(nodes.ctypes.data, 2, 3, C.byref(pn), C.byref(pt), None, C.byref(n)) == INVALID_ARG
