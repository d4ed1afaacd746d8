"""Per-feature contributions (TAHOE_CREATE_CONTRIBS, tahoe_forest_predict_contribs) without a GPU: the symbols, the cover checks
of create (they run before a device is touched), the NULL-handle refusal, and the two float64 references of tests/contribs_ref.py
against each other and against the oracle's float64 sums."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contribs_ref  # noqa: E402

INVALID_ARG, NO_DEVICE, INVALID_FOREST = 1, 4, 6
MISSING = -999.0


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def _create(ta, nodes, T, D, cols, num_classes=1, flags=0x4):
    params = ta.ForestParams(0, D, T, cols, 0, 0, 0.0, 0.0, 0, MISSING)
    h = C.c_void_p()
    if num_classes == 1:
        st = ta.lib.tahoe_forest_create_ex(C.byref(h), nodes.ctypes.data, C.byref(params), flags)
    else:
        st = ta.lib.tahoe_forest_create_multiclass(C.byref(h), nodes.ctypes.data, C.byref(params), num_classes, flags)
    if st != 0:
        assert not h.value  # nothing is created on a refused call
    else:  # accepted, on a machine with a GPU
        ta.lib.tahoe_forest_destroy(h)
    return st


def test_symbols_are_exported_and_bound(ta):
    assert ta.CREATE_CONTRIBS == 0x4 and ta.capi.CREATE_CONTRIBS == 0x4
    assert "tahoe_forest_predict_contribs" in ta.capi.EXPORTED_SYMBOLS
    assert hasattr(ta.lib, "tahoe_forest_predict_contribs")
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    assert " tahoe_forest_predict_contribs" in syms
    assert ta.lib.tahoe_abi_version() == 2


def test_predict_contribs_on_null_handle(ta):
    assert ta.lib.tahoe_forest_predict_contribs(None, None, None, 0, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_predict_contribs(None, None, None, 10, None) == INVALID_ARG


@pytest.mark.parametrize("bad", [0.0, -0.5, float("nan"), float("inf")])
@pytest.mark.parametrize("num_classes", [1, 2])
def test_bad_child_weights_are_refused(ta, bad, num_classes):
    T, D, cols = 4, 3, 5
    nodes = ta.synth_forest(T, D, cols, seed=3)
    per = ta.capi.tree_num_nodes(D)
    nodes["weight"] = 1.0
    # tree 2, node 1 (internal): its children 3 and 4
    if bad == 0.0:
        nodes["weight"][2 * per + 3] = 0.0
        nodes["weight"][2 * per + 4] = 0.0
    else:
        nodes["weight"][2 * per + 4] = bad
    assert _create(ta, nodes, T, D, cols, num_classes) == INVALID_FOREST
    msg = ta.lib.tahoe_last_error().decode()
    assert "tree 2 node 1" in msg, msg


def test_one_zero_child_weight_is_accepted(ta):
    T, D, cols = 2, 3, 5
    nodes = ta.synth_forest(T, D, cols, seed=3)
    nodes["weight"] = 1.0
    nodes["weight"][3] = 0.0  # one child of node 1 has cover 0, its sibling 1: a valid split
    assert _create(ta, nodes, T, D, cols) not in (INVALID_FOREST, INVALID_ARG)


def test_weights_below_a_leaf_are_ignored(ta):
    T, D, cols = 1, 3, 5
    nodes = ta.synth_forest(T, D, cols, seed=3)
    nodes["weight"] = 1.0
    nodes["bits"][1] = nodes["bits"][1] | np.int32(-2 ** 31)  # node 1 becomes a leaf: nodes 3, 4 and below are unreachable
    nodes["weight"][3] = np.nan
    nodes["weight"][4] = -1.0
    nodes["weight"][7] = 0.0
    nodes["weight"][8] = 0.0
    assert _create(ta, nodes, T, D, cols) not in (INVALID_FOREST, INVALID_ARG)
    # ... and the same weights at a reachable node are refused
    nodes["bits"][1] = nodes["bits"][1] & np.int32(0x7FFFFFFF)
    assert _create(ta, nodes, T, D, cols) == INVALID_FOREST


def test_flag_without_contribs_ignores_weights(ta):
    T, D, cols = 2, 3, 5
    nodes = ta.synth_forest(T, D, cols, seed=3)
    nodes["weight"] = np.nan
    assert _create(ta, nodes, T, D, cols, flags=0) not in (INVALID_FOREST, INVALID_ARG)
    assert _create(ta, nodes, T, D, cols, flags=0x1) not in (INVALID_FOREST, INVALID_ARG)


def test_python_forest_raises_on_bad_covers(ta):
    nodes = ta.synth_forest(3, 2, 4, seed=5)
    nodes["weight"] = -1.0
    with pytest.raises(ta.TahoeError) as e:
        ta.Forest(nodes, 3, 2, 4, contribs=True)
    assert e.value.status == INVALID_FOREST


def random_forest(ta, rng, T, D, cols, nan_thr=0.05):
    """synth_forest (u01 covers) with early leaves, a depth-0-like tree (root leaf) and some NaN thresholds."""
    nodes = ta.synth_forest(T, D, cols, seed=int(rng.integers(1 << 30)), leaf_prob=0.15)
    per = ta.capi.tree_num_nodes(D)
    nodes["weight"] = rng.uniform(0.05, 1.0, nodes.size).astype(np.float32)
    internal = (nodes["bits"].view(np.uint32) >> 31) == 0
    nodes["val"][internal & (rng.random(nodes.size) < nan_thr)] = np.nan
    nodes["bits"][0] = nodes["bits"][0] | np.int32(-2 ** 31)  # tree 0 is a single leaf
    assert per * T == nodes.size
    return nodes


def random_rows(ta, rng, rows, cols):
    x = ta.synth_data(rows, cols, seed=int(rng.integers(1 << 30)), missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    return x


@pytest.mark.parametrize("seed", range(6))
def test_references_agree(ta, seed):
    rng = np.random.default_rng(seed)
    T, D, cols = 5, int(rng.integers(1, 6)), int(rng.integers(2, 7))
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 40, cols)
    for C_, avg, bias in ((1, False, 0.0), (1, True, 0.5), (5, True, -0.25)):
        b = contribs_ref.brute(nodes, T, D, cols, x, MISSING, num_classes=C_, avg=avg, global_bias=bias)
        p, A, _ = contribs_ref.poly(nodes, T, D, cols, x, MISSING, num_classes=C_, avg=avg, global_bias=bias)
        scale = np.abs(b).sum(axis=-1, keepdims=True) + 1e-300
        assert np.all(np.abs(b - p) <= 1e-12 * scale), np.max(np.abs(b - p) / scale)
        assert np.all(A >= np.abs(p) - 1e-12 * scale)


def test_reference_additivity_against_oracle(ta):
    from oracle import oracle

    rng = np.random.default_rng(11)
    T, D, cols = 8, 5, 4  # few columns: features repeat on paths
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 64, cols)
    want = oracle.predict_f64(nodes, T, D, x, MISSING)
    p, A, _ = contribs_ref.poly(nodes, T, D, cols, x, MISSING)
    got = p[:, 0, :].sum(axis=1)
    # the bias column is float32; the rest is float64
    assert np.all(np.abs(got - want) <= 1e-6 * (np.abs(want) + A[:, 0, :].sum(axis=1))), np.max(np.abs(got - want))


def test_bias_is_float64_then_float32(ta):
    rng = np.random.default_rng(5)
    T, D, cols = 6, 4, 3
    nodes = random_forest(ta, rng, T, D, cols)
    b = contribs_ref.bias_f32(nodes, T, D, num_classes=2, avg=True, global_bias=0.125)
    per = nodes.size // T
    want = [np.float32(sum(contribs_ref.tree_expectation(nodes.reshape(T, per)[t]) for t in range(c, T, 2)) / 3 + 0.125)
            for c in range(2)]
    assert b.dtype == np.float32 and list(b) == want
