"""Multi-class forests through the C ABI without a GPU: the new symbols, and the argument checks of
tahoe_forest_create_multiclass, which all run before a device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    import sys

    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def _create(ta, num_trees, num_classes, output=0, flags=0, depth=2, cols=4):
    nodes = ta.synth_forest(max(num_trees, 1), depth, cols, seed=5)
    params = ta.ForestParams(0, depth, num_trees, cols, 0, output, 0.0, 0.0, 0, -999.0)
    h = C.c_void_p()
    st = ta.lib.tahoe_forest_create_multiclass(C.byref(h), nodes.ctypes.data, C.byref(params), num_classes, flags)
    assert not h.value  # nothing is created on a refused call
    return st


def test_symbols_are_exported_and_bound(ta):
    assert ta.OUT_SOFTMAX == 0x1000
    for name in ("tahoe_forest_create_multiclass", "tahoe_forest_num_classes"):
        assert name in ta.capi.EXPORTED_SYMBOLS
        assert hasattr(ta.lib, name)
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    assert " tahoe_forest_create_multiclass" in syms and " tahoe_forest_num_classes" in syms
    assert ta.lib.tahoe_abi_version() == 2


def test_num_classes_of_null_is_zero(ta):
    assert ta.lib.tahoe_forest_num_classes(None) == 0


@pytest.mark.parametrize("num_classes", [0, -1, 1025])
def test_num_classes_out_of_range(ta, num_classes):
    assert _create(ta, 6, num_classes) == INVALID_ARG
    assert "num_classes" in ta.lib.tahoe_last_error().decode()


def test_trees_not_a_multiple_of_classes(ta):
    assert _create(ta, 7, 3) == INVALID_ARG
    assert _create(ta, 10, 4) == INVALID_ARG


def test_threshold_with_several_classes(ta):
    assert _create(ta, 6, 3, output=ta.OUT_THRESHOLD) == INVALID_ARG


def test_softmax_with_sigmoid(ta):
    assert _create(ta, 6, 3, output=ta.OUT_SOFTMAX | ta.OUT_SIGMOID) == INVALID_ARG
    assert _create(ta, 6, 3, output=ta.OUT_SOFTMAX | ta.OUT_SIGMOID | ta.OUT_AVG) == INVALID_ARG


def test_softmax_with_one_class(ta):
    assert _create(ta, 6, 1, output=ta.OUT_SOFTMAX) == INVALID_ARG


def test_unknown_flag(ta):
    assert _create(ta, 6, 3, flags=0x2) == INVALID_ARG
    assert _create(ta, 6, 3, flags=0x80000000) == INVALID_ARG


def test_unknown_output_bits(ta):
    assert _create(ta, 6, 3, output=0x2000) == INVALID_ARG


def test_single_output_create_keeps_rejecting_softmax(ta):
    nodes = ta.synth_forest(6, 2, 4, seed=5)
    for output in (ta.OUT_SOFTMAX, ta.OUT_SOFTMAX | ta.OUT_AVG):
        params = ta.ForestParams(0, 2, 6, 4, 0, output, 0.0, 0.0, 0, -999.0)
        h = C.c_void_p()
        assert ta.lib.tahoe_forest_create(C.byref(h), nodes.ctypes.data, C.byref(params)) == INVALID_ARG
        assert ta.lib.tahoe_forest_create_ex(C.byref(h), nodes.ctypes.data, C.byref(params), 0) == INVALID_ARG
        assert not h.value


def test_python_forest_raises_on_refused_arguments(ta):
    nodes = ta.synth_forest(6, 2, 4, seed=5)
    with pytest.raises(ta.TahoeError) as e:
        ta.Forest(nodes, 6, 2, 4, num_classes=4)
    assert e.value.status == INVALID_ARG
    with pytest.raises(ta.TahoeError) as e:
        ta.Forest(nodes, 6, 2, 4, num_classes=3, output=ta.OUT_SOFTMAX | ta.OUT_SIGMOID)
    assert e.value.status == INVALID_ARG
