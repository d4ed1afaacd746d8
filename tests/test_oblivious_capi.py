"""tahoe_oblivious_forest_create without a GPU: the symbol, its binding and header, the Python class, and -- in a child process
that sees no device -- every argument refusal with its code and text (none may be TAHOE_ERR_NO_DEVICE: all checks run before a
device is touched) and a valid create that gets as far as the device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE, INVALID_FOREST, UNSUPPORTED = 0, 1, 4, 6, 7


@pytest.fixture(scope="module")
def ta(built):
    import tahoe_amd

    return tahoe_amd


def test_symbol_is_exported_bound_and_declared(ta):
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    assert "tahoe_oblivious_forest_create" in ta.capi.EXPORTED_SYMBOLS
    assert hasattr(ta.lib, "tahoe_oblivious_forest_create")
    assert " tahoe_oblivious_forest_create" in syms
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert "tahoe_status tahoe_oblivious_forest_create(" in header and "tahoe_oblivious_split;" in header
    assert "TAHOE_OBLIVIOUS_FORM_DIRECT = 24" in header and "TAHOE_OBLIVIOUS_FORM_TILE = 25" in header
    assert ta.lib.tahoe_abi_version() == 2
    assert ta.lib.tahoe_kernel_form_name(24) == b"oblivious_direct" and ta.lib.tahoe_kernel_form_name(25) == b"oblivious_tile"
    assert ta.lib.tahoe_kernel_form_name(23) == b"?" and ta.lib.tahoe_kernel_form_name(26) == b"?"  # 23 stays unassigned


def test_python_surface(ta):
    assert issubclass(ta.ObliviousForest, ta.Forest) and ta.ObliviousForest is ta.capi.ObliviousForest
    assert ta.strict_borders is ta.capi.strict_borders
    assert ta.capi.OBLIVIOUS_SPLIT_DTYPE.itemsize == 8
    with pytest.raises(ValueError):
        ta.ObliviousForest([1], [0, 1], [0.5, 0.5], [0, 0], [1.0, 2.0], 2)  # two splits for a sum of depths of 1
    with pytest.raises(ValueError):
        ta.ObliviousForest([1], [0], [0.5], [0], [1.0, 2.0, 3.0], 2)  # three leaves for a tree of depth 1


CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import tahoe_amd as ta

def create(depths, fids, leaves, cols, k=1, output=0, trees=None, null=()):
    depths = np.ascontiguousarray(depths, np.int32)
    splits = np.zeros(max(len(fids), 1), ta.capi.OBLIVIOUS_SPLIT_DTYPE)
    splits["bits"][:len(fids)] = fids
    leaves = np.ascontiguousarray(leaves, np.float32)
    params = ta.ForestParams(0, 0, len(depths) if trees is None else trees, cols, 0, output, 0.5, 0.0, 0, -999.0)
    h = C.c_void_p()
    st = ta.lib.tahoe_oblivious_forest_create(None if "out" in null else C.byref(h), None if "depths" in null else depths.ctypes.data,
                                              None if "splits" in null else splits.ctypes.data,
                                              None if "leaves" in null else leaves.ctypes.data,
                                              None if "params" in null else C.byref(params), k)
    assert not h.value
    return [st, ta.lib.tahoe_last_error().decode()]

good = dict(depths=[1, 0, 2], fids=[0, 1, 2], leaves=np.arange(7.0), cols=3)
two = dict(good, leaves=np.arange(14.0), k=2)
res = {}
for n in ("out", "depths", "leaves", "params", "splits"):
    res["null_" + n] = create(**good, null=(n,))
res["null_splits_depth0"] = create([0, 0], [], [1.0, 2.0], 3, null=("splits",))
res["neg_trees"] = create(**good, trees=-1)
res["leaf_dim_0"] = create(**dict(good, k=0))
res["leaf_dim_1025"] = create(**dict(good, k=1025))
res["softmax_k1"] = create(**good, output=ta.OUT_SOFTMAX)
res["softmax_sigmoid"] = create(**two, output=ta.OUT_SOFTMAX | ta.OUT_SIGMOID)
res["threshold_k2"] = create(**two, output=ta.OUT_THRESHOLD)
res["unknown_output"] = create(**good, output=0x2)
res["depth_17"] = create([1, 17, 0], [0] * 18, np.zeros(8), 3)
res["depth_neg"] = create([1, 0, -1], [0], np.zeros(8), 3)
res["fid"] = create([1, 0, 2], [0, 1, 3], np.arange(7.0), 3)
res["valid"] = create(**good)
res["valid_k2_softmax"] = create(**two, output=ta.OUT_SOFTMAX)
res["valid_odd_trees_k2"] = create(**two)  # 3 trees, 2 outputs: no multiple-of-classes rule
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def refusals(ta):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case,status,text", [
    ("null_out", INVALID_ARG, "null argument"), ("null_depths", INVALID_ARG, "null argument"),
    ("null_leaves", INVALID_ARG, "null argument"), ("null_params", INVALID_ARG, "null argument"),
    ("null_splits", INVALID_ARG, "splits is null"), ("neg_trees", INVALID_ARG, "num_trees"),
    ("leaf_dim_0", INVALID_ARG, "leaf_dim must be in [1,1024], got 0"), ("leaf_dim_1025", INVALID_ARG, "leaf_dim must be in [1,1024], got 1025"),
    ("softmax_k1", INVALID_ARG, ""), ("softmax_sigmoid", INVALID_ARG, "SOFTMAX and SIGMOID"),
    ("threshold_k2", INVALID_ARG, "THRESHOLD needs"), ("unknown_output", INVALID_ARG, "output should be"),
    ("depth_17", INVALID_ARG, "tree 1: depth 17"), ("depth_neg", INVALID_ARG, "tree 2: depth -1"),
    ("fid", INVALID_FOREST, "tree 2 level 1: fid 3 >= num_cols 3"),
])
def test_refusals_come_before_the_device(refusals, case, status, text):
    got, msg = refusals[case]
    assert got == status and got != NO_DEVICE, (got, msg)
    assert text in msg, msg


@pytest.mark.parametrize("case", ["valid", "valid_k2_softmax", "valid_odd_trees_k2", "null_splits_depth0"])
def test_a_valid_create_reaches_the_device(refusals, case):
    got, msg = refusals[case]
    assert got == NO_DEVICE, (got, msg)
