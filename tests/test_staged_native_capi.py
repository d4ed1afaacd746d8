"""TAHOE_CREATE_STAGED (staged prediction on oblivious and vector-leaf handles) without a GPU: the flag's value in the header and
the bindings, the constructors' staged= argument, and -- in a child process that sees no HIP device -- which creates accept the
bit and which refuse it, all answered before a device is touched."""
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, INVALID_ARG, NO_DEVICE, HIP = 0, 1, 4, 5


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def test_flag_value_in_header_and_bindings(ta):
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert re.search(r"^#define TAHOE_CREATE_STAGED 0x2000u$", header, re.M)
    assert ta.capi.CREATE_STAGED == ta.CREATE_STAGED == 0x2000
    others = [int(v, 16) for v in re.findall(r"^#define TAHOE_CREATE_\w+ (0x[0-9a-f]+)u$", header, re.M)]
    assert others.count(0x2000) == 1 and all(v & 0x2000 == 0 for v in others if v != 0x2000)  # a bit of its own
    assert ta.lib.tahoe_abi_version() == 2  # no new symbol, no new version


def test_constructors_take_staged(ta):
    for cls in (ta.capi.ObliviousForest, ta.capi.VectorForest):
        p = inspect.signature(cls.__init__).parameters
        assert "staged" in p and p["staged"].default is False, cls
    for method in ("set_stages", "predict_staged", "staged_strategy"):
        assert hasattr(ta.capi.ObliviousForest, method) and hasattr(ta.capi.VectorForest, method)


CHILD = r"""
import ctypes as C, json
import numpy as np
import tahoe_amd as ta
from tahoe_amd.capi import ForestParams, CategoricalSplits, OBLIVIOUS_SPLIT_DTYPE, SPARSE_NODE_DTYPE, NODE_DTYPE

lib, out = ta.lib, {}
def run(name, call):
    h = C.c_void_p()
    status = call(C.byref(h))
    out[name] = [status, lib.tahoe_last_error().decode()]
    if status == 0:
        lib.tahoe_forest_destroy(h)

# two stumps on one column: dense heap trees of depth 1, the same as sparse nodes, and as oblivious trees of depth 1
dense = np.zeros(6, NODE_DTYPE)
dense["bits"][[1, 2, 4, 5]] = np.int32(-(1 << 31))
dp = ForestParams(6, 1, 2, 1, 0, 0, 0.5, 0.0, 0, -999.0)
sparse = np.zeros(6, SPARSE_NODE_DTYPE)
sparse["bits"][[1, 2, 4, 5]] = np.int32(-(1 << 31))
sparse["left_idx"][[0, 3]] = 1
trees = np.array([0, 3], np.int32)
covers = np.ones(6, np.float32)
sp = ForestParams(6, 0, 2, 1, 0, 0, 0.5, 0.0, 0, -999.0)
nocats = CategoricalSplits()
depths = np.array([1, 1], np.int32)
splits = np.zeros(2, OBLIVIOUS_SPLIT_DTYPE)
leaves = np.arange(4, dtype=np.float32)
op = ForestParams(0, 0, 2, 1, 0, 0, 0.5, 0.0, 0, -999.0)
vnodes = sparse.copy()
vnodes["left_idx"][[1, 2, 4, 5]] = [0, 1, 2, 3]  # a leaf names its vector

S = 0x2000
run("dense_ex", lambda h: lib.tahoe_forest_create_ex(h, dense.ctypes.data, C.byref(dp), S))
run("dense_ex_contribs", lambda h: lib.tahoe_forest_create_ex(h, dense.ctypes.data, C.byref(dp), S | 0x4))
run("multiclass", lambda h: lib.tahoe_forest_create_multiclass(h, dense.ctypes.data, C.byref(dp), 2, S))
run("sparse_ex", lambda h: lib.tahoe_sparse_forest_create_ex(h, trees.ctypes.data, sparse.ctypes.data, covers.ctypes.data, C.byref(sp), 1, S))
run("sparse_ex_mc", lambda h: lib.tahoe_sparse_forest_create_ex(h, trees.ctypes.data, sparse.ctypes.data, None, C.byref(sp), 2, S))
run("sparse_cat", lambda h: lib.tahoe_sparse_forest_create_cat(h, trees.ctypes.data, sparse.ctypes.data, covers.ctypes.data, C.byref(sp), 1, S,
                                                               C.byref(nocats)))
run("oblivious_foreign", lambda h: lib.tahoe_oblivious_forest_create_ex(h, depths.ctypes.data, splits.ctypes.data, leaves.ctypes.data, None,
                                                                        C.byref(op), 1, S | 0x80))
run("oblivious_cat_foreign", lambda h: lib.tahoe_oblivious_forest_create_cat(h, depths.ctypes.data, splits.ctypes.data, leaves.ctypes.data,
                                                                            None, C.byref(op), 1, S | 0x80, None))
run("vector_foreign", lambda h: lib.tahoe_vector_forest_create_ex(h, trees.ctypes.data, vnodes.ctypes.data, leaves.ctypes.data, 4, None,
                                                                  C.byref(sp), 1, S | 0x200))
run("oblivious_contribs_no_covers", lambda h: lib.tahoe_oblivious_forest_create_ex(h, depths.ctypes.data, splits.ctypes.data,
                                                                                   leaves.ctypes.data, None, C.byref(op), 1, S | 0x4))
run("vector_contribs_no_covers", lambda h: lib.tahoe_vector_forest_create_ex(h, trees.ctypes.data, vnodes.ctypes.data, leaves.ctypes.data, 4,
                                                                             None, C.byref(sp), 1, S | 0x4))
run("oblivious_alone", lambda h: lib.tahoe_oblivious_forest_create_ex(h, depths.ctypes.data, splits.ctypes.data, leaves.ctypes.data, None,
                                                                      C.byref(op), 1, S))
run("oblivious_cat_alone", lambda h: lib.tahoe_oblivious_forest_create_cat(h, depths.ctypes.data, splits.ctypes.data, leaves.ctypes.data, None,
                                                                          C.byref(op), 1, S, None))
run("oblivious_beside_interventional", lambda h: lib.tahoe_oblivious_forest_create_ex(h, depths.ctypes.data, splits.ctypes.data,
                                                                                      leaves.ctypes.data, None, C.byref(op), 1, S | 0x200))
run("vector_alone", lambda h: lib.tahoe_vector_forest_create_ex(h, trees.ctypes.data, vnodes.ctypes.data, leaves.ctypes.data, 4, None,
                                                                C.byref(sp), 1, S))
run("vector_beside_interventional", lambda h: lib.tahoe_vector_forest_create_ex(h, trees.ctypes.data, vnodes.ctypes.data, leaves.ctypes.data,
                                                                                4, None, C.byref(sp), 1, S | 0x80))
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def refusals(ta):
    """name -> (status, text) of every create call of CHILD, made where no HIP device is visible"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_every_other_create_refuses_the_bit_as_unknown(refusals):
    for name, flags in (("dense_ex", 0x2000), ("dense_ex_contribs", 0x2004), ("multiclass", 0x2000), ("sparse_ex", 0x2000),
                        ("sparse_ex_mc", 0x2000), ("sparse_cat", 0x2000)):
        status, text = refusals[name]
        assert status == INVALID_ARG, (name, status, text)
        assert text.startswith(f"unknown create flags 0x{flags:x}"), (name, text)


def test_foreign_bits_stay_refused_beside_it(refusals):
    for name in ("oblivious_foreign", "oblivious_cat_foreign"):
        status, text = refusals[name]
        assert status == INVALID_ARG and "0x80" in text, (name, status, text)
        assert re.match(r"tahoe_oblivious_forest_create_ex: flags 0x[0-9a-f]+: only", text), text
    status, text = refusals["vector_foreign"]
    assert status == INVALID_ARG and text.startswith("unknown create flags 0x200 "), (status, text)
    # the flag lends no covers to a flag that needs them
    status, text = refusals["oblivious_contribs_no_covers"]
    assert status == INVALID_ARG and "leaf_covers is null" in text, (status, text)
    status, text = refusals["vector_contribs_no_covers"]
    assert status == INVALID_ARG and "TAHOE_CREATE_CONTRIBS needs covers" in text, (status, text)


def test_the_flag_alone_needs_no_covers(refusals):
    for name in ("oblivious_alone", "oblivious_cat_alone", "oblivious_beside_interventional", "vector_alone",
                 "vector_beside_interventional"):
        status, text = refusals[name]
        # every argument check has passed: the create fails only for want of a device, or succeeds
        assert status in (OK, NO_DEVICE, HIP), (name, status, text)
        assert "flags" not in text and "covers" not in text, (name, text)
