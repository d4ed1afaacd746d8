"""TAHOE_CREATE_CSR (CSR rows on oblivious and vector-leaf handles) without a GPU: the flag's value and the
two fused kernel forms in the header and the bindings, the constructors' csr= argument, and -- in a child process that sees no
HIP device -- which creates accept the bit and which refuse it, all answered before a device is touched."""
import inspect
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, INVALID_ARG, NO_DEVICE = 0, 1, 4


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def test_flag_and_forms_in_header_and_bindings(ta):
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert re.search(r"^#define TAHOE_CREATE_CSR 0x4000u$", header, re.M)
    assert ta.capi.CREATE_CSR == ta.CREATE_CSR == 0x4000
    others = [int(v, 16) for v in re.findall(r"^#define TAHOE_CREATE_\w+ (0x[0-9a-f]+)u$", header, re.M)]
    assert others.count(0x4000) == 1 and all(v & 0x4000 == 0 for v in others if v != 0x4000)  # a bit of its own
    assert re.search(r"^\s*TAHOE_OBLIVIOUS_FORM_CSR_TILE = 30,", header, re.M)
    assert re.search(r"^\s*TAHOE_VECTOR_FORM_CSR_TILE = 31\s", header, re.M)
    assert "tahoe_kernel_form_name(29)" in header  # the header says that 29 stays unassigned
    assert ta.lib.tahoe_abi_version() == 2  # no new symbol, no new version


def test_form_names(ta):
    name = lambda form: ta.lib.tahoe_kernel_form_name(form).decode()
    assert name(30) == "oblivious_csr_tile" and name(31) == "vector_csr_tile"
    assert name(29) == "?" and name(32) == "?"
    assert name(25) == "oblivious_tile" and name(28) == "vector_tile" and name(20) == "csr_rowtile"  # the others keep theirs


def test_constructors_take_csr(ta):
    for cls in (ta.capi.ObliviousForest, ta.capi.VectorForest):
        p = inspect.signature(cls.__init__).parameters
        assert "csr" in p and p["csr"].default is False, cls
        for method in ("predict_csr", "reserve_csr", "csr_plan"):  # inherited from Forest as they are
            assert getattr(cls, method) is getattr(ta.capi.Forest, method), (cls, method)


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

F = 0x4000
ob_ex = lambda flags: (lambda h: lib.tahoe_oblivious_forest_create_ex(h, depths.ctypes.data, splits.ctypes.data, leaves.ctypes.data, None,
                                                                      C.byref(op), 1, flags))
ob_cat = lambda flags: (lambda h: lib.tahoe_oblivious_forest_create_cat(h, depths.ctypes.data, splits.ctypes.data, leaves.ctypes.data, None,
                                                                        C.byref(op), 1, flags, None))
vec_ex = lambda flags: (lambda h: lib.tahoe_vector_forest_create_ex(h, trees.ctypes.data, vnodes.ctypes.data, leaves.ctypes.data, 4, None,
                                                                    C.byref(sp), 1, flags))
run("dense_ex", lambda h: lib.tahoe_forest_create_ex(h, dense.ctypes.data, C.byref(dp), F))
run("multiclass", lambda h: lib.tahoe_forest_create_multiclass(h, dense.ctypes.data, C.byref(dp), 2, F))
run("sparse_ex", lambda h: lib.tahoe_sparse_forest_create_ex(h, trees.ctypes.data, sparse.ctypes.data, covers.ctypes.data, C.byref(sp), 1, F))
run("sparse_cat", lambda h: lib.tahoe_sparse_forest_create_cat(h, trees.ctypes.data, sparse.ctypes.data, covers.ctypes.data, C.byref(sp), 1, F,
                                                               C.byref(nocats)))
run("oblivious_foreign", ob_ex(F | 0x80))
run("oblivious_cat_foreign", ob_cat(F | 0x80))
run("vector_foreign", vec_ex(F | 0x200))
run("oblivious_contribs_no_covers", ob_ex(F | 0x4))
run("vector_contribs_no_covers", vec_ex(F | 0x4))
run("oblivious_alone", ob_ex(F))
run("oblivious_beside_interventional", ob_ex(F | 0x200))  # (the flag of this create that needs no covers)
run("oblivious_beside_staged", ob_ex(F | 0x2000))
run("oblivious_cat_alone", ob_cat(F))
run("oblivious_cat_beside_staged", ob_cat(F | 0x2000))
run("vector_alone", vec_ex(F))
run("vector_beside_interventional", vec_ex(F | 0x80))
run("vector_beside_staged", vec_ex(F | 0x2000))
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
    for name in ("dense_ex", "multiclass", "sparse_ex", "sparse_cat"):
        status, text = refusals[name]
        assert status == INVALID_ARG, (name, status, text)
        assert text.startswith("unknown create flags 0x4000"), (name, text)


def test_foreign_bits_stay_refused_beside_it(refusals):
    for name in ("oblivious_foreign", "oblivious_cat_foreign"):
        status, text = refusals[name]
        assert status == INVALID_ARG, (name, status, text)
        assert text.startswith("tahoe_oblivious_forest_create_ex: flags 0x80: only"), text  # the bit is stripped before the text
    status, text = refusals["vector_foreign"]
    assert status == INVALID_ARG and text.startswith("unknown create flags 0x200 "), (status, text)
    # the flag lends no covers to a flag that needs them
    status, text = refusals["oblivious_contribs_no_covers"]
    assert status == INVALID_ARG and "leaf_covers is null" in text, (status, text)
    status, text = refusals["vector_contribs_no_covers"]
    assert status == INVALID_ARG and "TAHOE_CREATE_CONTRIBS needs covers" in text, (status, text)


def test_the_flag_passes_every_argument_check(refusals):
    for name in ("oblivious_alone", "oblivious_beside_interventional", "oblivious_beside_staged", "oblivious_cat_alone",
                 "oblivious_cat_beside_staged", "vector_alone", "vector_beside_interventional", "vector_beside_staged"):
        status, text = refusals[name]
        # every argument check has passed: the create fails only for want of a device
        assert status == NO_DEVICE, (name, status, text)
        assert "flags" not in text and "covers" not in text, (name, text)
