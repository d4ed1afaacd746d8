"""TAHOE_CREATE_NAN_MISSING (a NaN feature value is missing, beside the sentinel) without a GPU: the flag's
value in the header and the bindings, the constructors' nan_missing= argument and their ValueErrors, and -- in a child process
that sees no HIP device -- which creates accept the bit and which refuse it, with the flag's name in tahoe_last_error() and
before a device is touched."""
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, INVALID_ARG, NO_DEVICE, HIP = 0, 1, 4, 5
FLAG = 0x1000


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
    assert re.search(r"^#define TAHOE_CREATE_NAN_MISSING 0x1000u$", header, re.M)
    assert ta.capi.CREATE_NAN_MISSING == ta.CREATE_NAN_MISSING == FLAG
    values = [int(v, 16) for v in re.findall(r"^#define TAHOE_CREATE_\w+ (0x[0-9a-f]+)u$", header, re.M)]
    bound = {k: v for k, v in vars(ta.capi).items() if k.startswith("CREATE_")}
    assert len(values) == len(bound) and len(set(values)) == len(values)  # distinct from every other TAHOE_CREATE_*
    assert values.count(FLAG) == 1 and all(v & FLAG == 0 for v in values if v != FLAG)  # a bit of its own
    assert [k for k, v in bound.items() if v == FLAG] == ["CREATE_NAN_MISSING"]
    assert ta.lib.tahoe_abi_version() == 2  # no new symbol, no new version
    # the rule is spelled out once in the header, and the CSR and columns paragraphs refer to it
    assert header.count("isnan(x) || fabsf(x - params.missing) <= 1e-6f") == 1
    for call in ("tahoe_forest_predict_csr", "tahoe_forest_predict_columns"):
        doc = header[:header.index("tahoe_status " + call + "(")].rsplit("/*", 1)[1]
        assert "TAHOE_CREATE_NAN_MISSING" in doc, call


def test_constructors_take_nan_missing(ta):
    for cls in (ta.capi.Forest, ta.capi.SparseForest):
        p = inspect.signature(cls.__init__).parameters
        assert "nan_missing" in p and p["nan_missing"].default is False, cls
    for cls in (ta.capi.ObliviousForest, ta.capi.VectorForest):  # their creates refuse the flag
        assert "nan_missing" not in inspect.signature(cls.__init__).parameters, cls


def test_wrapper_raises_value_error_before_the_library_is_called(ta, monkeypatch):
    def no_call(*a, **k):
        raise AssertionError("the C create was called")

    for name in ("tahoe_forest_create", "tahoe_forest_create_ex", "tahoe_forest_create_multiclass", "tahoe_sparse_forest_create",
                 "tahoe_sparse_forest_create_ex", "tahoe_sparse_forest_create_cat"):
        monkeypatch.setattr(ta.lib, name, no_call)
    nodes = np.zeros(3, ta.NODE_DTYPE)
    for kw in ({"contribs": True}, {"approx_contribs": True}, {"contribs": True, "approx_contribs": True}):
        for nc in (1, 2):
            with pytest.raises(ValueError, match="TAHOE_CREATE_NAN_MISSING") as e:
                ta.capi.Forest(nodes, 1, 1, 1, nan_missing=True, num_classes=nc, **kw)
            assert all(k in str(e.value) for k in kw)
    sn = np.zeros(3, ta.capi.SPARSE_NODE_DTYPE)
    tr = np.zeros(1, np.int32)
    cv = np.ones(3, np.float32)
    for kw in ({"contribs": True}, {"approx_contribs": True}, {"partial_dependence": True}):
        for cats in (None, {0: [1, 2]}):
            with pytest.raises(ValueError, match="TAHOE_CREATE_NAN_MISSING") as e:
                ta.capi.SparseForest(sn, tr, 1, covers=cv, nan_missing=True, categories=cats, **kw)
            assert all(k in str(e.value) for k in kw)


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
dense["weight"] = 1.0
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

N = 0x1000
dense_ex = lambda fl: (lambda h: lib.tahoe_forest_create_ex(h, dense.ctypes.data, C.byref(dp), fl))
dense_mc = lambda fl: (lambda h: lib.tahoe_forest_create_multiclass(h, dense.ctypes.data, C.byref(dp), 2, fl))
sparse_ex = lambda fl, nc=1: (lambda h: lib.tahoe_sparse_forest_create_ex(h, trees.ctypes.data, sparse.ctypes.data, covers.ctypes.data,
                                                                         C.byref(sp), nc, fl))
sparse_cat = lambda fl: (lambda h: lib.tahoe_sparse_forest_create_cat(h, trees.ctypes.data, sparse.ctypes.data, covers.ctypes.data,
                                                                      C.byref(sp), 1, fl, C.byref(nocats)))
# accepted
run("ok_dense_ex", dense_ex(N))
run("ok_dense_ex_relayout", dense_ex(N | 0x1))
run("ok_multiclass", dense_mc(N))
run("ok_multiclass_relayout", dense_mc(N | 0x1))
run("ok_sparse_ex", sparse_ex(N))
run("ok_sparse_ex_mc", sparse_ex(N, 2))
run("ok_sparse_cat", sparse_cat(N))
# refused beside an explanation flag or partial dependence
for name, bit in (("contribs", 0x4), ("approx", 0x10), ("both", 0x14)):
    run("no_dense_ex_" + name, dense_ex(N | bit))
    run("no_multiclass_" + name, dense_mc(N | bit))
    run("no_sparse_ex_" + name, sparse_ex(N | bit))
    run("no_sparse_cat_" + name, sparse_cat(N | bit))
run("no_sparse_ex_pd", sparse_ex(N | 0x800))
run("no_sparse_cat_pd", sparse_cat(N | 0x800))
run("no_sparse_cat_cat_contribs", sparse_cat(N | 0x4 | 0x20))
# refused on oblivious and vector-leaf creates, alone and beside flags they take
for name, bit in (("alone", 0), ("staged", 0x2000), ("csr", 0x4000)):
    run("no_oblivious_" + name, lambda h: lib.tahoe_oblivious_forest_create_ex(h, depths.ctypes.data, splits.ctypes.data, leaves.ctypes.data,
                                                                             None, C.byref(op), 1, N | bit))
    run("no_oblivious_cat_" + name, lambda h: lib.tahoe_oblivious_forest_create_cat(h, depths.ctypes.data, splits.ctypes.data,
                                                                                  leaves.ctypes.data, None, C.byref(op), 1, N | bit, None))
    run("no_vector_" + name, lambda h: lib.tahoe_vector_forest_create_ex(h, trees.ctypes.data, vnodes.ctypes.data, leaves.ctypes.data, 4, None,
                                                                       C.byref(sp), 1, N | bit))
# an unknown bit beside the flag stays unknown
run("unknown_dense", dense_ex(N | 0x8000))
run("unknown_sparse", sparse_ex(N | 0x8000))
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def creates(ta):
    """name -> (status, text) of every create call of CHILD, made where no HIP device is visible"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_the_five_creates_accept_the_flag(creates):
    names = [n for n in creates if n.startswith("ok_")]
    assert len(names) == 7
    for name in names:
        status, text = creates[name]
        # every argument check has passed: the create fails only for want of a device, or succeeds
        assert status in (OK, NO_DEVICE, HIP), (name, status, text)
        assert "flags" not in text and "NAN_MISSING" not in text, (name, text)


def test_refusals_name_the_flag_and_come_before_a_device_is_touched(creates):
    names = [n for n in creates if n.startswith("no_")]
    assert len(names) == 12 + 3 + 9
    for name in names:
        status, text = creates[name]
        assert status == INVALID_ARG, (name, status, text)  # (not NO_DEVICE: no device was asked for)
        assert "TAHOE_CREATE_NAN_MISSING" in text, (name, text)
    assert "oblivious" in creates["no_oblivious_alone"][1] and "oblivious" in creates["no_oblivious_cat_staged"][1]
    assert "vector-leaf" in creates["no_vector_csr"][1]
    for name in ("no_dense_ex_contribs", "no_sparse_ex_pd", "no_sparse_cat_cat_contribs"):
        assert "TAHOE_CREATE_CONTRIBS" in creates[name][1] and "_PARTIAL_DEPENDENCE" in creates[name][1]


def test_an_unknown_bit_beside_the_flag_stays_unknown(creates):
    for name in ("unknown_dense", "unknown_sparse"):
        status, text = creates[name]
        assert status == INVALID_ARG and text.startswith("unknown create flags 0x9000"), (name, status, text)
