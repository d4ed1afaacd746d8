"""TAHOE_CREATE_VECTOR_INTERACTIONS without a GPU: the flag in the header and the Python layer, and -- in a child process that sees
no device -- which creates accept it and what tahoe_vector_forest_create_ex checks with it: it needs TAHOE_CREATE_CONTRIBS beside it,
then the covers as that flag does; TAHOE_CREATE_INTERVENTIONAL may join.  All of these run before a device is touched."""
import inspect
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE, INVALID_FOREST, UNSUPPORTED = 0, 1, 4, 6, 7


@pytest.fixture(scope="module")
def ta(built):
    import tahoe_amd

    return tahoe_amd


def test_flag_is_declared_and_bound(ta):
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert "#define TAHOE_CREATE_VECTOR_INTERACTIONS 0x100u" in header
    assert "#define TAHOE_CREATE_INTERACTIONS 0x40u" in header  # the oblivious create's flag keeps its bit
    assert ta.capi.CREATE_VECTOR_INTERACTIONS == 0x100 and ta.CREATE_VECTOR_INTERACTIONS == 0x100
    sig = inspect.signature(ta.VectorForest.__init__)
    assert sig.parameters["interactions"].default is False
    assert "interactions=True" in ta.VectorForest.__doc__ and "VectorForest" in ta.Forest.predict_interactions.__doc__


CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import tahoe_amd as ta

LEAF = -(1 << 31)
VI, IV, CONTRIBS = 0x100, 0x80, ta.capi.CREATE_CONTRIBS
lib = ta.lib

def create(nodes, trees, leaves, cols, covers, k=1, flags=VI | CONTRIBS, null_covers=False):
    n = np.zeros(max(len(nodes), 1), ta.capi.SPARSE_NODE_DTYPE)
    for i, (val, bits, left) in enumerate(nodes):
        n[i] = (val, bits, left)
    trees = np.ascontiguousarray(trees, np.int32)
    leaves = np.ascontiguousarray(leaves, np.float32)
    covers = np.ascontiguousarray(covers, np.float32)
    params = ta.ForestParams(len(nodes), 0, len(trees), cols, 0, 0, 0.5, 0.0, 0, -999.0)
    h = C.c_void_p()
    st = lib.tahoe_vector_forest_create_ex(C.byref(h), trees.ctypes.data, n.ctypes.data, leaves.ctypes.data, leaves.size // k,
                                           None if null_covers else covers.ctypes.data, C.byref(params), k, flags)
    assert not h.value
    return [st, lib.tahoe_last_error().decode()]

# tree 0: a stump on feature 1; tree 1: a single leaf; tree 2: x0, then x2 on the right
NODES = [(0.5, 1 | 1 << 30, 1), (0.0, LEAF, 3), (0.0, LEAF, 0),
         (0.0, LEAF, 2),
         (0.0, 0, 1), (0.0, LEAF, 1), (1.0, 2, 3), (0.0, LEAF, 3), (0.0, LEAF, 0)]
COVERS = [4.0, 1.0, 3.0, 5.0, 9.0, 2.0, 7.0, 3.0, 4.0]
GARBAGE = [float("nan"), -1.0, float("inf")] * 3
good = dict(nodes=NODES, trees=[0, 3, 4], leaves=np.arange(8.0), cols=3, covers=COVERS, k=2)

def chain(n):
    nodes = []
    for i in range(n):
        nodes += [(0.0, i, 2 * i + 1), (0.0, LEAF, 0)]
    return nodes + [(0.0, LEAF, 0)]

res = {}
res["with_contribs"] = create(**good)
res["with_contribs_k1"] = create(**dict(good, leaves=np.arange(4.0), k=1))
res["with_both"] = create(**good, flags=VI | CONTRIBS | IV)
res["chain_31"] = create(chain(31), [0], [1.0, 2.0], 40, np.ones(63), k=2)
res["alone"] = create(**good, flags=VI)
res["alone_null_covers"] = create(**good, flags=VI, null_covers=True)
res["with_interventional_only"] = create(**good, flags=VI | IV)
res["null_covers"] = create(**good, null_covers=True)
res["garbage_covers"] = create(**dict(good, covers=GARBAGE))
res["garbage_covers_with_both"] = create(**dict(good, covers=GARBAGE), flags=VI | CONTRIBS | IV)
res["chain_32"] = create(chain(32), [0], [1.0, 2.0], 40, np.ones(65), k=2)
res["with_0x40"] = create(**good, flags=VI | CONTRIBS | 0x40)
res["with_approx"] = create(**good, flags=VI | CONTRIBS | 0x10)
res["with_0x200"] = create(**good, flags=VI | CONTRIBS | 0x200)

# the other creates refuse the flag
h = C.c_void_p()
sn = np.zeros(3, ta.capi.SPARSE_NODE_DTYPE)
sn[0] = (0.5, 0, 1); sn[1] = (1.0, LEAF, 0); sn[2] = (2.0, LEAF, 0)
roots = np.zeros(1, np.int32)
cv = np.ones(3, np.float32)
sp = ta.ForestParams(3, 0, 1, 2, 0, 0, 0.5, 0.0, 0, -999.0)
dn = ta.synth_forest(2, 2, 3, seed=1)
dp = ta.ForestParams(dn.size, 2, 2, 3, 0, 0, 0.5, 0.0, 0, -999.0)
depths = np.array([1, 0, 2], np.int32)
splits = np.zeros(3, ta.capi.OBLIVIOUS_SPLIT_DTYPE)
splits["bits"] = [0, 1, 2]
ol, oc = np.arange(7.0, dtype=np.float32), np.ones(7, np.float32)
op = ta.ForestParams(0, 0, 3, 3, 0, 0, 0.5, 0.0, 0, -999.0)
cats, keep = ta.capi.pack_categorical({0: [1, 3]})
for name, fl in (("", VI), ("_with_contribs", VI | CONTRIBS)):
    res["sparse" + name] = [lib.tahoe_sparse_forest_create_ex(C.byref(h), roots.ctypes.data, sn.ctypes.data, cv.ctypes.data, C.byref(sp),
                                                              1, fl), lib.tahoe_last_error().decode()]
    assert not h.value
    res["dense" + name] = [lib.tahoe_forest_create_ex(C.byref(h), dn.ctypes.data, C.byref(dp), fl), lib.tahoe_last_error().decode()]
    assert not h.value
    res["oblivious" + name] = [lib.tahoe_oblivious_forest_create_ex(C.byref(h), depths.ctypes.data, splits.ctypes.data, ol.ctypes.data,
                                                                    oc.ctypes.data, C.byref(op), 1, fl), lib.tahoe_last_error().decode()]
    assert not h.value
    res["categorical" + name] = [lib.tahoe_sparse_forest_create_cat(C.byref(h), roots.ctypes.data, sn.ctypes.data, cv.ctypes.data,
                                                                    C.byref(sp), 1, fl, C.byref(cats)), lib.tahoe_last_error().decode()]
    assert not h.value
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def results(ta):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", ["with_contribs", "with_contribs_k1", "with_both", "chain_31"])
def test_the_flag_passes_the_checks_and_reaches_the_device(results, case):
    got, msg = results[case]
    assert got == NO_DEVICE and "unknown create flags" not in msg, (got, msg)


@pytest.mark.parametrize("case,status,texts", [
    ("alone", INVALID_ARG, ("TAHOE_CREATE_VECTOR_INTERACTIONS", "TAHOE_CREATE_CONTRIBS")),
    ("alone_null_covers", INVALID_ARG, ("TAHOE_CREATE_VECTOR_INTERACTIONS", "TAHOE_CREATE_CONTRIBS")),
    ("with_interventional_only", INVALID_ARG, ("TAHOE_CREATE_VECTOR_INTERACTIONS", "TAHOE_CREATE_CONTRIBS")),
    ("null_covers", INVALID_ARG, ("TAHOE_CREATE_CONTRIBS needs covers",)),
    ("garbage_covers", INVALID_FOREST, ("tree 0 node 0: child covers -1 and inf",)),
    ("garbage_covers_with_both", INVALID_FOREST, ("tree 0 node 0: child covers -1 and inf",)),
    ("chain_32", UNSUPPORTED, ("tree 0: a leaf's path has 32 distinct features",)),
    ("with_0x40", INVALID_ARG, ("unknown create flags 0x40",)),
    ("with_approx", INVALID_ARG, ("unknown create flags 0x10",)),
    ("with_0x200", INVALID_ARG, ("unknown create flags 0x200",)),
    ("sparse", INVALID_ARG, ("unknown create flags 0x100",)),
    ("sparse_with_contribs", INVALID_ARG, ("unknown create flags 0x104",)),
    ("dense", INVALID_ARG, ("unknown create flags 0x100",)),
    ("dense_with_contribs", INVALID_ARG, ("unknown create flags 0x104",)),
    ("categorical", INVALID_ARG, ("unknown create flags 0x100",)),
    ("categorical_with_contribs", INVALID_ARG, ("unknown create flags 0x104",)),
    ("oblivious", INVALID_ARG, ("tahoe_oblivious_forest_create_ex: flags 0x100: only",)),
    ("oblivious_with_contribs", INVALID_ARG, ("tahoe_oblivious_forest_create_ex: flags 0x104: only",)),
])
def test_refusals_come_before_the_device(results, case, status, texts):
    got, msg = results[case]
    assert got == status and got != NO_DEVICE, (got, msg)
    for text in texts:
        assert text in msg, msg
