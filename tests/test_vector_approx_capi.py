"""TAHOE_CREATE_VECTOR_APPROX without a GPU: the flag's value, binding and header text, the Python surface, and -- in a child
process that sees no device -- every refusal the flag adds to tahoe_vector_forest_create_ex, with its code and text (none may be
TAHOE_ERR_NO_DEVICE: all of them run before a device is touched), the flag on every other create function, and creates that get
as far as the device."""
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


def test_flag_header_and_python_surface(ta):
    import inspect

    assert ta.capi.CREATE_VECTOR_APPROX == 0x400
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert "#define TAHOE_CREATE_VECTOR_APPROX 0x400u" in header
    assert "unless the handle comes from _create_ex with TAHOE_CREATE_VECTOR_APPROX" in " ".join(header.split()).replace(" * ", " ")
    sig = inspect.signature(ta.VectorForest.__init__)
    assert sig.parameters["approx_contribs"].default is False
    assert "approx_contribs" in ta.VectorForest.__doc__
    nodes = np.zeros(3, ta.capi.SPARSE_NODE_DTYPE)
    with pytest.raises(ValueError):
        ta.VectorForest(nodes, [0], [[1.0, 2.0]], 2, covers=np.ones(2, np.float32), approx_contribs=True)  # covers.size != nodes.size
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    assert "vector_approx" not in syms and "vector_predict_approx" not in syms  # no new exported symbol


CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import tahoe_amd as ta

LEAF = -(1 << 31)
APPROX = ta.capi.CREATE_VECTOR_APPROX
CONTRIBS, IV, INTER = ta.capi.CREATE_CONTRIBS, ta.capi.CREATE_INTERVENTIONAL, ta.capi.CREATE_VECTOR_INTERACTIONS

def arrays(nodes, trees, leaves, covers):
    n = np.zeros(max(len(nodes), 1), ta.capi.SPARSE_NODE_DTYPE)
    for i, (val, bits, left) in enumerate(nodes):
        n[i] = (val, bits, left)
    return n, np.ascontiguousarray(trees, np.int32), np.ascontiguousarray(leaves, np.float32), np.ascontiguousarray(covers, np.float32)

def create(nodes, trees, leaves, cols, covers, k=1, flags=APPROX, null_covers=False):
    n, trees, leaves, covers = arrays(nodes, trees, leaves, covers)
    params = ta.ForestParams(len(nodes), 0, len(trees), cols, 0, 0, 0.5, 0.0, 0, -999.0)
    h = C.c_void_p()
    st = ta.lib.tahoe_vector_forest_create_ex(C.byref(h), trees.ctypes.data, n.ctypes.data, leaves.ctypes.data, leaves.size // k,
                                              None if null_covers else covers.ctypes.data, C.byref(params), k, flags)
    assert not h.value
    return [st, ta.lib.tahoe_last_error().decode()]

# tree 0: a stump on feature 1; tree 1: a single leaf; tree 2: x0, then x2 on the right
NODES = [(0.5, 1 | 1 << 30, 1), (0.0, LEAF, 3), (0.0, LEAF, 0),
         (0.0, LEAF, 2),
         (0.0, 0, 1), (0.0, LEAF, 1), (1.0, 2, 3), (0.0, LEAF, 3), (0.0, LEAF, 0)]
COVERS = [4.0, 1.0, 3.0, 5.0, 9.0, 2.0, 7.0, 3.0, 4.0]
good = dict(nodes=NODES, trees=[0, 3, 4], leaves=np.arange(8.0), cols=3, covers=COVERS, k=2)

def cover(i, v, j=None, w=None):
    c = list(COVERS)
    c[i] = v
    if j is not None:
        c[j] = w
    return dict(good, covers=c)

# a vine of n internal nodes on features 0 .. n - 1: internal i at 2 i, its left leaf at 2 i + 1, the next internal at 2 i + 2
def vine(n):
    nodes = []
    for i in range(n):
        nodes += [(0.0, i, 2 * i + 1), (0.0, LEAF, 0)]
    return nodes + [(0.0, LEAF, 0)]

res = {}
res["null_covers"] = create(**good, null_covers=True)
res["null_covers_with_contribs"] = create(**good, flags=APPROX | CONTRIBS, null_covers=True)
res["null_covers_with_interventional"] = create(**good, flags=APPROX | IV, null_covers=True)
res["nan_cover"] = create(**cover(7, float("nan")))
res["neg_cover"] = create(**cover(1, -1.0))
res["inf_cover"] = create(**cover(8, float("inf")))
res["both_zero"] = create(**cover(1, 0.0, 2, 0.0))
res["neg_cover_with_interventional"] = create(**cover(1, -1.0), flags=APPROX | IV)
res["unknown_beside"] = create(**good, flags=APPROX | 0x10)
res["unknown_beside_200"] = create(**good, flags=APPROX | 0x200)
res["unknown_beside_800"] = create(**good, flags=APPROX | CONTRIBS | 0x800)
res["interactions_without_contribs"] = create(**good, flags=APPROX | INTER)
res["vine_40_alone"] = create(vine(40), [0], [1.0, 2.0], 40, np.ones(81), k=2)
res["vine_40_with_contribs"] = create(vine(40), [0], [1.0, 2.0], 40, np.ones(81), k=2, flags=APPROX | CONTRIBS)
res["vine_40_with_interventional"] = create(vine(40), [0], [1.0, 2.0], 40, np.ones(81), k=2, flags=APPROX | IV)
res["valid"] = create(**good)
res["valid_k1"] = create(**dict(good, leaves=np.arange(4.0), k=1))
res["valid_one_zero"] = create(**cover(1, 0.0))
res["valid_unreachable_garbage"] = create(**cover(0, float("nan"), 3, -7.0))  # root covers and a root leaf's are never read
for name, fl in (("contribs", CONTRIBS), ("interventional", IV), ("all", CONTRIBS | IV | INTER)):
    res["valid_with_" + name] = create(**good, flags=APPROX | fl)

# the flag on every other create function
n, trees, leaves, covers = arrays(NODES, [0, 3, 4], np.arange(8.0), COVERS)
sn = n.copy()
sn["left_idx"][n["bits"] < 0] = 0
sp = ta.ForestParams(len(NODES), 0, 3, 3, 0, 0, 0.5, 0.0, 0, -999.0)
h = C.c_void_p()
st = ta.lib.tahoe_sparse_forest_create_ex(C.byref(h), trees.ctypes.data, sn.ctypes.data, covers.ctypes.data, C.byref(sp), 1, APPROX)
res["other:sparse_ex"] = [st, ta.lib.tahoe_last_error().decode()]
heap = ta.synth_forest(2, 2, 3, seed=1)
dp = ta.ForestParams(int(heap.size), 2, 2, 3, 0, 0, 0.5, 0.0, 0, -999.0)
st = ta.lib.tahoe_forest_create_ex(C.byref(h), heap.ctypes.data, C.byref(dp), APPROX)
res["other:dense_ex"] = [st, ta.lib.tahoe_last_error().decode()]
st = ta.lib.tahoe_forest_create_multiclass(C.byref(h), heap.ctypes.data, C.byref(dp), 2, APPROX)
res["other:multiclass"] = [st, ta.lib.tahoe_last_error().decode()]
st = ta.lib.tahoe_sparse_forest_create_cat(C.byref(h), trees.ctypes.data, sn.ctypes.data, covers.ctypes.data, C.byref(sp), 1, APPROX, None)
res["other:sparse_cat"] = [st, ta.lib.tahoe_last_error().decode()]
depths = np.array([1], np.int32)
splits = np.zeros(1, ta.capi.OBLIVIOUS_SPLIT_DTYPE)
op = ta.ForestParams(0, 0, 1, 3, 0, 0, 0.5, 0.0, 0, -999.0)
lv = np.arange(2, dtype=np.float32)
w = np.ones(2, np.float32)
st = ta.lib.tahoe_oblivious_forest_create_ex(C.byref(h), depths.ctypes.data, splits.ctypes.data, lv.ctypes.data, w.ctypes.data,
                                             C.byref(op), 1, APPROX)
res["other:oblivious_ex"] = [st, ta.lib.tahoe_last_error().decode()]
assert not h.value
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def refusals(ta):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case,status,text", [
    ("null_covers", INVALID_ARG, "TAHOE_CREATE_VECTOR_APPROX needs covers"),
    ("null_covers_with_contribs", INVALID_ARG, "needs covers"),
    ("null_covers_with_interventional", INVALID_ARG, "TAHOE_CREATE_VECTOR_APPROX needs covers"),
    ("nan_cover", INVALID_FOREST, "tree 2 node 2: child covers nan and 4"),
    ("neg_cover", INVALID_FOREST, "tree 0 node 0: child covers -1 and 3"),
    ("inf_cover", INVALID_FOREST, "tree 2 node 2: child covers 3 and inf"),
    ("both_zero", INVALID_FOREST, "tree 0 node 0: child covers 0 and 0"),
    ("neg_cover_with_interventional", INVALID_FOREST, "tree 0 node 0: child covers -1 and 3"),
    ("unknown_beside", INVALID_ARG, "unknown create flags 0x10"),
    ("unknown_beside_200", INVALID_ARG, "unknown create flags 0x200"),
    ("unknown_beside_800", INVALID_ARG, "unknown create flags 0x800"),
    ("interactions_without_contribs", INVALID_ARG, "TAHOE_CREATE_VECTOR_INTERACTIONS needs TAHOE_CREATE_CONTRIBS"),
    ("vine_40_with_contribs", UNSUPPORTED, "tree 0: a leaf's path has 32 distinct features"),
    ("vine_40_with_interventional", UNSUPPORTED, "tree 0: a leaf's path has 32 distinct features"),
])
def test_refusals_come_before_the_device(refusals, case, status, text):
    got, msg = refusals[case]
    assert got == status and got != NO_DEVICE, (got, msg)
    assert text in msg, msg


def test_the_unknown_flag_text_lists_the_new_flag(refusals):
    assert "TAHOE_CREATE_VECTOR_APPROX" in refusals["unknown_beside"][1]


@pytest.mark.parametrize("case", ["valid", "valid_k1", "valid_one_zero", "valid_unreachable_garbage", "vine_40_alone",
                                  "valid_with_contribs", "valid_with_interventional", "valid_with_all"])
def test_a_valid_create_reaches_the_device(refusals, case):
    got, msg = refusals[case]
    assert got == NO_DEVICE, (got, msg)


def test_every_other_create_refuses_the_flag(refusals):
    others = {k: v for k, v in refusals.items() if k.startswith("other:")}
    assert len(others) == 5
    for name, (got, msg) in others.items():
        assert got == INVALID_ARG, (name, got, msg)
        assert "0x400" in msg, (name, msg)
