"""tahoe_vector_forest_create_ex without a GPU: the symbol, its binding and header, the Python surface, and -- in a child process
that sees no device -- every refusal the TAHOE_CREATE_CONTRIBS flag adds, with its code and text (none may be
TAHOE_ERR_NO_DEVICE: all of them run before a device is touched), and creates that get as far as the device."""
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
    assert "tahoe_vector_forest_create_ex" in ta.capi.EXPORTED_SYMBOLS
    assert hasattr(ta.lib, "tahoe_vector_forest_create_ex")
    assert " tahoe_vector_forest_create_ex@@" in syms and " tahoe_vector_forest_create@@" in syms
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert "tahoe_status tahoe_vector_forest_create_ex(" in header
    decl = header[header.index("tahoe_status tahoe_vector_forest_create_ex("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl.endswith("const float *leaf_values, int64_t num_leaf_vectors, const float *covers, "
                         "const tahoe_forest_params *params, int leaf_dim, unsigned flags)")
    assert ta.lib.tahoe_abi_version() == 2


def test_python_surface(ta):
    import inspect

    sig = inspect.signature(ta.VectorForest.__init__)
    assert sig.parameters["covers"].default is None and sig.parameters["contribs"].default is False
    assert ta.VectorForest is ta.capi.VectorForest and hasattr(ta.VectorForest, "predict_contribs")
    nodes = np.zeros(3, ta.capi.SPARSE_NODE_DTYPE)
    with pytest.raises(ValueError):
        ta.VectorForest(nodes, [0], [[1.0, 2.0]], 2, covers=np.ones(2, np.float32), contribs=True)  # covers.size != nodes.size


CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import tahoe_amd as ta

LEAF = -(1 << 31)
CONTRIBS = ta.capi.CREATE_CONTRIBS

def create(nodes, trees, leaves, cols, covers, k=1, flags=CONTRIBS, null_covers=False):
    n = np.zeros(max(len(nodes), 1), ta.capi.SPARSE_NODE_DTYPE)
    for i, (val, bits, left) in enumerate(nodes):
        n[i] = (val, bits, left)
    trees = np.ascontiguousarray(trees, np.int32)
    leaves = np.ascontiguousarray(leaves, np.float32)
    covers = np.ascontiguousarray(covers, np.float32)
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

# a chain of 32 internal nodes on features 0 .. 31 (num_cols 40): node 3 i has children 3 i + 1 (a leaf) and 3 i + 2 ... laid
# out as: internal i at 2 i, its left leaf at 2 i + 1, the next internal at 2 i + 2
def chain(n):
    nodes = []
    for i in range(n):
        nodes += [(0.0, i, 2 * i + 1), (0.0, LEAF, 0)]
    return nodes + [(0.0, LEAF, 0)]

res = {}
res["unknown_flag"] = create(**good, flags=CONTRIBS | 0x10)
res["unknown_flag_alone"] = create(**good, flags=0x40)
res["null_covers"] = create(**good, null_covers=True)
res["nan_cover"] = create(**cover(7, float("nan")))
res["neg_cover"] = create(**cover(1, -1.0))
res["inf_cover"] = create(**cover(8, float("inf")))
res["both_zero"] = create(**cover(1, 0.0, 2, 0.0))
res["chain_32"] = create(chain(32), [0], [1.0, 2.0], 40, np.ones(65), k=2)
res["chain_31"] = create(chain(31), [0], [1.0, 2.0], 40, np.ones(63), k=2)
res["valid"] = create(**good)
res["valid_k1"] = create(**dict(good, leaves=np.arange(4.0), k=1))
res["valid_one_zero"] = create(**cover(1, 0.0))
res["valid_unreachable_garbage"] = create(**cover(0, float("nan"), 3, -7.0))  # root covers and a root leaf's are never read
res["plain_garbage_covers"] = create(**dict(good, covers=[float("nan"), -1.0, float("inf")] * 3), flags=0)
res["plain_null_covers"] = create(**good, flags=0, null_covers=True)
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def refusals(ta):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case,status,text", [
    ("unknown_flag", INVALID_ARG, "unknown create flags 0x10"),
    ("unknown_flag_alone", INVALID_ARG, "unknown create flags 0x40"),
    ("null_covers", INVALID_ARG, "TAHOE_CREATE_CONTRIBS needs covers"),
    ("nan_cover", INVALID_FOREST, "tree 2 node 2: child covers nan and 4"),
    ("neg_cover", INVALID_FOREST, "tree 0 node 0: child covers -1 and 3"),
    ("inf_cover", INVALID_FOREST, "tree 2 node 2: child covers 3 and inf"),
    ("both_zero", INVALID_FOREST, "tree 0 node 0: child covers 0 and 0"),
    ("chain_32", UNSUPPORTED, "tree 0: a leaf's path has 32 distinct features"),
])
def test_refusals_come_before_the_device(refusals, case, status, text):
    got, msg = refusals[case]
    assert got == status and got != NO_DEVICE, (got, msg)
    assert text in msg, msg


@pytest.mark.parametrize("case", ["valid", "valid_k1", "valid_one_zero", "valid_unreachable_garbage", "chain_31",
                                  "plain_garbage_covers", "plain_null_covers"])
def test_a_valid_create_reaches_the_device(refusals, case):
    got, msg = refusals[case]
    assert got == NO_DEVICE, (got, msg)
