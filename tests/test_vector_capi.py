"""tahoe_vector_forest_create without a GPU: the symbol, its binding and header, the Python class, and -- in a child process that
sees no device -- every argument refusal with its code and text (none may be TAHOE_ERR_NO_DEVICE: all checks run before a device
is touched) and valid creates that get as far as the device."""
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
    assert "tahoe_vector_forest_create" in ta.capi.EXPORTED_SYMBOLS
    assert hasattr(ta.lib, "tahoe_vector_forest_create")
    assert " tahoe_vector_forest_create" in syms
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert "tahoe_status tahoe_vector_forest_create(" in header
    assert "TAHOE_VECTOR_FORM_DIRECT = 27" in header and "TAHOE_VECTOR_FORM_TILE = 28" in header
    assert ta.lib.tahoe_abi_version() == 2


def test_kernel_form_names(ta):
    assert ta.lib.tahoe_kernel_form_name(27) == b"vector_direct" and ta.lib.tahoe_kernel_form_name(28) == b"vector_tile"
    assert ta.lib.tahoe_kernel_form_name(26) == b"?" and ta.lib.tahoe_kernel_form_name(23) == b"?"  # both stay unassigned
    assert ta.lib.tahoe_kernel_form_name(29) == b"?"
    assert ta.lib.tahoe_kernel_form_name(24) == b"oblivious_direct" and ta.lib.tahoe_kernel_form_name(25) == b"oblivious_tile"


def test_python_surface(ta):
    assert issubclass(ta.VectorForest, ta.Forest) and ta.VectorForest is ta.capi.VectorForest
    nodes = np.zeros(1, ta.capi.SPARSE_NODE_DTYPE)
    with pytest.raises(ValueError):
        ta.VectorForest(nodes, [0], [1.0, 2.0, 3.0], 2)  # flat leaf values without leaf_dim
    with pytest.raises(ValueError):
        ta.VectorForest(nodes, [0], [1.0, 2.0, 3.0], 2, leaf_dim=2)  # three values are no whole number of 2-vectors
    with pytest.raises(ValueError):
        ta.VectorForest(nodes, [0], [[1.0, 2.0, 3.0]], 2, leaf_dim=2)  # [L, 3] against leaf_dim = 2
    with pytest.raises(ValueError):
        ta.VectorForest(nodes, [0], np.zeros((1, 2, 2)), 2, leaf_dim=2)


CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import tahoe_amd as ta

LEAF = -(1 << 31)

def create(nodes, trees, leaves, cols, k=1, output=0, num_trees=None, num_nodes=None, num_vectors=None, null=()):
    n = np.zeros(max(len(nodes), 1), ta.capi.SPARSE_NODE_DTYPE)
    for i, (val, bits, left) in enumerate(nodes):
        n[i] = (val, bits, left)
    trees = np.ascontiguousarray(trees, np.int32)
    leaves = np.ascontiguousarray(leaves, np.float32)
    params = ta.ForestParams(len(nodes) if num_nodes is None else num_nodes, 0, len(trees) if num_trees is None else num_trees,
                             cols, 0, output, 0.5, 0.0, 0, -999.0)
    h = C.c_void_p()
    st = ta.lib.tahoe_vector_forest_create(None if "out" in null else C.byref(h), None if "trees" in null else trees.ctypes.data,
                                           None if "nodes" in null else n.ctypes.data,
                                           None if "leaves" in null else leaves.ctypes.data,
                                           leaves.size // max(k, 1) if num_vectors is None else num_vectors,
                                           None if "params" in null else C.byref(params), k)
    assert not h.value
    return [st, ta.lib.tahoe_last_error().decode()]

# tree 0: a stump on feature 1 (default left); tree 1: a single leaf; tree 2: x0, then x2 on the right
NODES = [(0.5, 1 | 1 << 30, 1), (0.0, LEAF, 3), (0.0, LEAF, 0),
         (0.0, LEAF, 2),
         (0.0, 0, 1), (0.0, LEAF, 1), (1.0, 2, 3), (0.0, LEAF, 3), (0.0, LEAF, 0)]
good = dict(nodes=NODES, trees=[0, 3, 4], leaves=np.arange(4.0), cols=3)
two = dict(good, leaves=np.arange(8.0), k=2)

def edit(i, node):
    return dict(good, nodes=NODES[:i] + [node] + NODES[i + 1:])

res = {}
for n in ("out", "params", "trees", "nodes", "leaves"):
    res["null_" + n] = create(**good, null=(n,))
res["null_arrays_no_trees"] = create([], [], [], 3, null=("trees", "nodes", "leaves"))
res["neg_trees"] = create(**good, num_trees=-1)
res["neg_nodes"] = create(**good, num_nodes=-1)
res["neg_vectors"] = create(**good, num_vectors=-1)
res["leaf_dim_0"] = create(**dict(good, k=0))
res["leaf_dim_1025"] = create(**dict(good, k=1025))
res["softmax_k1"] = create(**good, output=ta.OUT_SOFTMAX)
res["softmax_sigmoid"] = create(**two, output=ta.OUT_SOFTMAX | ta.OUT_SIGMOID)
res["threshold_k2"] = create(**two, output=ta.OUT_THRESHOLD)
res["unknown_output"] = create(**good, output=0x2)
res["neg_cols"] = create(**dict(good, cols=-1))
res["roots_descend"] = create(**dict(good, trees=[0, 4, 3]))
res["root_past_end"] = create(**dict(good, trees=[0, 3, 10]))
res["child_backwards"] = create(**edit(6, (1.0, 2, 2)))
res["child_self"] = create(**edit(4, (0.0, 0, 0)))
res["child_outside"] = create(**edit(6, (1.0, 2, 4)))
res["fid"] = create(**edit(6, (1.0, 3, 3)))
res["leaf_vector_high"] = create(**edit(7, (0.0, LEAF, 4)))
res["leaf_vector_neg"] = create(**edit(3, (0.0, LEAF, -1)))
res["leaf_vector_k2"] = create(**dict(two, num_vectors=3))  # the leaves name vectors 0 .. 3
res["leaf_no_vectors"] = create(**dict(good, leaves=[], null=("leaves",)))
res["valid"] = create(**good)
res["valid_k2_softmax"] = create(**two, output=ta.OUT_SOFTMAX)
res["valid_odd_trees_k2"] = create(**two)  # 3 trees, 2 outputs: no multiple-of-classes rule
res["valid_k1024"] = create(**dict(good, leaves=np.zeros(4 * 1024), k=1024))
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def refusals(ta):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case,status,text", [
    ("null_out", INVALID_ARG, "null argument"), ("null_params", INVALID_ARG, "null argument"),
    ("null_trees", INVALID_ARG, "trees / nodes is null"), ("null_nodes", INVALID_ARG, "trees / nodes is null"),
    ("null_leaves", INVALID_ARG, "leaf_values is null"),
    ("neg_trees", INVALID_ARG, "num_trees"), ("neg_nodes", INVALID_ARG, "num_nodes"),
    ("neg_vectors", INVALID_ARG, "num_leaf_vectors must be non-negative, got -1"),
    ("leaf_dim_0", INVALID_ARG, "leaf_dim must be in [1,1024], got 0"), ("leaf_dim_1025", INVALID_ARG, "leaf_dim must be in [1,1024], got 1025"),
    ("softmax_k1", INVALID_ARG, ""), ("softmax_sigmoid", INVALID_ARG, "SOFTMAX and SIGMOID"),
    ("threshold_k2", INVALID_ARG, "THRESHOLD needs"), ("unknown_output", INVALID_ARG, "output should be"),
    ("neg_cols", INVALID_ARG, "num_cols"),
    ("roots_descend", INVALID_FOREST, "tree 1: root offsets must be ascending"),
    ("root_past_end", INVALID_FOREST, "tree 1: root offsets must be ascending"),
    ("child_backwards", INVALID_FOREST, "tree 2 node 2: children 2, 3 are not after the node"),
    ("child_self", INVALID_FOREST, "tree 2 node 0: children 0, 1 are not after the node"),
    ("child_outside", INVALID_FOREST, "tree 2 node 2: children 4, 5 are not after the node and inside the tree"),
    ("fid", INVALID_FOREST, "tree 2 node 2: fid 3 >= num_cols 3"),
    ("leaf_vector_high", INVALID_FOREST, "tree 2 node 3: leaf vector 4 is outside [0, 4)"),
    ("leaf_vector_neg", INVALID_FOREST, "tree 1 node 0: leaf vector -1 is outside [0, 4)"),
    ("leaf_vector_k2", INVALID_FOREST, "tree 0 node 1: leaf vector 3 is outside [0, 3)"),
    ("leaf_no_vectors", INVALID_FOREST, "tree 0 node 1: leaf vector 3 is outside [0, 0)"),
])
def test_refusals_come_before_the_device(refusals, case, status, text):
    got, msg = refusals[case]
    assert got == status and got != NO_DEVICE, (got, msg)
    assert text in msg, msg


@pytest.mark.parametrize("case", ["valid", "valid_k2_softmax", "valid_odd_trees_k2", "valid_k1024", "null_arrays_no_trees"])
def test_a_valid_create_reaches_the_device(refusals, case):
    got, msg = refusals[case]
    assert got == NO_DEVICE, (got, msg)
