"""tahoe_oblivious_forest_create_cat without a GPU: the symbol, its binding and header, the Python class, and -- in a child process
that sees no device -- every argument refusal with its code and text (none may be TAHOE_ERR_NO_DEVICE: all checks run before a
device is touched), in the header's order, and valid creates that get as far as the device."""
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


def test_symbol_is_exported_bound_and_declared(ta):
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    assert "tahoe_oblivious_forest_create_cat" in ta.capi.EXPORTED_SYMBOLS
    assert hasattr(ta.lib, "tahoe_oblivious_forest_create_cat")
    assert " tahoe_oblivious_forest_create_cat" in syms
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert "tahoe_status tahoe_oblivious_forest_create_cat(" in header
    assert "one-hot and CTR splits are not" not in header
    assert ta.lib.tahoe_abi_version() == 2


def test_python_surface(ta):
    import inspect

    sig = inspect.signature(ta.ObliviousForest.__init__)
    assert sig.parameters["categories"].default is None and sig.parameters["members_left"].default == ()
    with pytest.raises(ValueError):  # pack_categorical's checks reach the caller before the library is called
        ta.ObliviousForest([1], [0], [0.5], [0], [1.0, 2.0], 2, categories={0: [1 << 24]})
    with pytest.raises(ValueError):
        ta.ObliviousForest([1], [0], [0.5], [0], [1.0, 2.0], 2, categories={0: [1]}, members_left=[3])


CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import tahoe_amd as ta

def create(depths, fids, leaves, cols, k=1, flags=0, covers=None, cats=None, null=(), node=None, offset=None, nsplits=None,
           ml=None, null_cats=()):
    depths = np.ascontiguousarray(depths, np.int32)
    splits = np.zeros(max(len(fids), 1), ta.capi.OBLIVIOUS_SPLIT_DTYPE)
    splits["bits"][:len(fids)] = fids
    leaves = np.ascontiguousarray(leaves, np.float32)
    cv = None if covers is None else np.ascontiguousarray(covers, np.float32)
    params = ta.ForestParams(0, 0, len(depths), cols, 0, 0, 0.5, 0.0, 0, -999.0)
    cs = None
    if cats is not None:
        cs, keep = ta.capi.pack_categorical(cats, ml or ())
        if node is not None:
            node = np.ascontiguousarray(node, np.int32)
            cs.node = node.ctypes.data
        if offset is not None:
            offset = np.ascontiguousarray(offset, np.int32)
            cs.offset = offset.ctypes.data
        if nsplits is not None:
            cs.num_splits = nsplits
        for name in null_cats:
            setattr(cs, name, None)
    h = C.c_void_p()
    st = ta.lib.tahoe_oblivious_forest_create_cat(None if "out" in null else C.byref(h), depths.ctypes.data, splits.ctypes.data,
                                                  leaves.ctypes.data, None if cv is None else cv.ctypes.data, C.byref(params), k,
                                                  flags, None if cs is None else C.byref(cs))
    assert not h.value
    return [st, ta.lib.tahoe_last_error().decode()]

good = dict(depths=[1, 0, 2], fids=[0, 1, 2], leaves=np.arange(7.0), cols=3)
sets = {0: [1, 2], 2: [40]}
res = {}
# the checks of tahoe_oblivious_forest_create_ex come first, with its texts, sets or not
res["null_out"] = create(**good, cats=sets, null=("out",))
res["leaf_dim_0"] = create(**dict(good, k=0), cats=sets)
res["depth_17"] = create([1, 17, 0], [0] * 18, np.zeros(8), 3, cats={0: [1]})
res["fid"] = create([1, 0, 2], [0, 1, 3], np.arange(7.0), 3, cats=sets)
res["flag_cat_contribs"] = create(**good, cats=sets, flags=ta.capi.CREATE_CAT_CONTRIBS | ta.capi.CREATE_CONTRIBS, covers=np.ones(7))
res["flag_unknown"] = create(**good, cats=sets, flags=0x80)
res["covers_null"] = create(**good, cats=sets, flags=ta.capi.CREATE_CONTRIBS)
res["cover_negative"] = create(**good, cats=sets, flags=ta.capi.CREATE_APPROX_CONTRIBS, covers=[1, 1, 1, 1, -1, 1, 1])
# ... before those of cats: a bad cover is reported although num_splits is bad too
res["cover_before_cats"] = create(**good, cats=sets, nsplits=-1, flags=ta.capi.CREATE_CONTRIBS, covers=[1, 1, 1, 1, -1, 1, 1])
# the cats checks of tahoe_sparse_forest_create_cat, bounded by the sum of the depths (3)
res["nsplits_negative"] = create(**good, cats=sets, nsplits=-1)
res["nsplits_above"] = create(**good, cats={0: [1], 1: [1], 2: [1]}, nsplits=4)
for name in ("node", "offset", "words"):
    res["null_" + name] = create(**good, cats=sets, null_cats=(name,))
res["node_outside"] = create(**good, cats=sets, node=[0, 3])
res["node_negative"] = create(**good, cats=sets, node=[-1, 2])
res["node_order"] = create(**good, cats=sets, node=[2, 0])
res["node_twice"] = create(**good, cats=sets, node=[2, 2])
res["offset0"] = create(**good, cats=sets, offset=[1, 2, 3])
res["offset_decreases"] = create(**good, cats=sets, offset=[0, 2, 1])
res["too_wide"] = create(**good, cats=sets, offset=[0, 1, (1 << 19) + 2])
# then the limit the split record leaves for fid
res["cols_above"] = create(**dict(good, cols=(1 << 28) + 1), cats=sets)
res["cols_above_but_cats_bad"] = create(**dict(good, cols=(1 << 28) + 1), cats=sets, node=[2, 0])
# valid creates reach the device
res["valid"] = create(**good, cats=sets, ml=[2])
res["valid_cols_at_limit"] = create(**dict(good, cols=1 << 28), cats=sets)
res["valid_cols_above_without_splits"] = create(**dict(good, cols=(1 << 28) + 1), cats={})
res["valid_cols_above_null"] = create(**dict(good, cols=(1 << 28) + 1))
res["valid_flags"] = create(**good, cats=sets, covers=np.ones(7),
                            flags=ta.capi.CREATE_CONTRIBS | ta.capi.CREATE_APPROX_CONTRIBS | ta.capi.CREATE_INTERACTIONS
                            | ta.capi.CREATE_OBLIVIOUS_INTERVENTIONAL)
res["valid_nsplits0_bad_rest"] = create(**good, cats=sets, nsplits=0, null_cats=("node", "offset", "words"))
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def refusals(ta):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case,status,text", [
    ("null_out", INVALID_ARG, "null argument"), ("leaf_dim_0", INVALID_ARG, "leaf_dim must be in [1,1024], got 0"),
    ("depth_17", INVALID_ARG, "tree 1: depth 17"), ("fid", INVALID_FOREST, "tree 2 level 1: fid 3 >= num_cols 3"),
    ("flag_cat_contribs", INVALID_ARG, "flags 0x24"), ("flag_unknown", INVALID_ARG, "flags 0x80"),
    ("covers_null", INVALID_ARG, "leaf_covers is null"), ("cover_negative", INVALID_FOREST, "tree 2 leaf 1: cover -1"),
    ("cover_before_cats", INVALID_FOREST, "tree 2 leaf 1: cover -1"),
    ("nsplits_negative", INVALID_ARG, "categorical splits: num_splits -1 is not in [0, num_nodes = 3]"),
    ("nsplits_above", INVALID_ARG, "categorical splits: num_splits 4 is not in [0, num_nodes = 3]"),
    ("null_node", INVALID_ARG, "node, offset and words must not be NULL"),
    ("null_offset", INVALID_ARG, "node, offset and words must not be NULL"),
    ("null_words", INVALID_ARG, "node, offset and words must not be NULL"),
    ("node_outside", INVALID_ARG, "node[1] = 3 is outside [0, num_nodes = 3)"),
    ("node_negative", INVALID_ARG, "node[0] = -1 is outside [0, num_nodes = 3)"),
    ("node_order", INVALID_ARG, "node[] must be strictly ascending (node[1] = 0 after 2)"),
    ("node_twice", INVALID_ARG, "node[] must be strictly ascending (node[1] = 2 after 2)"),
    ("offset0", INVALID_ARG, "offset[0] = 1, must be 0"), ("offset_decreases", INVALID_ARG, "offset[2] = 1 decreases from 2"),
    ("too_wide", INVALID_ARG, "split 1 has 524289 words, more than 2^19"),
    ("cols_above", UNSUPPORTED, "num_cols <= 2^28"), ("cols_above_but_cats_bad", INVALID_ARG, "strictly ascending"),
])
def test_refusals_come_before_the_device_in_order(refusals, case, status, text):
    got, msg = refusals[case]
    assert got == status and got != NO_DEVICE, (got, msg)
    assert text in msg, msg


@pytest.mark.parametrize("case", ["valid", "valid_cols_at_limit", "valid_cols_above_without_splits", "valid_cols_above_null",
                                  "valid_flags", "valid_nsplits0_bad_rest"])
def test_a_valid_create_reaches_the_device(refusals, case):
    got, msg = refusals[case]
    assert got == NO_DEVICE, (got, msg)
