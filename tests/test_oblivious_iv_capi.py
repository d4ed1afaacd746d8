"""TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL on tahoe_oblivious_forest_create_ex without a GPU: the flag's value in the header and the
binding, and in a child process that sees no device every refusal with its code and text (none may be TAHOE_ERR_NO_DEVICE: all
checks run before a device is touched) and the valid creates getting as far as the device.  The flag alone reads no cover; beside
TAHOE_CREATE_CONTRIBS, TAHOE_CREATE_APPROX_CONTRIBS or TAHOE_CREATE_INTERACTIONS those keep their cover checks."""
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


def test_flag_is_declared_and_bound_and_the_abi_version_stands(ta):
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert "#define TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL 0x200u" in header
    assert ta.capi.CREATE_OBLIVIOUS_INTERVENTIONAL == 0x200 and ta.CREATE_OBLIVIOUS_INTERVENTIONAL == 0x200
    assert ta.capi.CREATE_INTERVENTIONAL == 0x80
    assert ta.lib.tahoe_abi_version() == 2


def test_python_needs_covers_only_with_the_other_flags(ta):
    with pytest.raises(ValueError):
        ta.ObliviousForest([1], [0], [0.5], [0], [1.0, 2.0], 2, interventional=True, contribs=True)
    with pytest.raises(ValueError):
        ta.ObliviousForest([1], [0], [0.5], [0], [1.0, 2.0], 2, leaf_covers=[1.0, 2.0, 3.0], interventional=True, interactions=True)


CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import tahoe_amd as ta

def create(depths, fids, leaves, cols, covers=None, flags=0, k=1, output=0, null=(), ex=True):
    depths = np.ascontiguousarray(depths, np.int32)
    splits = np.zeros(max(len(fids), 1), ta.capi.OBLIVIOUS_SPLIT_DTYPE)
    splits["bits"][:len(fids)] = fids
    leaves = np.ascontiguousarray(leaves, np.float32)
    cv = None if covers is None else np.ascontiguousarray(covers, np.float32)
    params = ta.ForestParams(0, 0, len(depths), cols, 0, output, 0.5, 0.0, 0, -999.0)
    h = C.c_void_p()
    args = [None if "out" in null else C.byref(h), depths.ctypes.data, None if "splits" in null else splits.ctypes.data,
            None if "leaves" in null else leaves.ctypes.data]
    if ex:
        st = ta.lib.tahoe_oblivious_forest_create_ex(*args, None if cv is None else cv.ctypes.data, C.byref(params), k, flags)
    else:
        st = ta.lib.tahoe_oblivious_forest_create(*args, C.byref(params), k)
    assert not h.value
    return [st, ta.lib.tahoe_last_error().decode()]

IV = 0x200
INTER, CONTRIBS, APPROX = ta.capi.CREATE_INTERACTIONS, ta.capi.CREATE_CONTRIBS, ta.capi.CREATE_APPROX_CONTRIBS
good = dict(depths=[1, 0, 2], fids=[0, 1, 2], leaves=np.arange(7.0), cols=3)
ones = np.ones(7)
def bad(at, v):
    c = ones.copy(); c[at] = v; return c
res = {}
res["valid_alone_null_covers"] = create(**good, flags=IV)
res["valid_alone_bad_covers_ignored"] = create(**good, covers=bad(0, -1.0), flags=IV)
res["valid_alone_k2_avg"] = create(**dict(good, leaves=np.arange(14.0), k=2, output=1), flags=IV)
res["valid_no_trees"] = create([], [], [0.0], 3, flags=IV)
for name, other in (("contribs", CONTRIBS), ("approx", APPROX), ("inter", INTER)):
    res["valid_with_" + name] = create(**good, covers=ones, flags=IV | other)
    res["null_covers_with_" + name] = create(**good, flags=IV | other)
    res["negative_with_" + name] = create(**good, covers=bad(4, -0.5), flags=IV | other)
    res["nan_with_" + name] = create(**good, covers=bad(2, np.nan), flags=IV | other)
    res["inf_with_" + name] = create(**good, covers=bad(6, np.inf), flags=IV | other)
res["valid_all_four"] = create(**good, covers=ones, flags=IV | INTER | CONTRIBS | APPROX)
res["unknown_0x80"] = create(**good, covers=ones, flags=0x80)
res["unknown_0x201"] = create(**good, covers=ones, flags=0x201)
res["unknown_0x220"] = create(**good, covers=ones, flags=0x220)
res["unknown_0x280"] = create(**good, flags=0x280)
# the checks of tahoe_oblivious_forest_create come first, with their texts
res["old_null_leaves"] = create(**good, flags=0x201, null=("leaves",))
res["old_fid"] = create([1, 0, 2], [0, 1, 3], np.arange(7.0), 3, flags=IV)
res["old_depth"] = create([1, 17, 0], [0] * 18, np.zeros(8), 3, flags=IV)
res["old_leaf_dim"] = create(**good, flags=IV, k=0)
res["old_softmax_k1"] = create(**good, flags=IV, output=0x1000)
# tahoe_oblivious_forest_create as before
res["plain"] = create(**good, ex=False)
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def refusals(ta):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", ["valid_alone_null_covers", "valid_alone_bad_covers_ignored", "valid_alone_k2_avg", "valid_no_trees",
                                  "valid_with_contribs", "valid_with_approx", "valid_with_inter", "valid_all_four", "plain"])
def test_a_valid_create_reaches_the_device(refusals, case):
    got, msg = refusals[case]
    assert got == NO_DEVICE, (got, msg)


@pytest.mark.parametrize("other", ["contribs", "approx", "inter"])
@pytest.mark.parametrize("case,status,text", [
    ("null_covers_with_", INVALID_ARG, "leaf_covers is null"), ("negative_with_", INVALID_FOREST, "tree 2 leaf 1"),
    ("nan_with_", INVALID_FOREST, "tree 1 leaf 0"), ("inf_with_", INVALID_FOREST, "tree 2 leaf 3"),
])
def test_the_other_flags_keep_their_cover_checks(refusals, other, case, status, text):
    got, msg = refusals[case + other]
    assert got == status and got != NO_DEVICE, (got, msg)
    assert text in msg and "tahoe_oblivious_forest_create_ex" in msg, msg


@pytest.mark.parametrize("case,status,text", [
    ("unknown_0x80", INVALID_ARG, "flags 0x80"), ("unknown_0x201", INVALID_ARG, "flags 0x201"),
    ("unknown_0x220", INVALID_ARG, "flags 0x220"), ("unknown_0x280", INVALID_ARG, "flags 0x280"),
    ("old_null_leaves", INVALID_ARG, "tahoe_oblivious_forest_create: null argument"),
    ("old_fid", INVALID_FOREST, "tree 2 level 1: fid 3 >= num_cols 3"), ("old_depth", INVALID_ARG, "tree 1: depth 17"),
    ("old_leaf_dim", INVALID_ARG, "leaf_dim must be in [1,1024]"), ("old_softmax_k1", INVALID_ARG, ""),
])
def test_refusals_come_before_the_device(refusals, case, status, text):
    got, msg = refusals[case]
    assert got == status and got != NO_DEVICE, (got, msg)
    assert text in msg, msg
