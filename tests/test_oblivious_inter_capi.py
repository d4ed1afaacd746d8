"""TAHOE_CREATE_INTERACTIONS on tahoe_oblivious_forest_create_ex without a GPU: the flag's value in the header and the binding, and
in a child process that sees no device every refusal with its code and text (none may be TAHOE_ERR_NO_DEVICE: all checks run
before a device is touched) and the valid creates getting as far as the device."""
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
    assert "#define TAHOE_CREATE_INTERACTIONS 0x40u" in header
    assert ta.capi.CREATE_INTERACTIONS == 0x40 and ta.CREATE_INTERACTIONS == 0x40
    assert ta.lib.tahoe_abi_version() == 2


def test_python_needs_covers_with_the_flag(ta):
    with pytest.raises(ValueError):
        ta.ObliviousForest([1], [0], [0.5], [0], [1.0, 2.0], 2, interactions=True)
    with pytest.raises(ValueError):
        ta.ObliviousForest([1], [0], [0.5], [0], [1.0, 2.0], 2, leaf_covers=[1.0, 2.0, 3.0], interactions=True)


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

INTER, CONTRIBS, APPROX = ta.capi.CREATE_INTERACTIONS, ta.capi.CREATE_CONTRIBS, ta.capi.CREATE_APPROX_CONTRIBS
good = dict(depths=[1, 0, 2], fids=[0, 1, 2], leaves=np.arange(7.0), cols=3)
ones = np.ones(7)
def bad(at, v):
    c = ones.copy(); c[at] = v; return c
res = {}
res["valid_inter"] = create(**good, covers=ones, flags=INTER)
res["valid_all_three"] = create(**good, covers=ones, flags=INTER | CONTRIBS | APPROX)
res["valid_inter_contribs"] = create(**good, covers=ones, flags=INTER | CONTRIBS)
res["valid_zero_covers_k2"] = create(**dict(good, leaves=np.arange(14.0), k=2), covers=np.zeros(7), flags=INTER)
res["null_covers"] = create(**good, flags=INTER)
res["unknown_0x80"] = create(**good, covers=ones, flags=0x80)
res["unknown_0x41"] = create(**good, covers=ones, flags=0x41)
res["unknown_0x60"] = create(**good, covers=ones, flags=0x60)
res["negative"] = create(**good, covers=bad(4, -0.5), flags=INTER)
res["nan"] = create(**good, covers=bad(2, np.nan), flags=INTER)
res["inf"] = create(**good, covers=bad(6, np.inf), flags=INTER | CONTRIBS)
# the checks of tahoe_oblivious_forest_create come first, with their texts
res["old_null_leaves"] = create(**good, flags=0x80, null=("leaves",))
res["old_fid"] = create([1, 0, 2], [0, 1, 3], np.arange(7.0), 3, covers=bad(0, -1.0), flags=INTER)
res["old_depth"] = create([1, 17, 0], [0] * 18, np.zeros(8), 3, flags=INTER)
# tahoe_oblivious_forest_create as before
res["plain"] = create(**good, ex=False)
res["plain_fid"] = create([1, 0, 2], [0, 1, 3], np.arange(7.0), 3, ex=False)
res["flags0_bad_covers_ignored"] = create(**good, covers=bad(0, -1.0))
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def refusals(ta):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", ["valid_inter", "valid_all_three", "valid_inter_contribs", "valid_zero_covers_k2", "plain",
                                  "flags0_bad_covers_ignored"])
def test_a_valid_create_reaches_the_device(refusals, case):
    got, msg = refusals[case]
    assert got == NO_DEVICE, (got, msg)


@pytest.mark.parametrize("case,status,text", [
    ("null_covers", INVALID_ARG, "leaf_covers is null"),
    ("unknown_0x80", INVALID_ARG, "flags 0x80"), ("unknown_0x41", INVALID_ARG, "flags 0x41"), ("unknown_0x60", INVALID_ARG, "flags 0x60"),
    ("negative", INVALID_FOREST, "tree 2 leaf 1"), ("nan", INVALID_FOREST, "tree 1 leaf 0"), ("inf", INVALID_FOREST, "tree 2 leaf 3"),
    ("old_null_leaves", INVALID_ARG, "tahoe_oblivious_forest_create: null argument"),
    ("old_fid", INVALID_FOREST, "tree 2 level 1: fid 3 >= num_cols 3"), ("old_depth", INVALID_ARG, "tree 1: depth 17"),
    ("plain_fid", INVALID_FOREST, "tree 2 level 1: fid 3 >= num_cols 3"),
])
def test_refusals_come_before_the_device(refusals, case, status, text):
    got, msg = refusals[case]
    assert got == status and got != NO_DEVICE, (got, msg)
    assert text in msg, msg
