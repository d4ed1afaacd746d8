"""tahoe_oblivious_forest_create_ex without a GPU: the symbol, its binding and header; in a child process that sees no device
every refusal with its code and text (none may be TAHOE_ERR_NO_DEVICE: all checks run before a device is touched), flags == 0 and
valid flagged creates getting as far as the device; and tests/oblivious_shap_ref.py against itself and the project's other
references.  Covers in every cross-check with the heap expansion are positive integers <= 2^10: their subtree sums are exact in
float32, so the dense definitions see the same node covers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_contribs_ref  # noqa: E402
import contribs_ref  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, NO_DEVICE, INVALID_FOREST, UNSUPPORTED = 0, 1, 4, 6, 7


@pytest.fixture(scope="module")
def ta(built):
    import tahoe_amd

    return tahoe_amd


def test_symbol_is_exported_bound_and_declared(ta):
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    assert "tahoe_oblivious_forest_create_ex" in ta.capi.EXPORTED_SYMBOLS
    assert hasattr(ta.lib, "tahoe_oblivious_forest_create_ex")
    assert " tahoe_oblivious_forest_create_ex@@" in syms and " tahoe_oblivious_forest_create@@" in syms
    header = open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()
    assert "tahoe_status tahoe_oblivious_forest_create_ex(" in header and "const float *leaf_covers" in header
    assert ta.lib.tahoe_abi_version() == 2


def test_python_needs_covers_with_a_flag(ta):
    for kw in (dict(contribs=True), dict(approx_contribs=True)):
        with pytest.raises(ValueError):
            ta.ObliviousForest([1], [0], [0.5], [0], [1.0, 2.0], 2, **kw)
    with pytest.raises(ValueError):
        ta.ObliviousForest([1], [0], [0.5], [0], [1.0, 2.0], 2, leaf_covers=[1.0, 2.0, 3.0], contribs=True)


CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import tahoe_amd as ta

def create(depths, fids, leaves, cols, covers=None, flags=0, k=1, output=0, null=()):
    depths = np.ascontiguousarray(depths, np.int32)
    splits = np.zeros(max(len(fids), 1), ta.capi.OBLIVIOUS_SPLIT_DTYPE)
    splits["bits"][:len(fids)] = fids
    leaves = np.ascontiguousarray(leaves, np.float32)
    cv = None if covers is None else np.ascontiguousarray(covers, np.float32)
    params = ta.ForestParams(0, 0, len(depths), cols, 0, output, 0.5, 0.0, 0, -999.0)
    h = C.c_void_p()
    st = ta.lib.tahoe_oblivious_forest_create_ex(None if "out" in null else C.byref(h), depths.ctypes.data,
                                                 None if "splits" in null else splits.ctypes.data,
                                                 None if "leaves" in null else leaves.ctypes.data,
                                                 None if cv is None else cv.ctypes.data, C.byref(params), k, flags)
    assert not h.value
    return [st, ta.lib.tahoe_last_error().decode()]

CONTRIBS, APPROX = ta.capi.CREATE_CONTRIBS, ta.capi.CREATE_APPROX_CONTRIBS
good = dict(depths=[1, 0, 2], fids=[0, 1, 2], leaves=np.arange(7.0), cols=3)
ones = np.ones(7)
def bad(at, v):
    c = ones.copy(); c[at] = v; return c
res = {}
res["flags0_no_covers"] = create(**good)
res["flags0_bad_covers_ignored"] = create(**good, covers=bad(0, -1.0))
res["unknown_bit_1"] = create(**good, covers=ones, flags=0x1)
res["unknown_bit_cat"] = create(**good, covers=ones, flags=CONTRIBS | 0x20)
res["null_covers_contribs"] = create(**good, flags=CONTRIBS)
res["null_covers_approx"] = create(**good, flags=APPROX)
res["negative"] = create(**good, covers=bad(4, -0.5), flags=CONTRIBS)
res["nan"] = create(**good, covers=bad(2, np.nan), flags=APPROX)
res["inf"] = create(**good, covers=bad(6, np.inf), flags=CONTRIBS | APPROX)
# the checks of tahoe_oblivious_forest_create come first, with their texts
res["old_null_leaves"] = create(**good, flags=0x1, null=("leaves",))
res["old_leaf_dim"] = create(**dict(good, k=0), flags=0x1)
res["old_fid"] = create([1, 0, 2], [0, 1, 3], np.arange(7.0), 3, covers=bad(0, -1.0), flags=CONTRIBS)
res["old_depth"] = create([1, 17, 0], [0] * 18, np.zeros(8), 3, flags=CONTRIBS)
for name, fl in (("contribs", CONTRIBS), ("approx", APPROX), ("both", CONTRIBS | APPROX)):
    res["valid_" + name] = create(**good, covers=ones, flags=fl)
res["valid_zero_covers"] = create(**good, covers=np.zeros(7), flags=CONTRIBS | APPROX)
res["valid_k2"] = create(**dict(good, leaves=np.arange(14.0), k=2), covers=ones, flags=CONTRIBS | APPROX)
print(json.dumps(res))
"""


@pytest.fixture(scope="module")
def refusals(ta):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case,status,text", [
    ("unknown_bit_1", INVALID_ARG, "flags 0x1"), ("unknown_bit_cat", INVALID_ARG, "flags 0x24"),
    ("null_covers_contribs", INVALID_ARG, "leaf_covers is null"), ("null_covers_approx", INVALID_ARG, "leaf_covers is null"),
    ("negative", INVALID_FOREST, "tree 2 leaf 1"), ("nan", INVALID_FOREST, "tree 1 leaf 0"), ("inf", INVALID_FOREST, "tree 2 leaf 3"),
    ("old_null_leaves", INVALID_ARG, "tahoe_oblivious_forest_create: null argument"),
    ("old_leaf_dim", INVALID_ARG, "leaf_dim must be in [1,1024], got 0"),
    ("old_fid", INVALID_FOREST, "tree 2 level 1: fid 3 >= num_cols 3"), ("old_depth", INVALID_ARG, "tree 1: depth 17"),
])
def test_refusals_come_before_the_device(refusals, case, status, text):
    got, msg = refusals[case]
    assert got == status and got != NO_DEVICE, (got, msg)
    assert text in msg, msg


@pytest.mark.parametrize("case", ["flags0_no_covers", "flags0_bad_covers_ignored", "valid_contribs", "valid_approx", "valid_both",
                                  "valid_zero_covers", "valid_k2"])
def test_a_valid_create_reaches_the_device(refusals, case):
    got, msg = refusals[case]
    assert got == NO_DEVICE, (got, msg)


# ------------------------------------------------------------------------------------------------ the reference
def small(seed, k=1):
    forest = obr.make_forest([3, 0, 5, 1, 4], 4, k, seed=seed)  # 4 columns: features repeat within a tree
    return forest, obr.make_data(33, 4, seed=seed + 100)


def expansion(forest, covers):
    """The heap expansion as a multi-class forest: tree t * K + k carries class k's leaves"""
    k, T = forest["k"], len(forest["depths"])
    per_class = [osr.expand_with_covers(forest, covers, c) for c in range(k)]
    D = per_class[0][1]
    return np.stack([n.reshape(T, -1) for n, _ in per_class], axis=1).reshape(-1), T * k, D


@pytest.mark.parametrize("kind", ["int", "half", "most", "zero"])
@pytest.mark.parametrize("k", [1, 2])
def test_poly_equals_brute_force_shapley_values(kind, k):
    forest, data = small(3 + k, k)
    covers = osr.make_covers(forest, kind, seed=5)
    assert kind == "int" or (covers == 0).any()
    want = osr.brute(forest, covers, data, avg=(k == 2), global_bias=0.25)
    got, A, N = osr.poly(forest, covers, data, avg=(k == 2), global_bias=0.25)
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    assert (A >= np.abs(got) - 1e-12 * np.abs(got)).all() and N.max() > 0
    # additivity: the contributions and the bias sum to the margin
    margin = obr.ref_of(forest, data)[0].astype(np.float64)
    if k == 2:
        margin = margin / len(forest["depths"])
    assert np.abs(got.sum(axis=-1) - (margin + 0.25)).max() <= 1e-6 * np.abs(margin).max()


@pytest.mark.parametrize("k", [1, 3])
def test_poly_equals_the_dense_brute_force_on_the_expansion(k):
    forest, data = small(11, k)
    covers = osr.make_covers(forest, "int", seed=6)
    nodes, T, D = expansion(forest, covers)
    want = contribs_ref.brute(nodes, T, D, forest["cols"], data, obr.MISSING, num_classes=k, avg=True, global_bias=-0.5)
    got, _, _ = osr.poly(forest, covers, data, avg=True, global_bias=-0.5)
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    assert np.array_equal(got[:, :, -1].astype(np.float32).view(np.uint32), want[:, :, -1].astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("avg", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_saabas_equals_the_dense_reference_on_the_expansion_bit_for_bit(k, avg):
    forest, data = small(17, k)
    covers = osr.make_covers(forest, "int", seed=7)
    nodes, T, D = expansion(forest, covers)
    want = approx_contribs_ref.dense(nodes, T, D, forest["cols"], data, obr.MISSING, num_classes=k, avg=avg, global_bias=0.125)
    got = osr.saabas(forest, covers, data, avg=avg, global_bias=0.125)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("kind", ["half", "zero"])
def test_saabas_is_additive_with_empty_leaves(kind):
    forest, data = small(23, 2)
    covers = osr.make_covers(forest, kind, seed=8)
    got = osr.saabas(forest, covers, data).astype(np.float64)
    margin = obr.ref_of(forest, data)[0].astype(np.float64)
    assert np.abs(got.sum(axis=-1) - margin).max() <= 1e-5 * np.abs(margin).max()


def test_the_form_rule_against_a_table():
    lds = 160 * 1024
    table = {(319, 1): "lds", (320, 1): "inplace", (159, 3): "lds", (160, 3): "inplace", (127, 4): "lds", (128, 4): "inplace",
             (127, 9): "lds", (128, 9): "inplace", (12, 1): "lds", (0, 1): "lds"}
    for (used, k), form in table.items():
        assert osr.shap_form(used, k, lds) == form, (used, k)
        assert osr.shap_form(used, k, lds, forced_inplace=True) == "inplace"
