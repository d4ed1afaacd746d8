"""Typed, nullable tables (tahoe_table_create / _destroy, tahoe_forest_predict_table / reserve_table / get_table_plan) without a
GPU: the symbols, the descriptor's layout, every refusal of tahoe_table_create -- all of them come before a device is touched --
the refusals of the three forest calls on a NULL or zeroed handle, and the wrapper's ValueErrors, which are raised before the
library is called."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG = 0, 1
SYMBOLS = ("tahoe_table_create", "tahoe_table_destroy", "tahoe_forest_predict_table", "tahoe_forest_reserve_table",
           "tahoe_forest_get_table_plan")
TYPES = ("FLOAT32", "FLOAT64", "FLOAT16", "INT8", "INT16", "INT32", "INT64", "UINT8", "UINT16", "UINT32", "UINT64")


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def _error(ta):
    return ta.lib.tahoe_last_error().decode()


def _header():
    return open(os.path.join(ROOT, "include", "tahoe_amd.h")).read()


def test_symbols_are_exported_declared_and_bound(ta):
    out = subprocess.run(["nm", "-D", "--defined-only", ta.capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    header = _header()
    for name in SYMBOLS:
        assert name in ta.capi.EXPORTED_SYMBOLS
        assert name in exported
        assert re.search(rf"^(tahoe_status|void) +{name}\(", header, re.M), name
        assert getattr(ta.lib, name).argtypes is not None
    assert "typedef struct tahoe_column {" in header and "typedef struct tahoe_table tahoe_table;" in header
    for cls in (ta.capi.Forest, ta.capi.SparseForest, ta.capi.ObliviousForest, ta.capi.VectorForest):
        for method in ("predict_table", "reserve_table", "table_plan"):
            assert callable(getattr(cls, method)), (cls, method)
    assert callable(ta.Table) and ta.Table is ta.capi.Table
    assert ta.lib.tahoe_abi_version() == 2  # additive
    # no kernel form was added or named: 32 stays unassigned, TAHOE_FORM_* stays 0 .. 22
    assert ta.lib.tahoe_kernel_form_name(32).decode() == "?"
    assert sorted(int(v) for v in re.findall(r"\bTAHOE_FORM_\w+ = (\d+)", header)) == list(range(23))


def test_descriptor_layout_and_type_codes(ta):
    col = ta.capi.Column
    assert C.sizeof(col) == 32
    assert [(n, getattr(col, n).offset, getattr(col, n).size) for n, _ in col._fields_] == [
        ("data", 0, 8), ("validity", 8, 8), ("offset", 16, 8), ("type", 24, 4), ("reserved", 28, 4)]
    header = _header()
    # the header's struct, field by field and in this order
    body = re.search(r"typedef struct tahoe_column \{(.*?)\} tahoe_column;", header, re.S).group(1)
    fields = re.findall(r"^\s*(const void|const uint8_t|int64_t|int32_t)\s*\*?\s*\*?(\w+);", body, re.M)
    assert fields == [("const void", "data"), ("const uint8_t", "validity"), ("int64_t", "offset"), ("int32_t", "type"),
                      ("int32_t", "reserved")]
    for code, name in enumerate(TYPES):
        assert re.search(rf"\bTAHOE_COL_{name} = {code}\b", header), name
        assert getattr(ta.capi, "COL_" + name) == code


def _create(ta, cols, rows=10, num_cols=None):
    arr = (ta.capi.Column * max(len(cols), 1))(*cols)
    out = C.c_void_p(0xDEAD)
    status = ta.lib.tahoe_table_create(C.cast(arr, C.c_void_p), len(cols) if num_cols is None else num_cols, rows, C.byref(out))
    return status, out


def test_table_create_refusals_name_the_column(ta):
    col = ta.capi.Column
    good = col(64, None, 0, ta.capi.COL_FLOAT64, 0)  # (addresses are never read: every refusal comes before a device is touched)
    cases = [
        (col(64, None, 0, 11, 0), "unknown type"),
        (col(64, None, 0, -1, 0), "unknown type"),
        (col(None, None, 0, ta.capi.COL_INT8, 0), "null data"),
        (col(64, None, -1, ta.capi.COL_INT32, 0), "negative offset"),
        (col(68, None, 0, ta.capi.COL_FLOAT64, 0), "not aligned"),
        (col(66, None, 0, ta.capi.COL_UINT32, 0), "not aligned"),
        (col(65, None, 0, ta.capi.COL_FLOAT16, 0), "not aligned"),
        (col(64, None, 0, ta.capi.COL_FLOAT32, 1), "reserved"),
    ]
    for bad, what in cases:
        for at in (0, 2):  # the bad column first, and behind two good ones
            status, out = _create(ta, [good] * at + [bad] + [good])
            assert status == INVALID_ARG and out.value is None, (what, at)
            err = _error(ta)
            assert "tahoe_table_create" in err and f"column {at}" in err and what in err, err
    status, out = _create(ta, [good], num_cols=-1)
    assert status == INVALID_ARG and "tahoe_table_create" in _error(ta) and "num_cols" in _error(ta) and out.value is None
    assert ta.lib.tahoe_table_create(None, 2, 10, C.byref(out)) == INVALID_ARG and "cols_host" in _error(ta)
    assert ta.lib.tahoe_table_create(None, 0, 0, None) == INVALID_ARG and "out" in _error(ta)
    # one-byte types have no alignment to miss; a NULL data pointer is fine in a table without rows (both get past the checks to
    # the upload, which needs a device: whatever that gives, it is not a refusal of the argument)
    status, out = _create(ta, [col(65, None, 0, ta.capi.COL_UINT8, 0), col(None, None, 3, ta.capi.COL_INT64, 0)], rows=0)
    assert status != INVALID_ARG, _error(ta)
    if status == OK:
        ta.lib.tahoe_table_destroy(out)
    ta.lib.tahoe_table_destroy(None)  # a no-op


def test_forest_calls_refuse_null_arguments_by_name(ta):
    p = C.c_void_p(64)  # a non-NULL address that is never read
    handle = C.create_string_buffer(1 << 16)  # zeros: no check below may depend on what a handle holds
    h = C.cast(handle, C.c_void_p)
    predict, reserve, plan = ta.lib.tahoe_forest_predict_table, ta.lib.tahoe_forest_reserve_table, ta.lib.tahoe_forest_get_table_plan
    assert predict(None, p, p, None) == INVALID_ARG
    assert "tahoe_forest_predict_table" in _error(ta) and "forest" in _error(ta)
    assert predict(h, p, None, None) == INVALID_ARG
    assert "tahoe_forest_predict_table" in _error(ta) and "table" in _error(ta)
    assert predict(None, None, None, None) == INVALID_ARG
    assert reserve(None, 10) == INVALID_ARG and "tahoe_forest_reserve_table" in _error(ta)
    assert reserve(h, 0) == OK
    form, chunk = C.c_int(), C.c_size_t()
    assert plan(None, 10, C.byref(form), C.byref(chunk)) == INVALID_ARG and "tahoe_forest_get_table_plan" in _error(ta)
    assert plan(h, 10, None, C.byref(chunk)) == INVALID_ARG and "tahoe_forest_get_table_plan" in _error(ta)
    assert plan(h, 10, C.byref(form), None) == INVALID_ARG and "tahoe_forest_get_table_plan" in _error(ta)


class _Cai:
    """What a cuDF column publishes: __cuda_array_interface__ with an optional mask.  Never dereferenced here."""

    def __init__(self, n, typestr, ptr=256, mask=None, strides=None):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}
        if mask is not None:
            self.__cuda_array_interface__["mask"] = mask


def test_wrapper_raises_value_error_before_the_library_is_called(ta):
    import torch

    Table = ta.Table
    with pytest.raises(ValueError, match="CUDA"):
        Table([torch.zeros(5)])  # a CPU column
    with pytest.raises(ValueError, match="1-D"):
        Table([torch.zeros(5, 1)])
    with pytest.raises(ValueError, match="CUDA tensor or have __cuda_array_interface__"):
        Table([np.zeros(5, np.float32)])
    with pytest.raises(ValueError, match="unsupported dtype"):
        Table([_Cai(5, "<c8")])
    with pytest.raises(ValueError, match="unsupported dtype"):
        Table([_Cai(5, ">f4")])  # big-endian
    with pytest.raises(ValueError, match="contiguous"):
        Table([_Cai(5, "<f8", strides=(16,))])
    with pytest.raises(ValueError, match="unequal lengths"):
        Table([_Cai(5, "<f4"), _Cai(6, "<i8")])
    with pytest.raises(ValueError, match="unequal lengths"):
        Table([_Cai(6, "<f4"), _Cai(6, "<u2")], offsets=[0, 1])  # equal buffers, unequal rows behind the offsets
    with pytest.raises(ValueError, match="offset"):
        Table([_Cai(6, "<f4")], offsets=[-1])
    with pytest.raises(ValueError, match="offset"):
        Table([_Cai(6, "<f4")], offsets=[7])
    with pytest.raises(ValueError, match="shorter"):
        Table([_Cai(9, "<u4", mask=_Cai(1, "|u1"))])  # 9 rows need 2 bytes
    with pytest.raises(ValueError, match="shorter"):
        Table([_Cai(17, "<i2")], validity=[_Cai(2, "|u1")], offsets=[1])  # 16 rows: bits 1 .. 16 need 3 bytes
    with pytest.raises(ValueError, match="bytes"):
        Table([_Cai(8, "<i2")], validity=[_Cai(1, "<i4")])
    with pytest.raises(ValueError, match="validity entries"):
        Table([_Cai(8, "<i2")], validity=[None, None])

    class _NoHandle:
        num_cols = 3
        num_classes = 1

    with pytest.raises(ValueError, match="Table"):
        ta.Forest.predict_table(_NoHandle(), [torch.zeros(5)] * 3)
    t = Table.__new__(Table)  # a table of two columns that never reached the library
    t.num_cols, t.rows, t._h = 2, 5, None
    with pytest.raises(ValueError, match="2 columns"):
        ta.Forest.predict_table(_NoHandle(), t)
