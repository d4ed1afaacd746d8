"""Column-major batches (tahoe_forest_predict_columns / _column_ptrs / reserve_columns / get_columns_plan) without a GPU: the
symbols, every argument refusal -- all of them come before the handle or a device is touched, so a block of zeros stands in for
a handle here -- the form names, and the wrapper's ValueErrors, which are raised before the library is called."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG = 0, 1
SYMBOLS = ("tahoe_forest_predict_columns", "tahoe_forest_predict_column_ptrs", "tahoe_forest_reserve_columns",
           "tahoe_forest_get_columns_plan")


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
        assert re.search(rf"^tahoe_status {name}\(", header, re.M), name
        assert getattr(ta.lib, name).argtypes is not None
    for cls in (ta.capi.Forest, ta.capi.SparseForest, ta.capi.ObliviousForest, ta.capi.VectorForest):
        for method in ("predict_columns", "reserve_columns", "columns_plan"):
            assert callable(getattr(cls, method)), (cls, method)
    assert ta.lib.tahoe_abi_version() == 2  # additive


def test_form_names(ta):
    names = [ta.lib.tahoe_kernel_form_name(i).decode() for i in (31, 32, 33, 34, 35, 36)]
    assert names == ["vector_csr_tile", "?", "columns_rowtile", "columns_sparse_rowtile", "columns_sparse_top", "?"]
    header = _header()
    for name, value in (("ROWTILE", 33), ("SPARSE_ROWTILE", 34), ("SPARSE_TOP", 35)):
        assert re.search(rf"\bTAHOE_COLUMNS_FORM_{name} = {value}\b", header)
    # the regex of tests/test_formats_capi.py collects the TAHOE_FORM_ prefix and wants 0 .. n-1 without a gap: still 0 .. 22
    values = sorted(int(v) for v in re.findall(r"\bTAHOE_FORM_\w+ = (\d+)", header))
    assert values == list(range(23))


def test_null_handle_is_refused(ta):
    p = C.c_void_p(64)  # never read
    assert ta.lib.tahoe_forest_predict_columns(None, p, p, 10, 10, None) == INVALID_ARG
    assert "tahoe_forest_predict_columns" in _error(ta)
    assert ta.lib.tahoe_forest_predict_columns(None, None, None, 0, 0, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_predict_column_ptrs(None, p, p, 10, None) == INVALID_ARG
    assert "tahoe_forest_predict_column_ptrs" in _error(ta)
    assert ta.lib.tahoe_forest_predict_column_ptrs(None, None, None, 0, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_reserve_columns(None, 10) == INVALID_ARG
    assert "tahoe_forest_reserve_columns" in _error(ta)
    form, chunk = C.c_int(), C.c_size_t()
    assert ta.lib.tahoe_forest_get_columns_plan(None, 10, C.byref(form), C.byref(chunk)) == INVALID_ARG
    assert "tahoe_forest_get_columns_plan" in _error(ta)


def test_argument_refusals_come_before_the_handle_is_read(ta):
    handle = C.create_string_buffer(1 << 16)  # zeros: no check below may depend on what a handle holds
    h = C.cast(handle, C.c_void_p)
    p = C.c_void_p(64)  # a non-NULL address that is never read
    strided, table = ta.lib.tahoe_forest_predict_columns, ta.lib.tahoe_forest_predict_column_ptrs
    assert strided(h, None, p, 10, 10, None) == INVALID_ARG
    assert "tahoe_forest_predict_columns" in _error(ta) and "preds_dev" in _error(ta)
    assert strided(h, p, None, 10, 10, None) == INVALID_ARG
    assert "tahoe_forest_predict_columns" in _error(ta) and "data_dev" in _error(ta)
    assert strided(h, p, p, 10, 9, None) == INVALID_ARG
    assert "tahoe_forest_predict_columns" in _error(ta) and "col_stride" in _error(ta)
    assert strided(h, p, p, 1, 0, None) == INVALID_ARG and "col_stride" in _error(ta)
    assert table(h, None, p, 10, None) == INVALID_ARG
    assert "tahoe_forest_predict_column_ptrs" in _error(ta) and "preds_dev" in _error(ta)
    assert table(h, p, None, 10, None) == INVALID_ARG
    assert "tahoe_forest_predict_column_ptrs" in _error(ta) and "cols_dev" in _error(ta)
    # rows == 0: TAHOE_OK with nothing launched, NULL everything is fine
    assert strided(h, None, None, 0, 0, None) == OK
    assert strided(h, None, None, 0, 7, None) == OK
    assert table(h, None, None, 0, None) == OK
    assert ta.lib.tahoe_forest_reserve_columns(h, 0) == OK


class _NoHandle:
    """predict_columns' checks need num_cols only; a call that got past them would fail on the missing handle"""
    num_cols = 3
    num_classes = 1


def _predict_columns(ta, x):
    return ta.Forest.predict_columns(_NoHandle(), x)


def test_wrapper_raises_value_error_before_the_library_is_called(ta):
    import torch

    with pytest.raises(ValueError, match="column-major"):
        _predict_columns(ta, torch.zeros(5, 3))  # a CPU row-major tensor
    with pytest.raises(ValueError, match="CUDA"):
        _predict_columns(ta, torch.zeros(3, 5).t())  # column-major, but on the host
    with pytest.raises(ValueError, match="float32"):
        _predict_columns(ta, torch.zeros(3, 5, dtype=torch.float64).t())
    with pytest.raises(ValueError, match="float32"):
        _predict_columns(ta, [torch.zeros(5, dtype=torch.float16)] * 3)
    with pytest.raises(ValueError, match=r"\[rows, 3\]"):
        _predict_columns(ta, torch.zeros(4, 5).t())  # wrong column count
    with pytest.raises(ValueError, match="2 columns given"):
        _predict_columns(ta, [torch.zeros(5), torch.zeros(5)])
    with pytest.raises(ValueError, match="unequal lengths"):
        _predict_columns(ta, [torch.zeros(5), torch.zeros(6), torch.zeros(5)])  # ragged
    with pytest.raises(ValueError, match="1-D"):
        _predict_columns(ta, [torch.zeros(5, 1)] * 3)
    with pytest.raises(ValueError, match="CUDA"):
        _predict_columns(ta, [torch.zeros(5)] * 3)
