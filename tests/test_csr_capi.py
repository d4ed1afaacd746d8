"""CSR rows (tahoe_forest_predict_csr / tahoe_forest_reserve_csr) without a GPU: the symbols, every argument refusal -- all of
them come before the handle or a device is touched, so a block of zeros stands in for a handle here -- and the numpy helper
capi.dense_to_csr against a numpy densify."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG = 0, 1
MISSING = -999.0


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


def densify(indptr, indices, values, cols, missing):
    x = np.full((indptr.size - 1, cols), missing, dtype=np.float32)
    for r in range(indptr.size - 1):
        x[r, indices[indptr[r]:indptr[r + 1]]] = values[indptr[r]:indptr[r + 1]]
    return x


def test_symbols_are_exported_and_bound(ta):
    for name in ("tahoe_forest_predict_csr", "tahoe_forest_reserve_csr", "tahoe_forest_get_csr_plan"):
        assert name in ta.capi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", ta.capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert {"tahoe_forest_predict_csr", "tahoe_forest_reserve_csr"} <= exported
    assert hasattr(ta.Forest, "predict_csr") and hasattr(ta.Forest, "reserve_csr") and callable(ta.dense_to_csr)
    names = [ta.lib.tahoe_kernel_form_name(i).decode() for i in (19, 20, 21, 22, 23)]
    assert names == ["qring_region6", "csr_rowtile", "csr_sparse_rowtile", "csr_sparse_top", "?"]


def test_null_handle_is_refused(ta):
    p = C.c_void_p(64)  # never read
    assert ta.lib.tahoe_forest_predict_csr(None, None, None, None, None, 0, 0, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_predict_csr(None, p, p, p, p, 10, 5, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_reserve_csr(None, 10, 5) == INVALID_ARG
    form, chunk = C.c_int(), C.c_size_t()
    assert ta.lib.tahoe_forest_get_csr_plan(None, 10, 5, C.byref(form), C.byref(chunk)) == INVALID_ARG


def test_argument_refusals_come_before_the_handle_is_read(ta):
    handle = C.create_string_buffer(1 << 16)  # zeros: no check below may depend on what a handle holds
    h = C.cast(handle, C.c_void_p)
    p = C.c_void_p(64)  # a non-NULL address that is never read
    call = ta.lib.tahoe_forest_predict_csr
    assert call(h, None, p, p, p, 10, 5, None) == INVALID_ARG and "preds_dev" in _error(ta)
    assert call(h, p, None, p, p, 10, 5, None) == INVALID_ARG and "indptr_dev" in _error(ta)
    assert call(h, p, p, None, p, 10, 5, None) == INVALID_ARG and "indices_dev" in _error(ta)
    assert call(h, p, p, p, None, 10, 5, None) == INVALID_ARG and "values_dev" in _error(ta)
    assert call(h, p, p, None, None, 0, 5, None) == INVALID_ARG  # NULL entries with nnz > 0, whatever rows is
    assert call(h, p, p, p, p, 10, (1 << 63), None) == INVALID_ARG and "int64" in _error(ta)
    # rows == 0: TAHOE_OK with nothing launched -- NULL everything is fine, and so is nnz == 0 with NULL entry arrays
    assert call(h, None, None, None, None, 0, 0, None) == OK
    assert call(h, None, None, p, p, 0, 7, None) == OK


@pytest.mark.parametrize("shape", [(0, 5), (1, 1), (7, 13), (64, 33), (130, 500)])
@pytest.mark.parametrize("density", [0.0, 0.02, 0.4, 1.0])
def test_dense_to_csr_round_trips(ta, shape, density):
    rows, cols = shape
    rng = np.random.default_rng(rows * 1000 + cols + int(density * 100))
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    x[rng.random((rows, cols)) >= density] = MISSING
    indptr, indices, values = ta.dense_to_csr(x, MISSING)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and values.dtype == np.float32
    assert indptr.shape == (rows + 1,) and indptr[0] == 0 and indptr[-1] == indices.size == values.size
    assert np.all(np.diff(indptr) >= 0) and indices.size == int((x != np.float32(MISSING)).sum())
    for r in range(rows):  # sorted, unique column ids per row
        assert np.all(np.diff(indices[indptr[r]:indptr[r + 1]]) > 0)
    assert np.array_equal(densify(indptr, indices, values, cols, MISSING).view(np.uint32), x.view(np.uint32))


def test_dense_to_csr_sentinel_band_nan_and_negative_zero(ta):
    m = np.float32(0.5)  # a sentinel small enough for float32 to resolve the 1e-6 band around it
    eps = np.float32(1.0e-6)
    inside = [m, np.float32(m + np.float32(5e-7)), np.float32(m - np.float32(5e-7))]
    outside = [np.float32(m + np.float32(3e-6)), np.float32(m - np.float32(3e-6)), np.float32(np.nan), np.float32(-0.0),
               np.float32(0.0), np.float32(np.inf), np.float32(-np.inf)]
    for v in inside:
        assert abs(np.float32(v - m)) <= eps
    for v in outside[:2]:
        assert abs(np.float32(v - m)) > eps
    x = np.array([inside + outside, [m] * 10, outside + inside], dtype=np.float32)
    indptr, indices, values = ta.dense_to_csr(x, float(m))
    assert indptr.tolist() == [0, 7, 7, 14]  # the band is dropped, the empty row stays
    assert indices.tolist() == [3, 4, 5, 6, 7, 8, 9, 0, 1, 2, 3, 4, 5, 6]
    assert np.array_equal(values.view(np.uint32), np.array(outside + outside, np.float32).view(np.uint32))  # NaN, -0.0 bits kept
    back = densify(indptr, indices, values, 10, m)
    # what the library reads is unchanged: dropped entries were missing, and read as the sentinel they are missing again
    lib_missing = lambda a: np.abs(a - m) <= eps  # noqa: E731
    with np.errstate(invalid="ignore"):
        assert np.array_equal(lib_missing(back), lib_missing(x))
        keep = ~lib_missing(x)
    assert np.array_equal(back[keep].view(np.uint32), x[keep].view(np.uint32))
    # -999 (the sentinel of most tests): float32 has no neighbour within 1e-6, only the exact value is dropped
    y = np.array([[MISSING, np.nextafter(np.float32(MISSING), np.float32(0)), 1.0]], dtype=np.float32)
    assert ta.dense_to_csr(y, MISSING)[1].tolist() == [1, 2]
