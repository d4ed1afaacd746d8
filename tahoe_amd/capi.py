"""ctypes binding of include/tahoe_amd.h.

Plumbing only: torch (or anything else) owns device memory and streams; this module passes raw
device pointers through the C ABI.  If libtahoe_amd.so has not been built the import fails --
there is deliberately no pure-Python or CPU substitute.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtahoe_amd.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "or `make -C tahoe_amd/csrc`.  tahoe_amd has no fallback path."
    )

# torch bundles its own libamdhip64.so.7.  Two HIP runtimes in one process do not share a device
# context (the second one sees no GPU), so load torch's first: libtahoe_amd.so then binds to the
# already-loaded runtime by SONAME.  Without torch (the C++ CLI) the system runtime is used.
try:
    import torch  # noqa: F401
except ImportError:  # pragma: no cover
    pass

lib = C.CDLL(LIB_PATH)

# ---- constants mirrored from the header ----
OUT_RAW, OUT_AVG, OUT_SIGMOID, OUT_THRESHOLD = 0x0, 0x1, 0x10, 0x100
OUT_SOFTMAX = 0x1000  # multi-class handles only (tahoe_forest_create_multiclass)
STRATEGY_AUTO, STRATEGY_DIRECT, STRATEGY_ROWTILE, STRATEGY_TILEBLOCK, STRATEGY_TILERING, STRATEGY_QRING = range(6)
CREATE_PROB_RELAYOUT = 0x1
CREATE_CONTRIBS = 0x4  # per-feature contributions (tahoe_forest_predict_contribs); node weights are covers
CREATE_APPROX_CONTRIBS = 0x10  # Saabas contributions (tahoe_forest_predict_contribs_approx); node weights are covers
CREATE_CAT_CONTRIBS = 0x20  # tahoe_sparse_forest_create_cat: the two flags above on a handle with categorical splits
CREATE_INTERACTIONS = 0x40  # tahoe_oblivious_forest_create_ex: SHAP interaction values (tahoe_forest_predict_interactions)
CREATE_INTERVENTIONAL = 0x80  # tahoe_vector_forest_create_ex: interventional TreeSHAP (tahoe_forest_set_background), no covers needed
CREATE_VECTOR_INTERACTIONS = 0x100  # tahoe_vector_forest_create_ex, with CREATE_CONTRIBS: tahoe_forest_predict_interactions
CREATE_OBLIVIOUS_INTERVENTIONAL = 0x200  # tahoe_oblivious_forest_create_ex: interventional TreeSHAP (tahoe_forest_set_background), no covers needed
CREATE_PARTIAL_DEPENDENCE = 0x800  # tahoe_sparse_forest_create_ex / _cat: partial dependence (tahoe_forest_predict_partial_dependence); needs covers
CREATE_STAGED = 0x2000  # tahoe_oblivious_forest_create_ex / _cat, tahoe_vector_forest_create_ex: set_stages / predict_staged; no covers needed
CREATE_CSR = 0x4000  # the same three creates: predict_csr / reserve_csr / csr_plan; no covers needed
CREATE_NAN_MISSING = 0x1000  # dense, multi-class, sparse and categorical creates: a NaN feature value is missing, beside the sentinel
CREATE_VECTOR_APPROX = 0x400  # tahoe_vector_forest_create_ex: Saabas contributions (tahoe_forest_predict_contribs_approx); needs covers
STRATEGY_NAMES = {1: "direct", 2: "rowtile", 3: "tileblock", 4: "tilering", 5: "qring"}
STATUS_NAMES = {
    0: "TAHOE_OK",
    1: "TAHOE_ERR_INVALID_ARG",
    2: "TAHOE_ERR_IO",
    3: "TAHOE_ERR_NO_MEMORY",
    4: "TAHOE_ERR_NO_DEVICE",
    5: "TAHOE_ERR_HIP",
    6: "TAHOE_ERR_INVALID_FOREST",
    7: "TAHOE_ERR_UNSUPPORTED",
}

# dense_node_t (Struct.h:44-48): weight, val, bits
NODE_DTYPE = np.dtype([("weight", "<f4"), ("val", "<f4"), ("bits", "<i4")])


class ForestParams(C.Structure):
    """tahoe_forest_params == forest_params_t (Struct.h:166-189)."""

    _fields_ = [
        ("num_nodes", C.c_int),
        ("depth", C.c_int),
        ("num_trees", C.c_int),
        ("num_cols", C.c_int),
        ("algo", C.c_int),
        ("output", C.c_int),
        ("threshold", C.c_float),
        ("global_bias", C.c_float),
        ("strategy", C.c_int),
        ("missing", C.c_float),
    ]


class ForestInfo(C.Structure):
    _fields_ = [
        ("num_trees", C.c_int),
        ("depth", C.c_int),
        ("num_cols", C.c_int),
        ("bits_bytes", C.c_int),
        ("lds_levels", C.c_int),
        ("device_bytes", C.c_size_t),
        ("lds_bytes_per_block", C.c_int),
        ("device_id", C.c_int),
        ("num_cus", C.c_int),
        ("top_levels", C.c_int),
        ("tile_rows", C.c_int),
        ("tileblock_lds_bytes", C.c_int),
        ("qring_walkers", C.c_int),
        ("qring_lds_bytes", C.c_int),
        ("qring_groups", C.c_int),
        ("is_sparse", C.c_int),
        ("ring_rows", C.c_int),
        ("tilering_lds_bytes", C.c_int),
        ("qring_tile_rows", C.c_int),
        ("relayout", C.c_int),
        ("relayout_swaps", C.c_size_t),
        ("stream_slots", C.c_int),
        ("stream_levels", C.c_int),
        ("stream_key_ties", C.c_float),
    ]


class CategoricalSplits(C.Structure):
    """tahoe_categorical_splits: the arrays are owned by the caller (pack_categorical keeps them alive)."""

    _fields_ = [
        ("num_splits", C.c_int32),
        ("node", C.c_void_p),
        ("offset", C.c_void_p),
        ("words", C.c_void_p),
        ("members_left", C.c_void_p),
    ]


class Column(C.Structure):
    """tahoe_column: one typed, nullable column in the layout of the Arrow C data interface (device buffers of the caller)."""

    _fields_ = [
        ("data", C.c_void_p),
        ("validity", C.c_void_p),
        ("offset", C.c_int64),
        ("type", C.c_int32),
        ("reserved", C.c_int32),
    ]


# TAHOE_COL_*, by __cuda_array_interface__ typestr (little-endian; "|" for the one-byte types) and element size
(COL_FLOAT32, COL_FLOAT64, COL_FLOAT16, COL_INT8, COL_INT16, COL_INT32, COL_INT64, COL_UINT8, COL_UINT16, COL_UINT32,
 COL_UINT64) = range(11)
_COL_TYPESTR = {"<f4": COL_FLOAT32, "<f8": COL_FLOAT64, "<f2": COL_FLOAT16, "|i1": COL_INT8, "<i2": COL_INT16, "<i4": COL_INT32,
                "<i8": COL_INT64, "|u1": COL_UINT8, "|b1": COL_UINT8, "<u2": COL_UINT16, "<u4": COL_UINT32, "<u8": COL_UINT64}
_COL_SIZE = {COL_FLOAT32: 4, COL_FLOAT64: 8, COL_FLOAT16: 2, COL_INT8: 1, COL_INT16: 2, COL_INT32: 4, COL_INT64: 8, COL_UINT8: 1,
             COL_UINT16: 2, COL_UINT32: 4, COL_UINT64: 8}


class TahoeError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        msg = lib.tahoe_last_error().decode(errors="replace")
        super().__init__(f"{where}: {STATUS_NAMES.get(status, status)}: {msg}")


def _check(status: int, where: str) -> None:
    if status != 0:
        raise TahoeError(status, where)


_vp, _sz, _i, _f = C.c_void_p, C.c_size_t, C.c_int, C.c_float
_PROTOS = {
    "tahoe_last_error": (C.c_char_p, []),
    "tahoe_abi_version": (_i, []),
    "tahoe_encode_node": (None, [_vp, _i, _f, _i, _f, _i]),
    "tahoe_decode_node": (None, [_vp] + [_vp] * 5),
    "tahoe_tree_num_nodes": (_i, [_i]),
    "tahoe_forest_create": (_i, [C.POINTER(_vp), _vp, C.POINTER(ForestParams)]),
    "tahoe_forest_create_ex": (_i, [C.POINTER(_vp), _vp, C.POINTER(ForestParams), C.c_uint]),
    "tahoe_forest_destroy": (None, [_vp]),
    "tahoe_forest_create_multiclass": (_i, [C.POINTER(_vp), _vp, C.POINTER(ForestParams), _i, C.c_uint]),
    "tahoe_forest_num_classes": (_i, [_vp]),
    "tahoe_forest_predict_contribs": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "tahoe_forest_predict_interactions": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "tahoe_forest_set_background": (_i, [_vp, _vp, _sz, _vp]),
    "tahoe_forest_predict_contribs_interventional": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "tahoe_forest_predict_contribs_approx": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "tahoe_forest_predict_partial_dependence": (_i, [_vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "tahoe_sparse_forest_create": (_i, [C.POINTER(_vp), _vp, _vp, C.POINTER(ForestParams)]),
    "tahoe_sparse_forest_create_ex": (_i, [C.POINTER(_vp), _vp, _vp, _vp, C.POINTER(ForestParams), _i, C.c_uint]),
    "tahoe_sparse_forest_create_cat": (_i, [C.POINTER(_vp), _vp, _vp, _vp, C.POINTER(ForestParams), _i, C.c_uint,
                                            C.POINTER(CategoricalSplits)]),
    "tahoe_oblivious_forest_create": (_i, [C.POINTER(_vp), _vp, _vp, _vp, C.POINTER(ForestParams), _i]),
    "tahoe_oblivious_forest_create_ex": (_i, [C.POINTER(_vp), _vp, _vp, _vp, _vp, C.POINTER(ForestParams), _i, C.c_uint]),
    "tahoe_oblivious_forest_create_cat": (_i, [C.POINTER(_vp), _vp, _vp, _vp, _vp, C.POINTER(ForestParams), _i, C.c_uint,
                                               C.POINTER(CategoricalSplits)]),
    "tahoe_vector_forest_create": (_i, [C.POINTER(_vp), _vp, _vp, _vp, C.c_int64, C.POINTER(ForestParams), _i]),
    "tahoe_vector_forest_create_ex": (_i, [C.POINTER(_vp), _vp, _vp, _vp, C.c_int64, _vp, C.POINTER(ForestParams), _i, C.c_uint]),
    "tahoe_dense_to_sparse": (_i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_sz)]),
    "tahoe_dense_to_sparse_ex": (_i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_sz)]),
    "tahoe_synth_sparse_forest": (_i, [_vp, _vp, C.POINTER(_sz), _i, _i, _i, _i, _f, _i, C.c_uint64]),
    "tahoe_forest_predict": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "tahoe_forest_predict_csr": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _sz, _vp]),
    "tahoe_forest_reserve_csr": (_i, [_vp, _sz, _sz]),
    "tahoe_forest_get_csr_plan": (_i, [_vp, _sz, _sz, C.POINTER(_i), C.POINTER(_sz)]),
    "tahoe_forest_predict_columns": (_i, [_vp, _vp, _vp, _sz, _sz, _vp]),
    "tahoe_forest_predict_column_ptrs": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "tahoe_forest_reserve_columns": (_i, [_vp, _sz]),
    "tahoe_forest_get_columns_plan": (_i, [_vp, _sz, C.POINTER(_i), C.POINTER(_sz)]),
    "tahoe_table_create": (_i, [_vp, _i, _sz, C.POINTER(_vp)]),
    "tahoe_table_destroy": (None, [_vp]),
    "tahoe_forest_predict_table": (_i, [_vp, _vp, _vp, _vp]),
    "tahoe_forest_reserve_table": (_i, [_vp, _sz]),
    "tahoe_forest_get_table_plan": (_i, [_vp, _sz, C.POINTER(_i), C.POINTER(_sz)]),
    "tahoe_forest_predict_raw": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "tahoe_forest_predict_accumulate": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "tahoe_forest_predict_leaf_idx": (_i, [_vp, _vp, _vp, _vp, _sz, _vp]),
    "tahoe_forest_set_stages": (_i, [_vp, _vp, _i]),
    "tahoe_forest_predict_staged": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "tahoe_forest_get_staged_strategy": (_i, [_vp, _sz]),
    "tahoe_transform_preds": (_i, [_vp, _sz, _i, _i, _f, _f, _vp]),
    "tahoe_forest_set_strategy": (_i, [_vp, _i]),
    "tahoe_forest_get_strategy": (_i, [_vp, _sz]),
    "tahoe_forest_check": (_i, [_vp, _vp]),
    "tahoe_forest_reserve": (_i, [_vp, _sz]),
    "tahoe_forest_predict_host": (_i, [_vp, _vp, _vp, _sz, _sz]),
    "tahoe_host_alloc": (_i, [C.POINTER(_vp), _sz]),
    "tahoe_host_free": (_i, [_vp]),
    "tahoe_forest_get_info": (_i, [_vp, C.POINTER(ForestInfo)]),
    "tahoe_forest_get_kernel_form": (_i, [_vp, _sz]),
    "tahoe_kernel_form_name": (C.c_char_p, [_i]),
    "tahoe_forest_set_profiling": (_i, [_vp, _i]),
    "tahoe_forest_kernel_times": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "tahoe_forest_prepass_times": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "tahoe_load_model": (_i, [C.c_char_p, C.POINTER(_i), C.POINTER(_i), C.POINTER(_vp)]),
    "tahoe_load_data": (_i, [C.c_char_p, C.POINTER(_i), C.POINTER(_i), C.POINTER(_f), C.POINTER(_vp)]),
    "tahoe_write_model": (_i, [C.c_char_p, _i, _i, _vp]),
    "tahoe_write_data": (_i, [C.c_char_p, _i, _i, _f, _vp]),
    "tahoe_save_model_bin": (_i, [C.c_char_p, _i, _i, _vp]),
    "tahoe_load_model_bin": (_i, [C.c_char_p, C.POINTER(_i), C.POINTER(_i), C.POINTER(_vp)]),
    "tahoe_save_data_bin": (_i, [C.c_char_p, _i, _i, _f, _vp]),
    "tahoe_load_data_bin": (_i, [C.c_char_p, C.POINTER(_i), C.POINTER(_i), C.POINTER(_f), C.POINTER(_vp)]),
    "tahoe_load_model_cached": (_i, [C.c_char_p, C.POINTER(_i), C.POINTER(_i), C.POINTER(_vp), C.POINTER(_i)]),
    "tahoe_load_data_cached": (_i, [C.c_char_p, C.POINTER(_i), C.POINTER(_i), C.POINTER(_f), C.POINTER(_vp), C.POINTER(_i)]),
    "tahoe_free_host": (None, [_vp]),
    "tahoe_synth_forest": (None, [_vp, _i, _i, _i, C.c_uint64, _f]),
    "tahoe_synth_data": (None, [_vp, _sz, _sz, _i, C.c_uint64, _f, _f, _f]),
    "tahoe_synth_forest_hist": (_i, [_vp, _i, _i, _i, C.c_uint64, C.c_uint64, _i, _f, _f, _f]),
    "tahoe_synth_data_hist": (_i, [_vp, _sz, _sz, _i, C.c_uint64, C.c_uint64, _f, _f, _f]),
    "tahoe_device_count": (_i, [C.POINTER(_i)]),
    "tahoe_device_set": (_i, [_i]),
    "tahoe_device_alloc": (_i, [C.POINTER(_vp), _sz, _i]),
    "tahoe_device_free": (_i, [_vp]),
    "tahoe_device_memset": (_i, [_vp, _i, _sz, _vp]),
    "tahoe_widen_f32_to_f64": (_i, [_vp, _vp, _sz, _vp]),
    "tahoe_narrow_f64_to_f32": (_i, [_vp, _vp, _sz, _vp]),
    "tahoe_copy_to_device": (_i, [_vp, _vp, _sz, _vp]),
    "tahoe_copy_to_host": (_i, [_vp, _vp, _sz, _vp]),
    "tahoe_stream_create": (_i, [C.POINTER(_vp)]),
    "tahoe_stream_destroy": (_i, [_vp]),
    "tahoe_stream_synchronize": (_i, [_vp]),
    "tahoe_event_create": (_i, [C.POINTER(_vp)]),
    "tahoe_event_destroy": (_i, [_vp]),
    "tahoe_event_record": (_i, [_vp, _vp]),
    "tahoe_stream_wait_event": (_i, [_vp, _vp]),
    "tahoe_copy_peer": (_i, [_vp, _i, _vp, _i, _sz, _vp]),
    "tahoe_device_synchronize": (_i, []),
    "tahoe_device_lds_bytes": (_i, [C.POINTER(_i)]),
    "tahoe_compare_device": (_i, [_vp, _vp, _sz, _f, C.POINTER(_sz), _vp]),
}
for _name, (_res, _args) in _PROTOS.items():
    _fn = getattr(lib, _name)  # AttributeError here = the library does not export a declared symbol
    _fn.restype = _res
    _fn.argtypes = _args

EXPORTED_SYMBOLS = tuple(_PROTOS)


# ---- host-side helpers (formats, synthetic inputs) ----
class PinnedArray:
    """float32 [rows, cols] array in pinned host memory (tahoe_host_alloc); `.array` is the numpy view."""

    def __init__(self, rows: int, cols: int):
        self._p = _vp()
        _check(lib.tahoe_host_alloc(C.byref(self._p), max(rows * cols * 4, 4)), "tahoe_host_alloc")
        buf = (C.c_float * (rows * cols)).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=np.float32).reshape(rows, cols)

    def close(self) -> None:
        if self._p:
            self.array = None
            _check(lib.tahoe_host_free(self._p), "tahoe_host_free")
            self._p = None


def tree_num_nodes(depth: int) -> int:
    return lib.tahoe_tree_num_nodes(depth)


def _take_nodes(ptr, n):
    try:
        buf = (C.c_char * (n * NODE_DTYPE.itemsize)).from_address(ptr.value) if n else b""
        return np.frombuffer(buf, dtype=NODE_DTYPE, count=n).copy()
    finally:
        lib.tahoe_free_host(ptr)


def _take_floats(ptr, rows, cols):
    n = rows * cols
    try:
        buf = (C.c_char * (n * 4)).from_address(ptr.value) if n else b""
        return np.frombuffer(buf, dtype=np.float32, count=n).copy().reshape(rows, cols)
    finally:
        lib.tahoe_free_host(ptr)


def load_model(path: str, num_trees: int = 10, depth: int = 20, cached: bool = False):
    """-> (nodes[NODE_DTYPE], num_trees, depth).  Defaults are the BaseTahoeTest ctor defaults.
    cached=True: use / refresh the binary cache "<path>.tbin" (tahoe_load_model_cached)."""
    nt, d, ptr = _i(num_trees), _i(depth), _vp()
    if cached:
        _check(lib.tahoe_load_model_cached(os.fsencode(path), C.byref(nt), C.byref(d), C.byref(ptr), None),
               "tahoe_load_model_cached")
    else:
        _check(lib.tahoe_load_model(os.fsencode(path), C.byref(nt), C.byref(d), C.byref(ptr)), "tahoe_load_model")
    return _take_nodes(ptr, nt.value * tree_num_nodes(d.value)), nt.value, d.value


def load_data(path: str, num_rows: int = 1000, num_cols: int = 500, missing: float = 0.0, cached: bool = False):
    """-> (data[rows, cols] float32, missing)."""
    nr, nc, ms, ptr = _i(num_rows), _i(num_cols), _f(missing), _vp()
    if cached:
        _check(lib.tahoe_load_data_cached(os.fsencode(path), C.byref(nr), C.byref(nc), C.byref(ms), C.byref(ptr), None),
               "tahoe_load_data_cached")
    else:
        _check(lib.tahoe_load_data(os.fsencode(path), C.byref(nr), C.byref(nc), C.byref(ms), C.byref(ptr)),
               "tahoe_load_data")
    return _take_floats(ptr, nr.value, nc.value), ms.value


def save_model_bin(path: str, nodes: np.ndarray, num_trees: int, depth: int) -> None:
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    assert nodes.size == num_trees * tree_num_nodes(depth)
    _check(lib.tahoe_save_model_bin(os.fsencode(path), num_trees, depth, nodes.ctypes.data), "tahoe_save_model_bin")


def load_model_bin(path: str):
    nt, d, ptr = _i(0), _i(0), _vp()
    _check(lib.tahoe_load_model_bin(os.fsencode(path), C.byref(nt), C.byref(d), C.byref(ptr)), "tahoe_load_model_bin")
    return _take_nodes(ptr, nt.value * tree_num_nodes(d.value)), nt.value, d.value


def save_data_bin(path: str, data: np.ndarray, missing: float) -> None:
    data = np.ascontiguousarray(data, dtype=np.float32)
    _check(lib.tahoe_save_data_bin(os.fsencode(path), data.shape[0], data.shape[1], missing, data.ctypes.data),
           "tahoe_save_data_bin")


def load_data_bin(path: str):
    nr, nc, ms, ptr = _i(0), _i(0), _f(0.0), _vp()
    _check(lib.tahoe_load_data_bin(os.fsencode(path), C.byref(nr), C.byref(nc), C.byref(ms), C.byref(ptr)),
           "tahoe_load_data_bin")
    return _take_floats(ptr, nr.value, nc.value), ms.value


def write_model(path: str, nodes: np.ndarray, num_trees: int, depth: int) -> None:
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    assert nodes.size == num_trees * tree_num_nodes(depth)
    _check(lib.tahoe_write_model(os.fsencode(path), num_trees, depth, nodes.ctypes.data), "tahoe_write_model")


def write_data(path: str, data: np.ndarray, missing: float) -> None:
    data = np.ascontiguousarray(data, dtype=np.float32)
    _check(lib.tahoe_write_data(os.fsencode(path), data.shape[0], data.shape[1], missing, data.ctypes.data),
           "tahoe_write_data")


def synth_forest(num_trees: int, depth: int, num_cols: int, seed: int = 42, leaf_prob: float = 0.0) -> np.ndarray:
    nodes = np.empty(num_trees * tree_num_nodes(depth), dtype=NODE_DTYPE)
    lib.tahoe_synth_forest(nodes.ctypes.data, num_trees, depth, num_cols, seed, leaf_prob)
    return nodes


def synth_data(rows: int, num_cols: int, seed: int = 43, missing_prob: float = 0.0, missing: float = -999.0,
               nan_prob: float = 0.0, first_row: int = 0) -> np.ndarray:
    data = np.empty((rows, num_cols), dtype=np.float32)
    lib.tahoe_synth_data(data.ctypes.data, first_row, rows, num_cols, seed, missing_prob, missing, nan_prob)
    return data


def synth_forest_hist(num_trees: int, depth: int, num_cols: int, seed: int = 42, feature_seed: int = 7, max_bins: int = 255,
                      zipf_s: float = 1.0, leaf_prob: float = 0.02, scale_decades: float = 3.0) -> np.ndarray:
    """Forest in the style of histogram-trained GBDT models (tahoe_synth_forest_hist)."""
    nodes = np.zeros(num_trees * tree_num_nodes(depth), dtype=NODE_DTYPE)
    _check(lib.tahoe_synth_forest_hist(nodes.ctypes.data, num_trees, depth, num_cols, seed, feature_seed, max_bins, zipf_s, leaf_prob,
                                       scale_decades), "tahoe_synth_forest_hist")
    return nodes


def synth_data_hist(rows: int, num_cols: int, seed: int = 43, feature_seed: int = 7, scale_decades: float = 3.0,
                    missing_prob: float = 0.0, missing: float = -999.0, first_row: int = 0) -> np.ndarray:
    """Rows drawn from the per-feature distributions of synth_forest_hist (same feature_seed / scale_decades)."""
    out = np.empty((rows, num_cols), dtype=np.float32)
    _check(lib.tahoe_synth_data_hist(out.ctypes.data, first_row, rows, num_cols, seed, feature_seed, scale_decades, missing_prob,
                                     missing), "tahoe_synth_data_hist")
    return out


def set_probability_weights(nodes: np.ndarray, num_trees: int, depth: int, lo: float = -1.0, hi: float = 1.0) -> np.ndarray:
    """Fills dense_node_t.weight with the probability of reaching each node for features uniform in [lo, hi) and
    independent (what synth_data draws): root 1, left child p * P(x < thr), right child p * P(x >= thr).  Input
    preparation for the probability-guided re-layout (a trained model carries such weights from its training data)."""
    per = tree_num_nodes(depth)
    n = nodes.reshape(num_trees, per)
    w = np.zeros((num_trees, per), dtype=np.float64)
    w[:, 0] = 1.0
    thr = n["val"].astype(np.float64)
    is_leaf = (n["bits"].view(np.uint32) >> 31) != 0
    for level in range(depth):
        a, b = (1 << level) - 1, (2 << level) - 1
        p_right = np.clip((hi - thr[:, a:b]) / (hi - lo), 0.0, 1.0)
        p_right = np.where(np.isnan(p_right), 0.0, p_right)
        live = np.where(is_leaf[:, a:b], 0.0, w[:, a:b])  # nothing is reached below a leaf
        w[:, 2 * a + 1: 2 * b + 1: 2] = live * (1.0 - p_right)
        w[:, 2 * a + 2: 2 * b + 2: 2] = live * p_right
    n["weight"] = w.astype(np.float32)
    return nodes


def dense_to_csr(x: np.ndarray, missing: float):
    """(indptr int64[rows + 1], indices int32[nnz], values float32[nnz]) of a dense float32 matrix: the entries the library
    reads as missing (|x - missing| <= 1e-6 in float32, its own test) are dropped, everything else is stored, NaN included."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("x must be [rows, cols]")
    with np.errstate(invalid="ignore"):
        keep = ~(np.abs(x - np.float32(missing)) <= np.float32(1.0e-6))
    indptr = np.zeros(x.shape[0] + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    return indptr, np.nonzero(keep)[1].astype(np.int32), x[keep]


def encode_nodes(fid, value, def_left, weight, is_leaf) -> np.ndarray:
    """Vector form of encode_node (Struct.h:103-108) for building test forests by hand."""
    fid = np.asarray(fid, dtype=np.int64)
    nodes = np.empty(fid.shape, dtype=NODE_DTYPE)
    nodes["weight"] = np.asarray(weight, dtype=np.float32)
    nodes["val"] = np.asarray(value, dtype=np.float32)
    bits = (fid & ((1 << 30) - 1)) | (np.asarray(def_left, dtype=np.int64) != 0) * (1 << 30) | (
        np.asarray(is_leaf, dtype=np.int64) != 0) * (1 << 31)
    nodes["bits"] = bits.astype(np.uint32).view(np.int32)
    return nodes


# ---- the forest operator ----
def _ptr(t) -> int:
    """Device pointer of a torch tensor (or a raw int address)."""
    return t if isinstance(t, int) else t.data_ptr()


def _stream(stream) -> int:
    if stream is None:
        import torch

        return torch.cuda.current_stream().cuda_stream
    return stream if isinstance(stream, int) else stream.cuda_stream


def _check_nan_missing(nan_missing: bool, **others) -> None:
    """nan_missing=True beside an explanation or partial-dependence option: refused here as the C creates refuse the flags."""
    bad = [k for k, v in others.items() if v]
    if nan_missing and bad:
        raise ValueError("nan_missing=True (TAHOE_CREATE_NAN_MISSING) does not combine with " + ", ".join(bad)
                         + ": those kernels do not implement the rule")


def _torch_col_types():
    import torch

    types = {torch.float32: COL_FLOAT32, torch.float64: COL_FLOAT64, torch.float16: COL_FLOAT16, torch.int8: COL_INT8,
             torch.int16: COL_INT16, torch.int32: COL_INT32, torch.int64: COL_INT64, torch.uint8: COL_UINT8, torch.bool: COL_UINT8}
    for name, code in (("uint16", COL_UINT16), ("uint32", COL_UINT32), ("uint64", COL_UINT64)):
        if hasattr(torch, name):
            types[getattr(torch, name)] = code
    return types


def _column_buffer(col, what: str):
    """(device pointer, elements, TAHOE_COL_* or None, device index or None, mask object or None) of a 1-D contiguous CUDA tensor
    or of an object with __cuda_array_interface__; ValueError for anything else"""
    import torch

    if isinstance(col, torch.Tensor):
        if col.dim() != 1:
            raise ValueError(f"{what} must be 1-D, got shape {tuple(col.shape)}")
        if not col.is_cuda or not col.is_contiguous():
            raise ValueError(f"{what} must be a contiguous CUDA tensor")
        return col.data_ptr(), col.numel(), _torch_col_types().get(col.dtype), col.device.index, None
    cai = getattr(col, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise ValueError(f"{what} must be a CUDA tensor or have __cuda_array_interface__, got {type(col).__name__}")
    shape = tuple(cai["shape"])
    if len(shape) != 1:
        raise ValueError(f"{what} must be 1-D, got shape {shape}")
    code = _COL_TYPESTR.get(cai["typestr"])
    strides = cai.get("strides")
    if strides is not None and shape[0] > 1 and code is not None and tuple(strides) != (_COL_SIZE[code],):
        raise ValueError(f"{what} must be contiguous, got strides {tuple(strides)}")
    return int(cai["data"][0] or 0), int(shape[0]), code, None, cai.get("mask")


class Table:
    """A device table of typed, nullable columns (tahoe_table_create) for Forest.predict_table: a cuDF / Arrow table as it is.
    columns: a sequence of 1-D contiguous CUDA tensors (float32 / float64 / float16, int8 .. int64, uint8, bool as uint8) or of
    objects with __cuda_array_interface__, whose typestr gives the type (so the unsigned 16 / 32 / 64-bit types come in) and whose
    optional `mask` entry the validity bitmap, as a cuDF Series publishes it.  validity: per column None (no nulls) or the bitmap's
    bytes (uint8, bit offset + i of the buffer, LSB first, 1 = valid); it overrides a mask.  offsets: per column the element the
    column starts at in its buffers (default 0); the column's rows are what follows it.  Everything malformed is a ValueError
    raised before the library is called.  The table keeps the buffers referenced; they may be rewritten in place between
    calls.  close() destroys it."""

    def __init__(self, columns, validity=None, offsets=None):
        import torch

        columns = list(columns)
        n = len(columns)
        validity = [None] * n if validity is None else list(validity)
        offsets = [0] * n if offsets is None else [int(o) for o in offsets]
        if len(validity) != n or len(offsets) != n:
            raise ValueError(f"{n} columns, {len(validity)} validity entries, {len(offsets)} offsets")
        desc = (Column * max(n, 1))()
        lengths, device = [], None
        for c, (col, off) in enumerate(zip(columns, offsets)):
            ptr, numel, code, dev, mask = _column_buffer(col, f"column {c}")
            if code is None:
                raise ValueError(f"column {c}: unsupported dtype {getattr(col, 'dtype', None) or col.__cuda_array_interface__['typestr']}")
            if off < 0 or off > numel:
                raise ValueError(f"column {c}: offset {off} outside its {numel} elements")
            if dev is not None and device is not None and dev != device:
                raise ValueError(f"column {c} is on device {dev}, earlier ones on device {device}")
            device = dev if dev is not None else device
            lengths.append(numel - off)
            vptr = None
            bitmap = validity[c] if validity[c] is not None else mask
            if bitmap is not None:
                vptr, vbytes, vcode, _, _ = _column_buffer(bitmap, f"validity of column {c}")
                if vcode not in (COL_UINT8, COL_INT8):
                    raise ValueError(f"validity of column {c} must be bytes (uint8)")
                need = (off + lengths[-1] + 7) // 8
                if vbytes < need:
                    raise ValueError(f"validity of column {c}: mask of {vbytes} bytes is shorter than the {need} bytes of "
                                     f"{off} + {lengths[-1]} bits")
            desc[c] = Column(ptr or None, vptr, off, code, 0)
        if len(set(lengths)) > 1:
            raise ValueError(f"columns of unequal lengths: {sorted(set(lengths))}")
        self.rows = lengths[0] if lengths else 0
        self.num_cols = n
        self.device = torch.device("cuda", device if device is not None else torch.cuda.current_device())
        self._keep = (columns, validity)
        self._h = _vp()
        with torch.cuda.device(self.device):
            _check(lib.tahoe_table_create(C.cast(desc, _vp), n, self.rows, C.byref(self._h)), "tahoe_table_create")

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.tahoe_table_destroy(self._h)
            self._h = _vp()

    __del__ = close


class Forest:
    """Handle on a device forest: tahoe_forest_create / predict / destroy.

    Mirrors the reference's init_dense* + predict_dense* pair (BaseTahoeTest.h:519-547, :599-611).
    Tensors are torch CUDA tensors (float32 data [rows, cols] contiguous, float32 preds [rows]).
    num_classes > 1 (tahoe_forest_create_multiclass): tree t belongs to class t % num_classes, predict / predict_raw
    return [rows, num_classes] and predict_leaf_idx [rows, num_trees] leaves with [rows, num_classes] sums.
    nan_missing=True (TAHOE_CREATE_NAN_MISSING): a NaN is a missing value beside the sentinel and takes the node's default branch,
    in every predict call; not together with contribs / approx_contribs.  TILEBLOCK and TILERING are then not served."""

    def __init__(self, nodes: np.ndarray, num_trees: int, depth: int, num_cols: int, missing: float = 0.0,
                 output: int = OUT_RAW, threshold: float = 0.0, global_bias: float = 0.0, algo: int = 0,
                 strategy: int = 0, relayout: bool = False, num_classes: int = 1, contribs: bool = False,
                 approx_contribs: bool = False, nan_missing: bool = False):
        _check_nan_missing(nan_missing, contribs=contribs, approx_contribs=approx_contribs)
        nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
        if nodes.size != num_trees * tree_num_nodes(depth):
            raise ValueError("nodes.size != num_trees * tree_num_nodes(depth)")
        self.params = ForestParams(0, depth, num_trees, num_cols, algo, output, threshold, global_bias, strategy,
                                   missing)
        self._h = _vp()
        flags = ((CREATE_PROB_RELAYOUT if relayout else 0) | (CREATE_CONTRIBS if contribs else 0)
                 | (CREATE_APPROX_CONTRIBS if approx_contribs else 0) | (CREATE_NAN_MISSING if nan_missing else 0))
        if num_classes != 1:
            _check(lib.tahoe_forest_create_multiclass(C.byref(self._h), nodes.ctypes.data if nodes.size else None,
                                                      C.byref(self.params), num_classes, flags),
                   "tahoe_forest_create_multiclass")
        elif flags:  # re-layout by dense_node_t.weight (Struct.h:1775-1825) and / or the contribution tables / node deltas
            _check(lib.tahoe_forest_create_ex(C.byref(self._h), nodes.ctypes.data if nodes.size else None,
                                              C.byref(self.params), flags), "tahoe_forest_create_ex")
        else:
            _check(lib.tahoe_forest_create(C.byref(self._h), nodes.ctypes.data if nodes.size else None,
                                           C.byref(self.params)), "tahoe_forest_create")
        self.num_trees, self.depth, self.num_cols = num_trees, depth, num_cols
        self.num_classes = lib.tahoe_forest_num_classes(self._h)

    def _out_shape(self, rows: int):
        return (rows, self.num_classes) if self.num_classes > 1 else (rows,)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.tahoe_forest_destroy(self._h)
            self._h = _vp()

    __del__ = close

    def _check_data(self, data):
        assert data.is_cuda and data.is_contiguous() and data.dtype.is_floating_point and data.element_size() == 4
        assert data.dim() == 2 and data.shape[1] == self.num_cols, (tuple(data.shape), self.num_cols)

    def predict(self, data, preds=None, stream=None):
        import torch

        self._check_data(data)
        rows = data.shape[0]
        if preds is None:
            preds = torch.empty(self._out_shape(rows), dtype=torch.float32, device=data.device)
        _check(lib.tahoe_forest_predict(self._h, _ptr(preds), _ptr(data), rows, _stream(stream)),
               "tahoe_forest_predict")
        return preds

    def predict_csr(self, indptr, indices=None, values=None, out=None, stream=None):
        """predict on rows given as CSR (tahoe_forest_predict_csr): an entry that is not stored is missing.  CUDA tensors indptr
        [rows + 1], indices [nnz], values [nnz] (cast to int64 / int32 / float32 where needed), or one torch.sparse_csr tensor
        of shape [rows, num_cols].  Bit for bit what predict returns for the densified rows."""
        import torch

        if indices is None and values is None:
            t = indptr
            assert t.layout == torch.sparse_csr and tuple(t.shape)[1] == self.num_cols, (t.layout, tuple(t.shape), self.num_cols)
            indptr, indices, values = t.crow_indices(), t.col_indices(), t.values()
        assert indptr.is_cuda and indices.is_cuda and values.is_cuda and indptr.dim() == 1 and indptr.numel() >= 1
        assert indices.dim() == 1 and values.dim() == 1 and indices.numel() == values.numel()
        indptr = indptr.to(torch.int64).contiguous()
        indices = indices.to(torch.int32).contiguous()
        values = values.to(torch.float32).contiguous()
        rows, nnz = indptr.numel() - 1, values.numel()
        if out is None:
            out = torch.empty(self._out_shape(rows), dtype=torch.float32, device=values.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == self._out_shape(rows)
        _check(lib.tahoe_forest_predict_csr(self._h, _ptr(out), _ptr(indptr), _ptr(indices) if nnz else None,
                                            _ptr(values) if nnz else None, rows, nnz, _stream(stream)), "tahoe_forest_predict_csr")
        return out

    def reserve_csr(self, rows: int, nnz: int) -> None:
        """Sizes the workspace of predict_csr for batches of up to `rows` rows and `nnz` entries (tahoe_forest_reserve_csr)."""
        _check(lib.tahoe_forest_reserve_csr(self._h, rows, nnz), "tahoe_forest_reserve_csr")

    def csr_plan(self, rows: int, nnz: int):
        """(kernel form name, rows per densified chunk; 0 = the fused CSR kernel) of a predict_csr of that size."""
        form, chunk = _i(), _sz()
        _check(lib.tahoe_forest_get_csr_plan(self._h, rows, nnz, C.byref(form), C.byref(chunk)), "tahoe_forest_get_csr_plan")
        return lib.tahoe_kernel_form_name(form.value).decode(), chunk.value

    def predict_columns(self, x, out=None, stream=None):
        """predict on a column-major batch, without a row-major copy.  x is a 2-D float32 CUDA tensor [rows, num_cols] with
        x.stride(0) == 1 and x.stride(1) >= rows (a Fortran-ordered array, `rowmajor.t()` of a [num_cols, rows] tensor:
        tahoe_forest_predict_columns), or a sequence of num_cols 1-D contiguous float32 CUDA tensors of one length (the columns
        of a cuDF / Arrow table, in any allocation: tahoe_forest_predict_column_ptrs).  Bit for bit what predict returns for
        the row-major matrix of the same values.  Anything else is a ValueError raised before the library is called."""
        import torch

        if isinstance(x, torch.Tensor):
            if x.dim() != 2 or x.shape[1] != self.num_cols:
                raise ValueError(f"x must be [rows, {self.num_cols}], got {tuple(x.shape)}")
            if x.dtype != torch.float32:
                raise ValueError(f"x must be float32, got {x.dtype}")
            rows = x.shape[0]
            if rows > 0 and self.num_cols > 0 and not ((rows == 1 or x.stride(0) == 1) and (self.num_cols == 1 or x.stride(1) >= rows)):
                raise ValueError(f"x must be column-major (stride(0) == 1, stride(1) >= rows), got strides {tuple(x.stride())}; "
                                 "a row-major tensor goes to predict")
            if not x.is_cuda:
                raise ValueError("x must be a CUDA tensor")
            cols, device = None, x.device
            stride = max(x.stride(1), rows) if self.num_cols > 1 else rows
        else:
            cols = list(x)
            if len(cols) != self.num_cols:
                raise ValueError(f"{len(cols)} columns given, the forest has {self.num_cols}")
            for c in cols:
                if not isinstance(c, torch.Tensor) or c.dim() != 1 or c.dtype != torch.float32:
                    raise ValueError("every column must be a 1-D float32 tensor")
            if len({c.numel() for c in cols}) > 1:
                raise ValueError(f"columns of unequal lengths: {sorted({c.numel() for c in cols})}")
            if any(not c.is_cuda or not c.is_contiguous() for c in cols):
                raise ValueError("every column must be a contiguous CUDA tensor")
            rows = cols[0].numel() if cols else 0
            device = cols[0].device if cols else torch.device("cuda", torch.cuda.current_device())
        if out is None:
            out = torch.empty(self._out_shape(rows), dtype=torch.float32, device=device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == self._out_shape(rows)
        if cols is None:
            _check(lib.tahoe_forest_predict_columns(self._h, _ptr(out), _ptr(x), rows, stride, _stream(stream)),
                   "tahoe_forest_predict_columns")
            return out
        # The int64 pointer table is built on the host and copied on the call's stream, so the kernels read it in stream order;
        # table and columns stay referenced until the call has been enqueued (the caching allocator keeps the table's memory
        # for that stream's work afterwards).  The copy reads host memory of this call: capture the strided form instead.
        if stream is None:
            s = torch.cuda.current_stream(device)
        else:
            s = torch.cuda.ExternalStream(stream, device=device) if isinstance(stream, int) else stream
        with torch.cuda.stream(s):
            table = torch.tensor([c.data_ptr() for c in cols], dtype=torch.int64).to(device)
        keep = (cols, table)
        _check(lib.tahoe_forest_predict_column_ptrs(self._h, _ptr(out), _ptr(table) if cols else None, rows, _stream(stream)),
               "tahoe_forest_predict_column_ptrs")
        del keep
        return out

    def reserve_columns(self, rows: int) -> None:
        """Sizes the workspace of predict_columns for batches of up to `rows` rows (tahoe_forest_reserve_columns)."""
        _check(lib.tahoe_forest_reserve_columns(self._h, rows), "tahoe_forest_reserve_columns")

    def columns_plan(self, rows: int):
        """(kernel form name, rows per transposed chunk; 0 = the kernel reads the columns itself) of a predict_columns of that
        size."""
        form, chunk = _i(), _sz()
        _check(lib.tahoe_forest_get_columns_plan(self._h, rows, C.byref(form), C.byref(chunk)), "tahoe_forest_get_columns_plan")
        return lib.tahoe_kernel_form_name(form.value).decode(), chunk.value

    def predict_table(self, table, out=None, stream=None):
        """predict on a Table of typed, nullable columns (tahoe_forest_predict_table): bit for bit what predict returns for the
        row-major float32 matrix with `missing` at every null and (float)element elsewhere.  Uploads nothing: capturable after
        reserve_table."""
        import torch

        if not isinstance(table, Table):
            raise ValueError(f"table must be a tahoe_amd Table, got {type(table).__name__}")
        if table.num_cols != self.num_cols:
            raise ValueError(f"the table has {table.num_cols} columns, the forest {self.num_cols}")
        if out is None:
            out = torch.empty(self._out_shape(table.rows), dtype=torch.float32, device=table.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == self._out_shape(table.rows)
        if table.rows == 0:
            return out  # (an empty tensor has no address to hand on; the library launches nothing for such a table either)
        _check(lib.tahoe_forest_predict_table(self._h, _ptr(out), table._h, _stream(stream)), "tahoe_forest_predict_table")
        return out

    def reserve_table(self, rows: int) -> None:
        """Sizes the workspace of predict_table for tables of up to `rows` rows (tahoe_forest_reserve_table)."""
        _check(lib.tahoe_forest_reserve_table(self._h, rows), "tahoe_forest_reserve_table")

    def table_plan(self, rows: int):
        """(kernel form name, rows per converted chunk; 0 = the quantise pass reads the table itself) of a predict_table of that
        size."""
        form, chunk = _i(), _sz()
        _check(lib.tahoe_forest_get_table_plan(self._h, rows, C.byref(form), C.byref(chunk)), "tahoe_forest_get_table_plan")
        return lib.tahoe_kernel_form_name(form.value).decode(), chunk.value

    def predict_raw(self, data, sums=None, stream=None):
        import torch

        self._check_data(data)
        rows = data.shape[0]
        if sums is None:
            sums = torch.empty(self._out_shape(rows), dtype=torch.float32, device=data.device)
        _check(lib.tahoe_forest_predict_raw(self._h, _ptr(sums), _ptr(data), rows, _stream(stream)),
               "tahoe_forest_predict_raw")
        return sums

    def predict_accumulate(self, data, sums, stream=None):
        """Continues the running float32 sums in `sums` (the trees before this forest) through this forest's trees,
        in place (tahoe_forest_predict_accumulate): the step of a chained, bit-exact tree-sharded predict."""
        self._check_data(data)
        assert sums.is_cuda and sums.is_contiguous() and sums.dtype.is_floating_point and sums.element_size() == 4
        assert sums.numel() == data.shape[0]
        _check(lib.tahoe_forest_predict_accumulate(self._h, _ptr(sums), _ptr(data), data.shape[0], _stream(stream)),
               "tahoe_forest_predict_accumulate")
        return sums

    def predict_leaf_idx(self, data, want_sums: bool = True, stream=None, leaf=None, sums=None):
        """-> (leaf int32 [rows, num_trees], sums float32 like predict_raw's, or None without want_sums).  leaf= / sums=:
        the caller's output tensors (sums= only with want_sums)."""
        import torch

        self._check_data(data)
        rows = data.shape[0]
        if leaf is None:
            leaf = torch.empty((rows, self.num_trees), dtype=torch.int32, device=data.device)
        assert leaf.is_cuda and leaf.is_contiguous() and leaf.dtype == torch.int32 and tuple(leaf.shape) == (rows, self.num_trees)
        assert sums is None or want_sums, "sums= given, but want_sums is False"
        if want_sums and sums is None:
            sums = torch.empty(self._out_shape(rows), dtype=torch.float32, device=data.device)
        if want_sums:
            assert sums.is_cuda and sums.is_contiguous() and sums.dtype == torch.float32
            assert tuple(sums.shape) == self._out_shape(rows)
        _check(lib.tahoe_forest_predict_leaf_idx(self._h, _ptr(leaf), _ptr(sums) if want_sums else None,
                                                 _ptr(data), rows, _stream(stream)),
               "tahoe_forest_predict_leaf_idx")
        return leaf, sums

    def set_stages(self, rounds) -> None:
        """Stages of predict_staged (tahoe_forest_set_stages): strictly ascending counts of boosting rounds in
        [1, num_trees / num_classes]; None clears them.  Synchronous; a second call replaces the stages."""
        if rounds is None:
            _check(lib.tahoe_forest_set_stages(self._h, None, 0), "tahoe_forest_set_stages")
            self.num_stages = 0
            return
        r = np.ascontiguousarray([int(v) for v in rounds], dtype=np.int32)
        _check(lib.tahoe_forest_set_stages(self._h, r.ctypes.data if r.size else None, int(r.size)), "tahoe_forest_set_stages")
        self.num_stages = int(r.size)

    def predict_staged(self, data, out=None, stream=None):
        """The output after the first rounds[s] boosting rounds, for every stage s of set_stages, in one walk
        (tahoe_forest_predict_staged): float32 [rows, S], or [rows, S, num_classes] on a multi-class handle; out[:, s] carries
        the bits of predict on a handle created from the first rounds[s] * num_classes trees."""
        import torch

        self._check_data(data)
        rows, S = data.shape[0], getattr(self, "num_stages", 0)
        shape = (rows, S) + ((self.num_classes,) if self.num_classes > 1 else ())
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=data.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == shape
        _check(lib.tahoe_forest_predict_staged(self._h, _ptr(out), _ptr(data), rows, _stream(stream)),
               "tahoe_forest_predict_staged")
        return out

    def staged_strategy(self, rows: int) -> int:
        """Strategy predict_staged runs for `rows` rows; 0 when it would be refused (tahoe_forest_get_staged_strategy)."""
        return lib.tahoe_forest_get_staged_strategy(self._h, rows)

    def _shap_out(self, name, data, k, out, stream):
        """The SHAP predict_* methods: runs the C function `name` into `out` (allocated if None), float32 [rows, num_cols + 1
        (k times)], or [rows, num_classes, ...] on a multi-class handle."""
        import torch

        self._check_data(data)
        rows = data.shape[0]
        shape = (rows,) + ((self.num_classes,) if self.num_classes > 1 else ()) + (self.num_cols + 1,) * k
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=data.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == shape
        _check(getattr(lib, name)(self._h, _ptr(out), _ptr(data), rows, _stream(stream)), name)
        return out

    def predict_contribs(self, data, out=None, stream=None):
        """Per-feature contributions (path-dependent TreeSHAP, tahoe_forest_predict_contribs): [rows, num_cols + 1] float32,
        or [rows, num_classes, num_cols + 1] on a multi-class handle; the bias is the last column.  Needs contribs=True."""
        return self._shap_out("tahoe_forest_predict_contribs", data, 1, out, stream)

    def predict_interactions(self, data, out=None, stream=None):
        """SHAP interaction values (tahoe_forest_predict_interactions): [rows, num_cols + 1, num_cols + 1] float32, or
        [rows, num_classes, num_cols + 1, num_cols + 1] on a multi-class handle; index num_cols is the bias.  Needs
        contribs=True (an ObliviousForest or a VectorForest: interactions=True)."""
        return self._shap_out("tahoe_forest_predict_interactions", data, 2, out, stream)

    def predict_contribs_approx(self, data, out=None, stream=None):
        """Saabas contributions (XGBoost approx_contribs, tahoe_forest_predict_contribs_approx): [rows, num_cols + 1] float32, or
        [rows, num_classes, num_cols + 1] on a multi-class handle ([rows, K, num_cols + 1] on a VectorForest with K > 1); the
        bias is the last column.  Needs approx_contribs=True."""
        return self._shap_out("tahoe_forest_predict_contribs_approx", data, 1, out, stream)

    def partial_dependence(self, features, grid, out=None, stream=None):
        """Partial dependence on the target columns `features` (tahoe_forest_predict_partial_dependence; scikit-learn's
        partial_dependence(method="recursion")): raw sums, float32 [G], or [G, num_classes] on a multi-class handle.  grid: a
        float32 CUDA tensor [G, len(features)], column j the value of features[j]; or a sequence of 1-D axes (tensors or arrays),
        one per feature, whose Cartesian product (first axis slowest) is the grid -- the result then has the shape axes...
        (, num_classes), scikit-learn's layout.  Needs a SparseForest with partial_dependence=True."""
        import torch

        feats = np.ascontiguousarray(np.asarray(features, dtype=np.int32).reshape(-1))
        nt = int(feats.size)
        axes_shape = None
        if not (torch.is_tensor(grid) and grid.dim() == 2) and not (isinstance(grid, np.ndarray) and grid.ndim == 2):
            axes = [torch.as_tensor(a, dtype=torch.float32).reshape(-1).cuda() for a in grid]
            assert len(axes) == nt, (len(axes), nt)
            axes_shape = tuple(int(a.numel()) for a in axes)
            grid = (torch.cartesian_prod(*axes).reshape(-1, nt) if nt else torch.empty((1, 0), dtype=torch.float32, device="cuda"))
        grid = torch.as_tensor(grid, dtype=torch.float32)
        grid = grid.cuda().contiguous() if not grid.is_cuda else grid.contiguous()
        assert grid.dim() == 2 and grid.shape[1] == nt, (tuple(grid.shape), nt)
        rows = grid.shape[0]
        shape = self._out_shape(rows)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=grid.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == int(np.prod(shape))
        _check(lib.tahoe_forest_predict_partial_dependence(self._h, _ptr(out), feats.ctypes.data if nt else None, nt,
                                                           _ptr(grid) if nt and rows else None, rows, _stream(stream)),
               "tahoe_forest_predict_partial_dependence")
        if axes_shape is not None:
            return out.reshape(axes_shape + ((self.num_classes,) if self.num_classes > 1 else ()))
        return out

    def set_background(self, bg, stream=None) -> None:
        """Background data set of interventional TreeSHAP (tahoe_forest_set_background): float32 [B, num_cols], contiguous, on
        the handle's device; None clears it.  Synchronous; the handle keeps what it needs, so `bg` may be freed afterwards.
        Needs contribs=True (a VectorForest or an ObliviousForest: interventional=True)."""
        if bg is None:
            _check(lib.tahoe_forest_set_background(self._h, None, 0, None), "tahoe_forest_set_background")
            return
        self._check_data(bg)
        _check(lib.tahoe_forest_set_background(self._h, _ptr(bg), bg.shape[0], _stream(stream)), "tahoe_forest_set_background")

    def predict_contribs_interventional(self, data, out=None, stream=None):
        """Interventional TreeSHAP against the background of set_background (tahoe_forest_predict_contribs_interventional):
        [rows, num_cols + 1] float32, or [rows, num_classes, num_cols + 1] on a multi-class handle ([rows, K, num_cols + 1] on a
        VectorForest or an ObliviousForest with leaf_dim K > 1); the bias is the last column.  Needs contribs=True (a VectorForest
        or an ObliviousForest: interventional=True) and a background."""
        return self._shap_out("tahoe_forest_predict_contribs_interventional", data, 1, out, stream)

    def set_strategy(self, strategy: int) -> None:
        _check(lib.tahoe_forest_set_strategy(self._h, strategy), "tahoe_forest_set_strategy")

    def get_strategy(self, rows: int) -> int:
        return lib.tahoe_forest_get_strategy(self._h, rows)

    def kernel_form(self, rows: int) -> str:
        """Name of the kernel form a predict of `rows` rows launches (TAHOE_FORM_*, include/tahoe_amd.h)."""
        return lib.tahoe_kernel_form_name(lib.tahoe_forest_get_kernel_form(self._h, rows)).decode()

    def reserve(self, rows: int) -> None:
        _check(lib.tahoe_forest_reserve(self._h, rows), "tahoe_forest_reserve")

    def predict_host(self, data: np.ndarray, preds: np.ndarray = None, chunk_rows: int = 0) -> np.ndarray:
        """Host-resident batch: chunked upload overlapped with the traversal (tahoe_forest_predict_host)."""
        if data.dtype != np.float32 or data.ndim != 2 or data.shape[1] != self.num_cols or not data.flags.c_contiguous:
            raise ValueError(f"data must be C-contiguous float32 [rows, {self.num_cols}]")
        if preds is None:
            preds = np.empty(data.shape[0], dtype=np.float32)
        if (not isinstance(preds, np.ndarray) or preds.dtype != np.float32 or preds.shape != (data.shape[0],)
                or not preds.flags.c_contiguous or not preds.flags.writeable):
            raise ValueError(f"preds must be a writeable C-contiguous float32 array of shape ({data.shape[0]},)")
        _check(lib.tahoe_forest_predict_host(self._h, preds.ctypes.data, data.ctypes.data, data.shape[0], chunk_rows),
               "tahoe_forest_predict_host")
        return preds

    def check(self, stream=None) -> None:
        """Waits for the stream; raises if a kernel flagged an internal error."""
        _check(lib.tahoe_forest_check(self._h, _stream(stream)), "tahoe_forest_check")

    def info(self) -> ForestInfo:
        info = ForestInfo()
        _check(lib.tahoe_forest_get_info(self._h, C.byref(info)), "tahoe_forest_get_info")
        return info

    def set_profiling(self, max_launches: int) -> None:
        _check(lib.tahoe_forest_set_profiling(self._h, int(max_launches)), "tahoe_forest_set_profiling")

    def kernel_times_ms(self, capacity: int = 4096) -> np.ndarray:
        """Durations (ms) of the traversal kernels launched since set_profiling; waits for them."""
        out = np.empty(capacity, dtype=np.float32)
        n = _i()
        _check(lib.tahoe_forest_kernel_times(self._h, out.ctypes.data, capacity, C.byref(n)),
               "tahoe_forest_kernel_times")
        return out[: n.value].copy()

    def prepass_times_ms(self, capacity: int = 4096) -> np.ndarray:
        """Durations (ms) of the pre-pass kernel (QRING's quantise kernel) of the same launches."""
        out = np.empty(capacity, dtype=np.float32)
        n = _i()
        _check(lib.tahoe_forest_prepass_times(self._h, out.ctypes.data, capacity, C.byref(n)),
               "tahoe_forest_prepass_times")
        return out[: n.value].copy()


# ---- sparse (irregular) forests ----
SPARSE_NODE_DTYPE = np.dtype([("val", "<f4"), ("bits", "<i4"), ("left_idx", "<i4")])  # sparse_node_t, Struct.h:50-54


def dense_to_sparse(nodes: np.ndarray, num_trees: int, depth: int, covers: bool = False):
    """dense2sparse (BaseTahoeTest.h:728-764) -> (sparse nodes, root offsets int32[num_trees]); with covers=True also the
    float32 covers[num_nodes] (the dense weights, tahoe_dense_to_sparse_ex) as a third element."""
    nodes = np.ascontiguousarray(nodes, dtype=NODE_DTYPE)
    pn, pt, pc, n = _vp(), _vp(), _vp(), _sz()
    if covers:
        _check(lib.tahoe_dense_to_sparse_ex(nodes.ctypes.data, num_trees, depth, C.byref(pn), C.byref(pt), C.byref(pc),
                                            C.byref(n)), "tahoe_dense_to_sparse_ex")
    else:
        _check(lib.tahoe_dense_to_sparse(nodes.ctypes.data, num_trees, depth, C.byref(pn), C.byref(pt), C.byref(n)),
               "tahoe_dense_to_sparse")
    try:
        sn = np.frombuffer((C.c_char * (n.value * 12)).from_address(pn.value), dtype=SPARSE_NODE_DTYPE, count=n.value).copy()
        tr = np.frombuffer((C.c_char * (num_trees * 4)).from_address(pt.value), dtype=np.int32, count=num_trees).copy() \
            if num_trees else np.empty(0, np.int32)
        cv = np.frombuffer((C.c_char * (n.value * 4)).from_address(pc.value), dtype=np.float32, count=n.value).copy() \
            if covers else None
    finally:
        lib.tahoe_free_host(pn)
        lib.tahoe_free_host(pt)
        if covers:
            lib.tahoe_free_host(pc)
    return (sn, tr, cv) if covers else (sn, tr)


def synth_sparse_forest(num_trees: int, num_cols: int, min_depth: int = 4, max_depth: int = 24, leaf_prob: float = 0.32,
                        max_tree_nodes: int = 65535, seed: int = 44):
    """BASELINE config 5 generator -> (sparse nodes, root offsets)."""
    n = _sz()
    _check(lib.tahoe_synth_sparse_forest(None, None, C.byref(n), num_trees, num_cols, min_depth, max_depth, leaf_prob,
                                         max_tree_nodes, seed), "tahoe_synth_sparse_forest")
    nodes = np.empty(n.value, dtype=SPARSE_NODE_DTYPE)
    trees = np.empty(num_trees, dtype=np.int32)
    _check(lib.tahoe_synth_sparse_forest(nodes.ctypes.data, trees.ctypes.data, C.byref(n), num_trees, num_cols, min_depth,
                                         max_depth, leaf_prob, max_tree_nodes, seed), "tahoe_synth_sparse_forest")
    return nodes, trees


def pack_categorical(categories, members_left=()):
    """(CategoricalSplits, arrays) for tahoe_sparse_forest_create_cat: categories = {node index: iterable of category ids >= 0},
    members_left = node indices whose members go left.  Each split's bitset is as many 32-bit words as its largest category
    needs (none for an empty set); `arrays` owns the memory the struct points to."""
    keys = sorted(int(k) for k in categories)
    node = np.array(keys, dtype=np.int32)
    sets = [np.unique(np.asarray(list(categories[k]), dtype=np.int64)) for k in keys]
    for k, c in zip(keys, sets):
        if c.size and (c[0] < 0 or c[-1] >= 1 << 24):
            raise ValueError(f"categories of node {k} must be in [0, 2^24)")
    nwords = [int(c[-1]) // 32 + 1 if c.size else 0 for c in sets]
    offset = np.zeros(len(keys) + 1, dtype=np.int32)
    offset[1:] = np.cumsum(nwords)
    words = np.zeros(max(int(offset[-1]), 1), dtype=np.uint32)
    for k, c in enumerate(sets):
        np.bitwise_or.at(words, offset[k] + c // 32, (np.uint32(1) << (c % 32).astype(np.uint32)))
    left = set(int(k) for k in members_left)
    if not left <= set(keys):
        raise ValueError("members_left names a node without categories")
    ml = np.array([k in left for k in keys], dtype=np.uint8) if left else None
    arrays = (node, offset, words, ml)
    cats = CategoricalSplits(len(keys), node.ctypes.data if node.size else None, offset.ctypes.data, words.ctypes.data,
                             ml.ctypes.data if ml is not None else None)
    return cats, arrays


class SparseForest(Forest):
    """tahoe_sparse_forest_create: nodes[SPARSE_NODE_DTYPE] + root offsets; predict* as Forest.  covers (float32, one per
    node), num_classes, contribs and approx_contribs go through tahoe_sparse_forest_create_ex: tree t belongs to class
    t % num_classes, contribs=True builds the TreeSHAP path tables from the covers and approx_contribs=True the Saabas node
    deltas.  categories ({node index: category ids}) makes those nodes categorical splits, members going right unless the
    node is in members_left (tahoe_sparse_forest_create_cat; the node's val is then ignored).  categories together with
    contribs / approx_contribs sets TAHOE_CREATE_CAT_CONTRIBS: the four explanation calls then follow the category sets.
    partial_dependence=True (TAHOE_CREATE_PARTIAL_DEPENDENCE; needs covers) serves Forest.partial_dependence.
    nan_missing=True (TAHOE_CREATE_NAN_MISSING): as Forest's, under every strategy; at a categorical split a NaN then takes the
    default branch; not together with contribs / approx_contribs / partial_dependence.  A forest from dense_to_sparse gets the
    rule here."""

    def __init__(self, nodes: np.ndarray, trees: np.ndarray, num_cols: int, missing: float = 0.0, output: int = OUT_RAW,
                 threshold: float = 0.0, global_bias: float = 0.0, covers=None, num_classes: int = 1,
                 contribs: bool = False, approx_contribs: bool = False, categories=None, members_left=(),
                 partial_dependence: bool = False, nan_missing: bool = False):
        _check_nan_missing(nan_missing, contribs=contribs, approx_contribs=approx_contribs, partial_dependence=partial_dependence)
        nodes = np.ascontiguousarray(nodes, dtype=SPARSE_NODE_DTYPE)
        trees = np.ascontiguousarray(trees, dtype=np.int32)
        self.params = ForestParams(int(nodes.size), 0, int(trees.size), num_cols, 0, output, threshold, global_bias, 0,
                                   missing)
        self._h = _vp()
        flags = (CREATE_CONTRIBS if contribs else 0) | (CREATE_APPROX_CONTRIBS if approx_contribs else 0)
        shap_flags = flags
        flags |= (CREATE_PARTIAL_DEPENDENCE if partial_dependence else 0) | (CREATE_NAN_MISSING if nan_missing else 0)
        if categories:
            cv = None if covers is None else np.ascontiguousarray(covers, dtype=np.float32)
            if cv is not None and cv.size != nodes.size:
                raise ValueError("covers.size != nodes.size")
            cats, _keep = pack_categorical(categories, members_left)
            if shap_flags:  # the path elements / the Saabas walk then test category sets
                flags |= CREATE_CAT_CONTRIBS
            _check(lib.tahoe_sparse_forest_create_cat(C.byref(self._h), trees.ctypes.data if trees.size else None,
                                                      nodes.ctypes.data if nodes.size else None,
                                                      cv.ctypes.data if cv is not None else None,
                                                      C.byref(self.params), num_classes, flags, C.byref(cats)),
                   "tahoe_sparse_forest_create_cat")
        elif covers is not None or num_classes != 1 or flags:
            cv = None if covers is None else np.ascontiguousarray(covers, dtype=np.float32)
            if cv is not None and cv.size != nodes.size:
                raise ValueError("covers.size != nodes.size")
            _check(lib.tahoe_sparse_forest_create_ex(C.byref(self._h), trees.ctypes.data if trees.size else None,
                                                     nodes.ctypes.data if nodes.size else None,
                                                     cv.ctypes.data if cv is not None else None,
                                                     C.byref(self.params), num_classes, flags),
                   "tahoe_sparse_forest_create_ex")
        else:
            _check(lib.tahoe_sparse_forest_create(C.byref(self._h), trees.ctypes.data if trees.size else None,
                                                  nodes.ctypes.data if nodes.size else None, C.byref(self.params)),
                   "tahoe_sparse_forest_create")
        self.num_trees, self.depth, self.num_cols = int(trees.size), 0, num_cols
        self.num_classes = lib.tahoe_forest_num_classes(self._h)


# ---- oblivious (symmetric) forests: CatBoost models ----
OBLIVIOUS_SPLIT_DTYPE = np.dtype([("thr", "<f4"), ("bits", "<i4")])  # tahoe_oblivious_split


def strict_borders(b) -> np.ndarray:
    """Thresholds for CatBoost borders: CatBoost goes right iff x > border, this library iff x >= thr, and for every x that is
    not NaN x > border <=> x >= nextafter(float32(border), +inf)."""
    with np.errstate(over="ignore"):  # FLT_MAX -> +inf is meant
        return np.nextafter(np.asarray(b, dtype=np.float32), np.float32(np.inf))


class ObliviousForest(Forest):
    """tahoe_oblivious_forest_create: trees whose levels share one split each.  depths [T] (0 .. 16); fids, thresholds and
    def_left hold sum(depths) entries, tree-major, level 0 first; leaf_values holds sum(2 ** depths) * leaf_dim floats (tree,
    leaf index, then the leaf_dim values); level l sets bit l of the leaf index.  predict* as Forest, with leaf_dim > 1 in the
    shapes of a multi-class handle ([rows, leaf_dim]); AVG divides by the number of trees.  contribs=True / approx_contribs=True /
    interactions=True (tahoe_oblivious_forest_create_ex) serve predict_contribs / predict_contribs_approx / predict_interactions,
    each its own call only, and need leaf_covers: sum(2 ** depths) floats, the training weight of every leaf (CatBoost's
    leaf_weights); zeros are allowed.  interventional=True (TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL) serves set_background and
    predict_contribs_interventional; alone it needs no leaf_covers.  categories ({split index: category ids}, the index running
    over the flattened (tree, level) records) makes those levels category-set splits, members going right unless the index is in
    members_left (tahoe_oblivious_forest_create_cat; the level's threshold is then ignored); every call above follows the sets.
    staged=True (TAHOE_CREATE_STAGED; needs no leaf_covers) serves set_stages, predict_staged and staged_strategy: the outputs after
    the first rounds[s] trees, [rows, S] for leaf_dim == 1 and [rows, S, leaf_dim] otherwise (CatBoost's staged_predict).
    csr=True (TAHOE_CREATE_CSR; needs no leaf_covers) serves predict_csr, reserve_csr and csr_plan (a sparse Pool's rows)."""

    def __init__(self, depths, fids, thresholds, def_left, leaf_values, num_cols: int, leaf_dim: int = 1, missing: float = 0.0,
                 output: int = OUT_RAW, threshold: float = 0.5, global_bias: float = 0.0, leaf_covers=None, contribs: bool = False,
                 approx_contribs: bool = False, interactions: bool = False, interventional: bool = False, categories=None,
                 members_left=(), staged: bool = False, csr: bool = False):
        depths = np.ascontiguousarray(depths, dtype=np.int32).reshape(-1)
        fids = np.asarray(fids, dtype=np.int64).reshape(-1)
        nsplits = int(depths.astype(np.int64).sum())
        if not (fids.size == nsplits == np.size(thresholds) == np.size(def_left)):
            raise ValueError("fids, thresholds and def_left must hold sum(depths) entries")
        if fids.size and (fids.min() < 0 or fids.max() >= 1 << 30):
            raise ValueError("fids must be in [0, 2^30)")
        splits = np.empty(max(nsplits, 1), dtype=OBLIVIOUS_SPLIT_DTYPE)
        splits["thr"][:nsplits] = np.asarray(thresholds, dtype=np.float32).reshape(-1)
        splits["bits"][:nsplits] = (fids | (np.asarray(def_left).reshape(-1).astype(bool).astype(np.int64) << 30)).astype(np.int32)
        leaves = np.ascontiguousarray(leaf_values, dtype=np.float32).reshape(-1)
        if bool(((depths >= 0) & (depths <= 16)).all()) and leaf_dim >= 1:  # (else the C function refuses with its own text)
            if leaves.size != int((np.int64(1) << depths.astype(np.int64)).sum()) * leaf_dim:
                raise ValueError("leaf_values.size != sum(2 ** depths) * leaf_dim")
        dp = depths if depths.size else np.zeros(1, np.int32)  # (the C function refuses NULL arrays, also for no trees)
        lv = leaves if leaves.size else np.zeros(1, np.float32)
        self.params = ForestParams(0, 0, int(depths.size), num_cols, 0, output, threshold, global_bias, 0, missing)
        self._h = _vp()
        flags = ((CREATE_CONTRIBS if contribs else 0) | (CREATE_APPROX_CONTRIBS if approx_contribs else 0)
                 | (CREATE_INTERACTIONS if interactions else 0))
        if flags or interventional or categories or staged or csr:
            cv = None
            if flags:
                if leaf_covers is None:
                    raise ValueError("contribs / approx_contribs / interactions need leaf_covers")
                covers = np.ascontiguousarray(leaf_covers, dtype=np.float32).reshape(-1)
                if covers.size * leaf_dim != leaves.size:
                    raise ValueError("leaf_covers.size != sum(2 ** depths)")
                cv = covers if covers.size else np.zeros(1, np.float32)
            flags |= ((CREATE_OBLIVIOUS_INTERVENTIONAL if interventional else 0) | (CREATE_STAGED if staged else 0)
                      | (CREATE_CSR if csr else 0))
            if categories:
                cats, _keep = pack_categorical(categories, members_left)
                _check(lib.tahoe_oblivious_forest_create_cat(C.byref(self._h), dp.ctypes.data, splits.ctypes.data if nsplits else None,
                                                             lv.ctypes.data, None if cv is None else cv.ctypes.data,
                                                             C.byref(self.params), leaf_dim, flags, C.byref(cats)),
                       "tahoe_oblivious_forest_create_cat")
            else:
                _check(lib.tahoe_oblivious_forest_create_ex(C.byref(self._h), dp.ctypes.data, splits.ctypes.data if nsplits else None,
                                                            lv.ctypes.data, None if cv is None else cv.ctypes.data,
                                                            C.byref(self.params), leaf_dim, flags),
                       "tahoe_oblivious_forest_create_ex")
        else:
            _check(lib.tahoe_oblivious_forest_create(C.byref(self._h), dp.ctypes.data, splits.ctypes.data if nsplits else None,
                                                     lv.ctypes.data, C.byref(self.params), leaf_dim), "tahoe_oblivious_forest_create")
        self.num_trees, self.depth, self.num_cols = int(depths.size), int(depths.max()) if depths.size else 0, num_cols
        self.num_classes = lib.tahoe_forest_num_classes(self._h)


# ---- vector-leaf forests: irregular trees whose leaves hold leaf_dim values ----
class VectorForest(Forest):
    """tahoe_vector_forest_create: nodes[SPARSE_NODE_DTYPE] + root offsets as SparseForest takes them, except that a leaf's
    left_idx is the index of its vector in leaf_values ([L, K], or flat with leaf_dim given) and its val is ignored.  Leaves may
    share a vector.  predict* as Forest: [rows] for K == 1, [rows, K] otherwise; AVG divides by the number of trees; leaf
    indices are relative to the tree's root, as on a SparseForest.  covers (float32, one per node; scikit-learn's
    tree_.weighted_n_node_samples) and contribs=True go through tahoe_vector_forest_create_ex: predict_contribs then gives the
    TreeSHAP values of every output, [rows, K, num_cols + 1] ([rows, num_cols + 1] for K == 1).  interventional=True
    (TAHOE_CREATE_INTERVENTIONAL) serves set_background and predict_contribs_interventional in the same shape; alone it needs no
    covers.  interactions=True (TAHOE_CREATE_CONTRIBS | TAHOE_CREATE_VECTOR_INTERACTIONS; needs covers) serves predict_contribs and
    predict_interactions, [rows, K, num_cols + 1, num_cols + 1] ([rows, num_cols + 1, num_cols + 1] for K == 1).
    approx_contribs=True (TAHOE_CREATE_VECTOR_APPROX; needs covers, checks no path length) serves predict_contribs_approx: the
    Saabas contributions of every output, what treeinterpreter computes for a scikit-learn forest, in predict_contribs' shape.
    staged=True (TAHOE_CREATE_STAGED; needs no covers) serves set_stages, predict_staged and staged_strategy: the outputs after the
    first rounds[s] trees, [rows, S] for K == 1 and [rows, S, K] otherwise (XGBoost's iteration_range, a forest's error curve).
    csr=True (TAHOE_CREATE_CSR; needs no covers) serves predict_csr, reserve_csr and csr_plan (a forest fit on a scipy CSR matrix)."""

    def __init__(self, nodes: np.ndarray, trees: np.ndarray, leaf_values, num_cols: int, leaf_dim: int = None,
                 missing: float = 0.0, output: int = OUT_RAW, threshold: float = 0.5, global_bias: float = 0.0, covers=None,
                 contribs: bool = False, interventional: bool = False, interactions: bool = False,
                 approx_contribs: bool = False, staged: bool = False, csr: bool = False):
        nodes = np.ascontiguousarray(nodes, dtype=SPARSE_NODE_DTYPE)
        trees = np.ascontiguousarray(trees, dtype=np.int32).reshape(-1)
        lv = np.asarray(leaf_values, dtype=np.float32)
        if leaf_dim is None:
            if lv.ndim != 2:
                raise ValueError("leaf_values must be [L, K], or flat with leaf_dim given")
            leaf_dim = int(lv.shape[1])
        elif lv.ndim == 2 and lv.shape[1] != leaf_dim:
            raise ValueError(f"leaf_values.shape[1] = {lv.shape[1]} != leaf_dim = {leaf_dim}")
        elif lv.ndim > 2:
            raise ValueError("leaf_values must be [L, K], or flat with leaf_dim given")
        leaves = np.ascontiguousarray(lv).reshape(-1)
        if leaf_dim >= 1 and leaves.size % leaf_dim != 0:  # (leaf_dim < 1: the C function refuses with its own text)
            raise ValueError(f"leaf_values.size = {leaves.size} is no multiple of leaf_dim = {leaf_dim}")
        num_vectors = leaves.size // leaf_dim if leaf_dim >= 1 else 0
        self.params = ForestParams(int(nodes.size), 0, int(trees.size), num_cols, 0, output, threshold, global_bias, 0, missing)
        self._h = _vp()
        flags = ((CREATE_CONTRIBS if contribs else 0) | (CREATE_INTERVENTIONAL if interventional else 0)
                 | (CREATE_CONTRIBS | CREATE_VECTOR_INTERACTIONS if interactions else 0)
                 | (CREATE_VECTOR_APPROX if approx_contribs else 0) | (CREATE_STAGED if staged else 0)
                 | (CREATE_CSR if csr else 0))
        if covers is not None or flags:
            cv = None if covers is None else np.ascontiguousarray(covers, dtype=np.float32).reshape(-1)
            if cv is not None and cv.size != nodes.size:
                raise ValueError("covers.size != nodes.size")
            _check(lib.tahoe_vector_forest_create_ex(C.byref(self._h), trees.ctypes.data if trees.size else None,
                                                     nodes.ctypes.data if nodes.size else None,
                                                     leaves.ctypes.data if leaves.size else None, num_vectors,
                                                     cv.ctypes.data if cv is not None else None, C.byref(self.params),
                                                     leaf_dim, flags),
                   "tahoe_vector_forest_create_ex")
        else:
            _check(lib.tahoe_vector_forest_create(C.byref(self._h), trees.ctypes.data if trees.size else None,
                                                  nodes.ctypes.data if nodes.size else None,
                                                  leaves.ctypes.data if leaves.size else None, num_vectors, C.byref(self.params),
                                                  leaf_dim), "tahoe_vector_forest_create")
        self.num_trees, self.depth, self.num_cols = int(trees.size), 0, num_cols
        self.num_classes = lib.tahoe_forest_num_classes(self._h)


def transform_preds(preds, output: int, num_trees_total: int, threshold: float, global_bias: float, stream=None):
    _check(lib.tahoe_transform_preds(_ptr(preds), preds.numel(), output, num_trees_total, threshold, global_bias,
                                     _stream(stream)), "tahoe_transform_preds")
    return preds
