"""The row-major float32 matrix a typed, nullable table stands for (tahoe_forest_predict_table), in numpy:
the reference of tests/test_table_gpu.py, checked on its own by tests/test_table_ref.py.  Test infrastructure, not product.

materialise(columns, validity, offsets, missing): columns[c] is the numpy array of column c's whole data buffer (any of the served
dtypes), validity[c] None or the bitmap's bytes (uint8, bit i of the buffer LSB first, 1 = valid), offsets[c] the element the
column starts at in both buffers.  M[r][c] = missing where bit offsets[c] + r is 0, else float32(columns[c][offsets[c] + r]) by
numpy's astype -- C's conversion: round to nearest even, float64 overflow to +-inf, subnormal results kept.
"""
import numpy as np

DTYPES = ("float32", "float64", "float16", "int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64")


def pack_validity(valid, offset=0, before=0, after=0, pad_bytes=0):
    """The bitmap bytes for the booleans `valid` starting at bit `offset`; the bits before the offset are `before` (0 or 1), the
    bits behind the last row up to the end of the last byte -- and pad_bytes further bytes -- are `after`"""
    valid = np.asarray(valid, dtype=bool)
    n = offset + valid.size
    total = (n + 7) // 8 * 8 + 8 * pad_bytes
    bits = np.full(total, bool(after), dtype=bool)
    bits[:offset] = bool(before)
    bits[offset:n] = valid
    return np.packbits(bits, bitorder="little")


def materialise(columns, validity, offsets, missing):
    rows = {len(c) - o for c, o in zip(columns, offsets)}
    assert len(rows) <= 1, f"columns of unequal lengths: {sorted(rows)}"
    rows = rows.pop() if rows else 0
    out = np.empty((rows, len(columns)), dtype=np.float32)
    for c, (col, v, off) in enumerate(zip(columns, validity, offsets)):
        col = np.asarray(col)
        assert col.dtype.name in DTYPES and col.ndim == 1, col.dtype
        with np.errstate(over="ignore", invalid="ignore"):
            vals = col[off: off + rows].astype(np.float32)
        if v is not None:
            v = np.asarray(v, dtype=np.uint8)
            assert v.size >= (off + rows + 7) // 8, "bitmap shorter than offset + rows bits"
            valid = np.unpackbits(v, bitorder="little")[off: off + rows].astype(bool)
            vals = np.where(valid, vals, np.float32(missing))
        out[:, c] = vals
    return out
