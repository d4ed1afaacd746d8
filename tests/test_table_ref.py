"""tests/table_ref.py on its own, without a GPU: hand-written bitmaps and the conversions at the edges of float32."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_ref  # noqa: E402

S = np.float32(-999.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_hand_written_bitmaps():
    col = np.arange(10, dtype=np.int32)
    # bits 0..9, LSB first: 0b10110101 -> rows 0, 2, 4, 5, 7 valid; second byte 0b01 -> row 8 valid, row 9 null
    m = table_ref.materialise([col], [np.array([0b10110101, 0b01], np.uint8)], [0], S)
    assert m.shape == (10, 1) and m.dtype == np.float32
    assert m[:, 0].tolist() == [0, S, 2, S, 4, 5, S, 7, 8, S]
    # the same buffers from offset 3: rows are elements 3..9, bits 3..9
    m = table_ref.materialise([col], [np.array([0b10110101, 0b01], np.uint8)], [3], S)
    assert m[:, 0].tolist() == [S, 4, 5, S, 7, 8, S]
    # offset 8: the second byte alone
    m = table_ref.materialise([col], [np.array([0x00, 0b10], np.uint8)], [8], S)
    assert m[:, 0].tolist() == [S, 9]
    # no bitmap: every row valid; two columns with different offsets
    m = table_ref.materialise([col, np.arange(12, dtype=np.float64)], [None, None], [0, 2], S)
    assert m[:, 0].tolist() == list(range(10)) and m[:, 1].tolist() == list(range(2, 12))
    # what lies under a null does not show
    f = np.array([np.nan, np.inf, 1.0], np.float64)
    assert table_ref.materialise([f], [np.array([0b100], np.uint8)], [0], S)[:, 0].tolist() == [S, S, 1.0]


def test_pack_validity_round_trip():
    rng = np.random.default_rng(1)
    for off in (0, 1, 7, 8, 13, 67):
        for n in (1, 7, 8, 9, 63, 64, 65):
            valid = rng.random(n) < 0.5
            for garbage in (0, 1):
                v = table_ref.pack_validity(valid, off, before=garbage, after=garbage, pad_bytes=1)
                assert v.dtype == np.uint8 and v.size == (off + n + 7) // 8 + 1
                got = np.unpackbits(v, bitorder="little")
                assert np.array_equal(got[off: off + n].astype(bool), valid)
                assert np.all(got[:off] == garbage) and np.all(got[off + n:] == garbage)


def test_conversions_at_the_edges():
    def one(values, dtype):
        return table_ref.materialise([np.array(values, dtype=dtype)], [None], [0], S)[:, 0]

    # 2^24 + 1 is the first integer float32 cannot hold: ties to even, down to 2^24; 2^24 + 3 ties up to 2^24 + 4
    for dtype in (np.int32, np.int64):
        assert one([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1)], dtype).tolist() == [2.0 ** 24, 2.0 ** 24 + 4, -(2.0 ** 24)]
    assert one([np.iinfo(np.int64).min, np.iinfo(np.int64).max], np.int64).tolist() == [-(2.0 ** 63), 2.0 ** 63]
    assert one([np.iinfo(np.uint64).max], np.uint64).tolist() == [2.0 ** 64]
    assert one([np.iinfo(np.uint32).max, 0], np.uint32).tolist() == [2.0 ** 32, 0.0]
    assert one([np.iinfo(np.int32).min], np.int32).tolist() == [-(2.0 ** 31)]
    assert one([-128, 127], np.int8).tolist() == [-128.0, 127.0] and one([255], np.uint8).tolist() == [255.0]
    # float64: overflow to +-inf, NaN stays NaN, a float32 subnormal result is kept (not flushed), below half the least one -> 0
    f = one([1e300, -1e300, np.nan, 1e-40, 1e-46, -0.0], np.float64)
    assert f[0] == np.inf and f[1] == -np.inf and np.isnan(f[2])
    assert bits(f[3:4])[0] == bits(np.array([1e-40], np.float32))[0] and 0 < f[3] < np.finfo(np.float32).tiny
    assert bits(f[4:5])[0] == 0 and bits(f[5:6])[0] == 0x80000000  # +0.0 and -0.0
    # float16 subnormals are exact in float32; -0.0 keeps its sign
    h = np.array([6e-8, 5.96e-8, -0.0, 65504.0], np.float16)
    got = one(h, np.float16)
    assert got[0] == 2.0 ** -24 and got[1] == 2.0 ** -24 and bits(got[2:3])[0] == 0x80000000 and got[3] == 65504.0
    # float32 passes bit for bit, a NaN's payload included
    raw = np.array([0x7FC12345, 0x80000000, 0x00000001, 0xFF800000], np.uint32).view(np.float32)
    assert np.array_equal(bits(one(raw, np.float32)), raw.view(np.uint32))
