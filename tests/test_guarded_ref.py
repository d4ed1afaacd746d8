"""tests/guarded.py on torch CPU tensors and numpy arrays: planted writes are caught and named, clean runs pass, interiors are
aligned and contiguous.  CPU only.  This file is the only demonstration that the harness catches an overrun; no kernel is
broken on a GPU to show it."""
import numpy as np
import pytest
import torch

import guarded
from guarded import GUARD_F32, Guarded

BACKENDS = [("torch", torch), ("numpy", np)]
# [n], [n, C], [n, S, C], [n, T] (int32 leaves) and [0, C]
SHAPES = [((65,), "float32"), ((65, 3), "float32"), ((5, 4, 9), "float32"), ((7, 37), "int32"), ((0, 3), "float32")]


def make(xp, shape, dtype="float32", **kw):
    return Guarded(xp, shape, getattr(xp, dtype), **kw)


def poke(g, flat_index, value):
    """Writes one element of the flat buffer, as a stray store would."""
    g.flat[flat_index] = value


@pytest.mark.parametrize("xp", [b[1] for b in BACKENDS], ids=[b[0] for b in BACKENDS])
@pytest.mark.parametrize("shape,dtype", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_interiors_are_aligned_contiguous_and_of_the_callers_shape(xp, shape, dtype):
    g = make(xp, shape, dtype)
    assert tuple(g.view.shape) == shape and g.contiguous and g.aligned
    width = int(np.prod(shape[1:]))
    assert g.lead == g.tail and g.lead % 64 == 0 and g.lead >= 384 * width and g.lead - 384 * width < 64
    assert g.flat.shape[0] == g.lead + g.n + g.tail
    got = g.check("clean")  # a buffer nobody wrote passes
    assert got.shape == shape and got.dtype == np.dtype(dtype)
    word = guarded.GUARD_WORD[dtype]
    assert np.all(got.reshape(-1).view(np.uint32) == np.uint32(word))  # the interior starts out as guard too
    if dtype == "float32":
        assert word == int(np.array([-12345.678], np.float32).view(np.uint32)[0])
    else:
        assert word == 0xA5A5A5A5


@pytest.mark.parametrize("xp", [b[1] for b in BACKENDS], ids=[b[0] for b in BACKENDS])
def test_a_clean_run_passes_and_returns_what_was_written(xp):
    g = make(xp, (65, 3))
    vals = np.arange(195, dtype=np.float32).reshape(65, 3)
    g.view[...] = torch.from_numpy(vals) if g.is_torch else vals  # the "kernel" writes exactly its rows
    assert np.array_equal(g.check("clean"), vals)
    g.load(vals * 2)
    assert np.array_equal(g.check_unchanged("clean input"), vals * 2)


@pytest.mark.parametrize("xp", [b[1] for b in BACKENDS], ids=[b[0] for b in BACKENDS])
def test_planted_writes_are_reported_with_their_position(xp):
    C = 3
    cases = [
        # flat index relative to the interior's start / end, text the message must carry
        ("before", -1, "element 1 before the interior: (rows before the buffer) = 1, column 2"),
        ("far-before", None, "(rows before the buffer) = 384, column 0"),
        ("after", 0, "(row past the batch, column) = (0, 0)"),
        ("after-row1", C + 1, "(row past the batch, column) = (1, 1)"),
        ("far-after", None, "element"),
    ]
    for name, rel, text in cases:
        g = make(xp, (65, C))
        if name in ("before",):
            idx = g.lead + rel
        elif name == "far-before":
            idx = g.lead - 384 * C  # first column of the 384th row in front
            assert idx >= 0
        elif name == "far-after":
            idx = g.lead + g.n + g.tail - 1
            k = g.tail - 1
            text = f"(row past the batch, column) = ({k // C}, {k % C})"
        else:
            idx = g.lead + g.n + rel
        poke(g, idx, 1.5)
        with pytest.raises(AssertionError) as e:
            g.check(name)
        assert text in str(e.value) and name in str(e.value), str(e.value)
    # the very first word of the lead band, whatever the rounding made of it
    g = make(xp, (65, C))
    poke(g, 0, 0.0)
    with pytest.raises(AssertionError) as e:
        g.check("first word")
    assert f"element {g.lead} before the interior" in str(e.value)


@pytest.mark.parametrize("xp", [b[1] for b in BACKENDS], ids=[b[0] for b in BACKENDS])
def test_flat_and_int32_buffers_report_positions_too(xp):
    g = make(xp, (10,))
    poke(g, g.lead + g.n + 5, 0.0)
    with pytest.raises(AssertionError) as e:
        g.check("flat")
    assert "(row past the batch, column) = (5, 0)" in str(e.value)
    T = 37
    g = make(xp, (7, T), "int32")
    poke(g, g.lead + g.n + 2 * T + 4, 3)  # a plausible leaf index two rows past the batch
    with pytest.raises(AssertionError) as e:
        g.check("leaf")
    assert "(row past the batch, column) = (2, 4)" in str(e.value) and "0x3 " in str(e.value)
    g = make(xp, (0, 3))
    poke(g, g.lead, 1.0)  # no interior: the first element of the tail band
    with pytest.raises(AssertionError) as e:
        g.check("empty")
    assert "(row past the batch, column) = (0, 0)" in str(e.value)


@pytest.mark.parametrize("xp", [b[1] for b in BACKENDS], ids=[b[0] for b in BACKENDS])
def test_the_compare_is_on_bits(xp):
    nxt = np.nextafter(GUARD_F32, np.float32(0))  # the next float: one ulp, no NaN anywhere
    assert nxt != GUARD_F32 and np.isclose(nxt, GUARD_F32, rtol=1e-6, atol=0)
    for idx_of in (lambda g: g.lead - 1, lambda g: g.lead + g.n):
        g = make(xp, (65, 3))
        poke(g, idx_of(g), float(nxt))
        with pytest.raises(AssertionError):
            g.check("one ulp")
    # a read-modify-write that adds 0.0f onto the guard gives the guard's own bits back and is not seen: the stated hole
    g = make(xp, (65, 3))
    poke(g, g.lead + g.n, float(GUARD_F32 + np.float32(0.0)))
    g.check("guard + 0.0f")


@pytest.mark.parametrize("xp", [b[1] for b in BACKENDS], ids=[b[0] for b in BACKENDS])
def test_a_changed_input_is_reported(xp):
    vals = np.linspace(-1, 1, 65 * 3, dtype=np.float32).reshape(65, 3)
    vals[3, 1] = np.nan  # NaN inputs compare equal to themselves by bits
    g = guarded.guarded_input(xp, vals, xp.float32)
    g.check_unchanged("untouched")
    g.view[64, 2] = 7.0
    with pytest.raises(AssertionError) as e:
        g.check_unchanged("input")
    assert "changed its input" in str(e.value) and "(64, 2)" in str(e.value)
    ip = guarded.guarded_input(xp, np.arange(66, dtype=np.int64), xp.int64)  # CSR indptr
    assert ip.aligned and ip.contiguous
    ip.check_unchanged("indptr")
    poke(ip, ip.lead + ip.n, 0)
    with pytest.raises(AssertionError):
        ip.check_unchanged("indptr")


def test_the_band_can_be_raised():
    g = make(np, (5, 2), band_rows=1024)
    assert g.lead >= 2048 and g.aligned
