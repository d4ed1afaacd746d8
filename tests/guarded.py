"""Guard-band buffers: test infrastructure, not product.  A Guarded holds one flat allocation of lead + n + tail elements, the
interior (what the library is handed, as a contiguous tensor or array of the caller's shape) between two bands filled with a
guard pattern; check() compares every word of both bands with the pattern by bits and names the first one that changed.  The
bands are band_rows rows wide, 384 by default: the largest row tile of any kernel form, so a write-out that lost its row mask
lands in memory the test owns.  Both bands are rounded up to 64 elements and the flat buffer is cut from its allocation at a
256-byte boundary, so the interior starts 256-byte aligned; misaligned pointers are not tested, the header promises none and
the tile loaders read 16 bytes at a time.

Device-agnostic: torch CPU tensors, torch CUDA tensors (device="cuda") and numpy arrays (for predict_host).  Shared by
tests/test_guarded_ref.py (the harness itself, planted writes) and the test_guard_*_gpu.py / test_call_history_gpu.py files.
"""
from __future__ import annotations

import numpy as np

GUARD_F32 = np.float32(-12345.678)  # the value tests/shap_edges.py uses
GUARD_WORD = {"float32": int(np.array([GUARD_F32]).view(np.uint32)[0]), "int32": 0xA5A5A5A5, "int64": 0xA5A5A5A5A5A5A5A5}
BAND_ROWS = 384
ALIGN_ELEMS = 64


def _dtype_name(dtype):
    name = str(dtype)
    name = name.replace("torch.", "") if name.startswith("torch.") else np.dtype(dtype).name
    if name not in GUARD_WORD:
        raise ValueError(f"Guarded: no guard pattern for dtype {dtype}")
    return name


def _uint(name):
    return np.uint64 if name == "int64" else np.uint32


def _numpy_alloc(total, name):
    """A numpy array of `total` elements whose first byte is 256-byte aligned."""
    item = np.dtype(name).itemsize
    raw = np.empty(total * item + 256, dtype=np.uint8)
    off = (-raw.ctypes.data) % 256
    return raw[off: off + total * item].view(name)


class Guarded:
    def __init__(self, xp, shape, dtype, band_rows=BAND_ROWS, device=None):
        """xp: the torch module or the numpy module; dtype: float32 / int32 / int64 of that module (or its name)."""
        self.is_torch = getattr(xp, "__name__", "") == "torch"
        self.shape = tuple(int(s) for s in shape)
        assert len(self.shape) >= 1 and all(s >= 0 for s in self.shape) and band_rows >= 1
        self.name = _dtype_name(dtype)
        self.width = int(np.prod(self.shape[1:], dtype=np.int64))
        self.n = int(np.prod(self.shape, dtype=np.int64))
        self.lead = self.tail = -(-(band_rows * max(self.width, 1)) // ALIGN_ELEMS) * ALIGN_ELEMS
        total = self.lead + self.n + self.tail
        word = GUARD_WORD[self.name]
        pattern = np.array([word], dtype=_uint(self.name)).view(self.name)[0]
        if self.is_torch:
            item = np.dtype(self.name).itemsize
            raw = xp.empty(total + 256 // item, dtype=getattr(xp, self.name), device=device if device is not None else "cpu")
            off = ((-raw.data_ptr()) % 256) // item  # (0 on a device; torch's CPU allocator aligns to 64 bytes only)
            self.flat = raw[off: off + total]
            self.flat.fill_(pattern.item())
            # (fill_ takes a Python number; float32(-12345.678) -> double -> float32 is exact, and the int patterns are
            # passed as the signed value of the same bits)
        else:
            self.flat = _numpy_alloc(total, self.name)
            self.flat[:] = pattern
        self.view = self.flat[self.lead: self.lead + self.n].reshape(self.shape)
        self.loaded = None

    @property
    def aligned(self):
        ptr = self.view.data_ptr() if self.is_torch else self.view.ctypes.data
        return ptr % 256 == 0

    @property
    def contiguous(self):
        return bool(self.view.is_contiguous()) if self.is_torch else bool(self.view.flags.c_contiguous)

    def load(self, values):
        """Puts caller values into the interior (running sums, input data) and remembers their bits for check_unchanged()."""
        v = np.array(values, dtype=self.name, order="C").reshape(self.shape)  # (a copy: the caller's array may be read-only)
        if self.is_torch:
            import torch

            self.view.copy_(torch.from_numpy(v))
        else:
            self.view[...] = v
        self.loaded = v
        return self

    def _host(self):
        flat = self.flat.detach().cpu().numpy() if self.is_torch else self.flat
        return np.ascontiguousarray(flat).view(_uint(self.name))

    def _where(self, side, k):
        w = max(self.width, 1)
        if side == "tail":
            return (f"element {k} past the interior: (row past the batch, column) = ({k // w}, {k % w}) "
                    f"[row {self.shape[0] + k // w} of a buffer of {self.shape[0]} rows]")
        back = self.lead - k  # 1 = the element just in front of the interior
        return (f"element {back} before the interior: (rows before the buffer) = {-(-back // w)}, "
                f"column {(-back) % w}")

    def check(self, what=""):
        """-> the interior as numpy.  Fails if any word of either band differs from the guard by bits."""
        words = self._host()
        guard = _uint(self.name)(GUARD_WORD[self.name])
        lead, tail = words[: self.lead], words[self.lead + self.n:]
        bad = np.flatnonzero(tail != guard)
        if bad.size:
            k = int(bad[0])
            raise AssertionError(f"{what}: guard band touched, {bad.size} word(s); first at {self._where('tail', k)}: "
                                 f"0x{int(tail[k]):x} (guard 0x{int(guard):x})")
        bad = np.flatnonzero(lead != guard)
        if bad.size:
            k = int(bad[-1])  # the one nearest the interior
            raise AssertionError(f"{what}: guard band touched, {bad.size} word(s); nearest at {self._where('lead', k)}: "
                                 f"0x{int(lead[k]):x} (guard 0x{int(guard):x})")
        return words[self.lead: self.lead + self.n].view(self.name).reshape(self.shape).copy()

    def check_unchanged(self, what=""):
        """For inputs: the bands are intact and the interior still holds the bits load() put there."""
        assert self.loaded is not None, "check_unchanged() needs a load()"
        got = self.check(what)
        u = _uint(self.name)
        diff = np.flatnonzero(got.reshape(-1).view(u) != self.loaded.reshape(-1).view(u))
        if diff.size:
            k, w = int(diff[0]), max(self.width, 1)
            raise AssertionError(f"{what}: the call changed its input, {diff.size} word(s); first at (row, column) = "
                                 f"({k // w}, {k % w})")
        return got


def guarded_input(xp, values, dtype="float32", band_rows=BAND_ROWS, device=None):
    """A Guarded of values' shape holding values: an input whose bits and bands check_unchanged() verifies after the call."""
    v = np.asarray(values)
    return Guarded(xp, v.shape, dtype, band_rows=band_rows, device=device).load(v)
