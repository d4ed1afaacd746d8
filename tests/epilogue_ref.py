"""Reference of the output epilogues (AVG, global_bias, SIGMOID, THRESHOLD, row-wise SOFTMAX) and the margin table their tests
share.  TEST INFRASTRUCTURE: numpy only; the forest builders at the end also use tests/order_forests.py.

What is float32 in the kernels and has one rounding per statement is evaluated in numpy float32 in the kernels' order and is to
match bit for bit (the library is built without fast-math and with -ffp-contract=off, and float32 division is correctly
rounded): `r / (float)n`, `r + bias`, `r > threshold`, and the softmax's `d = r - m`.  What goes through expf is evaluated in
float64 on those float32 values and comes with a bar per element, u = 2^-24:

  sigmoid  1 / (1 + exp(-r))           bar 4u |ref| + 2^-149        (expf 1 ulp = 2u, the rounding of 1 + e u, the division u)
  softmax  m = fmax over the classes (NaN skipped), d = float32(r - m), e = exp(d), s = sum(e), p = e / s
                                       bar (C + 4)u |ref| + 2^-149  (two expf 2u each, the float32 sum of C positive terms in
                                                                     class order (C - 1)u, the division u)

An element whose reference is NaN must be NaN; one whose reference is +-inf, 0 or 1 exactly (an infinite margin, a saturated
tail) must match bit for bit.  Pinned by the kernels' statements: sigmoid(NaN) = NaN, sigmoid(+inf) = 1, sigmoid(-inf) = 0,
NaN > t is 0; a softmax row holding a NaN or a +inf margin, or only -inf, is NaN in every class (NaN - m and inf - inf are NaN
and poison the sum); -inf beside a finite maximum is exactly 0.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
TINY = 2.0 ** -149
FLT_MAX = np.finfo(np.float32).max
OUT_RAW, OUT_AVG, OUT_SIGMOID, OUT_THRESHOLD, OUT_SOFTMAX = 0x0, 0x1, 0x10, 0x100, 0x1000  # (checked against tahoe_amd's)


@dataclass
class Expected:
    ref: np.ndarray        # float64; float32 values where the statement is exact
    bar: np.ndarray        # float64 per element; 0: bit for bit
    ambiguous: np.ndarray  # bool: SIGMOID | THRESHOLD with the float64 sigmoid within its bar of the threshold


def linear(margins, output, global_bias, divisor):
    """AVG and bias in float32, one rounding per statement.  RAW without a bias runs no transform: the bits stay (-0.0 too)."""
    r = np.array(margins, dtype=F32)
    if output == OUT_RAW and F32(global_bias) == 0:
        return r
    with np.errstate(all="ignore"):
        if output & OUT_AVG:
            r = r / F32(divisor)
        r = r + F32(global_bias)
    assert r.dtype == F32
    return r


def sigmoid64(r32):
    with np.errstate(all="ignore"):
        ref = 1.0 / (1.0 + np.exp(-r32.astype(F64)))
    return ref, 4 * U * np.abs(ref) + TINY


def softmax64(r32):
    C = r32.shape[-1]
    with np.errstate(all="ignore"):
        m = np.fmax(F32(-np.inf), np.fmax.reduce(r32, axis=-1, keepdims=True))  # fmaxf from -INFINITY: NaN is skipped
        d = r32 - m
        assert d.dtype == F32  # the kernel's own rounding, shared
        e = np.exp(d.astype(F64))
        ref = e / e.sum(axis=-1, keepdims=True)
    bar = (C + 4) * U * np.abs(ref) + TINY
    return ref, np.where(np.isnan(ref), 0.0, bar)


def epilogue(margins, output, threshold=0.0, global_bias=0.0, divisor=1) -> Expected:
    """What a handle with these parameters returns for raw float32 margins [rows] or [rows, C]."""
    r = linear(margins, output, global_bias, divisor)
    ref, bar = r.astype(F64), np.zeros(r.shape)
    if output & OUT_SIGMOID:
        assert not output & OUT_SOFTMAX
        ref, bar = sigmoid64(r)
    if output & OUT_SOFTMAX:
        assert r.ndim == 2 and r.shape[1] > 1 and not output & OUT_THRESHOLD
        ref, bar = softmax64(r)
    ambiguous = np.zeros(r.shape, dtype=bool)
    if output & OUT_THRESHOLD:
        t = F64(F32(threshold))
        with np.errstate(invalid="ignore"):
            ambiguous = np.abs(ref - t) <= bar if output & OUT_SIGMOID else ambiguous
            ref = (ref > t).astype(F64)  # strict, and NaN > t is false
        bar = np.zeros(r.shape)
    return Expected(ref, bar, ambiguous)


def same_bits(a, b):
    """Bit equality of two float32 arrays, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def check(got, want: Expected, what=""):
    """Asserts `got` (float32) against the reference; -> (max error of the inexact elements in units of u |ref|, over normal
    references; max error in units of 2^-149 over subnormal references)."""
    got = np.ascontiguousarray(got, dtype=F32)
    ref, bar = want.ref, want.bar
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN where the reference has none, or the reverse",
                                                np.argwhere(np.isnan(got) != nan)[:4].tolist())
    exact = ~nan & ~want.ambiguous & ((bar == 0) | np.isinf(ref) | (ref == 0) | (ref == 1))
    ref32 = ref.astype(F32)
    bad = exact & (got.view(np.uint32) != ref32.view(np.uint32))
    assert not bad.any(), (what, "not bit-exact", [(i.tolist(), float(got[tuple(i)]), float(ref[tuple(i)])) for i in np.argwhere(bad)[:4]])
    rest = ~nan & ~exact & ~want.ambiguous
    err = np.abs(got.astype(F64) - np.where(rest, ref, 0.0))
    bad = rest & ~(err <= bar)
    assert not bad.any(), (what, "over the bar (index, got, ref, error / bar)",
                           [(i.tolist(), float(got[tuple(i)]), float(ref[tuple(i)]), float(err[tuple(i)] / bar[tuple(i)]))
                            for i in np.argwhere(bad)[:4]])
    normal = rest & (np.abs(ref) >= 2.0 ** -126)
    sub = rest & ~normal
    in_u = float((err[normal] / (U * np.abs(ref[normal]))).max()) if normal.any() else 0.0
    in_tiny = float((err[sub] / TINY).max()) if sub.any() else 0.0
    return in_u, in_tiny


# ---- the margin table ----
FIXED_MAGNITUDES = (0.0, 2.0 ** -149, 2.0 ** -126, 1.0,
                    16.635532,                               # sigmoid reaches 1 - u
                    17.0,
                    87.33654, 88.72283, 88.72284, 89.0,      # around ln FLT_MAX
                    103.27893, 104.0,                        # around ln 2^-149
                    1e30, float(FLT_MAX), np.inf)
N_UNIFORM, N_LOG = 200, 100
TABLE_SEED = 20


@functools.lru_cache(maxsize=None)
def fixed_table():
    m = np.array(FIXED_MAGNITUDES, dtype=F32)
    t = np.concatenate([np.stack([m, -m], axis=1).ravel(), F32([np.nan])])
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def margin_table():
    """float32 [331]: the fixed values (31, -0.0 among them), 200 uniform draws in [-20, 20], 100 log-uniform in magnitude over
    [2^-140, 2^100] with a random sign."""
    rng = np.random.default_rng(TABLE_SEED)
    uni = rng.uniform(-20.0, 20.0, N_UNIFORM).astype(F32)
    log = (2.0 ** rng.uniform(-140.0, 100.0, N_LOG) * rng.choice([-1.0, 1.0], N_LOG)).astype(F32)
    t = np.concatenate([fixed_table(), uni, log])
    t.setflags(write=False)
    return t


RANDOM_PART = slice(31, 31 + N_UNIFORM + N_LOG)
SHIFT = 64.0  # exact on the 2^-10 grid below


def _grid_rows(rng, n, C):
    """n rows of C margins on a 2^-10 grid in [-20, 20], each followed by the row + 64 and the row - 64 (all exact)."""
    base = (rng.integers(-20 * 1024, 20 * 1024 + 1, (n, C)) / 1024.0).astype(F32)
    rows = np.stack([base, base + F32(SHIFT), base - F32(SHIFT)], axis=1).reshape(3 * n, C)
    assert np.array_equal(rows[1::3].astype(F64), base.astype(F64) + SHIFT)
    return rows


@functools.lru_cache(maxsize=None)
def softmax_rows(C):
    """-> (float32 [rows, C], first row of the shift triples).  C = 3: every pair (a, b, 0.0) of the fixed values, rows of
    equal margins, one row with a spread of 200; C = 10: a row of seeded draws and the same special rows.  Then 8 triples
    (row, row + 64, row - 64) on a 2^-10 grid."""
    rng = np.random.default_rng(TABLE_SEED + C)
    if C == 3:
        f = fixed_table()
        a, b = np.meshgrid(f, f, indexing="ij")
        head = np.stack([a.ravel(), b.ravel(), np.zeros(a.size, F32)], axis=1)
    else:
        head = rng.uniform(-20.0, 20.0, (1, C)).astype(F32)
        poisoned = np.tile(rng.uniform(-20.0, 20.0, C).astype(F32), (5, 1))
        poisoned[0, 3] = np.nan
        poisoned[1, C - 1] = np.inf
        poisoned[2, 0] = -np.inf
        poisoned[3, :] = -np.inf
        poisoned[4, :] = np.nan
        head = np.concatenate([head, poisoned])
    equal = np.repeat(F32([0.0, -0.0, 1.0, -88.0, 2.0 ** -149, 1e30, FLT_MAX, -FLT_MAX])[:, None], C, axis=1)
    spread = np.linspace(100.0, -100.0, C).astype(F32)[None, :]
    rows = np.concatenate([head, equal, spread]).astype(F32)
    first = rows.shape[0]
    rows = np.concatenate([rows, _grid_rows(rng, 8, C)])
    rows.setflags(write=False)
    return rows, first


def softmax_invariants(p, z, want: Expected, first):
    """The properties of a softmax output p (float32 [rows, C]) of the margins z (after AVG and the bias), on every finite row:
    p in [0, 1]; the class of the maximum has p = 1 / s within its bar; |sum p - 1| <= (2C + 4)u (C terms of at most
    (C + 4)u p each, plus the float64 sum); and the rows from `first` on, triples (row, row + c, row - c), agree within twice
    the bar wherever the constant survived AVG and the bias exactly."""
    C = p.shape[1]
    fin = np.isfinite(z).all(axis=1)
    assert fin.sum() >= 8 and not np.isnan(p[fin]).any()
    q, ref, bar = p[fin], want.ref[fin], want.bar[fin]
    assert (q >= 0).all() and (q <= 1).all()
    assert (np.abs(q.astype(F64).sum(axis=1) - 1.0) <= (2 * C + 4) * U).all()
    top, i = np.argmax(ref, axis=1), np.arange(q.shape[0])
    with np.errstate(over="ignore"):
        s = np.exp((z[fin] - z[fin][i, top][:, None]).astype(F64)).sum(axis=1)
    assert (np.abs(q[i, top] - 1.0 / s) <= bar[i, top]).all()
    assert fin[first:].all() and (p.shape[0] - first) % 3 == 0
    base = z[first::3].astype(F64)
    checked = 0
    for k in (1, 2):
        shift = z[first + k::3].astype(F64) - base
        exact = (shift == shift[:, :1]).all(axis=1)
        diff = np.abs(p[first + k::3].astype(F64) - p[first::3].astype(F64))
        assert (diff[exact] <= 2 * want.bar[first::3][exact]).all()
        checked += int(exact.sum())
    return checked


def ambiguous_share(table, threshold, global_bias=0.0, divisor=1, output=OUT_SIGMOID | OUT_THRESHOLD):
    """Share of the table that SIGMOID | THRESHOLD leaves undecided (the float64 sigmoid within its bar of the threshold)."""
    return float(epilogue(table, output, threshold, global_bias, divisor).ambiguous.mean())


# ---- forests whose raw margins are the table ----
MISSING = -999.0
LOOKUP_COLS = 2


def lookup_forest(columns, depth, zero_trees=0, zeros_first=False):
    """A forest whose raw margin of row i, class c is 0.0f + columns[i, c]: per class one dense search tree on feature 0 with
    thresholds 1 .. 2^depth - 1 (row x0 = i ends in leaf i, which holds columns[i, c]), and `zero_trees` root leaves of +0.0
    per class, after the lookup trees or before them.  tree t belongs to class t % C.
    -> (nodes, num_trees, data float32 [n, 2], margins float32 [n, C])"""
    import order_forests as of
    import tahoe_amd as ta

    columns = np.asarray(columns, dtype=F32)
    n, C = columns.shape
    assert n <= 1 << depth
    thr = np.arange(1, 1 << depth, dtype=F32)
    look = []
    for c in range(C):
        leaves = np.zeros(1 << depth, dtype=F32)
        leaves[:n] = columns[:, c]
        look.append(of.bst_tree(thr, depth, 0, True, leaves)[0])
    per = look[0].size
    z = np.zeros(per, dtype=np.int64)
    zero = ta.capi.encode_nodes(fid=z, value=np.zeros(per, F32), def_left=z, weight=np.zeros(per, F32), is_leaf=z + 1)
    zeros = [zero] * (zero_trees * C)
    parts = zeros + look if zeros_first else look + zeros
    data = np.full((n, LOOKUP_COLS), 0.5, dtype=F32)
    data[:, 0] = np.arange(n, dtype=F32)
    with np.errstate(invalid="ignore"):
        margins = F32(0.0) + columns  # the kernels sum from 0.0f in tree order: -0.0 becomes +0.0
        for _ in range(zero_trees):
            margins = margins + F32(0.0)
    return np.concatenate(parts), len(parts), data, margins


def oracle_margins(oracle, nodes, T, depth, data, C):
    """The CPU oracle's raw sums [rows, C] of a forest whose tree t belongs to class t % C."""
    per = nodes.size // T
    trees = nodes.reshape(T, per)
    return np.stack([oracle.predict(np.ascontiguousarray(trees[c::C]).ravel(), T // C, depth, data, MISSING)[0] for c in range(C)],
                    axis=1)
