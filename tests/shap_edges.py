"""Adversarial inputs for the three SHAP entry points and the Saabas one, and the checks the GPU files apply to them: test
infrastructure, not product.  Shared by tests/test_shap_edges_capi.py (the float64 references against their subset brute force,
the Saabas reference against its float64 restatement), tests/test_shap_edges_gpu.py (the exact kernels against the same
references) and tests/test_approx_edges_gpu.py (approx_kernel against tests/approx_contribs_ref.py, bit for bit).

Pools: covers (zero, spanning 1e-30 .. 1e30, ratios within 1e-8 of 1, float32 subnormals, a float32 sum that overflows, ratios
down to 1e-300 for the float64 references), thresholds and data (+-0, +-inf, NaN, subnormals, float32 neighbours of the
thresholds, values inside and at the edge of the missing band, the missing sentinel itself).  Forests are complete dense trees
(tahoe_dense_node, heap order) with early leaves whose subtrees hold garbage."""
from __future__ import annotations

import numpy as np

import approx_contribs_ref
import contribs_ref
import interactions_ref
import interventional_ref as ivr

U = 2.0 ** -24
Z_MIN = 2.0 ** -121  # create stores a zero fraction below this as 0 (include/tahoe_amd.h, TAHOE_CREATE_CONTRIBS)
F32 = np.float32


def encode(fid, val, def_left, weight, is_leaf):
    from tahoe_amd import capi

    return capi.encode_nodes(fid, val, def_left, weight, is_leaf)


def band_edges(missing):
    """float32 values around the edges of the missing band |float32(x - missing)| <= 1e-6, inside and outside."""
    m = F32(missing)
    if not np.isfinite(m):
        return []
    out = [m]
    for s in (1.0, -1.0):
        e = F32(m + F32(s * 1e-6))
        for k in range(-2, 3):
            v = e
            for _ in range(abs(k)):
                v = np.nextafter(v, F32(np.inf) if k > 0 else F32(-np.inf))
            out.append(F32(v))
        out.append(F32(m + F32(s * 5e-7)))
    return out


def threshold_pool(missing):
    base = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, 1.17549435e-38, 0.5, -0.5, 1.0, 3.0, 5.0, -2.0]
    pool = [F32(v) for v in base]
    if np.isfinite(missing):
        pool.append(F32(missing))  # a threshold equal to the missing sentinel
    return np.array(pool, F32)


def data_pool(missing):
    thr = threshold_pool(missing)
    out = list(thr)
    for t in thr:
        if np.isfinite(t):
            out += [np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf))]
    out += band_edges(missing)
    out += [F32(missing), F32(np.nan), F32(2.0), F32(-7.0)]
    return np.array(out, F32)


COVER_MODES = ("zero", "span", "near_one", "subnormal", "f32_overflow", "tiny", "mixed")


def cover_pair(rng, mode):
    """Child covers (wl, wr) of one internal node: finite, >= 0, positive sum (float32 values)."""
    if mode == "mixed":
        mode = COVER_MODES[int(rng.integers(0, len(COVER_MODES) - 1))]
    u = rng.random()
    if mode == "zero":
        a = [(0.0, float(rng.uniform(0.1, 1.0))), (float(rng.uniform(0.1, 1.0)), 0.0), (0.25, 0.75)][int(u * 3)]
    elif mode == "span":
        a = (10.0 ** rng.uniform(-30, 30), 10.0 ** rng.uniform(-30, 30))
    elif mode == "near_one":
        e = float(rng.uniform(1e-9, 1e-8))
        a = (1.0, e) if u < 0.5 else (e, 1.0)
    elif mode == "subnormal":
        a = [(1e-45, 1.0), (1.0, 1e-45), (1e-45, 1e-45), (3e-42, 1e-40)][int(u * 4)]
    elif mode == "f32_overflow":
        a = [(3e38, 3e38), (3e38, 1.0), (2e38, 3.3e38)][int(u * 3)]
    elif mode == "tiny":
        a = [(1e-39, 1.0), (1.0, 1e-39), (1e-20, 1e20), (1e20, 1e-20)][int(u * 4)]
    else:
        a = (float(rng.uniform(0.05, 1.0)), float(rng.uniform(0.05, 1.0)))
    return F32(a[0]), F32(a[1])


def random_forest(rng, T, D, F, missing, covers="benign", leaf_prob=0.15, thresholds=None, leaves=None):
    """T complete trees of depth D on features 0 .. F - 1, heap order; a node under a leaf holds garbage (the library ignores
    it).  thresholds: the pool internal nodes draw from (default threshold_pool(missing)); covers: a cover_pair mode."""
    per = 2 ** (D + 1) - 1
    thr = threshold_pool(missing) if thresholds is None else thresholds
    fid = np.zeros(T * per, np.int64)
    val = np.zeros(T * per, F32)
    dl = np.zeros(T * per, bool)
    w = np.ones(T * per, F32)
    leaf = np.zeros(T * per, bool)
    for t in range(T):
        o = t * per
        live = np.zeros(per, bool)
        live[0] = True
        for i in range(per):
            depth = int(np.floor(np.log2(i + 1)))
            if not live[i]:  # garbage below a leaf
                fid[o + i] = int(rng.integers(0, 1 << 20))
                val[o + i] = F32(rng.normal() * 1e30)
                dl[o + i] = bool(rng.integers(0, 2))
                leaf[o + i] = bool(rng.integers(0, 2))
                w[o + i] = F32(np.nan) if rng.random() < 0.5 else F32(-1.0)
                continue
            if depth == D or (i > 0 and rng.random() < leaf_prob):
                leaf[o + i] = True
                val[o + i] = F32(rng.uniform(-4, 4)) if leaves is None else F32(rng.choice(leaves))
                continue
            fid[o + i] = int(rng.integers(0, F))
            val[o + i] = F32(rng.choice(thr))
            dl[o + i] = bool(rng.integers(0, 2))
            w[o + 2 * i + 1], w[o + 2 * i + 2] = cover_pair(rng, covers)
            live[2 * i + 1] = live[2 * i + 2] = True
    return encode(fid, val, dl, w, leaf)


def random_data(rng, rows, F, missing, pool=None):
    pool = data_pool(missing) if pool is None else pool
    return np.ascontiguousarray(rng.choice(pool, size=(rows, F)).astype(F32))


def spine(D, fids, thresholds, covers=(0.3, 0.7), leaf0=1.0, right=None):
    """One tree of depth D whose internal nodes form a single spine: node k of the spine (depth k, feature fids[k], threshold
    thresholds[k]) has a leaf on one side and the next spine node on the other (right[k]; default alternating)."""
    per = 2 ** (D + 1) - 1
    fid = np.zeros(per, np.int64)
    val = np.zeros(per, F32)
    dl = np.zeros(per, bool)
    w = np.full(per, F32(np.nan))
    leaf = np.ones(per, bool)
    w[0] = 1.0
    i = 0
    for k in range(D):
        fid[i], val[i], dl[i], leaf[i] = fids[k], thresholds[k], k % 3 == 0, False
        go_right = (k % 2 == 0) if right is None else right[k]
        l_, r_ = 2 * i + 1, 2 * i + 2
        w[l_], w[r_] = covers if go_right else covers[::-1]
        off = r_ if not go_right else l_
        val[off] = F32(leaf0 + 0.25 * k)
        i = r_ if go_right else l_
    val[i] = F32(leaf0 - 1.5)
    return encode(fid, val, dl, w, leaf)


def stump(wl, wr, thr=0.5, leaves=(2.0, 3.0), fid=0, def_left=False):
    return encode([fid, 0, 0], [thr, leaves[0], leaves[1]], [def_left, 0, 0], [1.0, wl, wr], [0, 1, 1])


# ---- host-side facts about what create builds (preconditions of the GPU cases) ----
def path_lengths(nodes, T):
    """Elements per path (root included), in the order create packs them (class-major is the caller's job)."""
    per = nodes.size // max(T, 1)
    return [len(p[1]) + 1 for t in range(T) for p in contribs_ref._paths(nodes.reshape(T, per)[t])]


def pack_bins(nodes, T, num_classes=1):
    """Next-fit packing of create (contribs_build): per class, in tree then leaf order, paths into 64-lane bins -> list of bins,
    each a list of (length, [fids]) paths."""
    per = nodes.size // max(T, 1)
    bins = []
    for c in range(num_classes):
        cur, fill = [], 0
        for t in range(c, T, num_classes):
            for leafv, elems in contribs_ref._paths(nodes.reshape(T, per)[t]):
                L = len(elems) + 1
                if fill + L > 64:
                    bins.append(cur)
                    cur, fill = [], 0
                cur.append((L, [e[0] for e in elems]))
                fill += L
        if cur:
            bins.append(cur)
    return bins


def bin_rounds(b):
    """Rounds of ordered adds of a bin: the most lanes of the bin on one feature."""
    counts = {}
    for _, fids in b:
        for f in fids:
            counts[f] = counts.get(f, 0) + 1
    return max(counts.values()) if counts else 0


def min_zero_fraction_not_followed(nodes, T, x, missing):
    """Smallest float64 zero fraction z of an element that some row of x does not follow (inf if none)."""
    per = nodes.size // max(T, 1)
    best = np.inf
    for t in range(T):
        for _, elems in contribs_ref._paths(nodes.reshape(T, per)[t]):
            for f, z, edges in elems:
                o = np.ones(x.shape[0], bool)
                for thr, dleft, right in edges:
                    o &= contribs_ref.go_right(x[:, f], thr, dleft, missing) == right
                if not o.all():
                    best = min(best, z)
    return best


def contribs_tile_rows(F):
    """Rows per workgroup of contribs_kernel by the rule of contribs_build: the largest power of two <= 64 whose row tile and
    four slabs (20 B per column and row) fit 80 KiB, else 1."""
    R = 64
    while R > 1 and R * 20 * F > 80 * 1024:
        R //= 2
    return R


def interactions_tile_rows(F):
    """(LDS slab form?, rows per tile) of interactions_kernel by the rule of contribs_build."""
    row = (F + 4 * F * F) * 4
    if row > 80 * 1024:
        return False, 1
    R = 32
    while R > 1 and R * row > 80 * 1024:
        R //= 2
    return True, R


def interventional_shape(F, lds=160 * 1024):
    """(rows per tile, weight table in LDS?) of interventional_kernel by the rule of iv_shape."""
    per_row, table = 20 * F, 4 * 32 * 32
    R = 8
    while R > 1 and R * per_row + table > 80 * 1024:
        R //= 2
    return R, R * per_row + table <= lds


def approx_form(F, lds_bytes, forced=0):
    """(LDS slab form?, waves per workgroup) of approx_kernel by the rule of finish_build (approx.hip): a wave's slab is 64 rows
    of stride (F + 1) | 1 floats; the slab while two wave slabs fit lds_bytes, then as many waves (1 .. 4) as fit 64 KiB; in
    place, 4 waves.  forced = TAHOE_APPROX_FORM: 1 takes the slab while one wave slab fits, 2 never.  The library does not
    report the form it picks, so tests assert this restatement against an expected table, not the library itself: a later
    change to the rule in finish_build must update it, or the cases drift off the boundaries without failing."""
    wave_bytes = 64 * ((F + 1) | 1) * 4
    slab = 2 * wave_bytes <= lds_bytes
    if forced == 1:
        slab = wave_bytes <= lds_bytes
    if forced == 2:
        slab = False
    return slab, (min(max(65536 // wave_bytes, 1), 4) if slab else 4)


def max_abs_leaf(nodes, T, num_classes=1, avg=False):
    """max |leaf| over reachable leaves (divided by Tc with AVG): the L of the floor."""
    per = nodes.size // max(T, 1)
    m = 0.0
    for t in range(T):
        for leafv, _ in contribs_ref._paths(nodes.reshape(T, per)[t]):
            m = max(m, abs(leafv))
    Tc = T // max(num_classes, 1)
    return m / Tc if avg and Tc > 0 else m


# ---- GPU checks ----
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _outputs(torch, out, ndim):
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    return a if a.ndim == ndim else a[:, None]


def gpu_phi(env, forest, x):
    return _outputs(env[1], forest.predict_contribs(dev(env[1], x)), 3)


def gpu_inter(env, forest, x):
    return _outputs(env[1], forest.predict_interactions(dev(env[1], x)), 4)


def gpu_iv(env, forest, x):
    return _outputs(env[1], forest.predict_contribs_interventional(dev(env[1], x)), 3)


def single_rows_match(fn, forest, x, full, rows=None):
    """Bitwise: each listed row run as a batch of one equals its row of the full batch."""
    n = x.shape[0]
    rows = sorted({0, n - 1, n // 2} if rows is None else rows)
    for r in rows:
        one = fn(forest, x[r:r + 1])
        assert np.array_equal(bits(one), bits(full[r:r + 1])), f"row {r} alone differs from the full batch"


def floor_term(nodes, T, D, N, num_classes, avg, k_step):
    """floor = (N + k_step (D + 2)) 2^-121 L, L = max |leaf| (/ Tc with AVG): per term, create's cut of a zero fraction below
    2^-121 moves the exact value by <= 2^-121 |leaf| (Shapley values are multilinear in z, slopes <= |leaf|), and each float32
    rounding whose result lies below 2^-126 adds <= 2^-150 of absolute error, carried to the output scaled by at most
    (ud + 1) / (ud - i) <= 32 (a division by pre = (ud - i) z / (ud + 1) undone by the term's factor z): 32 2^-150 < 2^-121 per
    operation, over the same per-term operation count as gamma."""
    L = max_abs_leaf(nodes, T, num_classes, avg)
    return (N + k_step * (D + 2)) * Z_MIN * L


def check_contribs(env, nodes, T, D, F, x, missing, num_classes=1, output=0, bias=0.0, label="", brute=False):
    """predict_contribs against contribs_ref.poly (and brute): every output finite, |phi - phi64| <= gamma A + floor, gamma =
    (N + 4 (D + 2)) 2^-24 as tests/test_contribs_gpu.py; the bias column bit for bit; additivity against the library's margin;
    single-row batches bitwise equal to the full batch."""
    ta, torch = env
    avg = (output & ta.OUT_AVG) != 0
    f = ta.Forest(nodes, T, D, F, missing=missing, output=output, global_bias=bias, num_classes=num_classes, contribs=True)
    got32 = gpu_phi(env, f, x)
    assert np.all(np.isfinite(got32)), f"{label}: non-finite outputs at {np.argwhere(~np.isfinite(got32))[:5]}"
    got = got32.astype(np.float64)
    want, A, N = contribs_ref.poly(nodes, T, D, F, x, missing, num_classes=num_classes, avg=avg, global_bias=bias)
    if brute:
        b = contribs_ref.brute(nodes, T, D, F, x, missing, num_classes=num_classes, avg=avg, global_bias=bias)
        scale = np.abs(b).sum(axis=-1, keepdims=True)
        assert np.all(np.abs(b - want) <= 1e-12 * scale), f"{label}: poly vs brute"
    gamma = (N[None] + 4 * (D + 2)) * U
    floor = floor_term(nodes, T, D, N, num_classes, avg, 4)[None]
    assert np.all(floor <= 1e-30), f"{label}: the floor {floor.max():.3e} could mask a normal-range error"
    err = np.abs(got - want)[..., :-1]
    bound = (gamma * A + floor)[..., :-1]
    assert np.all(err <= bound), f"{label}: bound exceeded at {np.argwhere(err > bound)[:5]}"
    bb = contribs_ref.bias_f32(nodes, T, D, num_classes, avg, bias)
    assert np.array_equal(bits(got32[..., -1]), bits(np.broadcast_to(bb, got32[..., -1].shape))), f"{label}: bias column"
    m = ta.Forest(nodes, T, D, F, missing=missing, output=output & ta.OUT_AVG, global_bias=bias, num_classes=num_classes)
    margin = m.predict(dev(torch, x)).cpu().numpy().astype(np.float64).reshape(x.shape[0], num_classes)
    m.close()
    Tc = T // num_classes
    tol = (bound.sum(-1) + (Tc + 4) * U * (A.sum(-1) + np.abs(margin)) + F * U * np.abs(got).sum(-1))
    assert np.all(np.abs(got.sum(-1) - margin) <= tol), f"{label}: additivity"
    single_rows_match(lambda g, xx: gpu_phi(env, g, xx), f, x, got32)
    return f, got32


def host_diagonal(m, phi):
    """float32: phi_i - (0.0f + M[i][0] + ... + M[i][F-1], j != i, ascending)."""
    F = m.shape[-1] - 1
    off = m[..., :F, :F].astype(np.float32)
    want = np.empty(m.shape[:-2] + (F,), np.float32)
    for i in range(F):
        cols = [j for j in range(F) if j != i]
        terms = np.concatenate([np.zeros(m.shape[:-2] + (1,), np.float32), off[..., i, cols]], axis=-1)
        want[..., i] = phi[..., i].astype(np.float32) - np.add.accumulate(terms, axis=-1, dtype=np.float32)[..., -1]
    return want


def check_exact(env, f, got, x):
    """Bits that follow from the definition: symmetry, diagonal, bias corner, zero row / column F."""
    F = got.shape[-1] - 1
    assert np.array_equal(bits(got), bits(got.swapaxes(-1, -2))), "not exactly symmetric"
    phi = gpu_phi(env, f, x)
    idx = np.arange(F)
    assert np.array_equal(bits(got[..., idx, idx]), bits(host_diagonal(got, phi))), "diagonal"
    assert np.array_equal(bits(got[..., F, F]), bits(phi[..., F])), "bias corner"
    assert not np.any(bits(got[..., F, :F])) and not np.any(bits(got[..., :F, F])), "row / column F not +0.0"
    return phi


def interactions_rounding_count(D):
    """n of the interactions bar: the most float32 roundings on any path from an input to one off-diagonal term.  Conditioned
    extend, <= D steps: a weight takes x zd, x a, + and a = (float)(d - p) x c_inv[d + 1] two more: 5 per step.  Unwind, <= D
    steps, through the followed branch: tmp = next x (ud) x c_inv[i + 1] (3), pre = (udk - i) x (z / ud) with z rounded from
    float64 (3), x pre and - (2): 8 per step (the zero branch: pre (3), v_rcp_f32 (1 ulp: 2), x and + (2): 7); the running
    total takes one add per step.  The term: (o - z), the leaf, (o_k - z_k) x 0.5 and their storage (5), the AVG division (1),
    the 3 slab merges (3): 9.  n = 14 D + 9 <= 14 (D + 2)."""
    return 14 * (D + 2)


def check_interactions(env, nodes, T, D, F, x, missing, num_classes=1, output=0, bias=0.0, label="", brute=False,
                       need_pairs=True):
    """predict_interactions against interactions_ref.poly (and brute): every output finite; off-diagonals within
    gamma_n Aabs + floor; check_exact; additivity; single-row batches.

    Bar.  The kernel evaluates each term by a straight-line program of +, - and x (rcp(pre) is a coefficient computed from z
    alone).  For such a program |fl(t) - t| <= gamma_n t~, gamma_n = n 2^-24 / (1 - n 2^-24), where t~ is the program run on
    the absolute values of its inputs with every subtraction made an addition and n the most roundings on one input-to-output
    path (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., sec. 3.1).  The conditioned unwind subtracts
    (n_one = pwi - tmp x pre), so t~ is interactions_ref's term with _unwound_sum(absolute=True); Aabs sums |t~| over the terms
    of an entry, and the float32 sum of its N terms adds N roundings: |Phi - Phi64| <= gamma_{N + n} Aabs + floor, n =
    interactions_rounding_count(D).  On short paths Aabs is within a small factor of A; on a depth-22 spine the unwind's
    cancellation makes Aabs up to ~2500 A, and the kernel's error follows Aabs, not A (a float32 host emulation of the
    recursion gives errors of the same size).  Where tests/test_interactions_gpu.py asserts its
    (N + 6 (D + 2)) 2^-24 A bar (depth <= 12), that bar is asserted here too."""
    ta, torch = env
    avg = (output & ta.OUT_AVG) != 0
    f = ta.Forest(nodes, T, D, F, missing=missing, output=output, global_bias=bias, num_classes=num_classes, contribs=True)
    got32 = gpu_inter(env, f, x)
    assert np.all(np.isfinite(got32)), f"{label}: non-finite outputs at {np.argwhere(~np.isfinite(got32))[:5]}"
    got = got32.astype(np.float64)
    want, A, N, Aabs = interactions_ref.poly(nodes, T, D, F, x, missing, num_classes=num_classes, avg=avg, global_bias=bias,
                                             cond=True)
    if brute:
        b = interactions_ref.brute(nodes, T, D, F, x, missing, num_classes=num_classes, avg=avg, global_bias=bias)
        scale = np.abs(b).reshape(b.shape[0], -1).sum(axis=-1)[:, None, None, None]
        assert np.all(np.abs(b - want) <= 1e-12 * scale), f"{label}: poly vs brute"
    off = ~np.eye(F + 1, dtype=bool)
    off[F, :] = off[:, F] = False
    n = N[None] + interactions_rounding_count(D)
    gamma = n * U / (1 - n * U)
    floor = floor_term(nodes, T, D, N, num_classes, avg, 6)[None]
    assert np.all(floor <= 1e-30), f"{label}: the floor {floor.max():.3e} could mask a normal-range error"
    err = np.abs(got - want)[..., off]
    bound = (gamma * Aabs + floor)[..., off]
    assert np.all(err <= bound), f"{label}: bound exceeded at {np.argwhere(err > bound)[:5]}"
    if D <= 12:
        short = ((N[None] + 6 * (D + 2)) * U * A + floor)[..., off]
        assert np.all(err <= short), f"{label}: the (N + 6 (D + 2)) 2^-24 A bar exceeded at {np.argwhere(err > short)[:5]}"
    if need_pairs:
        assert np.count_nonzero(want[..., off]) > 0, f"{label}: a forest without interactions tests nothing"
    phi = check_exact(env, f, got32, x)
    m = ta.Forest(nodes, T, D, F, missing=missing, output=output & ta.OUT_AVG, global_bias=bias, num_classes=num_classes)
    margin = m.predict(dev(torch, x)).cpu().numpy().astype(np.float64).reshape(x.shape[0], num_classes)
    m.close()
    cw, cA, cN = contribs_ref.poly(nodes, T, D, F, x, missing, num_classes=num_classes, avg=avg, global_bias=bias)
    cfloor = floor_term(nodes, T, D, cN, num_classes, avg, 4)[None]
    Tc = T // num_classes
    tol = (((cN[None] + 4 * (D + 2)) * U * cA + cfloor)[..., :-1].sum(-1) + (Tc + 4) * U * (cA.sum(-1) + np.abs(margin))
           + F * U * np.abs(phi.astype(np.float64)).sum(-1) + (F + 2) * U * np.abs(got).sum(axis=(-1, -2)))
    assert np.all(np.abs(got.sum(axis=(-1, -2)) - margin) <= tol), f"{label}: additivity"
    single_rows_match(lambda g, xx: gpu_inter(env, g, xx), f, x, got32)
    return f, got32


def abs_leaf_sums(nodes, T, D, data, missing, num_classes):
    """sum over class c's trees of |the leaf the row reaches| (float64), [rows, C]."""
    from oracle import oracle

    a = nodes.copy()
    leaf = (a["bits"].view(np.uint32) >> 31) == 1
    a["val"][leaf] = np.abs(a["val"][leaf])
    return np.stack([oracle.predict_f64(ivr.sub_forest(a, T, num_classes, c), T // num_classes, D, data, missing)
                     for c in range(num_classes)], axis=1)


def check_interventional(env, nodes, T, D, F, x, bg, missing, num_classes=1, output=0, bias=0.0, label="", brute=False):
    """predict_contribs_interventional against interventional_ref.paths (and brute): every output finite, |phi - phi64| <=
    (N + B + 8) 2^-24 A as tests/test_interventional_gpu.py (the covers do not enter this game: no floor); the bias column bit
    for bit against the host formula on the library's raw sums of the background; additivity; single-row batches."""
    ta, torch = env
    avg = (output & ta.OUT_AVG) != 0
    f = ta.Forest(nodes, T, D, F, missing=missing, output=output, global_bias=bias, num_classes=num_classes, contribs=True)
    bgd = dev(torch, bg)
    f.set_background(bgd)
    got32 = gpu_iv(env, f, x)
    assert np.all(np.isfinite(got32)), f"{label}: non-finite outputs at {np.argwhere(~np.isfinite(got32))[:5]}"
    got = got32.astype(np.float64)
    want, A, N = ivr.paths(nodes, T, D, F, x, bg, missing, num_classes=num_classes, avg=avg, global_bias=bias)
    B = bg.shape[0]
    if brute:
        b = ivr.brute(nodes, T, D, F, x, bg, missing, num_classes=num_classes, avg=avg, global_bias=bias)
        scale = np.abs(b).sum(axis=-1, keepdims=True) + 1e-300
        assert np.all(np.abs(b - want) <= 1e-12 * scale), f"{label}: paths vs brute"
    gamma = (N[None] + B + 8) * U
    err = np.abs(got - want)[..., :-1]
    bound = (gamma * A)[..., :-1]
    assert np.all(err <= bound), f"{label}: bound exceeded at {np.argwhere(err > bound)[:5]}"
    Tc = T // num_classes
    if T > 0:
        raw = ta.Forest(nodes, T, D, F, missing=missing, num_classes=num_classes).predict_raw(bgd).cpu().numpy()
        raw = raw.reshape(B, num_classes)
    else:
        raw = np.zeros((B, num_classes), np.float32)
    want_bias = np.array([ivr.bias_from_raw(raw[:, c], Tc, avg, bias) for c in range(num_classes)]).astype(np.float32)
    assert np.array_equal(bits(got32[..., -1]), bits(np.broadcast_to(want_bias, got32[..., -1].shape))), f"{label}: bias"
    if T > 0:
        m = ta.Forest(nodes, T, D, F, missing=missing, output=output & ta.OUT_AVG, global_bias=bias, num_classes=num_classes)
        margin = m.predict(dev(torch, x)).cpu().numpy().astype(np.float64).reshape(x.shape[0], num_classes)
        m.close()
        div = Tc if avg and Tc > 0 else 1
        sx = abs_leaf_sums(nodes, T, D, x, missing, num_classes) / div
        sr = abs_leaf_sums(nodes, T, D, bg, missing, num_classes).mean(axis=0)[None, :] / div
        tol = bound.sum(-1) + (Tc + 4) * U * (sx + sr) + 4 * U * (np.abs(margin) + np.abs(got[..., -1]) + abs(bias))
        assert np.all(np.abs(got.sum(-1) - margin) <= tol), f"{label}: additivity"
    single_rows_match(lambda g, xx: gpu_iv(env, g, xx), f, x, got32)
    return f, got32


# ---- cases shared by the reference checks and the GPU file ----
MISSINGS = {"-999": -999.0, "0.5": 0.5, "0": 0.0, "nan": float("nan")}


def contradictory_tree(missing):
    """Depth 3 on features 0 and 1: the root sends x0 >= 5 right, where x0 >= 3 is asked again, so its left child (x0 < 3) is
    reached by no non-missing row; a missing x0 reaches it (the root's default is right, the second node's left).  Both
    children of the second node split x1 on a NaN threshold (every non-missing x1 goes left; a missing one by its default)."""
    nan = F32(np.nan)
    fid = [0, 1, 0, 0, 0, 1, 1] + [0] * 8
    val = [5.0, 0.5, 3.0, -1.0, 1.5, nan, nan] + [9.0] * 4 + [1.0, 2.0, 3.0, 4.0]
    dl = [0, 1, 1, 0, 0, 0, 1] + [0] * 8
    w = [1.0, 0.4, 0.6, 0.5, 0.5, 0.3, 0.7] + [np.nan] * 4 + [0.25, 0.75, 0.6, 0.4]
    leaf = [0, 0, 0, 1, 1, 0, 0] + [1] * 8
    return encode(fid, val, dl, w, leaf), 1, 3, 2


def edge_case(kind, seed):
    """-> (nodes, T, D, F, x, bg, missing) for kind 'covers:<mode>', 'branch:<missing>', 'contradictory:<missing>' or
    'sweep'.  Covers and pools as in the module docstring; fixed seeds."""
    rng = np.random.default_rng(seed)
    head, _, arg = kind.partition(":")
    if head == "covers":
        missing = 0.5
        T, D, F = 4, 3, 5
        nodes = random_forest(rng, T, D, F, missing, covers=arg, leaf_prob=0.1)
    elif head == "branch":
        missing = MISSINGS[arg]
        T, D, F = 5, 4, 4
        nodes = random_forest(rng, T, D, F, missing, covers="benign", leaf_prob=0.15)
    elif head == "contradictory":
        missing = MISSINGS[arg]
        nodes, T, D, F = contradictory_tree(missing)
    else:
        missing = list(MISSINGS.values())[int(rng.integers(0, len(MISSINGS)))]
        T, D, F = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(1, 6))
        covers = ("benign", "mixed", "zero", "span", "tiny")[int(rng.integers(0, 5))]
        nodes = random_forest(rng, T, D, F, missing, covers=covers, leaf_prob=float(rng.uniform(0, 0.3)))
    x = random_data(rng, 29, F, missing)
    bg = random_data(rng, 5, F, missing)
    return nodes, T, D, F, x, bg, missing


def tiny_stump_case(zero_on_path):
    """The stump with child covers (1e-39, 1) (rows on both sides); with zero_on_path, the right child splits again on feature 1
    with covers (0, 1), so rows that go left there do not follow a zero-cover element on the tiny-ratio path."""
    if not zero_on_path:
        nodes, T, D, F = stump(F32(1e-39), F32(1.0)), 1, 1, 1
        x = np.array([[0.0], [1.0], [0.5], [-1.0], [7.0]], F32)
    else:
        nodes = encode([0, 0, 1, 0, 0, 0, 0], [0.5, 2.0, 0.5, 0, 0, 4.0, 5.0], [0] * 7,
                       [1.0, 1e-39, 1.0, np.nan, np.nan, 0.0, 1.0], [0, 1, 0, 1, 1, 1, 1])
        T, D, F = 1, 2, 2
        x = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.5]], F32)
    return nodes, T, D, F, x


# ---- Saabas contributions (tahoe_forest_predict_contribs_approx): cases, host-side facts, GPU checks ----
UNSUPPORTED = 7
SPARSE_STRATEGIES = (0, 1, 2, 3, 5)  # the strategies a sparse handle serves
SPARSE_QRING_MAX_COLS = 256  # ... QRING (5) up to this width only (include/tahoe_amd.h, "On a sparse handle"); wider, it is refused
FLT_MAX = float(np.finfo(F32).max)
FLT_MIN = float(np.finfo(F32).tiny)
LEAF_POOLS = {"subnormal": (1e-45, 1e-40, 1.2e-38, 1e-30), "large": (1e30, 1e37), "overflow": (3e38, FLT_MAX)}
# (T, D, F) per pool; "large": 2 T D max |leaf| = 3.2e38 < FLT_MAX, so no delta and no partial sum of a row can overflow
LEAF_SHAPES = {"subnormal": (6, 4, 5), "large": (4, 4, 5), "overflow": (6, 3, 12)}


def leaf_case(kind, seed=0):
    """-> (nodes, T, D, F, x, missing): benign covers, leaves drawn from +-LEAF_POOLS[kind], 120 rows of the data pool."""
    rng = np.random.default_rng(7000 + 10 * seed + len(kind))
    mags = np.array(LEAF_POOLS[kind], F32)
    T, D, F = LEAF_SHAPES[kind]
    missing = -999.0
    nodes = random_forest(rng, T, D, F, missing, covers="benign", leaf_prob=0.1, leaves=np.concatenate([mags, -mags]))
    return nodes, T, D, F, random_data(rng, 120, F, missing), missing


def reachable(tree):
    """Heap indices of the nodes of one tree that a walk can reach, parents before children."""
    leaf = (tree["bits"].view(np.uint32) >> 31) == 1
    out, level = [], [0]
    while level:
        out += level
        level = [c for i in level if not leaf[i] for c in (2 * i + 1, 2 * i + 2)]
    return np.array(out, np.int64)


def reachable_leaves(nodes, T):
    """float32 values of every reachable leaf, root leaves included."""
    per = nodes.size // max(T, 1)
    vals = [np.zeros(0, F32)]
    for tree in (nodes.reshape(T, per) if T else []):
        r = reachable(tree)
        vals.append(tree["val"][r][(tree["bits"].view(np.uint32)[r] >> 31) == 1])
    return np.concatenate(vals)


def approx_walks(nodes, T, D, x, missing):
    """Per tree (E, path): E[per] the float64 node means of approx_contribs_ref (garbage at unreachable nodes) and
    path[rows, D + 1] the heap indices a row visits, root first, -1 after its leaf."""
    per = (1 << (D + 1)) - 1
    left = 2 * np.arange(per, dtype=np.int64) + 1
    x = np.ascontiguousarray(x, F32)
    out = []
    for tree in nodes.reshape(T, per):
        fid, dl, leaf, val, w = contribs_ref._decode(tree)
        E = approx_contribs_ref._means(val.astype(F32), leaf, left, w, True)
        path = np.full((x.shape[0], D + 1), -1, np.int64)
        path[:, 0] = 0
        for l in range(D):
            i = path[:, l]
            r = np.nonzero((i >= 0) & ~leaf[np.maximum(i, 0)])[0]
            n = i[r]
            path[r, l + 1] = left[n] + approx_contribs_ref._go_right(x[r, fid[n]], val[n], dl[n], missing)
        out.append((E, path))
    return out


def zero_cover_visits(nodes, T, D, x, missing):
    """(taken, avoided): over every visit of a (row, tree) walk to an internal node one of whose children has cover 0, how many
    go to that child and how many to its sibling."""
    per = (1 << (D + 1)) - 1
    taken = avoided = 0
    for tree, (_, path) in zip(nodes.reshape(T, per), approx_walks(nodes, T, D, x, missing)):
        w = tree["weight"]
        child = path[:, 1:]
        on = child >= 0
        c = np.maximum(child, 0)
        sibling = np.where(c % 2 == 1, c + 1, c - 1)
        taken += int((on & (w[c] == 0)).sum())
        avoided += int((on & (w[c] != 0) & (w[sibling] == 0)).sum())
    return taken, avoided


GUARD_ROWS = 256  # the most rows a workgroup of approx_kernel covers (4 waves of 64)
GUARD_VALUE = F32(-12345.678)


def gpu_approx(env, forest, x):
    """predict_contribs_approx into the first rows of a buffer GUARD_ROWS rows longer, filled with GUARD_VALUE: the rows past
    the batch must come back untouched (a write-out that counts rows by another wave's tile would land there)."""
    torch = env[1]
    n, width = x.shape[0], forest.num_classes * (forest.num_cols + 1)
    shape = (n + GUARD_ROWS,) + ((forest.num_classes,) if forest.num_classes > 1 else ()) + (forest.num_cols + 1,)
    big = dev(torch, np.full(shape, GUARD_VALUE, F32))
    forest.predict_contribs_approx(dev(torch, x), out=big[:n])
    torch.cuda.synchronize()
    a = big.cpu().numpy().reshape(n + GUARD_ROWS, width)
    touched = np.argwhere(bits(a[n:]) != bits(GUARD_VALUE))
    assert touched.size == 0, f"{len(touched)} values written past the batch's {n} rows, first at row {n + touched[0][0]}"
    return a[:n].reshape(n, forest.num_classes, forest.num_cols + 1)


def assert_same_bits(got, want, label):
    """uint32 equality; a NaN need only be a NaN at the same place (host and device produce different default NaNs, so sign
    and payload are not compared)."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, f"{label}: shapes {got.shape} and {want.shape}"
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{label}: {int(bad.sum())} outputs differ, first at {i}: {got[i]!r} vs {want[i]!r}")


def approx_handles(env, nodes, T, D, F, missing, num_classes=1, output=0, bias=0.0, sparse=True):
    """The handles check_approx_batch compares: 'dense' (approx_contribs=True), 'relayout' (the same with
    TAHOE_CREATE_PROB_RELAYOUT: exchange bits wherever a left child is the lighter one; None without trees), 'exact'
    (contribs=True; None where create answers TAHOE_ERR_UNSUPPORTED), 'sparse' (the tahoe_dense_to_sparse_ex conversion with
    approx_contribs=True; None without trees or with sparse=False)."""
    ta, _ = env
    kw = dict(missing=missing, output=output, global_bias=bias, num_classes=num_classes)
    h = {"dense": ta.Forest(nodes, T, D, F, approx_contribs=True, **kw), "relayout": None, "exact": None, "sparse": None}
    if T > 0:
        h["relayout"] = ta.Forest(nodes, T, D, F, approx_contribs=True, relayout=True, **kw)
    try:
        h["exact"] = ta.Forest(nodes, T, D, F, contribs=True, **kw)
    except ta.TahoeError as e:
        if e.status != UNSUPPORTED:
            raise
    if sparse and T > 0:
        sn, tr, cv = ta.capi.dense_to_sparse(nodes, T, D, covers=True)
        h["sparse"] = ta.capi.SparseForest(sn, tr, F, covers=cv, approx_contribs=True, **kw)
    return h


def check_approx_batch(env, h, nodes, T, D, F, x, missing, num_classes=1, output=0, bias=0.0, label=""):
    """One batch on the handles of approx_handles: the checks of check_approx.  -> the dense handle's output."""
    from test_approx_contribs_gpu import check_additivity

    ta, torch = env
    f = h["dense"]
    got = gpu_approx(env, f, x)
    want, S, N = approx_contribs_ref.dense(nodes, T, D, F, x, missing, num_classes=num_classes,
                                           avg=(output & ta.OUT_AVG) != 0, global_bias=bias, scale=True)
    assert_same_bits(got, want, f"{label}: against the reference")
    if h["exact"] is not None:
        assert_same_bits(got[..., -1], gpu_phi(env, h["exact"], x)[..., -1], f"{label}: bias column against predict_contribs")
    if T > 0:
        # the bound counts roundings, so it holds on rows without an overflow: a finite reference, and a float32 margin of
        # the library that stayed finite (leaves near FLT_MAX can overflow predict_raw's sum where no delta overflows)
        raw = f.predict_raw(dev(torch, x)).cpu().numpy().reshape(x.shape[0], num_classes)
        ok = np.isfinite(want).all(axis=(1, 2)) & np.isfinite(raw).all(axis=1)
        if ok.any():
            check_additivity(env, f, np.ascontiguousarray(x[ok]), got[ok], S[ok], N[ok], T // num_classes,
                             reachable_leaves(nodes, T), label)
    single_rows_match(lambda g, xx: gpu_approx(env, g, xx), f, x, got)
    if h["relayout"] is not None:
        assert_same_bits(gpu_approx(env, h["relayout"], x), got, f"{label}: re-laid-out handle")
    if h["sparse"] is not None:
        for s in SPARSE_STRATEGIES:
            if s == ta.STRATEGY_QRING and F > SPARSE_QRING_MAX_COLS:
                try:
                    h["sparse"].set_strategy(s)
                except ta.TahoeError as e:
                    assert e.status == UNSUPPORTED, f"{label}: {e}"
                    continue
                raise AssertionError(f"{label}: QRING accepted on a sparse handle of {F} columns")
            h["sparse"].set_strategy(s)  # every other refusal fails the test
            assert_same_bits(gpu_approx(env, h["sparse"], x), got, f"{label}: converted sparse handle, strategy {s}")
    return got


def check_approx(env, nodes, T, D, F, x, missing, num_classes=1, output=0, bias=0.0, label="", sparse=True):
    """predict_contribs_approx on a dense handle against approx_contribs_ref.dense, bit for bit (assert_same_bits); the bias
    column bit for bit predict_contribs' of a contribs=True handle; additivity against predict_raw within the bound of
    tests/test_approx_contribs_gpu.py, (2 N + Tc + 8) 2^-24 (S + |bias| + sum |leaf|), on the rows without an overflow;
    single-row batches bitwise equal to the full batch; the handle created with TAHOE_CREATE_PROB_RELAYOUT bit for bit the
    plain one; with sparse=True the tahoe_dense_to_sparse_ex handle under every strategy a sparse handle serves, bit for bit
    the dense handle; every call writes nothing past its rows (gpu_approx).  -> (the dense handle, its output)."""
    h = approx_handles(env, nodes, T, D, F, missing, num_classes, output, bias, sparse)
    assert h["exact"] is not None, f"{label}: the contribs=True handle of the bias check was refused"
    got = check_approx_batch(env, h, nodes, T, D, F, x, missing, num_classes, output, bias, label)
    for k in ("relayout", "exact", "sparse"):
        if h[k] is not None:
            h[k].close()
    return h["dense"], got
