"""References for the SHAP interaction values of an oblivious handle (tahoe_oblivious_forest_create_ex with
TAHOE_CREATE_INTERACTIONS), written from the definition in include/tahoe_amd.h: test infrastructure, not product.  Forests, covers,
the implicit heap and the game are those of tests/oblivious_shap_ref.py.  Every function returns Phi[rows, K, F + 1, F + 1]: the
off-diagonals, the diagonal phi_i - sum_{j != i} Phi_ij, [F][F] the float32 bias, everything else zero.

- brute (float64): the Shapley interaction index from its definition over the subsets of the features a tree uses (<= 8),
  Phi_ij = sum_{S in U \\ {i,j}} |S|! (n - |S| - 2)! / (2 (n - 1)!) (v(S + ij) - v(S + i) - v(S + j) + v(S)); phi from
  oblivious_shap_ref.brute.
- poly (float64): per tree the elements e = 0 .. M - 1 (distinct features in order of first appearance), per leaf j the row
  weighs, per pair c < e the term w_e(P \\ {c}) (o_c ? 1 - z_c : -z_c) / 2 leaf[j][k]: EXTEND over the M - 1 other elements in
  their order and e's unwound sum times (o_e - z_e) (where o_e = 0 the division form of the sum, not the kernel's -S0').  Also
  A = the sum of |terms| and N = the number of terms per entry, both [rows, K, F + 1, F + 1], zero off the off-diagonals.
- emulate (float32): oblivious_inter_kernel restated operation for operation from the header comment of oblivious_shap.hip: the
  bits of predict_interactions, not a bound.  phi is oblivious_shap_ref.emulate.
- expand: oblivious_shap_ref.expand_with_covers."""
from __future__ import annotations

import itertools
import math

import numpy as np

import oblivious_ref as obr
import oblivious_shap_ref as osr

expand = osr.expand_with_covers


def _finish(off, phi):
    """off [rows, K, F, F] (final) and phi [rows, K, F + 1] of one dtype -> Phi"""
    rows, k, F, _ = off.shape
    out = np.zeros((rows, k, F + 1, F + 1), off.dtype)
    out[:, :, :F, :F] = off
    i = np.arange(F)
    out[:, :, i, i] = phi[:, :, :F] - off.sum(axis=-1)
    out[:, :, F, F] = phi[:, :, F]
    return out


def brute(forest, covers, data, missing=obr.MISSING, avg=False, global_bias=0.0):
    data = np.ascontiguousarray(data, np.float32)
    rows, k, F = data.shape[0], forest["k"], forest["cols"]
    off = np.zeros((rows, k, F, F))
    for t, D, fids, sl, lv, cv in osr._trees(forest, covers):
        _, ratio = osr.heap(D, cv)
        right = osr._bits(forest, sl, data, missing)
        U = sorted(set(int(f) for f in fids))
        assert len(U) <= 8

        def value(S):
            V = np.broadcast_to(lv.astype(np.float64)[:, None, :], (1 << D, rows, k))
            for l in range(D - 1, -1, -1):
                n = 1 << l
                left, rgt = V[:n], V[n:]
                if int(fids[l]) in S:
                    V = np.where(right[l][None, :, None], rgt, left)
                else:
                    V = ratio[l + 1][:n, None, None] * left + ratio[l + 1][n:, None, None] * rgt
            return V[0]

        vals = {S: value(set(S)) for n in range(len(U) + 1) for S in itertools.combinations(U, n)}
        n = len(U)
        for i, j in itertools.combinations(U, 2):
            rest = [u for u in U if u not in (i, j)]
            acc = np.zeros((rows, k))
            for size in range(n - 1):
                w = math.factorial(size) * math.factorial(n - size - 2) / (2 * math.factorial(n - 1))
                for S in itertools.combinations(rest, size):
                    acc += w * (vals[tuple(sorted(S + (i, j)))] - vals[tuple(sorted(S + (i,)))] - vals[tuple(sorted(S + (j,)))]
                                + vals[S])
            off[:, :, i, j] += acc
            off[:, :, j, i] += acc
    T = len(forest["depths"])
    if avg and T > 0:
        off /= T
    return _finish(off, osr.brute(forest, covers, data, missing, avg, global_bias))


def _tree_tables(forest, D, fids, sl, cv, data, missing):
    """-> (feats, masks, Z [M, leaves] float64 uncut, idx [rows])"""
    _, ratio = osr.heap(D, cv)
    feats, masks, Z = osr.shap_tables(D, fids, ratio)
    right = osr._bits(forest, sl, data, missing)
    idx = np.zeros(data.shape[0], np.int64)
    for l in range(D):
        idx |= right[l].astype(np.int64) << l
    return feats, masks, Z, idx


def poly(forest, covers, data, missing=obr.MISSING, avg=False, global_bias=0.0):
    """-> (Phi, A, N), each [rows, K, F + 1, F + 1] float64"""
    data = np.ascontiguousarray(data, np.float32)
    rows, k, F = data.shape[0], forest["k"], forest["cols"]
    off, A, N = np.zeros((rows, k, F, F)), np.zeros((rows, k, F, F)), np.zeros((rows, k, F, F))
    for t, D, fids, sl, lv, cv in osr._trees(forest, covers):
        feats, masks, Z, idx = _tree_tables(forest, D, fids, sl, cv, data, missing)
        M, nleaf = len(feats), 1 << D
        if M < 2:
            continue
        Zc = np.where(Z < osr.MIN_Z, 0.0, Z)
        mism = idx[None, :] ^ np.arange(nleaf)[:, None]  # [leaves, rows]
        O = np.array([(mism & masks[e]) == 0 for e in range(M)])
        live = ~np.any((Zc[:, :, None] == 0.0) & ~O, axis=0)
        leaf = lv.astype(np.float64)
        for c in range(M - 1):
            path = [e for e in range(M) if e != c]
            R = M - 1
            W = np.zeros((R + 1, nleaf, rows))
            W[0] = 1.0
            for p, e in enumerate(path):
                l = p + 1
                z, o = Zc[e][:, None], O[e]
                for i in range(l - 1, -1, -1):
                    W[i + 1] = W[i + 1] + o * W[i] * (i + 1) / (l + 1)
                    W[i] = z * W[i] * (l - i) / (l + 1)
            cond = np.where(O[c], 1.0 - Zc[c][:, None], -Zc[c][:, None]) / 2
            for e in path:
                if e < c:
                    continue
                z, o = Zc[e][:, None], O[e]
                nxt = W[R].copy()
                one, zero = np.zeros((nleaf, rows)), np.zeros((nleaf, rows))
                for i in range(R - 1, -1, -1):
                    tmp = nxt * (R + 1) / (i + 1)
                    one += tmp
                    nxt = W[i] - tmp * z * (R - i) / (R + 1)
                    pre = z * (R - i) / (R + 1)
                    zero += np.where(pre > 0, W[i] / np.where(pre > 0, pre, 1.0), 0.0)
                w = np.where(live, np.where(o, one, zero) * (o - z) * cond, 0.0)
                with np.errstate(invalid="ignore"):  # (an infinite leaf the row does not weigh: 0 * inf, then dropped)
                    term = np.where(live[:, :, None], w[:, :, None] * leaf[:, None, :], 0.0)  # [leaves, rows, K]
                lo, hi = min(feats[c], feats[e]), max(feats[c], feats[e])
                for a, b in ((lo, hi), (hi, lo)):
                    off[:, :, a, b] += term.sum(axis=0)
                    A[:, :, a, b] += np.abs(term).sum(axis=0)
                    N[:, :, a, b] += live.sum(axis=0)[:, None]
    T = len(forest["depths"])
    if avg and T > 0:
        off /= T
        A /= T
    phi, _, _ = osr.poly(forest, covers, data, missing, avg, global_bias)

    def pad(x):
        out = np.zeros((rows, k, F + 1, F + 1))
        out[:, :, :F, :F] = x
        return out

    return _finish(off, phi), pad(A), pad(N)


def emulate(forest, covers, data, missing=obr.MISSING, avg=False, global_bias=0.0):
    """-> Phi float32.  Every coefficient is a float64 quotient rounded once; every product and sum below is one float32
    operation, in the kernel's order.  A leaf the row does not weigh adds +0.0f in place of being skipped, which gives the same
    bits (oblivious_shap_ref.emulate says why)."""
    f32 = np.float32
    data = np.ascontiguousarray(data, f32)
    rows, k, F = data.shape[0], forest["k"], forest["cols"]
    acc = np.zeros((rows, k, F, F), f32)  # [lo][hi] of every pair, from +0.0f through all trees in order
    with np.errstate(all="ignore"):
        for t, D, fids, sl, lv, cv in osr._trees(forest, covers):
            feats, masks, Z, idx = _tree_tables(forest, D, fids, sl, cv, data, missing)
            M, nleaf = len(feats), 1 << D
            if M < 2:
                continue
            R = M - 1
            zf = np.where(Z < osr.MIN_Z, 0.0, Z).astype(f32)  # the zz table: {z, 1 - z}
            omz = (1.0 - Z).astype(f32)
            zmask = np.zeros(nleaf, np.int64)
            for e in range(M):
                zmask |= np.where(zf[e] == 0, masks[e], 0)
            # arrays are [rows, leaves]: the leaves, the long axis, are contiguous
            mism = idx[:, None] ^ np.arange(nleaf)[None, :]
            live = (mism & zmask[None, :]) == 0
            keep = np.nonzero(live.any(axis=0))[0]  # the leaves some row weighs, ascending (the wave skips the others too)
            mism, live, zf, omz, nleaf = mism[:, keep], live[:, keep], zf[:, keep], omz[:, keep], keep.size
            O = [(mism & masks[e]) == 0 for e in range(M)]
            zero = np.zeros((rows, nleaf), f32)
            leaf = np.ascontiguousarray(np.asarray(lv, f32)[keep].T)  # [K, leaves]
            for c in range(R):
                path = [p + (1 if p >= c else 0) for p in range(R)]  # position p is element path[p]
                cf = np.where(O[c], omz[c][None, :], -zf[c][None, :]) * f32(0.5)
                pw = [np.ones((rows, nleaf), f32)]
                for p, e in enumerate(path):  # EXTEND
                    l = p + 1
                    pw.append(zero.copy())
                    for i in range(l - 1, -1, -1):
                        tt = pw[i] * f32((i + 1) / (l + 1))
                        pw[i + 1] = pw[i + 1] + np.where(O[e], tt, zero)
                        pw[i] = pw[i] * (zf[e] * f32((l - i) / (l + 1)))[None, :]
                s0 = zero.copy()
                for i in range(R):
                    s0 = s0 + pw[i] * f32((R + 1) / (R - i))
                for p, e in enumerate(path):
                    if p < c:
                        continue
                    nxt, tot = pw[R], zero.copy()
                    for i in range(R - 1, -1, -1):
                        tmp = nxt * f32((R + 1) / (i + 1))
                        tot = tot + tmp
                        if i > 0:
                            nxt = pw[i] - tmp * (zf[e] * f32((R - i) / (R + 1)))[None, :]
                    w = np.where(O[e], tot * omz[e][None, :], -s0)
                    wc = w * cf
                    term = np.where(live[:, None, :], wc[:, None, :] * leaf[None, :, :], f32(0.0))  # [rows, K, leaves]
                    lo, hi = min(feats[c], feats[e]), max(feats[c], feats[e])
                    run = np.concatenate([acc[:, :, lo, hi, None], term], axis=-1)
                    acc[:, :, lo, hi] = np.add.accumulate(run, axis=-1, dtype=f32)[..., -1]
        T = len(forest["depths"])
        div = f32(T) if avg and T > 0 else f32(1.0)
        phi = osr.emulate(forest, covers, data, missing, avg, global_bias)
        used = sorted(set(int(f) for f in forest["fids"]))
        out = np.zeros((rows, k, F + 1, F + 1), f32)
        for a, b in itertools.combinations(used, 2):
            q = acc[:, :, a, b] / div
            out[:, :, a, b] = q
            out[:, :, b, a] = q
        for a in used:
            s = np.zeros((rows, k), f32)
            for b in used:
                if b != a:
                    s = s + out[:, :, a, b]
            out[:, :, a, a] = phi[:, :, a] - s
    out[:, :, F, F] = phi[:, :, F]
    return out
