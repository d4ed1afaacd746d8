"""Two float64 references for SHAP interaction values, written from the definition in include/tahoe_amd.h
(tahoe_forest_predict_interactions): test infrastructure, not product.  Decoding, paths, v(S) and the bias come from
tests/contribs_ref.py (the same game as tahoe_forest_predict_contribs).

- brute(): per tree, every subset S of the features the tree uses, v(S) by the recursive expectation, and the Shapley
  interaction index Phi_ij = sum_{S in U \\ {i,j}} |S|! (n - |S| - 2)! / (2 (n - 1)!) (v(S+ij) - v(S+i) - v(S+j) + v(S)), n = |U|
  (features a tree does not use are dummies: they change no Phi_ij).  <= ~10 features per tree.
- poly(): the per-path conditioned recursion (XGBoost's PredictInteractionContributions): for every path and every pair of its
  elements k < j, leaf (o_j - z_j)(o_k - z_k) U_j(P \\ {k}) / 2 into [k][j] and [j][k], U_j(P \\ {k}) = j's unwound-path sum
  (Lundberg et al. 2018, Algorithm 2) on the path without k; vectorised over rows and paths.  Also returns A = sum of |per-path
  terms| feeding each output and N = their count, for error bounds.
Both return Phi[rows, C, F + 1, F + 1]: off-diagonals summed over the class's trees (divided by Tc with AVG), the diagonal
phi_i - sum_{j != i} Phi_ij with phi_i from the matching contribs_ref function, [F][F] the float32 bias, the rest of row and column
F zero."""
from __future__ import annotations

import itertools
import math

import numpy as np

import contribs_ref


def _finish(off, phi, T, num_classes, avg):
    """off [rows, C, F, F] float64 (trees summed) and phi [rows, C, F + 1] -> Phi [rows, C, F + 1, F + 1]."""
    rows, C, F, _ = off.shape
    Tc = T // num_classes
    if avg and Tc > 0:
        off = off / Tc
    out = np.zeros((rows, C, F + 1, F + 1))
    out[:, :, :F, :F] = off
    idx = np.arange(F)
    out[:, :, idx, idx] = phi[:, :, :F] - off.sum(axis=-1)
    out[:, :, F, F] = phi[:, :, F]
    return out


def brute(nodes, T, D, F, data, missing, num_classes=1, avg=False, global_bias=0.0):
    data = np.ascontiguousarray(data, np.float32)
    rows = data.shape[0]
    per = nodes.size // max(T, 1)
    off = np.zeros((rows, num_classes, F, F))
    for t in range(T):
        tree = nodes.reshape(T, per)[t]
        U = contribs_ref._used_features(tree)
        n = len(U)
        if n < 2:
            continue
        vals = {}
        for k in range(n + 1):
            for S in itertools.combinations(U, k):
                vals[S] = contribs_ref._value(tree, data, missing, set(S))
        for i, j in itertools.combinations(U, 2):
            rest = [u for u in U if u not in (i, j)]
            acc = np.zeros(rows)
            for k in range(n - 1):
                wgt = math.factorial(k) * math.factorial(n - k - 2) / (2 * math.factorial(n - 1))
                for S in itertools.combinations(rest, k):
                    acc += wgt * (vals[tuple(sorted(S + (i, j)))] - vals[tuple(sorted(S + (i,)))]
                                  - vals[tuple(sorted(S + (j,)))] + vals[S])
            off[:, t % num_classes, i, j] += acc
            off[:, t % num_classes, j, i] += acc
    phi = contribs_ref.brute(nodes, T, D, F, data, missing, num_classes=num_classes, avg=avg, global_bias=global_bias)
    return _finish(off, phi, T, num_classes, avg)


def _extend(Z, O):
    """Permutation weights of a path: Z [P, L] zero fractions, O [P, L, rows] one-fractions (element 0 the root: z = o = 1)
    -> W [L, P, rows]."""
    P, L = Z.shape
    rows = O.shape[2]
    W = np.zeros((L, P, rows))
    W[0] = 1.0
    for j in range(1, L):
        zj, oj = Z[:, j][:, None], O[:, j]
        for i in range(j - 1, -1, -1):
            W[i + 1] += oj * W[i] * (i + 1) / (j + 1)
            W[i] = zj * W[i] * (j - i) / (j + 1)
    return W


def _unwound_sum(W, zk, ok, absolute=False):
    """Algorithm 2's UNWOUND-SUM of the element (zk [P, 1], ok [P, rows]) on the path of weights W [L, P, rows].  absolute:
    the same recursion with its one subtraction (the unwound weight of a followed element) made an addition -- every
    intermediate then bounds the absolute value of the exact one's terms, the magnitude a float32 run of the recursion rounds."""
    ud = W.shape[0] - 1
    nxt = W[ud].copy()
    t_one = np.zeros_like(nxt)
    t_zero = np.zeros_like(nxt)
    for i in range(ud - 1, -1, -1):
        tmp = nxt * (ud + 1) / (i + 1)
        t_one += tmp
        nxt = (W[i] + tmp * zk * (ud - i) / (ud + 1)) if absolute else (W[i] - tmp * zk * (ud - i) / (ud + 1))
        pre = zk * (ud - i) / (ud + 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t_zero += np.where(pre > 0, W[i] / np.where(pre > 0, pre, 1.0), 0.0)
    return np.where(ok > 0, t_one, t_zero)


def poly(nodes, T, D, F, data, missing, num_classes=1, avg=False, global_bias=0.0, chunk=2048, cond=False):
    """-> (Phi [rows, C, F + 1, F + 1], A [rows, C, F + 1, F + 1], N [C, F + 1, F + 1]) in float64; A and N cover the
    off-diagonal entries (zero elsewhere).  cond: also returns Aabs [rows, C, F + 1, F + 1], A with each term's unwound sum
    taken by _unwound_sum(absolute=True) (>= A; equal where no followed element's weight is unwound)."""
    data = np.ascontiguousarray(data, np.float32)
    rows = data.shape[0]
    per = nodes.size // max(T, 1)
    offT = np.zeros((num_classes, F * F, rows))
    AT = np.zeros((num_classes, F * F, rows))
    AbsT = np.zeros((num_classes, F * F, rows)) if cond else None
    NF = np.zeros((num_classes, F * F))
    for t in range(T):
        c = t % num_classes
        by_len = {}
        for p in contribs_ref._paths(nodes.reshape(T, per)[t]):
            by_len.setdefault(len(p[1]) + 1, []).append(p)
        for L, paths in by_len.items():
            if L < 3:
                continue
            for lo in range(0, len(paths), chunk):
                _poly_chunk(paths[lo:lo + chunk], L, F, data, missing, offT[c], AT[c], NF[c],
                            AbsT[c] if cond else None)
    # the upper triangle holds each pair's sum; [j][i] is the same number as [i][j]
    off = offT.transpose(2, 0, 1).reshape(rows, num_classes, F, F)
    off = off + off.swapaxes(-1, -2)
    A_off = AT.transpose(2, 0, 1).reshape(rows, num_classes, F, F)
    A_off = A_off + A_off.swapaxes(-1, -2)
    NF = NF.reshape(num_classes, F, F)
    NF = NF + NF.swapaxes(-1, -2)
    phi, _, _ = contribs_ref.poly(nodes, T, D, F, data, missing, num_classes=num_classes, avg=avg, global_bias=global_bias)
    out = _finish(off, phi, T, num_classes, avg)
    Tc = T // num_classes
    if avg and Tc > 0:
        A_off = A_off / Tc
    A = np.zeros_like(out)
    A[:, :, :F, :F] = A_off
    N = np.zeros((num_classes, F + 1, F + 1))
    N[:, :F, :F] = NF
    if not cond:
        return out, A, N
    Abs = AbsT.transpose(2, 0, 1).reshape(rows, num_classes, F, F)
    Abs = Abs + Abs.swapaxes(-1, -2)
    if avg and Tc > 0:
        Abs = Abs / Tc
    Aabs = np.zeros_like(out)
    Aabs[:, :, :F, :F] = Abs
    return out, A, N, Aabs


def _poly_chunk(paths, L, F, data, missing, offT, AT, N, AbsT=None):
    P, rows = len(paths), data.shape[0]
    Z = np.ones((P, L))
    O = np.ones((P, L, rows))
    fids = np.zeros((P, L), np.int64)
    leafv = np.array([p[0] for p in paths])
    for a, (_, elems) in enumerate(paths):
        for j, (f, z, edges) in enumerate(elems, start=1):
            Z[a, j], fids[a, j] = z, f
            o = np.ones(rows, bool)
            for thr, dleft, right in edges:
                o &= contribs_ref.go_right(data[:, f], thr, dleft, missing) == right
            O[a, j] = o
    for k in range(1, L - 1):
        keep = [e for e in range(L) if e != k]
        W = _extend(Z[:, keep], O[:, keep])
        cond = leafv[:, None] * (O[:, k] - Z[:, k][:, None]) / 2
        for j in range(k + 1, L):
            U = _unwound_sum(W, Z[:, j][:, None], O[:, j])
            term = cond * (O[:, j] - Z[:, j][:, None]) * U
            dst = np.minimum(fids[:, k], fids[:, j]) * F + np.maximum(fids[:, k], fids[:, j])  # mirrored by poly()
            np.add.at(offT, dst, term)
            np.add.at(AT, dst, np.abs(term))
            np.add.at(N, dst, 1)
            if AbsT is not None:
                Ua = _unwound_sum(W, Z[:, j][:, None], O[:, j], absolute=True)
                np.add.at(AbsT, dst, np.abs(cond * (O[:, j] - Z[:, j][:, None])) * Ua)
