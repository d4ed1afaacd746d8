"""Two float64 references for interventional TreeSHAP on an oblivious handle (TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL,
tahoe_forest_predict_contribs_interventional), written from the definition in include/tahoe_amd.h: test infrastructure, not
product.

v_r(S) = f(x_S, r_{N \\ S}) for a background row r; phi_i(x) = (1 / B) sum_r phi_i(x, r), the exact Shapley values, per output k
over all trees; with AVG divided by T.

- brute(): for each background row, the Shapley formula over all subsets of the features the forest uses (at most 8), v_r(S)
  from the leaf indices oblivious_ref reports for the hybrid rows, the leaves summed in float64: independent of any formulation.
- paths(): the histogram form.  A background row enters a tree only through its leaf index R, so per tree the background is its
  occupied leaves with integer counts.  With X the row's leaf index, diff = X ^ R and the tree's distinct features e with level
  masks mask_e, the players are U = {e : diff & mask_e != 0}, u = |U|; the live leaves are j = R ^ (diff & OR_{e in S} mask_e) for
  S a subset of U, s = |S|; leaf j gives e in S the weight +(s - 1)! (u - s)! / u! and e in U \\ S the weight -s! (u - s - 1)! / u!,
  times count times leaf[j][k].  It also returns per output A (the sum of the absolute terms feeding it, scaled like phi) and N
  (the number of (tree, occupied leaf, subset) terms feeding it).
Both return phi[rows, K, F + 1] with the bias column of tahoe_forest_set_background last."""
from __future__ import annotations

import math

import numpy as np

import interventional_ref as ivr
import oblivious_ref as obr


def _offsets(forest):
    d = np.asarray(forest["depths"], np.int64)
    return d, np.concatenate([[0], np.cumsum(d)]), np.concatenate([[0], np.cumsum(1 << d)])


def bias(forest, bg, missing=obr.MISSING, avg=False, global_bias=0.0):
    """The host formula of tahoe_forest_set_background on raw_k(r) = oblivious_ref's float32 tree-order sums -> float32 [K]"""
    raw, _ = obr.ref_of(forest, bg, missing)
    T = len(forest["depths"])
    return np.array([np.float32(ivr.bias_from_raw(raw[:, k], T, avg, global_bias)) for k in range(forest["k"])], np.float32)


def elements(fids):
    """The distinct features of a tree's levels in order of first appearance from level 0 -> (features, level masks)"""
    feats, masks = [], []
    for l, f in enumerate(fids):
        f = int(f)
        if f not in feats:
            feats.append(f)
            masks.append(0)
        masks[feats.index(f)] |= 1 << l
    return feats, masks


def brute(forest, data, bg, missing=obr.MISSING, avg=False, global_bias=0.0):
    data, bg = np.ascontiguousarray(data, np.float32), np.ascontiguousarray(bg, np.float32)
    F, K = forest["cols"], forest["k"]
    d, _, lo = _offsets(forest)
    T, rows, B = d.size, data.shape[0], bg.shape[0]
    used = sorted(set(int(f) for f in forest["fids"]))
    n = len(used)
    assert n <= 8
    leaves = np.asarray(forest["leaves"], np.float32).reshape(-1, K).astype(np.float64)
    from_x = np.zeros((1 << n, F), bool)  # subset s: bit p set = feature used[p] comes from x
    for s in range(1 << n):
        for p, f in enumerate(used):
            from_x[s, f] = (s >> p) & 1
    size = np.array([bin(s).count("1") for s in range(1 << n)])
    phi = np.zeros((rows, K, F + 1))
    for r in range(B):
        hybrid = np.where(from_x[None, :, :], data[:, None, :], bg[r][None, None, :]).reshape(-1, F)
        _, leaf = obr.ref_of(forest, hybrid, missing)
        v = np.zeros((hybrid.shape[0], K))
        for t in range(T):
            v += leaves[lo[t] + leaf[:, t].astype(np.int64)]
        v = v.reshape(rows, 1 << n, K)
        for p, f in enumerate(used):
            for s in range(1 << n):
                if (s >> p) & 1:
                    continue
                wgt = math.factorial(size[s]) * math.factorial(n - size[s] - 1) / math.factorial(n)
                phi[:, :, f] += wgt * (v[:, s | (1 << p)] - v[:, s])
    phi /= B
    if avg and T > 0:
        phi /= T
    phi[:, :, F] = bias(forest, bg, missing, avg, global_bias)
    return phi


def w_plus(u, s):
    return math.factorial(s - 1) * math.factorial(u - s) / math.factorial(u) if 1 <= s <= u else 0.0


def w_minus(u, s):
    return math.factorial(s) * math.factorial(u - s - 1) / math.factorial(u) if 0 <= s < u else 0.0


_WP = np.array([[w_plus(u, s) for s in range(17)] for u in range(17)])
_WM = np.array([[w_minus(u, s) for s in range(17)] for u in range(17)])


def occupancy(forest, bg, missing=obr.MISSING):
    """Per tree the occupied leaves, ascending, and their counts -> list of (leaves int64, counts int64)"""
    _, leaf = obr.ref_of(forest, np.ascontiguousarray(bg, np.float32), missing)
    return [np.unique(leaf[:, t].astype(np.int64), return_counts=True) for t in range(leaf.shape[1])]


def paths(forest, data, bg, missing=obr.MISSING, avg=False, global_bias=0.0):
    """-> (phi, A, N), each [rows, K, F + 1] in float64; A's bias column is |bias|, N's is 0."""
    data, bg = np.ascontiguousarray(data, np.float32), np.ascontiguousarray(bg, np.float32)
    F, K = forest["cols"], forest["k"]
    d, so, lo = _offsets(forest)
    T, rows, B = d.size, data.shape[0], bg.shape[0]
    leaves = np.asarray(forest["leaves"], np.float32).reshape(-1, K).astype(np.float64)
    _, xleaf = obr.ref_of(forest, data, missing)
    occ = occupancy(forest, bg, missing)
    phi, A, N = np.zeros((rows, K, F + 1)), np.zeros((rows, K, F + 1)), np.zeros((rows, K, F + 1))
    for t in range(T):
        feats, masks = elements(np.asarray(forest["fids"])[so[t]:so[t + 1]])
        m = len(feats)
        X = xleaf[:, t].astype(np.int64)
        for R, count in zip(*occ[t]):
            diff = X ^ int(R)
            dU = np.zeros(rows, np.int64)
            for e in range(m):
                dU |= ((diff & masks[e]) != 0).astype(np.int64) << e
            for players in np.unique(dU):
                players = int(players)
                if players == 0:
                    continue
                at = np.nonzero(dU == players)[0]
                u = bin(players).count("1")
                subs, sub = [], players  # every submask of the player set
                while True:
                    subs.append(sub)
                    if sub == 0:
                        break
                    sub = (sub - 1) & players
                subs = np.array(subs, np.int64)
                s = np.zeros(subs.size, np.int64)
                lm = np.zeros(subs.size, np.int64)
                for e in range(m):
                    bit = (subs >> e) & 1
                    s += bit
                    lm |= bit * masks[e]
                j = int(R) ^ (diff[at][:, None] & lm[None, :])
                val = leaves[lo[t] + j]  # [rows of the group, subsets, K]
                wp, wm = _WP[u][s], _WM[u][s]
                for e in range(m):
                    if not (players >> e) & 1:
                        continue
                    w = np.where((subs >> e) & 1, wp, -wm)[None, :, None] * float(count)
                    phi[at, :, feats[e]] += (w * val).sum(axis=1)
                    A[at, :, feats[e]] += (np.abs(w) * np.abs(val)).sum(axis=1)
                    N[at, :, feats[e]] += subs.size
    phi /= B
    A /= B
    if avg and T > 0:
        phi /= T
        A /= T
    phi[:, :, F] = bias(forest, bg, missing, avg, global_bias)
    A[:, :, F] = np.abs(phi[:, :, F])
    return phi, A, N
