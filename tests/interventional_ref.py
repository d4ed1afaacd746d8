"""Two float64 references for interventional TreeSHAP (tahoe_forest_predict_contribs_interventional), written from the definition
in include/tahoe_amd.h: test infrastructure, not product.

v_r(S) = f(x_S, r_{N \\ S}) for a background row r; phi_i(x) = (1 / B) sum_r phi_i(x, r), the exact Shapley values, per class c
over its trees c, c + C, ...; with AVG divided by Tc.  Every node applies the library's rule to the value it gets: |float32(v -
missing)| <= 1e-6 -> the default branch, else right iff v >= thr (NaN goes left).

- brute(): for each background row, the Shapley formula over all subsets of the F features (F <= ~10), v_r(S) evaluated by
  oracle.predict_f64 on the hybrid rows of each class's sub-forest: independent of any path formulation.
- paths(): the per-leaf-path closed form (Lundberg et al. 2020): A = path features only x follows, B = those only r follows, a
  feature neither follows kills the path; i in A gets +v (|A|-1)! |B|! / (|A|+|B|)!, j in B gets -v |A|! (|B|-1)! / (|A|+|B|)!.
  It walks the caller's nodes itself, merging repeated features, and also returns per output A (the sum of the absolute per-path
  terms feeding it, averaged over the background like phi) and N (the number of path elements feeding it).
Both return phi[rows, C, F + 1] with the bias column of tahoe_forest_set_background (bias_f32) last."""
from __future__ import annotations

import itertools
import math

import numpy as np

EPS = np.float32(1e-6)


def _decode(tree):
    bits = tree["bits"].view(np.uint32)
    return (bits & 0x3FFFFFFF).astype(np.int64), ((bits >> 30) & 1).astype(bool), (bits >> 31).astype(bool), tree["val"]


def go_right(x, thr, def_left, missing):
    """The library's rule on float32 values: x [n] float32 -> bool [n]."""
    with np.errstate(invalid="ignore"):
        is_missing = np.abs(x - np.float32(missing)) <= EPS
        return np.where(is_missing, not def_left, x >= np.float32(thr))


def sub_forest(nodes, T, num_classes, c):
    per = nodes.size // max(T, 1)
    return np.ascontiguousarray(nodes.reshape(T, per)[c::num_classes]).reshape(-1)


def bias_f32(nodes, T, D, bg, missing, num_classes=1, avg=False, global_bias=0.0):
    """The host formula of tahoe_forest_set_background on raw_c(r) = the oracle's float32 tree-order sums (the bits of
    tahoe_forest_predict_raw): (float)((sum_r (double)raw_c(r)) / B / div_c + global_bias)."""
    from oracle import oracle

    bg = np.ascontiguousarray(bg, np.float32)
    Tc = T // num_classes
    out = np.empty(num_classes, np.float32)
    for c in range(num_classes):
        raw = oracle.predict(sub_forest(nodes, T, num_classes, c), Tc, D, bg, missing)[0]
        out[c] = np.float32(bias_from_raw(raw, Tc, avg, global_bias))
    return out


def bias_from_raw(raw, Tc, avg, global_bias):
    s = 0.0
    for v in np.asarray(raw, np.float32):  # background order, float64
        s += float(v)
    m = s / len(raw)
    if avg and Tc > 0:
        m /= Tc
    return m + float(np.float32(global_bias))


def brute(nodes, T, D, F, data, bg, missing, num_classes=1, avg=False, global_bias=0.0):
    from oracle import oracle

    data = np.ascontiguousarray(data, np.float32)
    bg = np.ascontiguousarray(bg, np.float32)
    rows, B, Tc = data.shape[0], bg.shape[0], T // num_classes
    subsets = list(itertools.product((False, True), repeat=F))  # mask of S (True = the feature comes from x)
    masks = np.array(subsets, bool)                                # [2^F, F]
    index = {s: k for k, s in enumerate(subsets)}
    phi = np.zeros((rows, num_classes, F + 1))
    for c in range(num_classes):
        sub = sub_forest(nodes, T, num_classes, c)
        for r in range(B):
            hybrid = np.where(masks[None, :, :], data[:, None, :], bg[r][None, None, :]).reshape(-1, F)
            v = oracle.predict_f64(sub, Tc, D, hybrid, missing).reshape(rows, len(subsets))
            for i in range(F):
                for s, k in index.items():
                    if s[i]:
                        continue
                    n = sum(s)
                    wgt = math.factorial(n) * math.factorial(F - n - 1) / math.factorial(F)
                    with_i = s[:i] + (True,) + s[i + 1:]
                    phi[:, c, i] += wgt * (v[:, index[with_i]] - v[:, k])
    phi[:, :, :F] /= B
    if avg and Tc > 0:
        phi[:, :, :F] /= Tc
    phi[:, :, F] = bias_f32(nodes, T, D, bg, missing, num_classes, avg, global_bias)
    return phi


def _paths(tree):
    """-> list of (leaf value, [(fid, [(thr, def_left, right), ...]) per unique feature in order of first appearance])."""
    fid, dl, leaf, val = _decode(tree)
    out = []

    def rec(i, edges):
        if leaf[i]:
            if edges:
                elems = {}
                for node, right in edges:
                    elems.setdefault(int(fid[node]), []).append((val[node], bool(dl[node]), right))
                out.append((float(val[i]), list(elems.items())))
            return
        rec(2 * i + 1, edges + [(i, False)])
        rec(2 * i + 2, edges + [(i, True)])

    rec(0, [])
    return out


def weight(p, q):
    """(p - 1)! q! / (p + q)! for p >= 1, else 0 (float64)."""
    return 0.0 if p < 1 else math.factorial(p - 1) * math.factorial(q) / math.factorial(p + q)


_W = np.array([[weight(p, q) for q in range(33)] for p in range(33)])


def _follows(v, edges, missing):
    o = np.ones(v.shape[0], bool)
    for thr, dleft, right in edges:
        o &= go_right(v, thr, dleft, missing) == right
    return o


def paths(nodes, T, D, F, data, bg, missing, num_classes=1, avg=False, global_bias=0.0, budget=1 << 22):
    """-> (phi [rows, C, F + 1], A [rows, C, F + 1], N [C, F + 1]) in float64; A's bias column is |bias|."""
    data = np.ascontiguousarray(data, np.float32)
    bg = np.ascontiguousarray(bg, np.float32)
    rows, B = data.shape[0], bg.shape[0]
    per = nodes.size // max(T, 1)
    phiT = np.zeros((num_classes, F + 1, rows))
    AT = np.zeros((num_classes, F + 1, rows))
    N = np.zeros((num_classes, F + 1))
    for t in range(T):
        c = t % num_classes
        by_len = {}
        for p in _paths(nodes.reshape(T, per)[t]):
            by_len.setdefault(len(p[1]), []).append(p)
        for L, group in by_len.items():
            chunk = max(1, budget // max(1, rows * B * L))
            for lo in range(0, len(group), chunk):
                _paths_chunk(group[lo:lo + chunk], L, data, bg, missing, phiT[c], AT[c], N[c])
    phi = np.ascontiguousarray(phiT.transpose(2, 0, 1)) / B
    A = np.ascontiguousarray(AT.transpose(2, 0, 1)) / B
    Tc = T // num_classes
    if avg and Tc > 0:
        phi[:, :, :F] /= Tc
        A[:, :, :F] /= Tc
    phi[:, :, F] = bias_f32(nodes, T, D, bg, missing, num_classes, avg, global_bias)
    A[:, :, F] = np.abs(phi[:, :, F])
    return phi, A, N


def _paths_chunk(group, L, data, bg, missing, phiT, AT, N):
    P = len(group)
    Ox = np.zeros((P, L, data.shape[0]), bool)
    Or = np.zeros((P, L, bg.shape[0]), bool)
    fids = np.zeros((P, L), np.int64)
    leafv = np.array([g[0] for g in group])
    for a, (_, elems) in enumerate(group):
        for j, (f, edges) in enumerate(elems):
            fids[a, j] = f
            Ox[a, j] = _follows(data[:, f], edges, missing)
            Or[a, j] = _follows(bg[:, f], edges, missing)
    inA = Ox[:, :, :, None] & ~Or[:, :, None, :]  # [P, L, rows, B]
    inB = ~Ox[:, :, :, None] & Or[:, :, None, :]
    dead = (~Ox[:, :, :, None] & ~Or[:, :, None, :]).any(axis=1)  # [P, rows, B]
    na, nb = inA.sum(axis=1), inB.sum(axis=1)
    live = leafv[:, None, None] * ~dead
    wa, wb = _W[na, nb] * live, _W[nb, na] * live  # [P, rows, B]
    for j in range(L):
        term = np.where(inA[:, j], wa, 0.0) - np.where(inB[:, j], wb, 0.0)
        np.add.at(phiT, fids[:, j], term.sum(axis=-1))
        np.add.at(AT, fids[:, j], np.abs(term).sum(axis=-1))
        np.add.at(N, fids[:, j], 1)
