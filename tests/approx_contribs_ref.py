"""Numpy restatement of Saabas contributions (TAHOE_CREATE_APPROX_CONTRIBS, tahoe_forest_predict_contribs_approx), written from
the definition in include/tahoe_amd.h: test infrastructure, not product.

Node means in float64 from the caller's trees: E(leaf) = val, E(n) = (wl * E(l) + wr * E(r)) / (wl + wr); each child of an internal
node carries d(child) = float32(E(child) - E(n)).  Per row and tree the row follows predict's path (|float32(x - missing)| <= 1e-6
-> default branch, else right iff x >= thr; NaN goes left) and every internal node on it adds d(child taken) to phi[c][fid] in
float32.  The sums start from +0.0 and run over class c's trees c, c + C, ... in order, root to leaf within a tree: one float32 add
per (tree, level), vectorised over rows, so the result is bit-exact by construction.  AVG divides the finished sums by
float32(Tc); the bias column is contribs_ref's (dense) or sparse_shap_ref's (sparse) bias column.

dense() / sparse() return phi[rows, C, F + 1]; with scale=True also S[rows, C] = the float64 sum of |d| over every add and
N[rows, C] = the number of adds, for error bounds.  direct64() is an independent per-row loop in float64 (no vectorisation, no
float32 rounding) for cross-checks on small forests."""
from __future__ import annotations

import numpy as np

import contribs_ref
import sparse_shap_ref

EPS = np.float32(1e-6)


def _go_right(x, thr, def_left, missing):
    """Per-row rule on float32 arrays: x, thr, def_left [n] -> bool [n]."""
    with np.errstate(invalid="ignore"):
        is_missing = np.abs(x - np.float32(missing)) <= EPS
        return np.where(is_missing, ~def_left, x >= thr)


def _means(val, is_leaf, left, w, heap):
    """E[n] for every node of one tree in float64; children lie after their parent (heap or sparse order).  Nodes no walk reaches
    may get any value."""
    n = val.size
    E = np.zeros(n)
    inner = ~is_leaf & (left + 1 < n)
    E[is_leaf] = val[is_leaf].astype(np.float64)
    if heap and n > 1:  # a complete heap: level by level, bottom up, elementwise float64 (same operations, same order)
        lv = n.bit_length() - 1
        for l in range(lv - 1, -1, -1):
            i = np.arange((1 << l) - 1, (2 << l) - 1)
            i = i[inner[i]]
            wl, wr = w[2 * i + 1].astype(np.float64), w[2 * i + 2].astype(np.float64)
            with np.errstate(all="ignore"):
                E[i] = (wl * E[2 * i + 1] + wr * E[2 * i + 2]) / (wl + wr)
        return E
    for i in range(n - 1, -1, -1):
        if inner[i]:
            l = int(left[i])
            wl, wr = float(w[l]), float(w[l + 1])
            E[i] = (wl * E[l] + wr * E[l + 1]) / (wl + wr) if wl + wr != 0.0 else np.nan
    return E


def _tree_arrays(tree, left, w, heap):
    bits = tree["bits"].view(np.uint32)
    fid = (bits & 0x3FFFFFFF).astype(np.int64)
    def_left = ((bits >> 30) & 1).astype(bool)
    is_leaf = (bits >> 31).astype(bool)
    val = tree["val"].astype(np.float32)
    E = _means(val, is_leaf, left, w, heap)
    d = np.zeros(val.size, np.float32)  # d of every child, by the child's index
    i = np.nonzero(~is_leaf & (left + 1 < val.size))[0]
    with np.errstate(all="ignore"):
        d[left[i]] = (E[left[i]] - E[i]).astype(np.float32)
        d[left[i] + 1] = (E[left[i] + 1] - E[i]).astype(np.float32)
    return fid, def_left, is_leaf, val, d


def _walk(phi, S, N, c, arrays, left, x, missing):
    fid, def_left, is_leaf, val, d = arrays
    rows = x.shape[0]
    idx = np.zeros(rows, np.int64)
    active = np.full(rows, not is_leaf[0])
    while active.any():
        r = np.nonzero(active)[0]
        i = idx[r]
        f = fid[i]
        go = _go_right(x[r, f], val[i], def_left[i], missing)
        child = left[i] + go.astype(np.int64)
        with np.errstate(over="ignore", invalid="ignore"):  # leaves near FLT_MAX: +-inf and NaN sums are the IEEE results
            phi[r, c, f] += d[child]  # one float32 add per row: rows are distinct
        if S is not None:
            S[r, c] += np.abs(d[child].astype(np.float64))
            N[r, c] += 1
        idx[r] = child
        active[r] = ~is_leaf[child]


def _finish(phi, S, N, C, Tc, avg, bias, F, scale):
    if avg and Tc > 0:
        phi[:, :, :F] /= np.float32(Tc)
    phi[:, :, F] = bias[None, :]
    return (phi, S, N) if scale else phi


def dense(nodes, T, D, F, x, missing, num_classes=1, avg=False, global_bias=0.0, scale=False):
    x = np.ascontiguousarray(x, np.float32)
    per = (1 << (D + 1)) - 1
    C, rows = num_classes, x.shape[0]
    phi = np.zeros((rows, C, F + 1), np.float32)
    S = np.zeros((rows, C)) if scale else None
    N = np.zeros((rows, C), np.int64) if scale else None
    left = 2 * np.arange(per, dtype=np.int64) + 1
    by_tree = nodes.reshape(T, per) if T else nodes.reshape(0, per)
    for c in range(C):
        for t in range(c, T, C):
            tree = by_tree[t]
            _walk(phi, S, N, c, _tree_arrays(tree, left, tree["weight"], True), left, x, missing)
    bias = contribs_ref.bias_f32(nodes, T, D, C, avg, global_bias)
    return _finish(phi, S, N, C, T // C, avg, bias, F, scale)


def sparse(sn, tr, covers, F, x, missing, num_classes=1, avg=False, global_bias=0.0, scale=False):
    x = np.ascontiguousarray(x, np.float32)
    C, rows, T = num_classes, x.shape[0], tr.size
    phi = np.zeros((rows, C, F + 1), np.float32)
    S = np.zeros((rows, C)) if scale else None
    N = np.zeros((rows, C), np.int64) if scale else None
    ends = np.append(tr[1:], sn.size)
    for c in range(C):
        for t in range(c, T, C):
            a, b = int(tr[t]), int(ends[t])
            tree = sn[a:b]
            left = tree["left_idx"].astype(np.int64)
            _walk(phi, S, N, c, _tree_arrays(tree, left, covers[a:b], False), left, x, missing)
    bias = sparse_shap_ref.bias_column(sn, tr, covers, C, avg, global_bias)
    return _finish(phi, S, N, C, T // C, avg, bias, F, scale)


def direct64(nodes, T, D, F, x, missing, num_classes=1, avg=False, global_bias=0.0):
    """Saabas sums in float64, row by row and node by node, with node means by recursion: [rows, C, F + 1] float64."""
    per = (1 << (D + 1)) - 1
    by_tree = nodes.reshape(T, per)
    C, Tc = num_classes, T // num_classes
    out = np.zeros((x.shape[0], C, F + 1))

    def mean(tree, i):
        bits = int(tree["bits"][i]) & 0xFFFFFFFF
        if bits >> 31:
            return float(tree["val"][i])
        wl, wr = float(tree["weight"][2 * i + 1]), float(tree["weight"][2 * i + 2])
        return (wl * mean(tree, 2 * i + 1) + wr * mean(tree, 2 * i + 2)) / (wl + wr)

    for t in range(T):
        tree, c = by_tree[t], t % C
        for r in range(x.shape[0]):
            i = 0
            while not (int(tree["bits"][i]) & 0xFFFFFFFF) >> 31:
                bits = int(tree["bits"][i]) & 0xFFFFFFFF
                f, dl = bits & 0x3FFFFFFF, bool((bits >> 30) & 1)
                xv = np.float32(x[r, f])
                with np.errstate(invalid="ignore"):
                    if abs(np.float32(xv - np.float32(missing))) <= EPS:
                        right = not dl
                    else:
                        right = bool(xv >= tree["val"][i])
                child = 2 * i + 1 + int(right)
                out[r, c, f] += mean(tree, child) - mean(tree, i)
                i = child
    if avg:
        out[:, :, :F] /= Tc
    for c in range(C):
        out[:, c, F] = sum(contribs_ref.tree_expectation(by_tree[t]) for t in range(c, T, C)) / (Tc if avg else 1) + global_bias
    return out
