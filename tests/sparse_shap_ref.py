"""Float64 brute-force references for TreeSHAP on sparse (irregular) forests, written from the definitions in include/tahoe_amd.h:
test infrastructure, not product.  The references of contribs_ref / interactions_ref / interventional_ref walk complete heaps;
these walk sparse trees (left child left_idx, right child left_idx + 1, relative to the tree's root) of any depth.

Branch rule: |float32(x - missing)| <= 1e-6 -> the default branch, else right iff x >= thr (NaN goes left).  Tree t belongs to class
t % C.  Every feature of [0, F) is a player (features a tree does not use are dummies), so F must stay small (2^F subsets).

- contribs(): Shapley values of v(S) = E[f(x) | x_S] (cover-weighted mix at nodes whose feature is not in S), bias last;
  bias_column() the library's float32 bias column, summed in its order.
- interactions(): the Shapley interaction index of the same game off the diagonal; the diagonal as the library defines it
  (phi_i minus the row's off-diagonal sum) is left to the caller.
- interventional(): Shapley values of v_r(S) = f(x_S, r_rest), averaged over the background rows, bias last (from the float32 raw
  sums of the background, as tahoe_forest_set_background computes it).
- bound_scale(): per (row, class) an upper bound of the sum of |per-path terms| the kernels add (sum over leaves of |leaf| x the
  path's distinct features), for error bars of the kind the dense SHAP tests use."""
from __future__ import annotations

import itertools
import math

import numpy as np

EPS = np.float32(1e-6)
LEAF = 1 << 31


def trees_of(sn, tr):
    """[(nodes of tree t as a view, t)] -- node indices inside a view are root-relative."""
    ends = np.append(tr[1:], sn.size)
    return [sn[int(tr[t]):int(ends[t])] for t in range(tr.size)]


def sub_forest(sn, tr, c, C, covers=None):
    """Trees c, c + C, ... of a sparse forest, concatenated, root offsets rebased (and their covers)."""
    trees = trees_of(sn, tr)
    ends = np.append(tr[1:], sn.size)
    idx = list(range(c, tr.size, C))
    nodes = np.concatenate([trees[t] for t in idx]) if idx else sn[:0]
    roots = np.cumsum([0] + [trees[t].size for t in idx[:-1]]).astype(np.int32) if idx else np.zeros(0, np.int32)
    if covers is None:
        return nodes, roots
    cv = np.concatenate([covers[int(tr[t]):int(ends[t])] for t in idx]) if idx else covers[:0]
    return nodes, roots, cv


def _go_right(x, thr, def_left, missing):
    with np.errstate(invalid="ignore"):
        is_missing = np.abs(x - np.float32(missing)) <= EPS
        return np.where(is_missing, not def_left, x >= np.float32(thr))


def _cond_exp(tree, cov, x, S, missing):
    """v(S) for every row of x: float64 [rows]."""
    bits = tree["bits"].view(np.uint32)

    def rec(i):
        if bits[i] >> 31:
            return np.full(x.shape[0], float(tree["val"][i]))
        fid, dl = int(bits[i] & 0x3FFFFFFF), bool((bits[i] >> 30) & 1)
        li = int(tree["left_idx"][i])
        if fid in S:
            r = _go_right(x[:, fid], tree["val"][i], dl, missing)
            return np.where(r, rec(li + 1), rec(li))
        wl, wr = float(cov[li]), float(cov[li + 1])
        return (wl * rec(li) + wr * rec(li + 1)) / (wl + wr)

    return rec(0)


def _games(sn, tr, covers, x, F, missing, C):
    """v[c][mask] = sum over class c's trees of v_t(S), S = the bits of mask: float64 [rows]."""
    ends = np.append(tr[1:], sn.size)
    v = [[np.zeros(x.shape[0]) for _ in range(1 << F)] for _ in range(C)]
    for t in range(tr.size):
        tree, cov = sn[int(tr[t]):int(ends[t])], covers[int(tr[t]):int(ends[t])]
        for mask in range(1 << F):
            S = {i for i in range(F) if mask >> i & 1}
            v[t % C][mask] += _cond_exp(tree, cov, x, S, missing)
    return v


def expectation(tree, cov):
    """E_t as the library sums it in float64: leaves in pre-order (left first), leaf x the product of the cover ratios from the
    root down."""
    bits = tree["bits"].view(np.uint32)
    total, stack = 0.0, [(0, 1.0)]
    while stack:
        i, p = stack.pop()
        if bits[i] >> 31:
            total += float(tree["val"][i]) * p
            continue
        li = int(tree["left_idx"][i])
        wl, wr = float(cov[li]), float(cov[li + 1])
        stack.append((li + 1, p * (wr / (wl + wr))))
        stack.append((li, p * (wl / (wl + wr))))
    return total


def bias_column(sn, tr, covers, C=1, avg=False, global_bias=0.0):
    """[C] float32: the bias column of tahoe_forest_predict_contribs, bit for bit."""
    ends = np.append(tr[1:], sn.size)
    Tc = tr.size // C
    out = np.empty(C, np.float32)
    for c in range(C):
        e = 0.0
        for t in range(c, tr.size, C):
            e += expectation(sn[int(tr[t]):int(ends[t])], covers[int(tr[t]):int(ends[t])])
        out[c] = np.float32((e / Tc if avg and Tc else e) + float(global_bias))
    return out


def contribs(sn, tr, covers, x, F, missing, C=1, avg=False, global_bias=0.0):
    x = np.ascontiguousarray(x, np.float32)
    v = _games(sn, tr, covers, x, F, missing, C)
    Tc = tr.size // C
    phi = np.zeros((x.shape[0], C, F + 1))
    for c in range(C):
        for i in range(F):
            for mask in range(1 << F):
                if mask >> i & 1:
                    continue
                s = bin(mask).count("1")
                w = math.factorial(s) * math.factorial(F - s - 1) / math.factorial(F)
                phi[:, c, i] += w * (v[c][mask | 1 << i] - v[c][mask])
        phi[:, c, F] = v[c][0]
        if avg and Tc:
            phi[:, c, :] /= Tc
        phi[:, c, F] += global_bias
    return phi


def interactions(sn, tr, covers, x, F, missing, C=1, avg=False):
    """Off-diagonal Shapley interaction index [rows, C, F, F] (diagonal zero)."""
    x = np.ascontiguousarray(x, np.float32)
    v = _games(sn, tr, covers, x, F, missing, C)
    Tc = tr.size // C
    out = np.zeros((x.shape[0], C, F, F))
    for c in range(C):
        for i, j in itertools.combinations(range(F), 2):
            acc = np.zeros(x.shape[0])
            for mask in range(1 << F):
                if mask >> i & 1 or mask >> j & 1:
                    continue
                s = bin(mask).count("1")
                w = math.factorial(s) * math.factorial(F - s - 2) / (2 * math.factorial(F - 1))
                acc += w * (v[c][mask | 1 << i | 1 << j] - v[c][mask | 1 << i] - v[c][mask | 1 << j] + v[c][mask])
            out[:, c, i, j] = out[:, c, j, i] = acc / (Tc if avg and Tc else 1)
    return out


def _predict64(sn, tr, data, missing, C):
    """Raw per-class sums in float64 [rows, C]."""
    ends = np.append(tr[1:], sn.size)
    out = np.zeros((data.shape[0], C))
    for t in range(tr.size):
        tree = sn[int(tr[t]):int(ends[t])]
        bits = tree["bits"].view(np.uint32)
        node = np.zeros(data.shape[0], np.int64)
        while True:
            b = bits[node]
            inner = (b >> 31) == 0
            if not inner.any():
                break
            fid = (b & 0x3FFFFFFF).astype(np.int64)
            xv = data[np.arange(data.shape[0]), np.where(inner, fid, 0)]
            thr = tree["val"][node]
            with np.errstate(invalid="ignore"):
                is_missing = np.abs(xv - np.float32(missing)) <= EPS
                right = np.where(is_missing, ((b >> 30) & 1) == 0, xv >= thr)
            node = np.where(inner, tree["left_idx"][node] + right.astype(np.int64), node)
        out[:, t % C] += tree["val"][node]
    return out


def interventional(sn, tr, x, bg, F, missing, C=1, avg=False, global_bias=0.0, bg_raw=None):
    """phi [rows, C, F + 1]; bg_raw: float32 raw sums [B, C] of the background (the library's), for the bias column."""
    x = np.ascontiguousarray(x, np.float32)
    bg = np.ascontiguousarray(bg, np.float32)
    R, B = x.shape[0], bg.shape[0]
    Tc = tr.size // C
    masks = np.array([[mask >> i & 1 for i in range(F)] for mask in range(1 << F)], bool)  # [2^F, F]
    hyb = np.where(masks[:, None, None, :], x[None, :, None, :], bg[None, None, :, :])  # [2^F, R, B, F]
    v = _predict64(sn, tr, hyb.reshape(-1, F), missing, C).reshape(1 << F, R, B, C)
    phi = np.zeros((R, C, F + 1))
    for i in range(F):
        for mask in range(1 << F):
            if mask >> i & 1:
                continue
            s = bin(mask).count("1")
            w = math.factorial(s) * math.factorial(F - s - 1) / math.factorial(F)
            phi[:, :, i] += w * (v[mask | 1 << i] - v[mask]).mean(axis=1)
    if avg and Tc:
        phi[:, :, :F] /= Tc
    raw = bg_raw.astype(np.float64) if bg_raw is not None else _predict64(sn, tr, bg, missing, C)
    m = np.zeros(C)
    for r in range(B):  # in background order, as the library sums
        m += raw[r]
    m /= B
    if avg and Tc:
        m /= Tc
    phi[:, :, F] = (m + global_bias).astype(np.float32)
    return phi


def bound_scale(sn, tr, C=1):
    """[C]: sum over reachable leaves of |leaf| x (distinct features on its path), per class; and the longest path, the
    number of paths."""
    ends = np.append(tr[1:], sn.size)
    scale = np.zeros(C)
    depth = paths = 0
    for t in range(tr.size):
        tree = sn[int(tr[t]):int(ends[t])]
        bits = tree["bits"].view(np.uint32)
        stack = [(0, frozenset(), 0)]
        while stack:
            i, feats, d = stack.pop()
            if bits[i] >> 31:
                scale[t % C] += abs(float(tree["val"][i])) * len(feats)
                depth, paths = max(depth, d), paths + 1
                continue
            f2 = feats | {int(bits[i] & 0x3FFFFFFF)}
            li = int(tree["left_idx"][i])
            stack += [(li, f2, d + 1), (li + 1, f2, d + 1)]
    return scale, depth, paths
