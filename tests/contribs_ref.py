"""Two float64 references for per-feature contributions (path-dependent TreeSHAP), written from the definition in
include/tahoe_amd.h (tahoe_forest_predict_contribs): test infrastructure, not product.

Decision at a node: |float32(x - missing)| <= 1e-6 -> the default branch, else right iff x >= thr (NaN goes left).  Cover ratio of
a child: w_child / (w_l + w_r).  v(S) = E[f(x) | x_S]: follow the row at nodes whose feature is in S, else mix the children by their
cover ratios.

- brute(): every subset S of the features a tree uses, v(S) by the recursive expectation, the Shapley formula (<= ~10 features).
- poly(): Lundberg et al. 2018, Algorithm 2 (EXTEND / UNWOUND-SUM per leaf path, repeated features merged), vectorised over rows
  and paths; also returns A = sum of |per-path terms| feeding each output, for error bounds.
Both return phi[rows, C, F + 1] (bias last, AVG and global_bias applied as the library does)."""
from __future__ import annotations

import itertools
import math

import numpy as np

EPS = np.float32(1e-6)


def _decode(tree):
    bits = tree["bits"].view(np.uint32)
    return (bits & 0x3FFFFFFF).astype(np.int64), ((bits >> 30) & 1).astype(bool), (bits >> 31).astype(bool), tree["val"], tree["weight"]


def go_right(x, thr, def_left, missing):
    """The library's rule on float32 values: x [rows] float32 -> bool [rows]."""
    with np.errstate(invalid="ignore"):
        is_missing = np.abs(x - np.float32(missing)) <= EPS
        return np.where(is_missing, not def_left, x >= np.float32(thr))


def _ratios(w, i):
    wl, wr = float(w[2 * i + 1]), float(w[2 * i + 2])
    return wl / (wl + wr), wr / (wl + wr)


def tree_expectation(tree):
    """E_t: sum over reachable leaves, left to right, of leaf x product of cover ratios (float64)."""
    fid, dl, leaf, val, w = _decode(tree)
    total = 0.0
    stack = [(0, 1.0)]
    while stack:
        i, p = stack.pop()
        if leaf[i]:
            total += float(val[i]) * p
            continue
        rl, rr = _ratios(w, i)
        stack.append((2 * i + 2, p * rr))
        stack.append((2 * i + 1, p * rl))
    return total


def bias_f32(nodes, T, D, num_classes=1, avg=False, global_bias=0.0):
    per = nodes.size // max(T, 1)
    by_tree = nodes.reshape(T, per) if T else nodes.reshape(0, per)
    out = np.empty(num_classes, np.float32)
    Tc = T // num_classes
    for c in range(num_classes):
        s = 0.0
        for t in range(c, T, num_classes):
            s += tree_expectation(by_tree[t])
        if avg and Tc > 0:
            s = s / Tc
        out[c] = np.float32(s + float(np.float32(global_bias)))
    return out


def _used_features(tree):
    fid, dl, leaf, val, w = _decode(tree)
    used, stack = set(), [0]
    while stack:
        i = stack.pop()
        if leaf[i]:
            continue
        used.add(int(fid[i]))
        stack += [2 * i + 1, 2 * i + 2]
    return sorted(used)


def _value(tree, data, missing, S):
    fid, dl, leaf, val, w = _decode(tree)

    def rec(i):
        if leaf[i]:
            return np.full(data.shape[0], float(val[i]))
        f = int(fid[i])
        if f in S:
            right = go_right(data[:, f], val[i], dl[i], missing)
            return np.where(right, rec(2 * i + 2), rec(2 * i + 1))
        rl, rr = _ratios(w, i)
        return rl * rec(2 * i + 1) + rr * rec(2 * i + 2)

    return rec(0)


def _finish(phi, T, num_classes, avg, bias):
    Tc = T // num_classes
    if avg and Tc > 0:
        phi[:, :, :-1] /= Tc
    phi[:, :, -1] = bias
    return phi


def brute(nodes, T, D, F, data, missing, num_classes=1, avg=False, global_bias=0.0):
    data = np.ascontiguousarray(data, np.float32)
    rows = data.shape[0]
    per = nodes.size // max(T, 1)
    phi = np.zeros((rows, num_classes, F + 1))
    for t in range(T):
        tree = nodes.reshape(T, per)[t]
        U = _used_features(tree)
        n = len(U)
        vals = {}
        for k in range(n + 1):
            for S in itertools.combinations(U, k):
                vals[S] = _value(tree, data, missing, set(S))
        for i in U:
            rest = [u for u in U if u != i]
            acc = np.zeros(rows)
            for k in range(n):
                wgt = math.factorial(k) * math.factorial(n - k - 1) / math.factorial(n)
                for S in itertools.combinations(rest, k):
                    with_i = tuple(sorted(S + (i,)))
                    acc += wgt * (vals[with_i] - vals[S])
            phi[:, t % num_classes, i] += acc
    return _finish(phi, T, num_classes, avg, bias_f32(nodes, T, D, num_classes, avg, global_bias))


def _paths(tree):
    """-> list of (leaf value, [(fid, z, [(thr, def_left, right), ...]) per unique feature in order of first appearance])."""
    fid, dl, leaf, val, w = _decode(tree)
    out = []

    def rec(i, edges):
        if leaf[i]:
            if edges:
                elems = {}
                for (node, right) in edges:
                    rl, rr = _ratios(w, node)
                    f = int(fid[node])
                    e = elems.setdefault(f, [1.0, []])
                    e[0] *= rr if right else rl
                    e[1].append((val[node], bool(dl[node]), right))
                out.append((float(val[i]), [(f, z, ed) for f, (z, ed) in elems.items()]))
            return
        rec(2 * i + 1, edges + [(i, False)])
        rec(2 * i + 2, edges + [(i, True)])

    rec(0, [])
    return out


def poly(nodes, T, D, F, data, missing, num_classes=1, avg=False, global_bias=0.0, chunk=4096):
    """-> (phi [rows, C, F + 1], A [rows, C, F + 1], N [C, F + 1]) in float64; A's bias column is |bias|; N counts the per-path
    terms that feed each output (the n of a recursive-summation bound)."""
    data = np.ascontiguousarray(data, np.float32)
    rows = data.shape[0]
    per = nodes.size // max(T, 1)
    phiT = np.zeros((num_classes, F + 1, rows))
    AT = np.zeros((num_classes, F + 1, rows))
    N = np.zeros((num_classes, F + 1))
    for t in range(T):
        c = t % num_classes
        by_len = {}
        for p in _paths(nodes.reshape(T, per)[t]):
            by_len.setdefault(len(p[1]) + 1, []).append(p)
        for L, paths in by_len.items():
            for lo in range(0, len(paths), chunk):
                _poly_chunk(paths[lo:lo + chunk], L, data, missing, phiT[c], AT[c], N[c])
    phi = np.ascontiguousarray(phiT.transpose(2, 0, 1))
    A = np.ascontiguousarray(AT.transpose(2, 0, 1))
    _finish(phi, T, num_classes, avg, bias_f32(nodes, T, D, num_classes, avg, global_bias))
    Tc = T // num_classes
    if avg and Tc > 0:
        A[:, :, :-1] /= Tc
    A[:, :, -1] = np.abs(phi[:, :, -1])
    return phi, A, N


def _poly_chunk(paths, L, data, missing, phiT, AT, N, dtype=np.float64):
    """dtype: the type the recursion runs in (phiT and AT should have it too): np.longdouble, where it is wider, for paths
    long enough that the unwound sum loses digits a float64 comparison needs"""
    P, rows = len(paths), data.shape[0]
    Z = np.ones((P, L), dtype)
    O = np.ones((P, L, rows), dtype)
    fids = np.zeros((P, L), np.int64)
    leafv = np.array([p[0] for p in paths], dtype)
    for a, (_, elems) in enumerate(paths):
        for j, (f, z, edges) in enumerate(elems, start=1):
            Z[a, j], fids[a, j] = z, f
            o = np.ones(rows, bool)
            for thr, dleft, right in edges:
                o &= go_right(data[:, f], thr, dleft, missing) == right
            O[a, j] = o
    # EXTEND, element by element (the root element first: z = o = 1)
    W = np.zeros((L, P, rows), dtype)
    W[0] = 1.0
    for j in range(1, L):
        zj, oj = Z[:, j][:, None], O[:, j]
        for i in range(j - 1, -1, -1):
            W[i + 1] += oj * W[i] * (i + 1) / (j + 1)
            W[i] = zj * W[i] * (j - i) / (j + 1)
    ud = L - 1
    for k in range(1, L):
        ok, zk = O[:, k], Z[:, k][:, None]
        nxt = W[ud].copy()
        t_one = np.zeros((P, rows), dtype)
        t_zero = np.zeros((P, rows), dtype)
        for i in range(ud - 1, -1, -1):
            tmp = nxt * (ud + 1) / (i + 1)
            t_one += tmp
            nxt = W[i] - tmp * zk * (ud - i) / (ud + 1)
            pre = zk * (ud - i) / (ud + 1)
            with np.errstate(divide="ignore", invalid="ignore"):
                t_zero += np.where(pre > 0, W[i] / np.where(pre > 0, pre, 1.0), 0.0)
        total = np.where(ok > 0, t_one, t_zero)
        term = leafv[:, None] * total * (ok - zk)
        np.add.at(phiT, fids[:, k], term)
        np.add.at(AT, fids[:, k], np.abs(term))
        np.add.at(N, fids[:, k], 1)
