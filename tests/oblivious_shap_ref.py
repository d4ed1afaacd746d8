"""Float64 references for the explanations of an oblivious handle (tahoe_oblivious_forest_create_ex), written from the definition
in include/tahoe_amd.h: test infrastructure, not product.

A forest is oblivious_ref.make_forest's dict; covers holds one float per leaf in the order of the leaves.  The implicit heap of a
tree of depth D: level l has 2^l nodes numbered by the l low bits of the leaf index; the children of node p of level l are p
(left) and p | 1 << l (right) of level l + 1.  A node's cover is the float64 sum of the leaf covers below it; a node of positive
cover mixes its children by w_child / (w_l + w_r), a node of cover 0 by 1/2 and 1/2.

- bias_f32: sum_t E_t[k] (/ T with AVG) + global_bias in float64, rounded once; E_t[k] = the leaves in heap order left to right,
  each times the product of its path's ratios multiplied root first (contribs_ref.tree_expectation on the expansion).
- brute: Shapley values from the definition, v(S) = E[f(x) | x_S], over the subsets of the features a tree uses (<= 8).
- poly: per leaf j the EXTEND / unwound-sum recursion over the tree's m distinct features, o_e = ((idx ^ j) & mask_e) == 0, a leaf
  with z_e == 0 and o_e == 0 for some e skipped; also A = the sum of |per-leaf terms| and N = their count, per output.
- emulate: the kernel's tables and its per-leaf recursion restated operation for operation in float32: bit-exact by construction.
- saabas: float64 node means, float32 deltas, one float32 add per (tree, level) in order: bit-exact by construction.
- expand_with_covers: the heap expansion (oblivious_ref.expand_to_dense) with `weight` = the subtree cover.
- shap_form: the rule by which the library picks the LDS or the in-place form."""
from __future__ import annotations

import itertools
import math

import numpy as np

import oblivious_ref as obr

MIN_Z = 2.0 ** -121  # zero fractions below it count as 0 (kContribMinZ)
CLASS_BLOCK = 4      # kObShapClasses


def shap_form(used: int, k: int, lds_bytes: int, forced_inplace: bool = False) -> str:
    """'lds' when the 64-row tile of the used features and the slab of min(k, 4) classes (odd row stride) fit the device's LDS"""
    stride = (min(k, CLASS_BLOCK) * used) | 1
    return "inplace" if forced_inplace or 256 * (used + stride) > lds_bytes else "lds"


def _offsets(forest):
    d = np.asarray(forest["depths"], np.int64)
    return d, np.concatenate([[0], np.cumsum(d)]), np.concatenate([[0], np.cumsum(1 << d)])


def heap(depth, leaf_covers):
    """-> (cover[l][node], ratio[l][node] for l >= 1) of one tree, float64"""
    cover = [None] * (depth + 1)
    ratio = [None] * (depth + 1)
    cover[depth] = np.asarray(leaf_covers, np.float64).copy()
    for l in range(depth - 1, -1, -1):
        n = 1 << l
        wl, wr = cover[l + 1][:n], cover[l + 1][n:]
        cover[l] = wl + wr
        pos = cover[l] > 0
        safe = np.where(pos, cover[l], 1.0)
        ratio[l + 1] = np.concatenate([np.where(pos, wl / safe, 0.5), np.where(pos, wr / safe, 0.5)])
    return cover, ratio


def node_means(depth, cover, leaf_vals):
    """E[l][node, k] in float64: (w_l E(l) + w_r E(r)) / (w_l + w_r), or (E(l) + E(r)) / 2 at a node of cover 0"""
    E = [None] * (depth + 1)
    E[depth] = np.asarray(leaf_vals, np.float64)
    for l in range(depth - 1, -1, -1):
        n = 1 << l
        wl, wr = cover[l + 1][:n, None], cover[l + 1][n:, None]
        el, er = E[l + 1][:n], E[l + 1][n:]
        pos = (wl + wr) > 0
        E[l] = np.where(pos, (wl * el + wr * er) / np.where(pos, wl + wr, 1.0), (el + er) / 2.0)
    return E


def tree_expect(depth, ratio, leaf_vals):
    """E_t[k]: sum over the leaves, heap order left to right, of value x product of the ratios root first"""
    prod = np.ones(1)
    for l in range(depth):
        q = np.arange(2 << l)
        prod = prod[q & ((1 << l) - 1)] * ratio[l + 1]
    e = np.zeros(leaf_vals.shape[1])
    for h in range(1 << depth):
        j = int(obr.bitreverse(h, depth))
        e = e + leaf_vals[j].astype(np.float64) * prod[j]
    return e


def _trees(forest, covers):
    d, s, lo = _offsets(forest)
    k = forest["k"]
    leaves = np.asarray(forest["leaves"], np.float32).reshape(-1, k)
    covers = np.asarray(covers, np.float32)
    for t in range(d.size):
        D = int(d[t])
        yield t, D, np.asarray(forest["fids"][s[t]:s[t + 1]], np.int64), slice(s[t], s[t + 1]), leaves[lo[t]:lo[t + 1]], \
            covers[lo[t]:lo[t + 1]]


def bias_f32(forest, covers, avg=False, global_bias=0.0):
    k, T = forest["k"], len(forest["depths"])
    total = np.zeros(k)
    for t, D, fids, sl, lv, cv in _trees(forest, covers):
        _, ratio = heap(D, cv)
        total = total + tree_expect(D, ratio, lv)
    if avg and T > 0:
        total = total / T
    return (total + float(np.float32(global_bias))).astype(np.float32)


def _bits(forest, sl, data, missing):
    """right[l, rows] of the tree's levels, predict's rule"""
    out = []
    with np.errstate(invalid="ignore"):
        for s in range(sl.start, sl.stop):
            x = data[:, int(forest["fids"][s])]
            miss = np.abs(x - np.float32(missing)) <= np.float32(1e-6)
            out.append(np.where(miss, not bool(forest["def_left"][s]), x >= np.float32(forest["thr"][s])))
    return np.array(out, bool).reshape(len(out), data.shape[0])


def _finish(phi, forest, covers, avg, global_bias):
    T = len(forest["depths"])
    if avg and T > 0:
        phi[:, :, :-1] /= T
    phi[:, :, -1] = bias_f32(forest, covers, avg, global_bias)[None, :]
    return phi


def brute(forest, covers, data, missing=obr.MISSING, avg=False, global_bias=0.0):
    data = np.ascontiguousarray(data, np.float32)
    rows, k, F = data.shape[0], forest["k"], forest["cols"]
    phi = np.zeros((rows, k, F + 1))
    for t, D, fids, sl, lv, cv in _trees(forest, covers):
        _, ratio = heap(D, cv)
        right = _bits(forest, sl, data, missing)
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
        for i in U:
            rest = [u for u in U if u != i]
            for size in range(n):
                w = math.factorial(size) * math.factorial(n - size - 1) / math.factorial(n)
                for S in itertools.combinations(rest, size):
                    phi[:, :, i] += w * (vals[tuple(sorted(S + (i,)))] - vals[S])
    return _finish(phi, forest, covers, avg, global_bias)


def poly(forest, covers, data, missing=obr.MISSING, avg=False, global_bias=0.0):
    """-> (phi, A, N), each [rows, K, F + 1] float64; A's bias column is |bias|, N's is 0"""
    data = np.ascontiguousarray(data, np.float32)
    rows, k, F = data.shape[0], forest["k"], forest["cols"]
    phi = np.zeros((rows, k, F + 1))
    A = np.zeros((rows, k, F + 1))
    N = np.zeros((rows, k, F + 1))
    for t, D, fids, sl, lv, cv in _trees(forest, covers):
        if D == 0:
            continue
        _, ratio = heap(D, cv)
        right = _bits(forest, sl, data, missing)
        idx = np.zeros(rows, np.int64)
        for l in range(D):
            idx |= right[l].astype(np.int64) << l
        feats, masks = [], []
        for l in range(D):
            f = int(fids[l])
            if f not in feats:
                feats.append(f)
                masks.append(0)
            masks[feats.index(f)] |= 1 << l
        m, nleaf = len(feats), 1 << D
        j = np.arange(nleaf)
        Z = np.ones((m, nleaf))
        for e in range(m):
            for l in range(D):
                if masks[e] >> l & 1:
                    Z[e] = Z[e] * ratio[l + 1][j & ((2 << l) - 1)]
        Zc = np.where(Z < MIN_Z, 0.0, Z)
        mism = idx[None, :] ^ j[:, None]  # [leaves, rows]
        O = np.array([(mism & masks[e]) == 0 for e in range(m)])  # [m, leaves, rows]
        live = ~np.any((Zc[:, :, None] == 0.0) & ~O, axis=0)
        # EXTEND
        W = np.zeros((m + 1, nleaf, rows))
        W[0] = 1.0
        for e in range(m):
            l = e + 1
            z, o = Zc[e][:, None], O[e]
            for i in range(l - 1, -1, -1):
                W[i + 1] = W[i + 1] + o * W[i] * (i + 1) / (l + 1)
                W[i] = z * W[i] * (l - i) / (l + 1)
        for e in range(m):
            z, o = Zc[e][:, None], O[e]
            nxt = W[m].copy()
            one = np.zeros((nleaf, rows))
            zero = np.zeros((nleaf, rows))
            for i in range(m - 1, -1, -1):
                tmp = nxt * (m + 1) / (i + 1)
                one += tmp
                nxt = W[i] - tmp * z * (m - i) / (m + 1)
                pre = z * (m - i) / (m + 1)
                zero += np.where(pre > 0, W[i] / np.where(pre > 0, pre, 1.0), 0.0)
            total = np.where(o, one, zero)
            w = np.where(live, total * (o - z), 0.0)  # [leaves, rows]
            term = w[:, :, None] * lv.astype(np.float64)[:, None, :]  # [leaves, rows, K]
            phi[:, :, feats[e]] += term.sum(axis=0)
            A[:, :, feats[e]] += np.abs(term).sum(axis=0)
            N[:, :, feats[e]] += live.sum(axis=0)[:, None]
    _finish(phi, forest, covers, avg, global_bias)
    T = len(forest["depths"])
    if avg and T > 0:
        A[:, :, :-1] /= T
    A[:, :, -1] = np.abs(phi[:, :, -1])
    return phi, A, N


def shap_tables(D, fids, ratio):
    """-> (feats, masks, Z): a tree's elements in order of first appearance from level 0, their level masks, and Z[m, leaves] =
    the float64 product of the leaf's path ratios over each element's levels, levels ascending (oblivious_shap_build's zz)"""
    feats, masks = [], []
    for l in range(D):
        f = int(fids[l])
        if f not in feats:
            feats.append(f)
            masks.append(0)
        masks[feats.index(f)] |= 1 << l
    j = np.arange(1 << D)
    Z = np.ones((len(feats), 1 << D))
    for e, mask in enumerate(masks):
        for l in range(D):
            if mask >> l & 1:
                Z[e] = Z[e] * ratio[l + 1][j & ((2 << l) - 1)]
    return feats, masks, Z


def emulate(forest, covers, data, missing=obr.MISSING, avg=False, global_bias=0.0):
    """-> phi [rows, K, F + 1] float32: oblivious_shap_build's tables and ob_shap_tree (oblivious_shap.hip) restated operation for
    operation in np.float32, from the file's header comment and the kernel's loops: the bits of predict_contribs, not a bound.
    Every coefficient is a float64 quotient rounded once; every product and sum below is one float32 operation (the library
    is built without contraction), in the kernel's order."""
    f32 = np.float32
    data = np.ascontiguousarray(data, f32)
    rows, k, F = data.shape[0], forest["k"], forest["cols"]
    acc = np.zeros((rows, k, F + 1), f32)  # one accumulator per (row, class, column), from +0.0f through all trees in order
    with np.errstate(all="ignore"):
        for t, D, fids, sl, lv, cv in _trees(forest, covers):
            _, ratio = heap(D, cv)
            feats, masks, Z = shap_tables(D, fids, ratio)
            M, nleaf = len(feats), 1 << D
            if M == 0:
                continue
            zf = np.where(Z < MIN_Z, 0.0, Z).astype(f32)  # [M, leaves]
            omz = (1.0 - Z).astype(f32)
            zmask = np.zeros(nleaf, np.int64)
            for e in range(M):
                zmask |= np.where(zf[e] == 0, masks[e], 0)
            right = _bits(forest, sl, data, missing)
            idx = np.zeros(rows, np.int64)
            for l in range(D):
                idx |= right[l].astype(np.int64) << l
            mism = idx[None, :] ^ np.arange(nleaf)[:, None]  # [leaves, rows]
            live = (mism & zmask[:, None]) == 0
            O = [(mism & masks[e]) == 0 for e in range(M)]
            zero = np.zeros((nleaf, rows), f32)
            pw = [np.ones((nleaf, rows), f32)]
            for e in range(M):  # EXTEND
                l = e + 1
                pw.append(zero.copy())
                for i in range(l - 1, -1, -1):
                    tt = pw[i] * f32((i + 1) / (l + 1))
                    pw[i + 1] = pw[i + 1] + np.where(O[e], tt, zero)
                    pw[i] = pw[i] * (zf[e] * f32((l - i) / (l + 1)))[:, None]
            s0 = zero.copy()
            for i in range(M):
                s0 = s0 + pw[i] * f32((M + 1) / (M - i))
            leaf = np.ascontiguousarray(lv, f32)  # [leaves, K]
            for e in range(M):
                nxt, tot = pw[M], zero.copy()
                for i in range(M - 1, -1, -1):
                    tmp = nxt * f32((M + 1) / (i + 1))
                    tot = tot + tmp
                    if i > 0:
                        nxt = pw[i] - tmp * (zf[e] * f32((M - i) / (M + 1)))[:, None]
                w = np.where(O[e], tot * omz[e][:, None], -s0)
                # The ordered sum stays sequential: np.add.accumulate adds the leaves' terms one by one, ascending, onto the
                # running sum.  A leaf the row does not weigh (not live) adds +0.0f in place of being skipped, which gives the
                # same bits: the accumulator starts at +0.0f, a float32 sum is -0.0f only when both its operands are, so it
                # never becomes -0.0f, and x + 0.0f == x for every other x (a NaN stays a NaN).
                term = np.where(live[:, :, None], w[:, :, None] * leaf[:, None, :], f32(0.0))  # [leaves, rows, K]
                run = np.concatenate([acc[None, :, :, feats[e]], term], axis=0)
                acc[:, :, feats[e]] = np.add.accumulate(run, axis=0, dtype=f32)[-1]
        T = len(forest["depths"])
        if avg and T > 0:
            acc[:, :, :F] = acc[:, :, :F] / f32(T)
    acc[:, :, F] = bias_f32(forest, covers, avg, global_bias)[None, :]
    return acc


def saabas(forest, covers, data, missing=obr.MISSING, avg=False, global_bias=0.0):
    """-> phi [rows, K, F + 1] float32"""
    data = np.ascontiguousarray(data, np.float32)
    rows, k, F = data.shape[0], forest["k"], forest["cols"]
    phi = np.zeros((rows, k, F + 1), np.float32)
    r = np.arange(rows)
    for t, D, fids, sl, lv, cv in _trees(forest, covers):
        cover, _ = heap(D, cv)
        E = node_means(D, cover, lv)
        right = _bits(forest, sl, data, missing)
        idx = np.zeros(rows, np.int64)
        for l in range(D):
            parent = idx.copy()
            idx |= right[l].astype(np.int64) << l
            with np.errstate(over="ignore", invalid="ignore"):  # leaves near FLT_MAX: a delta rounds to +-inf, inf - inf is NaN
                d = (E[l + 1][idx] - E[l][parent]).astype(np.float32)  # [rows, K]
                phi[r, :, int(fids[l])] += d
    T = len(forest["depths"])
    if avg and T > 0:
        phi[:, :, :F] /= np.float32(T)
    phi[:, :, F] = bias_f32(forest, covers, avg, global_bias)[None, :]
    return phi


def expand_with_covers(forest, covers, cls=0):
    """-> (nodes, D): oblivious_ref.expand_to_dense for output `cls`, every reachable node's weight = its subtree cover"""
    nodes, D = obr.dense_of(forest, cls)
    per = (1 << (D + 1)) - 1
    for t, d, fids, sl, lv, cv in _trees(forest, covers):
        cover, _ = heap(d, cv)
        tree = nodes[t * per:(t + 1) * per]
        for l in range(d + 1):
            tree["weight"][(1 << l) - 1:(2 << l) - 1] = cover[l][obr.bitreverse(np.arange(1 << l), l)].astype(np.float32)
    return nodes, D


def make_covers(forest, kind, seed):
    """Leaf covers: 'int' = integers in [1, 1024]; 'half' / 'most' = those with 50 % / 90 % set to 0; 'zero' = all 0"""
    rng = np.random.default_rng(seed)
    n = int((1 << np.asarray(forest["depths"], np.int64)).sum())
    c = rng.integers(1, 1025, n).astype(np.float32)
    if kind == "half":
        c[rng.random(n) < 0.5] = 0.0
    elif kind == "most":
        c[rng.random(n) < 0.9] = 0.0
    elif kind == "zero":
        c[:] = 0.0
    else:
        assert kind == "int"
    return c
