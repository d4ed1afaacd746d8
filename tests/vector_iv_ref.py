"""Float64 references of interventional TreeSHAP on a vector-leaf forest (tahoe_vector_forest_create_ex with
TAHOE_CREATE_INTERVENTIONAL), written from the definition in include/tahoe_amd.h, and the library's class-block / tile-row rule
restated: test infrastructure, not product.

A forest is tests/vector_ref.py's dict.  v_r(S)[k] = f_k(x_S, r_{N \\ S}) for a background row r; phi_i(x)[k] = (1 / B) sum_r of
the exact Shapley value of v_r, all K outputs of a leaf at once; with AVG divided by the number of trees.

- brute(): per background row the Shapley formula over all subsets of the num_cols <= 8 features, v_r(S) = tests/vector_edges
  .margins64 on the hybrid rows: independent of any path formulation.
- paths(): the per-leaf-path closed form on tests/vector_edges.leaf_paths: A = the path's features only x follows, B' = those only
  r follows, a feature neither follows kills the path; i in A gets +leaf W(|A|, |B'|), j in B' gets -leaf W(|B'|, |A|), W(p, q) =
  (p - 1)! q! / (p + q)!.  Returns (phi, A, N) as tests/interventional_ref.paths does: A the sum of the absolute per-path terms
  behind each value, averaged over the background like phi; N [K, cols + 1] the number of path elements feeding it.
- paths_expansion(): the same closed form evaluated class by class on the scalar-leaf trees of tests/vector_ref.expand, with a
  tree walk of its own.
The bias column of all three is float64: mean over the background of the margins / (AVG ? T : 1) + global_bias (A's: |bias|).
The GPU tests check the handle's bias column bit for bit against the host formula on the handle's own raw sums instead."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interventional_ref as ivr  # noqa: E402
import vector_edges as ve  # noqa: E402
import vector_ref as vr  # noqa: E402

MISSING = vr.MISSING

# ---- the rule of vector_iv_shape (vector_iv.hip) ----
LDS_BUDGET = 80 * 1024   # kIvLdsBudget
LDS_DEVICE = 160 * 1024  # the LDS of a CDNA4 compute unit
TABLE = 32 * 32 * 4      # the weight table
MAX_ROWS = 8             # kIvMaxTileRows

# num_cols of the tiles cases (one 3-tree forest, K = 9) -> (KB, R, WLDS): both sides of every step of the rule
TILE_COLS = {73: (8, 8, True), 74: (8, 4, True), 147: (8, 4, True), 148: (8, 2, True), 294: (8, 2, True), 295: (8, 1, True),
             589: (8, 1, True), 590: (4, 1, True), 1144: (4, 1, True), 1145: (2, 1, True), 2161: (2, 1, True), 2162: (1, 1, True),
             3891: (1, 1, True), 3892: (1, 1, True), 7987: (1, 1, True), 7988: (1, 1, False), 8192: (1, 1, False)}
TILE_REFUSED = 8193  # 20 B of LDS per column no longer fit the device


def tile_rows(F, kb):
    """Rows of a tile for class block kb: the largest power of two <= 8 that fits the budget with the table, 0 if none"""
    per_row, r = (1 + 4 * kb) * F * 4, MAX_ROWS
    while r > 1 and r * per_row + TABLE > LDS_BUDGET:
        r //= 2
    return r if r * per_row + TABLE <= LDS_BUDGET else 0


def iv_shape(cols, K, forced=None):
    """(KB, R, WLDS, bytes of dynamic LDS) of a handle of num_cols = cols and K outputs; forced = TAHOE_VECTOR_SHAP_KB"""
    if forced in (1, 2, 4, 8):
        kb = forced if tile_rows(cols, forced) else 1
    else:
        kb = next((c for c in (8, 4, 2) if c < 2 * K and tile_rows(cols, c)), 1)
    R = max(tile_rows(cols, kb), 1)
    body = (1 + 4 * kb) * R * cols * 4
    wlds = body + TABLE <= LDS_DEVICE
    return kb, R, wlds, body + (TABLE if wlds else 0)


# ---- references ----
def _bias(forest, bg, missing, avg, global_bias):
    T = forest["trees"].size
    m = ve.margins64(forest, bg, missing).mean(axis=0)
    return (m / T if avg and T else m) + float(global_bias)


def _finish(forest, phi, bg, missing, avg, global_bias):
    T, F = forest["trees"].size, forest["cols"]
    if avg and T:
        phi[:, :, :F] /= T
    phi[:, :, F] = _bias(forest, bg, missing, avg, global_bias)
    return phi


def brute(forest, data, bg, missing=MISSING, avg=False, global_bias=0.0):
    """phi float64 [rows, K, cols + 1]; every feature of [0, cols) is a player (cols <= 8)"""
    data, bg = np.ascontiguousarray(data, np.float32), np.ascontiguousarray(bg, np.float32)
    K, F, rows = forest["k"], forest["cols"], data.shape[0]
    assert F <= 8
    masks = np.array([[(m >> i) & 1 for i in range(F)] for m in range(1 << F)], bool).reshape(1 << F, F)
    phi = np.zeros((rows, K, F + 1))
    wgt = [math.factorial(s) * math.factorial(F - s - 1) / math.factorial(F) for s in range(F)] if F else []
    size = masks.sum(axis=1)
    for r in range(bg.shape[0]):
        hybrid = np.where(masks[None, :, :], data[:, None, :], bg[r][None, None, :]).reshape(-1, F)
        v = ve.margins64(forest, np.ascontiguousarray(hybrid), missing).reshape(rows, 1 << F, K)
        for i in range(F):
            for m in range(1 << F):
                if not (m >> i) & 1:
                    phi[:, :, i] += wgt[size[m]] * (v[:, m | 1 << i] - v[:, m])
    phi[:, :, :F] /= bg.shape[0]
    return _finish(forest, phi, bg, missing, avg, global_bias)


def _path_terms(elems, data, bg, missing):
    """[L, rows, B] float64: the signed weight of each element of one path for every (row, background row), leaf = 1"""
    Ox = np.stack([ivr._follows(data[:, f], edges, missing) for f, edges in elems])  # [L, rows]
    Or = np.stack([ivr._follows(bg[:, f], edges, missing) for f, edges in elems])    # [L, B]
    inA = Ox[:, :, None] & ~Or[:, None, :]
    inB = ~Ox[:, :, None] & Or[:, None, :]
    dead = (~Ox[:, :, None] & ~Or[:, None, :]).any(axis=0)
    na, nb = inA.sum(axis=0), inB.sum(axis=0)
    wa, wb = ivr._W[na, nb] * ~dead, ivr._W[nb, na] * ~dead
    return np.where(inA, wa[None], 0.0) - np.where(inB, wb[None], 0.0)


def paths(forest, data, bg, missing=MISSING, avg=False, global_bias=0.0):
    """-> (phi [rows, K, cols + 1], A [rows, K, cols + 1], N [K, cols + 1]) in float64"""
    data, bg = np.ascontiguousarray(data, np.float32), np.ascontiguousarray(bg, np.float32)
    K, F, T, rows, B = forest["k"], forest["cols"], forest["trees"].size, data.shape[0], bg.shape[0]
    phi, A, N = np.zeros((rows, K, F + 1)), np.zeros((rows, K, F + 1)), np.zeros((K, F + 1))
    for per_tree in ve.leaf_paths(forest, np.ones(forest["nodes"].size, np.float32)):  # (the covers only feed z, unused here)
        for vec, elems in per_tree:
            if not elems:
                continue
            term = _path_terms([(f, ed) for f, _, ed in elems], data, bg, missing)
            leaf = forest["leaves"][vec].astype(np.float64)
            for j, (f, _, _) in enumerate(elems):
                phi[:, :, f] += term[j].sum(axis=-1)[:, None] * leaf[None, :]
                A[:, :, f] += np.abs(term[j]).sum(axis=-1)[:, None] * np.abs(leaf)[None, :]
                N[:, f] += 1
    phi[:, :, :F] /= B
    A[:, :, :F] /= B
    if avg and T:
        A[:, :, :F] /= T
    phi = _finish(forest, phi, bg, missing, avg, global_bias)
    A[:, :, F] = np.abs(phi[:, :, F])
    return phi, A, N


def _scalar_paths(tree):
    """One sparse tree with scalar leaves -> [(leaf value, [(fid, [(thr, def_left, right), ...]) per distinct feature])]"""
    out, stack = [], [(0, ())]
    while stack:
        i, edges = stack.pop()
        n = tree[i]
        if n["bits"] < 0:
            elems = {}
            for node, right in edges:
                m = tree[node]
                elems.setdefault(int(m["bits"]) & vr.FID_MASK, []).append((m["val"], bool(int(m["bits"]) & vr.DEF_LEFT), right))
            out.append((float(n["val"]), list(elems.items())))
            continue
        li = int(n["left_idx"])
        stack += [(li + 1, edges + ((i, True),)), (li, edges + ((i, False),))]
    return out


def paths_expansion(forest, data, bg, missing=MISSING, avg=False, global_bias=0.0):
    """phi [rows, K, cols + 1]: class k from the trees k, k + K, ... of tests/vector_ref.expand(forest), one scalar leaf at a time"""
    data, bg = np.ascontiguousarray(data, np.float32), np.ascontiguousarray(bg, np.float32)
    K, F = forest["k"], forest["cols"]
    nodes, roots = vr.expand(forest)
    bounds = list(roots) + [nodes.size]
    phi = np.zeros((data.shape[0], K, F + 1))
    for t in range(roots.size):
        for leaf, elems in _scalar_paths(nodes[int(bounds[t]):int(bounds[t + 1])]):
            if not elems:
                continue
            term = _path_terms(elems, data, bg, missing)
            for j, (f, _) in enumerate(elems):
                phi[:, t % K, f] += leaf * term[j].sum(axis=-1)
    phi[:, :, :F] /= bg.shape[0]
    return _finish(forest, phi, bg, missing, avg, global_bias)
