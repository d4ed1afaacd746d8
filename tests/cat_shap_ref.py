"""Float64 references for the four explanation calls on sparse forests with categorical splits (TAHOE_CREATE_CAT_CONTRIBS): test
infrastructure, not product.  They are the references of sparse_shap_ref / approx_contribs_ref with the branch rule swapped for
the categorical one that categorical_ref restates:
  missing (|float32(x - missing)| <= 1e-6): the default branch;
  numeric node: right iff x >= val;
  split k: member = 0 <= x < 32 nwords and bit trunc(x) of the split's words; right iff member != members_left[k].

A forest is a CatForest: sparse nodes, root offsets, {node index: category ids} and the nodes whose members go left.  A split has
as many words as its largest category needs (none for an empty set), as tahoe_amd.capi.pack_categorical packs it.

- contribs() / interactions(): sparse_shap_ref's subset enumerations over the conditional expectation computed here by recursion.
- interventional(): sparse_shap_ref's per-background-row definition over the leaves categorical_ref.predict reaches.
- saabas(): approx_contribs_ref's float32 operation order with the walk's decision swapped.
- fold() / element_follows(): the set algebra of one path element (allowed set + outside_ok), for the host-only check."""
from __future__ import annotations

import contextlib

import numpy as np

import approx_contribs_ref
import categorical_ref
import sparse_shap_ref as ref

EPS = np.float32(1e-6)


class CatForest:
    def __init__(self, sn, tr, cats=None, left=()):
        self.sn, self.tr = sn, np.asarray(tr, np.int32)
        self.cats = {int(k): np.unique(np.asarray(list(v), np.int64)) for k, v in (cats or {}).items()}
        self.left = {int(k) for k in left}
        self.keys = sorted(self.cats)
        self.nwords = {k: (int(self.cats[k][-1]) // 32 + 1 if self.cats[k].size else 0) for k in self.keys}

    def arrays(self):
        """node, offset, words, members_left as categorical_ref.predict takes them."""
        node = np.array(self.keys, np.int64)
        offset = np.zeros(len(self.keys) + 1, np.int64)
        offset[1:] = np.cumsum([self.nwords[k] for k in self.keys])
        words = np.zeros(int(offset[-1]), np.uint32)
        for i, k in enumerate(self.keys):
            c = self.cats[k]
            np.bitwise_or.at(words, offset[i] + c // 32, np.uint32(1) << (c % 32).astype(np.uint32))
        ml = np.array([k in self.left for k in self.keys], np.uint8)
        return node, offset, words, ml

    def sub(self, c, C, covers):
        """Class c's sub-forest (trees c, c + C, ...) with its splits renumbered, and its covers."""
        ends = np.append(self.tr[1:], self.sn.size)
        parts, roots, cv, cats, left, off = [], [], [], {}, set(), 0
        for t in range(c, self.tr.size, C):
            a, b = int(self.tr[t]), int(ends[t])
            parts.append(self.sn[a:b])
            cv.append(covers[a:b])
            roots.append(off)
            for k in self.keys:
                if a <= k < b:
                    cats[k - a + off] = self.cats[k]
                    if k in self.left:
                        left.add(k - a + off)
            off += b - a
        return CatForest(np.concatenate(parts), np.array(roots, np.int32), cats, left), np.concatenate(cv)


def member(ids, nwords, x):
    """The set test on float32 values x: in range and bit trunc(x)."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        in_range = (x >= np.float32(0.0)) & (x < np.float32(32 * nwords))
    c = np.where(in_range, x, 0.0).astype(np.int64)
    return in_range & np.isin(c, ids)


def go_right(forest, g, x, missing):
    """The branch of every value of x (float32 [n]) at node g (an index into forest.sn)."""
    bits = int(forest.sn["bits"][g]) & 0xFFFFFFFF
    def_left = bool((bits >> 30) & 1)
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        is_missing = np.abs(x - np.float32(missing)) <= EPS
        if g in forest.cats:
            right = member(forest.cats[g], forest.nwords[g], x) != (g in forest.left)
        else:
            right = x >= np.float32(forest.sn["val"][g])
    return np.where(is_missing, not def_left, right)


def _cond_exp(forest, t, cov, right, rows, S):
    """v_t(S) for every row; right[g]: the rows' branch at internal node g (it does not depend on S)."""
    root = int(forest.tr[t])
    sn = forest.sn
    bits = sn["bits"].view(np.uint32)

    def rec(i):
        g = root + i
        if bits[g] >> 31:
            return np.full(rows, float(sn["val"][g]))
        fid, li = int(bits[g] & 0x3FFFFFFF), int(sn["left_idx"][g])
        if fid in S:
            return np.where(right[g], rec(li + 1), rec(li))
        wl, wr = float(cov[root + li]), float(cov[root + li + 1])
        return (wl * rec(li) + wr * rec(li + 1)) / (wl + wr)

    return rec(0)


def games(forest, covers, x, F, missing, C):
    """v[c][mask]: float64 [rows], as sparse_shap_ref._games (kept per forest and input: contribs and interactions share it)."""
    key = (x.tobytes(), np.asarray(covers).tobytes(), F, float(missing), C)
    cache = forest.__dict__.setdefault("_games", {})
    if key in cache:
        return cache[key]
    bits = forest.sn["bits"].view(np.uint32)
    right = {int(g): go_right(forest, int(g), x[:, int(bits[g] & 0x3FFFFFFF)], missing) for g in np.nonzero((bits >> 31) == 0)[0]}
    v = [[np.zeros(x.shape[0]) for _ in range(1 << F)] for _ in range(C)]
    for t in range(forest.tr.size):
        for mask in range(1 << F):
            S = {i for i in range(F) if mask >> i & 1}
            v[t % C][mask] += _cond_exp(forest, t, covers, right, x.shape[0], S)
    cache[key] = v
    return v


def predict64(forest, data, missing, C):
    """Raw per-class sums in float64 [rows, C] over the leaves categorical_ref.predict reaches."""
    node, offset, words, ml = forest.arrays()
    _, leaf = categorical_ref.predict(forest.sn, forest.tr, data, missing, node, offset, words, ml)
    out = np.zeros((data.shape[0], C))
    for t in range(forest.tr.size):
        out[:, t % C] += forest.sn["val"][int(forest.tr[t]) + leaf[:, t].astype(np.int64)]
    return out


@contextlib.contextmanager
def _rule(forest):
    """sparse_shap_ref with its two evaluators of the branch rule swapped for the categorical ones."""
    old = ref._games, ref._predict64
    ref._games = lambda sn, tr, covers, x, F, missing, C: games(forest, covers, x, F, missing, C)
    ref._predict64 = lambda sn, tr, data, missing, C: predict64(forest, data, missing, C)
    try:
        yield
    finally:
        ref._games, ref._predict64 = old


def contribs(forest, covers, x, F, missing, C=1, avg=False, global_bias=0.0):
    with _rule(forest):
        return ref.contribs(forest.sn, forest.tr, covers, x, F, missing, C, avg, global_bias)


def interactions(forest, covers, x, F, missing, C=1, avg=False):
    with _rule(forest):
        return ref.interactions(forest.sn, forest.tr, covers, x, F, missing, C, avg)


def interventional(forest, x, bg, F, missing, C=1, avg=False, global_bias=0.0, bg_raw=None):
    with _rule(forest):
        return ref.interventional(forest.sn, forest.tr, x, bg, F, missing, C, avg, global_bias, bg_raw=bg_raw)


def saabas(forest, covers, F, x, missing, num_classes=1, avg=False, global_bias=0.0):
    """approx_contribs_ref.sparse with the walk's decision swapped: one float32 add per (tree, level), tree order."""
    x = np.ascontiguousarray(x, np.float32)
    sn, tr = forest.sn, forest.tr
    C, rows, T = num_classes, x.shape[0], tr.size
    phi = np.zeros((rows, C, F + 1), np.float32)
    ends = np.append(tr[1:], sn.size)
    for c in range(C):
        for t in range(c, T, C):
            a, b = int(tr[t]), int(ends[t])
            left = sn[a:b]["left_idx"].astype(np.int64)
            fid, _, is_leaf, _, d = approx_contribs_ref._tree_arrays(sn[a:b], left, covers[a:b], False)
            for r in range(rows):
                i = 0
                while not is_leaf[i]:
                    f = int(fid[i])
                    child = int(left[i]) + int(go_right(forest, a + i, x[r:r + 1, f], missing)[0])
                    phi[r, c, f] += d[child]
                    i = child
    bias = ref.bias_column(sn, tr, covers, C, avg, global_bias)
    if avg and T // C > 0:
        phi[:, :, :F] /= np.float32(T // C)
    phi[:, :, F] = bias[None, :]
    return phi


# ---- the set algebra of one path element ----

def fold(edges):
    """edges: [(ids, nwords, need)] of one feature on one path, need = the path wants member == need.  Returns (allowed, W,
    outside_ok): allowed = bool [32 W], W the largest nwords; a shorter set is zero-extended; bit c set iff bit_k(c) == need_k
    for every edge; outside_ok iff no edge has need."""
    W = max([nw for _, nw, _ in edges], default=0)
    allowed = np.ones(32 * W, bool)
    for ids, nw, need in edges:
        bit = np.zeros(32 * W, bool)
        bit[np.asarray(ids, np.int64)] = True
        allowed &= bit == bool(need)
    return allowed, W, not any(need for _, _, need in edges)


def element_follows(allowed, W, outside_ok, x):
    """The set part of the one-fraction for non-missing float32 values x."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        in_range = (x >= np.float32(0.0)) & (x < np.float32(32 * W))
    c = np.where(in_range, x, 0.0).astype(np.int64)
    bit = allowed[c] if allowed.size else np.zeros(c.shape, bool)
    return np.where(in_range, bit, outside_ok)
