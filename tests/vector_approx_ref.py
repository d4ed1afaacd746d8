"""Numpy restatement of Saabas contributions on a vector-leaf handle (tahoe_vector_forest_create_ex with
TAHOE_CREATE_VECTOR_APPROX, tahoe_forest_predict_contribs_approx), written from the definition in include/tahoe_amd.h: test
infrastructure, not product.

Node means per output k in float64 from the caller's trees: E_k(leaf) = float64(leaves[left_idx, k]), E_k(n) = (wl * E_k(l) + wr *
E_k(r)) / (wl + wr); each child of an internal node carries d_k(child) = float32(E_k(child) - E_k(n)).  The row follows predict's
path (tests/approx_contribs_ref._go_right) and every internal node on it adds the taken child's d_k to phi[k][fid] in float32:
one add per (tree, level), trees in order, root to leaf, from +0.0, vectorised over rows and outputs -- rows and outputs are
distinct cells, so the result is bit-exact by construction.  AVG divides the finished sums by float32(T); the bias column is
vector_shap_ref.bias_column.

contribs() -> phi [rows, K, F + 1] float32; with scale=True also S [rows, K] = the float64 sum of |d| over the adds and N [rows] =
the number of adds.  direct64() -> the same sums in float64 with unrounded deltas.  path_deltas64() -> per (tree, leaf) the float64
deltas of the leaf's path.  form_rule() restates the library's choice of class block and accumulation form (DESIGN.md section
29); table_bytes() what the flag adds to device_bytes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_contribs_ref as acr  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

LDS_LIMIT = 160 * 1024      # MI355X: LDS a workgroup may take
WAVE_SLAB_MAX = 40 * 1024   # the widest wave slab the class-block rule takes
SLAB_BUDGET = 64 * 1024     # LDS per workgroup of the slab form when several waves' slabs fit


def _tree_means(tree, cov, leaves):
    """E [n, K] float64 of one tree; children lie after their parent"""
    n, K = tree.size, leaves.shape[1]
    E = np.zeros((n, K))
    leaf = tree["bits"] < 0
    E[leaf] = leaves[tree["left_idx"][leaf]].astype(np.float64)
    for i in range(n - 1, -1, -1):
        if not leaf[i]:
            l = int(tree["left_idx"][i])
            wl, wr = float(cov[l]), float(cov[l + 1])
            with np.errstate(all="ignore"):
                E[i] = (wl * E[l] + wr * E[l + 1]) / (wl + wr) if wl + wr != 0.0 else np.nan
    return E


def _trees(forest, covers):
    nodes, trees = forest["nodes"], forest["trees"]
    bounds = list(trees) + [nodes.size]
    for t in range(trees.size):
        lo, hi = int(bounds[t]), int(bounds[t + 1])
        yield nodes[lo:hi], covers[lo:hi]


def _deltas(tree, E):
    """d64 [n, K]: E(child) - E(parent) by the child's index (the root's row 0)"""
    d = np.zeros_like(E)
    inner = np.nonzero(tree["bits"] >= 0)[0]
    left = tree["left_idx"][inner].astype(np.int64)
    with np.errstate(all="ignore"):
        d[left] = E[left] - E[inner]
        d[left + 1] = E[left + 1] - E[inner]
    return d


def _sums(forest, covers, x, missing, dtype, want_scale):
    x = np.ascontiguousarray(x, np.float32)
    K, F, rows = forest["k"], forest["cols"], x.shape[0]
    phi = np.zeros((rows, K, F + 1), dtype)
    S = np.zeros((rows, K)) if want_scale else None
    N = np.zeros(rows, np.int64) if want_scale else None
    for tree, cov in _trees(forest, covers):
        bits = tree["bits"].view(np.uint32)
        fid = (bits & 0x3FFFFFFF).astype(np.int64)
        def_left = ((bits >> 30) & 1).astype(bool)
        is_leaf = (bits >> 31).astype(bool)
        left = tree["left_idx"].astype(np.int64)
        val = tree["val"].astype(np.float32)
        with np.errstate(all="ignore"):
            d = _deltas(tree, _tree_means(tree, cov, forest["leaves"])).astype(dtype)
        idx = np.zeros(rows, np.int64)
        active = np.full(rows, not is_leaf[0])
        while active.any():
            r = np.nonzero(active)[0]
            i = idx[r]
            f = fid[i]
            child = left[i] + acr._go_right(x[r, f], val[i], def_left[i], missing).astype(np.int64)
            with np.errstate(over="ignore", invalid="ignore"):  # leaves near FLT_MAX: +-inf and NaN sums are the IEEE results
                phi[r, :, f] += d[child]  # one add per (row, k): (r, f) pairs are distinct
            if want_scale:
                S[r] += np.abs(d[child].astype(np.float64))
                N[r] += 1
            idx[r] = child
            active[r] = ~is_leaf[child]
    return phi, S, N


def contribs(forest, covers, x, missing=vr.MISSING, avg=False, global_bias=0.0, scale=False):
    T, F = forest["trees"].size, forest["cols"]
    phi, S, N = _sums(forest, covers, x, missing, np.float32, scale)
    if avg and T > 0:
        with np.errstate(over="ignore", invalid="ignore"):
            phi[:, :, :F] /= np.float32(T)
    phi[:, :, F] = vsr.bias_column(forest, covers, avg, global_bias)[None, :]
    return (phi, S, N) if scale else phi


def direct64(forest, covers, x, missing=vr.MISSING):
    """The sums of unrounded float64 deltas, RAW, the bias column left 0: [rows, K, F + 1] float64"""
    return _sums(forest, covers, x, missing, np.float64, False)[0]


def path_deltas64(forest, covers):
    """[(t, leaf node, sum over the path of the float64 deltas [K], leaf vector - E(root) [K], sum of |delta| [K])] of every
    reachable leaf"""
    out = []
    for t, (tree, cov) in enumerate(_trees(forest, covers)):
        E = _tree_means(tree, cov, forest["leaves"])
        d = _deltas(tree, E)
        stack = [(0, np.zeros(E.shape[1]), np.zeros(E.shape[1]))]
        while stack:
            i, s, a = stack.pop()
            if tree["bits"][i] < 0:
                out.append((t, i, s, E[i] - E[0], a))
                continue
            l = int(tree["left_idx"][i])
            stack += [(l + 1, s + d[l + 1], a + np.abs(d[l + 1])), (l, s + d[l], a + np.abs(d[l]))]
    return out


def wave_slab_bytes(cols, kb):
    return 64 * ((kb * (cols + 1)) | 1) * 4


def form_rule(cols, K, forced_kb=None, forced_form=None, lds=LDS_LIMIT):
    """-> (class block KB, slab form?, waves per workgroup), the rule of vector_approx_shape: in place with class block 4 (2 or 1
    where K rounded up to one of them is smaller) where two wave slabs of one output do not fit the LDS; else the slab with the
    largest class block (8, 4, 2 or 1, not above K rounded up to one of them) whose wave slab stays within WAVE_SLAB_MAX (at
    least 1).  forced_kb = TAHOE_VECTOR_SHAP_KB,
    forced_form = TAHOE_APPROX_FORM (1: the slab wherever one wave's slab fits, 2: in place)."""
    cap = 1
    while cap < 8 and cap < K:
        cap *= 2
    if forced_kb in (1, 2, 4, 8):
        kb = forced_kb
    elif 2 * wave_slab_bytes(cols, 1) > lds:
        kb = min(cap, 4)
    else:
        kb = cap
        while kb > 1 and wave_slab_bytes(cols, kb) > WAVE_SLAB_MAX:
            kb //= 2
    wb = wave_slab_bytes(cols, kb)
    slab = 2 * wb <= lds
    if forced_form == 1:
        slab = wb <= lds
    if forced_form == 2:
        slab = False
    waves = max(1, min(4, SLAB_BUDGET // wb)) if slab else 4
    return kb, slab, waves


def table_bytes(forest, kb):
    """What TAHOE_CREATE_VECTOR_APPROX adds to device_bytes: 4 Kp max(num_nodes, 1) bytes of deltas, Kp = K rounded up to a
    multiple of the class block, and 4 K bytes of bias"""
    K = forest["k"]
    kp = (K + kb - 1) // kb * kb
    return 4 * kp * max(forest["nodes"].size, 1) + 4 * K


# ---- the forests of the tests beyond vector_shap_ref.case ----
_cache = {}


def _frozen(key, build):
    if key not in _cache:
        out = build()
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
            elif isinstance(a, dict):
                for v in a.values():
                    if isinstance(v, np.ndarray):
                        v.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def with_leaves(forest, leaves):
    leaves = np.ascontiguousarray(leaves, np.float32)
    return dict(forest, leaves=leaves, k=leaves.shape[1])


def k_case(K, cols=5, kinds=(4, "stump", "leaf", 5, "chain"), seed=7100, rows=vr.ROWS):
    """(forest of K outputs, data [rows, cols], covers): the class blocks and their partial last ones"""
    def build():
        forest = vr.make_named(list(kinds), cols, K, seed=seed + K)
        return forest, vr.make_data(rows, cols, seed=seed + 1), vsr.consistent_covers(forest, seed + 2)
    return _frozen(("k", K, cols, tuple(kinds), seed, rows), build)


def vine_case(depth=300, cols=7, K=3, seed=7300):
    """A depth-`depth` vine (every internal node: a leaf on one side, the vine on the other, the side at random) beside a stump
    and a single leaf"""
    def build():
        rng = np.random.default_rng(seed)
        nv = 13
        spec = int(rng.integers(0, nv))
        for _ in range(depth):
            leaf = int(rng.integers(0, nv))
            thr = float(vr.GRID[0]) if rng.random() < 0.9 else float(rng.choice(vr.GRID))
            node = (int(rng.integers(0, cols)), thr, bool(rng.integers(0, 2)))
            spec = node + ((leaf, spec) if rng.random() < 0.85 else (spec, leaf))
        forest = vr.make([spec, vr.stump(rng, cols, nv), int(rng.integers(0, nv))], vr.mixed_leaves(rng, nv, K), K, cols)
        return forest, vr.make_data(vr.ROWS, cols, seed=seed + 1), vsr.unrelated_covers(forest, seed + 2)
    return _frozen(("vine", depth, cols, K, seed), build)


def pool_case(missing, seed=7400, cols=6, K=3, T=6, depth=5):
    """Thresholds and data from shap_edges' pools (+-0, +-inf, NaN, subnormals, neighbours of thresholds, the edges of the missing
    band) for the sentinel `missing`"""
    import shap_edges as se

    def build():
        rng = np.random.default_rng(seed)
        thr = se.threshold_pool(missing)

        def tree(d):
            if d >= depth or (d > 0 and rng.random() < 0.25):
                return int(rng.integers(0, 9))
            return (int(rng.integers(0, cols)), float(rng.choice(thr)), bool(rng.integers(0, 2)), tree(d + 1), tree(d + 1))

        forest = vr.make([tree(0) for _ in range(T)], vr.mixed_leaves(rng, 9, K), K, cols)
        data = rng.choice(se.data_pool(missing), (vr.ROWS, cols)).astype(np.float32)
        return forest, data, vsr.consistent_covers(forest, seed + 2)
    return _frozen(("pool", repr(missing), seed, cols, K, T, depth), build)


def value_case(kind, seed=7500, cols=5, K=3):
    """kind "subnormal": leaf vectors of subnormal magnitude, so that every delta is subnormal or 0; "overflow": leaf vectors near
    +-3e38, so that deltas overflow to +-inf and sums of both signs give NaN"""
    def build():
        rng = np.random.default_rng(seed + len(kind))
        forest = vr.make_named([4, 3, "stump", 4, 5, 3, 4, 2], cols, K, seed=seed)
        L = forest["leaves"].shape[0]
        if kind == "subnormal":
            lv = rng.choice(np.array([1e-45, 3e-42, 1e-40, 7e-39, 1.1e-38], np.float32), (L, K)) * rng.choice([-1.0, 1.0], (L, K))
        else:
            lv = rng.choice(np.array([3e38, 3.3e38, 2.5e38, 1e37], np.float32), (L, K)) * rng.choice([-1.0, 1.0], (L, K))
        forest = with_leaves(forest, lv.astype(np.float32))
        return forest, vr.make_data(vr.ROWS, cols, seed=seed + 1), vsr.unrelated_covers(forest, seed + 2)
    return _frozen(("value", kind, seed, cols, K), build)


def leaves_only_case(K=9, T=5, seed=7600):
    """Single-leaf trees only: nothing to add"""
    def build():
        forest = vr.make_named(["leaf"] * T, 3, K, seed=seed)
        return forest, vr.make_data(vr.ROWS, 3, seed=seed + 1), np.ones(forest["nodes"].size, np.float32)
    return _frozen(("leaves", K, T, seed), build)


def wide_case(cols, K=9, seed=7700):
    """4 shallow trees on `cols` columns, features spread over the whole width"""
    def build():
        forest = vr.make_named([4, 3, "stump", 4], cols, K, seed=seed + cols)
        return forest, vr.make_data(WIDE_ROWS, cols, seed=seed + 1), vsr.consistent_covers(forest, seed + 2)
    return _frozen(("wide", cols, K, seed), build)


WIDE_ROWS = 128 * 4 + 1  # two workgroups of four waves and one row
