"""Search-tree forests with a closed-form answer (numpy and ta.capi.encode_nodes only; no GPU, no oracle).

A dense tree that is a balanced binary search tree over the sorted thresholds `s` of ONE feature (the sorted array laid out
in-order into the heap) sends a row with value x, ties going right, to bottom leaf number k = #{s <= x}: heap index
2^D - 1 + k, duplicates in `s` included.  The search for x = thr passes through the node holding thr, so the rows
(thr, nextafter down, nextafter up) of every threshold put every tie and every neighbouring compare on some row's path, at
every level of the tree.  When the tree holds all thresholds of its feature, k is that feature's rank code: a wrong code is a
wrong leaf index in a known column.  The irregular variant (sparse handles) is an unbalanced search tree; there the row ends
at the k-th leaf of the in-order leaf sequence.

Everything here is checked against the CPU oracle by tests/test_order_forests.py before a kernel is judged by it.
"""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny
DENORM_MIN = np.float32(1.0e-45)
EPS_BAND = np.float32(1.0e-6)  # |x - missing| <= 1e-6 in float32: the row takes !def_left
BENIGN = np.float32(0.5)
SPARSE_NODE_DTYPE = np.dtype([("val", "<f4"), ("bits", "<i4"), ("left_idx", "<i4")])
LEAF_BIT = np.int32(-2**31)


def _enc():
    import tahoe_amd as ta

    return ta.capi.encode_nodes


# ---- dense search trees ----
def pad_sorted(sorted_thresholds, D, pad=np.inf):
    """The 2^D - 1 entries of a depth-D tree: the thresholds, then `pad` (+inf, or "repeat": the largest value again)."""
    s = np.asarray(sorted_thresholds, dtype=np.float32)
    n = (1 << D) - 1
    assert s.size <= n and (s[1:] >= s[:-1]).all(), "thresholds must be sorted and fit the tree"
    fill = (s[-1] if isinstance(pad, str) else np.float32(pad))
    assert not isinstance(pad, str) or pad == "repeat"
    return np.concatenate([s, np.full(n - s.size, fill, dtype=np.float32)])


def inorder_to_heap(D):
    """heap index i (inner nodes of a depth-D tree) -> position in the sorted array."""
    i = np.arange((1 << D) - 1, dtype=np.int64)
    level = np.floor(np.log2(i + 1)).astype(np.int64)
    p = i + 1 - (1 << level)
    return (2 * p + 1) * (1 << (D - 1 - level)) - 1


def bst_tree(sorted_thresholds, D, fid, def_left, leaf_values, pad=np.inf):
    """Dense nodes (2^(D+1) - 1) of one depth-D search tree on feature `fid`; -> (nodes, s) with s the padded sorted array."""
    s = pad_sorted(sorted_thresholds, D, pad)
    leaf_values = np.asarray(leaf_values, dtype=np.float32)
    assert leaf_values.size == 1 << D
    n_in = (1 << D) - 1
    val = np.concatenate([s[inorder_to_heap(D)], leaf_values])
    is_leaf = np.concatenate([np.zeros(n_in, np.int64), np.ones(1 << D, np.int64)])
    nodes = _enc()(fid=np.full(val.size, fid), value=val, def_left=np.full(val.size, int(bool(def_left))),
                   weight=np.zeros(val.size), is_leaf=is_leaf)
    return nodes, s


class OrderForest:
    """Dense forest of search trees: .nodes, .T, .D, .cols and per tree (s, fid, def_left, leaf_values)."""

    def __init__(self, D, cols):
        self.D, self.cols, self.trees, self._parts = D, cols, [], []

    def add(self, sorted_thresholds, fid, def_left, leaf_values=None, pad=np.inf, seed=None):
        if leaf_values is None:
            rng = np.random.default_rng(1000 + len(self.trees) if seed is None else seed)
            leaf_values = rng.standard_normal(1 << self.D).astype(np.float32)
        assert 0 <= fid < self.cols
        nodes, s = bst_tree(sorted_thresholds, self.D, fid, def_left, leaf_values, pad)
        self._parts.append(nodes)
        self.trees.append((s, fid, bool(def_left), np.asarray(leaf_values, dtype=np.float32)))
        return self

    @property
    def T(self):
        return len(self.trees)

    @property
    def nodes(self):
        return np.concatenate(self._parts)

    def thresholds_by_fid(self):
        out = {}
        for s, fid, _, _ in self.trees:
            out.setdefault(fid, []).append(s)
        return {f: np.concatenate(v) for f, v in out.items()}

    def most_distinct(self):
        """Distinct thresholds of the busiest feature, as the library counts them (-0.0 == 0.0)."""
        return max(np.unique(v + np.float32(0.0)).size for v in self.thresholds_by_fid().values())


def bst_forest(D, cols, specs):
    """specs: iterable of dicts for OrderForest.add (sorted_thresholds, fid, def_left, ...)."""
    of = OrderForest(D, cols)
    for sp in specs:
        of.add(**sp)
    return of


def in_band(x, missing):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(x - np.float32(missing)) <= EPS_BAND


def rank_of(s, x):
    """#{s <= x} with NaN -> 0 (x >= thr is never true)."""
    k = np.searchsorted(s, x, side="right").astype(np.int64)
    return np.where(np.isnan(x), 0, k)


def expected_leaf(of, data, missing):
    """uint32 [rows, T]: 2^D - 1 + #{s <= x}; inside the missing band every node takes !def_left."""
    D = of.D
    out = np.empty((data.shape[0], of.T), dtype=np.uint32)
    for t, (s, fid, dl, _) in enumerate(of.trees):
        x = data[:, fid]
        k = rank_of(s, x)
        k = np.where(in_band(x, missing), 0 if dl else (1 << D) - 1, k)
        out[:, t] = (1 << D) - 1 + k
    return out


def expected_sums(of, leaf, num_classes=1):
    """float32 sums of the leaf values in tree order; [rows] or [rows, num_classes] (tree t belongs to class t % num_classes)."""
    base = (1 << of.D) - 1
    acc = np.zeros((leaf.shape[0], num_classes), dtype=np.float32)
    for t, (_, _, _, lv) in enumerate(of.trees):
        acc[:, t % num_classes] = acc[:, t % num_classes] + lv[leaf[:, t].astype(np.int64) - base]
    return acc[:, 0] if num_classes == 1 else acc


# ---- rows ----
def specials(missing):
    m = np.float32(missing)
    band = [m, m + F32(5e-7), m - F32(5e-7), m + F32(1e-6), m - F32(1e-6), m + F32(2e-6), m - F32(2e-6)]
    past = [np.nextafter(m + F32(1e-6), F32(np.inf)), np.nextafter(m - F32(1e-6), F32(-np.inf)),
            np.nextafter(np.nextafter(m + F32(1e-6), F32(np.inf)), F32(np.inf)),
            np.nextafter(np.nextafter(m - F32(1e-6), F32(-np.inf)), F32(-np.inf))]
    fixed = [0.0, -0.0, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX, DENORM_MIN, -DENORM_MIN, FLT_MIN, -FLT_MIN]
    return np.array(fixed + band + past, dtype=np.float32)


def critical_values(thresholds, missing, n_random=300, seed=0):
    """-> (triples, rest): every threshold with both float32 neighbours; the specials and `n_random` uniform values."""
    t = np.asarray(thresholds, dtype=np.float32)
    with np.errstate(over="ignore"):
        triples = np.stack([np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))], axis=1).reshape(-1)
    rng = np.random.default_rng(seed)
    fin = t[np.isfinite(t)]
    lo, hi = (float(fin.min()), float(fin.max())) if fin.size else (-1.0, 1.0)
    span = max(hi - lo, 1.0) if np.isfinite(hi - lo) else float(FLT_MAX) / 2
    rnd = rng.uniform(max(lo - 0.1 * span, -float(FLT_MAX)), min(hi + 0.1 * span, float(FLT_MAX)), n_random).astype(np.float32)
    return triples.astype(np.float32), np.concatenate([specials(missing), rnd])


def critical_matrix(thr_by_fid, cols, missing, n_random=300, seed=0, max_rows=None):
    """-> (float32 [rows, cols], rows of the first block).  Column f holds the critical values of its own thresholds: a block
    of triples, then a block of specials and random values; shorter columns repeat theirs, and every column is rotated inside
    each block so that one row does not hold the same special everywhere.  Columns without thresholds hold a fixed benign
    value.  max_rows: only that many rows (take_rows) are built -- wide rows, where the full set would be too large."""
    parts = {f: critical_values(t, missing, n_random, seed + 17 * f) for f, t in thr_by_fid.items()}
    n_a = max(p[0].size for p in parts.values())
    n_b = max(p[1].size for p in parts.values())
    idx = take_rows(n_a + n_b, n_a, max_rows if max_rows else n_a + n_b)
    data = np.full((idx.size, cols), BENIGN, dtype=np.float32)
    for j, (f, (a, b)) in enumerate(sorted(parts.items())):
        col = np.concatenate([np.roll(np.resize(a, n_a), 3 * j), np.roll(np.resize(b, n_b), 5 * j)])
        data[:, f] = col[idx]
    return data, int((idx < n_a).sum())


def critical_rows(thresholds, cols, fid, missing, n_random=300, seed=0):
    """One feature's critical rows; all other columns hold the benign value."""
    return critical_matrix({fid: thresholds}, cols, missing, n_random, seed)[0]


def take_rows(n_total, n_triples, n):
    """Row indices of a batch of n rows: 7/8 spread evenly over the triples block, 1/8 over the specials block, in that order
    (so a 513-row batch has a 512-row chunk that sees the sentinel and a chunk that does not)."""
    if n >= n_total:
        return np.arange(n_total)
    nb = min(n // 8, n_total - n_triples)
    na = n - nb
    a = np.linspace(0, n_triples - 1, na).astype(np.int64) if na > 1 else np.zeros(na, np.int64)
    b = n_triples + (np.linspace(0, n_total - n_triples - 1, nb).astype(np.int64) if nb > 1 else np.zeros(nb, np.int64))
    return np.concatenate([a, b])


def distinct_sorted(rng, n, scale=1.0, loc=0.0):
    """n distinct float32 values, sorted."""
    v = np.unique((rng.standard_normal(2 * n + 16) * scale + loc).astype(np.float32))
    assert v.size >= n
    return np.sort(rng.choice(v, n, replace=False))


def first_mismatch(of, data, want_leaf, got_leaf):
    """Report of the first bad (row, tree): feature, x as hex bits, expected rank, got rank."""
    bad = np.argwhere(want_leaf != got_leaf)
    if bad.size == 0:
        return ""
    r, t = (int(v) for v in bad[0])
    fid = of.trees[t][1]
    base = (1 << of.D) - 1
    xb = int(np.ascontiguousarray(data[r, fid:fid + 1]).view(np.uint32)[0])
    return (f"{bad.shape[0]} wrong leaf indices; first at row {r}, tree {t}: feature {fid}, x = 0x{xb:08x} ({data[r, fid]!r}), "
            f"expected rank {int(want_leaf[r, t]) - base}, got rank {int(got_leaf[r, t]) - base}")


# ---- irregular search trees (sparse handles) ----
def sparse_bst(thresholds, fid, def_left, order, leaf_values=None, max_depth=24, seed=0):
    """Search tree grown by inserting `thresholds` in `order` ("random": seeded shuffle; "sorted": a vine), ties going right,
    insertions that would pass `max_depth` dropped.  -> (nodes[SPARSE_NODE_DTYPE], s, leaf_pos): s = the sorted thresholds
    kept, leaf_pos[k] = position relative to the root of the leaf a row of rank k = #{s <= x} ends in."""
    rng = np.random.default_rng(seed)
    t = np.asarray(thresholds, dtype=np.float32)
    seq = rng.permutation(t) if order == "random" else np.sort(t)
    val, left, right = [], [], []  # a pointer tree first
    for v in seq:
        if not val:
            val.append(v), left.append(-1), right.append(-1)
            continue
        at, depth = 0, 1
        while True:
            side = right if v >= val[at] else left
            if side[at] < 0:
                if depth < max_depth:
                    side[at] = len(val)
                    val.append(v), left.append(-1), right.append(-1)
                break
            at, depth = side[at], depth + 1
    n_in = len(val)
    nodes = np.zeros(2 * n_in + 1, dtype=SPARSE_NODE_DTYPE)
    if leaf_values is None:
        leaf_values = rng.standard_normal(n_in + 1).astype(np.float32)
    # children adjacent and after their parent, left_idx relative to the root (the reference's dense2sparse layout rule)
    leaf_pos, kept = [], []
    nxt = 1
    stack = [(0, 0, False)]  # (pointer node or -1, position, visited)
    while stack:
        p, pos, seen = stack.pop()
        if p < 0:
            nodes["val"][pos] = leaf_values[len(leaf_pos)]
            nodes["bits"][pos] = LEAF_BIT
            leaf_pos.append(pos)
            continue
        if seen:
            kept.append(val[p])
            continue
        nodes["val"][pos] = val[p]
        nodes["bits"][pos] = np.int32(fid | ((1 << 30) if def_left else 0))
        nodes["left_idx"][pos] = nxt
        l_pos, nxt = nxt, nxt + 2
        stack.append((right[p], l_pos + 1, False))   # in-order: left subtree, this node, right subtree
        stack.append((p, pos, True))
        stack.append((left[p], l_pos, False))
    s = np.array(kept, dtype=np.float32)
    assert s.size == n_in and (s[1:] >= s[:-1]).all() and len(leaf_pos) == n_in + 1
    return nodes, s, np.array(leaf_pos, dtype=np.int64)


def sparse_leaf_order(nodes, root):
    """Positions (relative to `root`) of a sparse tree's leaves in in-order: leaf k is where rank k ends."""
    bits = nodes["bits"].view(np.uint32)
    out, stack = [], [0]
    while stack:
        pos = stack.pop()
        if bits[root + pos] >> 31:
            out.append(pos)
        else:
            li = int(nodes["left_idx"][root + pos])
            stack.append(li + 1)
            stack.append(li)
    return np.array(out, dtype=np.int64)


class SparseOrderForest:
    """Sparse forest of search trees: .nodes, .roots, .cols and per tree (s, fid, def_left, leaf_pos)."""

    def __init__(self, cols):
        self.cols, self.trees, self._parts = cols, [], []

    def add(self, nodes, s, fid, def_left, leaf_pos):
        self._parts.append(nodes)
        self.trees.append((np.asarray(s, dtype=np.float32), fid, bool(def_left), leaf_pos))
        return self

    @property
    def T(self):
        return len(self.trees)

    @property
    def nodes(self):
        return np.concatenate(self._parts)

    @property
    def roots(self):
        return np.cumsum([0] + [p.size for p in self._parts[:-1]]).astype(np.int32)

    def thresholds_by_fid(self):
        out = {}
        for s, fid, _, _ in self.trees:
            out.setdefault(fid, []).append(s)
        return {f: np.concatenate(v) for f, v in out.items()}


def sparse_from_dense(of, sparse_nodes, roots):
    """The converted (dense_to_sparse) form of a dense search-tree forest: ranks map through the in-order leaf sequence."""
    sf = SparseOrderForest(of.cols)
    bounds = list(roots) + [sparse_nodes.size]
    for t, (s, fid, dl, _) in enumerate(of.trees):
        part = sparse_nodes[bounds[t]:bounds[t + 1]]
        sf.add(part, s, fid, dl, sparse_leaf_order(part, 0))
    return sf


def sparse_expected_leaf(sf, data, missing):
    out = np.empty((data.shape[0], sf.T), dtype=np.uint32)
    for t, (s, fid, dl, leaf_pos) in enumerate(sf.trees):
        x = data[:, fid]
        k = np.where(in_band(x, missing), 0 if dl else s.size, rank_of(s, x))
        out[:, t] = leaf_pos[k]
    return out


def sparse_expected_sums(sf, leaf, num_classes=1):
    acc = np.zeros((leaf.shape[0], num_classes), dtype=np.float32)
    for t, part in enumerate(sf._parts):
        acc[:, t % num_classes] = acc[:, t % num_classes] + part["val"][leaf[:, t].astype(np.int64)]
    return acc[:, 0] if num_classes == 1 else acc


def sparse_first_mismatch(sf, data, want_leaf, got_leaf):
    bad = np.argwhere(want_leaf != got_leaf)
    if bad.size == 0:
        return ""
    r, t = (int(v) for v in bad[0])
    s, fid, _, leaf_pos = sf.trees[t]
    xb = int(np.ascontiguousarray(data[r, fid:fid + 1]).view(np.uint32)[0])
    got = np.flatnonzero(leaf_pos == int(got_leaf[r, t]))
    return (f"{bad.shape[0]} wrong leaf positions; first at row {r}, tree {t}: feature {fid}, x = 0x{xb:08x} ({data[r, fid]!r}), "
            f"expected rank {int(np.flatnonzero(leaf_pos == int(want_leaf[r, t]))[0])}, "
            f"got rank {int(got[0]) if got.size else 'none (position %d is no leaf)' % int(got_leaf[r, t])}")


# ---- the forests and row sets of tests/test_rank_exact_gpu.py (every one is pinned to the oracle by test_order_forests.py) ----
M_IN = 0.25     # a sentinel inside the data range: its band (+-1e-6) is ~33 float32 steps wide on each side
M_FAR = -999.0  # the usual sentinel: the band is narrower than one float32 step


def _case(of, missing, n_random=300, seed=0, max_rows=None):
    data, n_triples = critical_matrix(of.thresholds_by_fid(), of.cols, missing, n_random, seed, max_rows)
    return of, data, n_triples, missing


@functools.lru_cache(maxsize=None)
def quantiser_case(cols, D):
    """One depth-D tree on every feature (127 thresholds: u8 codes; 1023: u16), def_left alternating."""
    rng = np.random.default_rng(10 * cols + D)
    of = OrderForest(D, cols)
    for f in range(cols):
        of.add(distinct_sorted(rng, (1 << D) - 1, scale=1.0 + f % 3, loc=0.1 * f), f, f % 2 == 0)
    return _case(of, M_IN)


@functools.lru_cache(maxsize=None)
def u8_limit_case(extra):
    """Two depth-7 trees on feature 0 with disjoint thresholds: 254 distinct values, the last u8 table; extra = 1: a third tree
    holding one more distinct value 127 times -> 255, the handle must leave u8.  Feature 1 carries 127 thresholds."""
    rng = np.random.default_rng(254)
    v = distinct_sorted(rng, 255 + 127)
    of = OrderForest(7, 4)
    of.add(np.sort(v[0:254:2]), 0, True)
    of.add(np.sort(v[1:254:2]), 0, False)
    if extra:
        of.add(v[254:255], 0, True, pad="repeat")
    of.add(np.sort(rng.permutation(v[255:])[:127]), 1, False)
    assert of.most_distinct() == 254 + extra
    return _case(of, M_IN)


TABLE_SIZES = (1, 2, 3, 255, 256, 257, 1023, 1024)


@functools.lru_cache(maxsize=None)
def table_size_case(n):
    """Feature 0 sees exactly n distinct thresholds (the tree is filled by repeating the largest; n = 1024: a second tree with
    one more value), feature 1 about a third as many, feature 3 a single one: unequal pairs.  cols = 6."""
    rng = np.random.default_rng(n)
    D = 2 if n <= 3 else 8 if n <= 255 else 9 if n <= 511 else 10
    first = min(n, (1 << D) - 1)
    v = distinct_sorted(rng, n)
    of = OrderForest(D, 6)
    of.add(v[:first], 0, True, pad="repeat")
    if n > first:
        of.add(v[first:], 0, False, pad="repeat")
    of.add(distinct_sorted(rng, max(1, n // 3), scale=3.0), 1, False, pad="repeat")
    of.add(distinct_sorted(rng, 1), 3, True, pad="repeat")
    assert of.most_distinct() == n
    return _case(of, M_IN)


@functools.lru_cache(maxsize=None)
def large_case(kind):
    """32767 distinct thresholds on a feature (the last u16 table): "pair" both features of cols = 2, "together" one large and
    one 4095-entry feature, "single" cols = 1, "groups" two trees with disjoint thresholds on feature 0 (65534: two groups)."""
    rng = np.random.default_rng(15)
    D, n = 15, 32767
    if kind == "groups":
        v = distinct_sorted(rng, 2 * n, scale=4.0)
        of = OrderForest(D, 2)
        of.add(np.sort(v[0::2]), 0, True)
        of.add(np.sort(v[1::2]), 0, False)
    elif kind == "single":
        of = OrderForest(D, 1).add(distinct_sorted(rng, n, scale=4.0), 0, True)
    else:
        of = OrderForest(D, 2).add(distinct_sorted(rng, n, scale=4.0), 0, True)
        if kind == "pair":
            of.add(distinct_sorted(rng, n, scale=0.5, loc=0.25), 1, False)
        else:
            of.add(distinct_sorted(rng, 4095, scale=2.0), 1, False, pad="repeat")
    return _case(of, M_IN)


BUCKET_KINDS = ("edges", "sliver", "equal", "inf_only", "denormals", "log_uniform", "full_range", "sentinel")


def bucket_thresholds(kind, n, rng, missing):
    if kind == "edges":  # lo + k (hi - lo) / 4096 on [-1, 1]: bucket edges for every B = 256 ... 4096
        k = np.arange(4097)
        k = np.concatenate([k[:1], np.sort(rng.choice(k[1:-1], n - 2, replace=False)), k[-1:]])
        return (k / 2048.0 - 1.0).astype(np.float32)
    if kind == "sliver":  # one very long run, two outliers
        return np.sort(np.concatenate([(1.0 + 1e-4 * rng.standard_normal(n - 2)).astype(np.float32), F32([-1e30, 1e30])]))
    if kind == "equal":
        return np.full(n, 0.75, dtype=np.float32)
    if kind == "inf_only":
        return np.sort(np.where(np.arange(n) % 2 == 0, -np.inf, np.inf).astype(np.float32))
    if kind == "denormals":  # multiples of the smallest denormal around zero, both zeros
        k = np.arange(n) - n // 2
        v = (k * 2.0 ** -149).astype(np.float32)
        v[n // 2 - 1] = -0.0
        return np.sort(v)
    if kind == "log_uniform":  # 80 decades, both signs
        return np.sort((np.exp(rng.uniform(-96.0, 88.0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32))
    if kind == "full_range":  # hi - lo overflows: the bucket scale is not finite
        v = rng.uniform(-1.0, 1.0, n - 2) * float(FLT_MAX)
        return np.sort(np.concatenate([v.astype(np.float32), F32([-FLT_MAX, FLT_MAX])]))
    if kind == "sentinel":  # the sentinel, its band and the values just outside among the thresholds
        sp = specials(missing)[11:]
        v = np.unique(np.concatenate([sp, (missing + 1e-5 * rng.standard_normal(n)).astype(np.float32)]))
        keep = np.concatenate([sp, rng.permutation(v[~np.isin(v, sp)])[: n - sp.size]])
        return np.sort(keep)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def bucket_case(kind):
    """cols = 6 (the pair quantise kernels), depth 12: 4095 thresholds of the distribution on feature 0, 1023 on feature 1."""
    rng = np.random.default_rng(BUCKET_KINDS.index(kind))
    of = OrderForest(12, 6)
    of.add(bucket_thresholds(kind, 4095, rng, M_IN), 0, True)
    of.add(bucket_thresholds(kind, 1023, rng, M_IN), 1, False, pad="repeat")
    of.add(distinct_sorted(rng, 100), 4, True, pad="repeat")
    return _case(of, M_IN)


LEVEL_DEPTHS = (2, 9, 10, 11, 12, 14)


@functools.lru_cache(maxsize=None)
def levels_case(cols, D):
    """Depth-D trees on the first, a middle and the last feature: LDS top, heap levels, bottom blocks."""
    rng = np.random.default_rng(100 * D + cols)
    of = OrderForest(D, cols)
    for j, f in enumerate((0, cols // 2 + 1, cols - 1)):
        of.add(distinct_sorted(rng, (1 << D) - 1, scale=1.0 + j), f, j % 2 == 0)
    return _case(of, M_IN if D != 11 else M_FAR, n_random=100)


@functools.lru_cache(maxsize=None)
def slices_case():
    """132 depth-8 trees on 18 features (the tree-slice form at 1000 rows)."""
    rng = np.random.default_rng(132)
    of = OrderForest(8, 18)
    for t in range(132):
        of.add(distinct_sorted(rng, 255, scale=1.0 + t % 4), t % 18, t % 3 == 0)
    return _case(of, M_IN)


@functools.lru_cache(maxsize=None)
def wide_case(cols, D):
    """Search trees on a handful of features of wide rows."""
    rng = np.random.default_rng(cols + D)
    of = OrderForest(D, cols)
    for j, f in enumerate((0, 1, cols // 2, cols - 3, cols - 1)):
        of.add(distinct_sorted(rng, (1 << D) - 1, scale=1.0 + j), f, j % 2 == 1)
    return _case(of, M_IN, n_random=60, max_rows=2048)  # (an even sample of the depth-13 triples: 5000 columns per row)


STREAM_KINDS = ("fine_grid", "two_scales", "constant")


@functools.lru_cache(maxsize=None)
def stream_case(kind):
    """cols = 1024, one affine 16-bit key map over all thresholds.  fine_grid: thresholds one float32 step apart beside a
    feature spanning +-1000 (neighbours share a key); two_scales: one feature 1000 x the others; constant: a feature whose
    thresholds are all equal."""
    rng = np.random.default_rng(STREAM_KINDS.index(kind))
    D, cols = 8, 1024
    n = (1 << D) - 1
    of = OrderForest(D, cols)
    if kind == "fine_grid":
        g = np.float32(1.0) + np.arange(n, dtype=np.float32) * np.float32(2.0 ** -23)
        of.add(g, 0, True)
        of.add(np.sort(np.float32(-3.0) - np.arange(n, dtype=np.float32) * np.float32(2.0 ** -22)), 5, False)
        of.add(distinct_sorted(rng, n, scale=1000.0), 511, True)
    elif kind == "two_scales":
        of.add(distinct_sorted(rng, n), 0, True)
        of.add(distinct_sorted(rng, n, scale=1000.0), 1, False)
        of.add(distinct_sorted(rng, n), 1023, False)
    else:
        of.add(np.full(n, 0.75, dtype=np.float32), 7, True)
        of.add(distinct_sorted(rng, n), 8, False)
        of.add(np.full(n, -2.5, dtype=np.float32), 1000, False)
    for t in range(9):  # a few more trees: the form's lanes are trees
        of.add(distinct_sorted(rng, n), 16 + 100 * t, t % 2 == 0)
    return _case(of, M_IN, n_random=60)


@functools.lru_cache(maxsize=None)
def multiclass_case():
    """Nine depth-7 trees on 8 features, three classes."""
    rng = np.random.default_rng(3)
    of = OrderForest(7, 8)
    for t in range(9):
        of.add(distinct_sorted(rng, 127), (3 * t) % 8, t % 2 == 0)
    return _case(of, M_IN)


@functools.lru_cache(maxsize=None)
def irregular_case(cols):
    """Unbalanced search trees (random insertion order, depth capped at 24) and vines (sorted insertion: 24 levels)."""
    rng = np.random.default_rng(24 + cols)
    sf = SparseOrderForest(cols)
    for t, (n, order) in enumerate([(3000, "random"), (200, "sorted"), (800, "random"), (24, "sorted"), (1, "random"),
                                    (5000, "random"), (60, "sorted")]):
        fid = (5 * t) % cols
        dl = t % 2 == 0
        nodes, s, leaf_pos = sparse_bst(distinct_sorted(rng, n, scale=1.0 + t), fid, dl, order, seed=t)
        sf.add(nodes, s, fid, dl, leaf_pos)
    data, n_triples = critical_matrix(sf.thresholds_by_fid(), cols, M_IN, 200, 1)
    return sf, data, n_triples, M_IN
