"""Decoder forests for category-set splits, with a closed-form answer (numpy only; no GPU, no oracle, nothing of the library but
the sparse node dtype, which the callers pass in; the oblivious decoder hands its category ids to the handle, whose packer stores
them in as many words as the largest needs).

A decoder forest is T <= 24 sparse trees that share one split pool.  Tree k is a run of numeric "pilot" nodes on column 0 -- every
test row holds 0.0 there, the threshold is -1 and the default side is right, so every row passes every pilot node to the right --
and below it ONE categorical node on column f_k with the set S_k (stored in W_k 32-bit words), members_left ml_k and def_left
dl_k, whose two leaves hold 0.0f and 2^k.  The pilots form a chain of d_k nodes (each with a stray leaf on its left) or a
complete tree of L_k levels whose right-most bottom node is the categorical one.  A row's sum over the trees is exact in float32
and its binary digits are the branches; predict_leaf_idx gives the branch directly.  The pool order is the tree order (the
split list ascends by node index), so neighbouring trees hold neighbouring sets.

The closed form is the documented rule (include/tahoe_amd.h, tahoe_sparse_forest_create_cat) said with Python sets and math.trunc:
  missing -- |x - missing| <= 1e-6 in float32, a null, or a NaN on a nan_missing handle --: right iff not def_left;
  else member = 0 <= x < 2^24 and trunc(x) in S_k; right iff member != ml_k.
It reads no bitset: the words are built from S_k for the library and for tests/categorical_ref.py alone, and
tests/test_cat_edges_ref.py holds the two against each other, and the closed form against answers typed by hand.
"""
import math

import numpy as np

F32 = np.float32
LEAF = np.int32(-(1 << 31))
DEF_LEFT = 1 << 30
PILOT_FID = 0
PAIRS = ((False, False), (False, True), (True, False), (True, True))  # (members_left, def_left)
SENTINELS = (-999.0, 5.0, 0.0, float("nan"), float("inf"))
BATCHES = (1, 63, 64, 65, 257)
WIDEST_WORDS = 1 << 19  # the widest set the create accepts: categories < 2^24
CAT_VAL = F32(-3.0)     # val of a categorical node: ignored by the rule; read as a threshold it would send most rows right


# ---- sets ----
class CatSet:
    """A set of categories stored in W words: members is a frozenset of ints in [0, 32 W)."""

    def __init__(self, W, members, name):
        self.W, self.members, self.name = int(W), frozenset(int(m) for m in members), name
        assert all(0 <= m < 32 * self.W for m in self.members), name

    def words(self):
        w = np.zeros(self.W, np.uint32)
        for m in self.members:
            w[m // 32] |= np.uint32(1 << (m % 32))
        return w

    def __repr__(self):
        return self.name


def single(b, W=None):
    W = b // 32 + 1 if W is None else W
    return CatSet(W, [b], f"bit{b}/W{W}")


def ones(W):
    return CatSet(W, range(32 * W), f"ones/W{W}")


def ones_but(W, b):
    return CatSet(W, [m for m in range(32 * W) if m != b], f"ones-but-{b}/W{W}")


def alternating(W, odd):
    return CatSet(W, range(int(odd), 32 * W, 2), f"alt{int(odd)}/W{W}")


def empty(W=0):
    return CatSet(W, [], f"empty/W{W}")


def widest(seed=19):
    rng = np.random.default_rng(seed)
    m = {0, 31, 32, (1 << 24) - 32, (1 << 24) - 1} | {int(v) for v in rng.integers(0, 1 << 24, 300)}
    return CatSet(WIDEST_WORDS, m, "widest")


WORDS = (0, 1, 2, 3, 31, 32, 33)


def sets_of_interest():
    out = [single(b) for b in (0, 1, 30, 31, 32, 33, 62, 63, 64)]
    out += [single(32 * W - 1) for W in (3, 31, 32, 33)]          # the last bit of the last word (31 and 63 are above)
    out += [single(0, 33), single(31, 2), single(32, 33)]         # a low member under words of zeros
    out += [ones(W) for W in WORDS[1:]]
    out += [ones_but(1, 31), ones_but(2, 32), ones_but(3, 63), ones_but(32, 0), ones_but(33, 32 * 33 - 1)]
    out += [alternating(1, 0), alternating(2, 1), alternating(33, 0)]
    out += [empty(0), empty(1), empty(2), empty(33)]
    return out


# ---- trees and forests ----
class Tree:
    """shape "chain": d pilot nodes in a row; "full": a complete pilot tree of d levels."""

    def __init__(self, cset, ml, dl, d=0, shape="chain"):
        self.cset, self.ml, self.dl, self.d, self.shape = cset, bool(ml), bool(dl), int(d), shape


class DecoderForest:
    """.sn / .tr: the sparse nodes and root offsets; .node / .offset / .words / .ml: the split arrays of tahoe_categorical_splits;
    .cols, .fid[k]; .left_pos[k]: the position (relative to the root) of tree k's 0.0f leaf, the 2^k leaf follows it."""

    def __init__(self, node_dtype, trees, cols=None, fid_base=1, name="", fids=None, pilot_fid=PILOT_FID):
        assert 1 <= len(trees) <= 24
        self.trees, self.name, self.pilot_fid = list(trees), name, pilot_fid
        self.T = len(trees)
        self.fid = [fid_base + k for k in range(self.T)] if fids is None else [int(v) for v in fids]
        self.cols = max(self.fid) + 1 if cols is None else cols
        assert len(self.fid) == self.T == len(set(self.fid)) and max(self.fid + [pilot_fid]) < self.cols and pilot_fid not in self.fid
        parts, self.left_pos, node, roots, at = [], [], [], [], 0
        for k, t in enumerate(self.trees):
            sn, cat = _tree_nodes(node_dtype, t, self.fid[k], k, pilot_fid)
            parts.append(sn)
            roots.append(at)
            node.append(at + cat)
            self.left_pos.append(cat + 1)
            at += sn.size
        self.sn = np.concatenate(parts)
        self.tr = np.array(roots, np.int32)
        self.node = np.array(node, np.int32)
        self.offset = np.zeros(self.T + 1, np.int32)
        self.offset[1:] = np.cumsum([t.cset.W for t in self.trees])
        self.words = np.concatenate([t.cset.words() for t in self.trees] + [np.zeros(1, np.uint32)])  # (never an empty array)
        self.ml = np.array([t.ml for t in self.trees], np.uint8)

    def __repr__(self):
        return self.name

    def goes_right(self, data, missing, nan_missing=False, null=None):
        """bool [rows, T] by the closed form; null: bool [rows, cols], a null entry is missing whatever lies under it."""
        data = np.ascontiguousarray(data, dtype=np.float32)
        out = np.empty((data.shape[0], self.T), bool)
        for k, t in enumerate(self.trees):
            x = data[:, self.fid[k]]
            miss = is_missing(x, missing, nan_missing)
            if null is not None:
                miss = miss | null[:, self.fid[k]]
            uniq, inv = np.unique(x.view(np.uint32), return_inverse=True)
            member = np.array([is_member(float(u.view(np.float32)), t.cset.members) for u in uniq], bool)[inv.reshape(-1)]
            out[:, k] = np.where(miss, not t.dl, member != t.ml)
        return out

    def expected_leaf(self, right):
        return (np.array(self.left_pos, np.uint32)[None, :] + right.astype(np.uint32)).astype(np.uint32)

    def expected_sums(self, right, num_classes=1, init=None, num_trees=None):
        """float32 sums in tree order: [rows] or [rows, num_classes]; tree k belongs to class k % num_classes."""
        rows = right.shape[0]
        acc = np.zeros((rows, num_classes), np.float32)
        if init is not None:
            acc[:] = np.asarray(init, np.float32).reshape(rows, num_classes)
        for k in range(self.T if num_trees is None else num_trees):
            acc[:, k % num_classes] = acc[:, k % num_classes] + np.where(right[:, k], F32(2.0 ** k), F32(0.0))
        return acc[:, 0] if num_classes == 1 else acc

    def rows(self, missing, min_rows=max(BATCHES)):
        """float32 [rows, cols]: the pilot column 0.0, column f_k the edge values of S_k (rotated by 7 k so that one row does
        not hold the same value everywhere), the shorter lists repeated; the other columns 0.5."""
        vals = [edge_values(t.cset, missing) for t in self.trees]
        n = max(max(v.size for v in vals), min_rows)
        n += n % 64 == 0  # (a last tile that is not full)
        data = np.full((n, self.cols), 0.5, np.float32)
        data[:, self.pilot_fid] = 0.0
        for k, v in enumerate(vals):
            data[:, self.fid[k]] = np.roll(np.resize(v, n), 7 * k)
        return data


def _tree_nodes(dtype, t, fid, k, pilot_fid=PILOT_FID):
    if t.shape == "chain":
        sn = np.zeros(2 * t.d + 3, dtype)
        for i in range(t.d):
            sn[2 * i] = (-1.0, pilot_fid, 2 * i + 1)
            sn[2 * i + 1] = (0.0, LEAF, 0)
        cat = 2 * t.d
    else:
        assert t.shape == "full"
        inner = (1 << t.d) - 1  # the pilots, as a heap; the bottom level: stray leaves and, last, the categorical node
        sn = np.zeros(2 * inner + 3, dtype)
        h = np.arange(inner)
        sn["val"][:inner], sn["bits"][:inner], sn["left_idx"][:inner] = -1.0, pilot_fid, 2 * h + 1
        sn["bits"][inner:2 * inner] = LEAF
        cat = 2 * inner
    sn[cat] = (CAT_VAL, fid | (DEF_LEFT if t.dl else 0), cat + 1)
    sn[cat + 1] = (0.0, LEAF, 0)
    sn[cat + 2] = (2.0 ** k, LEAF, 0)
    return sn, cat


# ---- the closed form ----
def is_missing(x, missing, nan_missing=False):
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        band = np.abs(x - F32(missing)) <= F32(1.0e-6)
    return band | np.isnan(x) if nan_missing else band


def is_member(x, members):
    """x: a Python float holding a float32 value.  NaN fails the range test; -0.0 passes it and truncates to 0."""
    return 0.0 <= x < 16777216.0 and math.trunc(x) in members


# ---- rows ----
def _f32(values):
    with np.errstate(over="ignore"):
        return np.array(values, dtype=np.float64).astype(np.float32)


FIXED = _f32([-0.0, 2.0 ** -149, -2.0 ** -149, np.nextafter(F32(1), F32(0)), -0.5, -1.0, -1e9, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 2,
              2.0 ** 31, 2.0 ** 32, 2.0 ** 32 + 512, 3e38, np.inf, -np.inf, np.nan])


def sentinel_values(missing):
    """The sentinel, the two edges of its band as float32 computes them, and both float32 neighbours of each."""
    m = F32(missing)
    if not np.isfinite(m):
        return np.array([m], np.float32)
    edges = [m, m + F32(1e-6), m - F32(1e-6)]
    with np.errstate(over="ignore"):
        return np.array(edges + [np.nextafter(e, F32(s)) for e in edges[1:] for s in (-np.inf, np.inf)], np.float32)


def edge_categories(cset):
    """The boundary categories of the words, and every member (of a large set: those on a word's first or last bit and the two
    at either end) with both neighbours."""
    W = cset.W
    cats = {0, 31, 32, 32 * W - 1, 32 * W, 32 * W + 1, 32 * W + 31, 32 * W + 32}
    mem = sorted(cset.members)
    if len(mem) > 8:
        mem = sorted(set(mem[:2] + mem[-2:] + [m for m in mem if m % 32 in (0, 31)]))
    for m in mem:
        cats |= {m - 1, m, m + 1}
    return sorted(c for c in cats if c >= 0)


def edge_values(cset, missing):
    c = np.array(edge_categories(cset), np.float64)
    per_cat = np.stack([c.astype(np.float32), (c + 0.5).astype(np.float32), np.nextafter((c + 1).astype(np.float32), F32(0))], axis=1)
    return np.concatenate([per_cat.reshape(-1), FIXED, sentinel_values(missing)]).astype(np.float32)


# ---- the forests ----
def _pad3(trees):
    """A tree count that three classes divide."""
    fill = [Tree(ones(1), False, True), Tree(empty(1), True, False)]
    return trees + fill[: (-len(trees)) % 3]


def neighbour_forest(dtype, xs, phase, **kw):
    """Every set of xs once between all-ones sets (three words: the header that follows a set has its low bits set) and once between
    words of zeros.  Appearance a of set i takes the (members_left, def_left) pair i + 2 a + phase: phases 0 and 1 give all four."""
    assert len(xs) <= 5
    trees = []
    for a, nb in enumerate((ones(3), empty(2))):
        trees.append(Tree(nb, a, not a))
        for i, x in enumerate(xs):
            ml, dl = PAIRS[(i + 2 * a + phase) % 4]
            trees += [Tree(x, ml, dl), Tree(nb, (i + a) % 2, (i + phase) % 2)]
    return DecoderForest(dtype, _pad3(trees), name=f"neighbours[{','.join(x.name for x in xs)}]p{phase}", **kw)


def ends_forest(dtype, first, last, phase=0, **kw):
    """`first` opens the pool (its header is word 0), sits in the middle between a set of ones and words of zeros, and `last` ends the
    pool: behind its words (or, for an empty set, behind its header) the pool is over."""
    p = [PAIRS[(i + phase) % 4] for i in range(6)]
    trees = [Tree(first, *p[0]), Tree(ones(3), *p[1]), Tree(first, *p[2]), Tree(empty(2), *p[3]), Tree(ones(1), *p[4]), Tree(last, *p[5])]
    return DecoderForest(dtype, trees, name=f"ends[{first.name}..{last.name}]p{phase}", **kw)


def neighbour_forests(dtype, **kw):
    xs = sets_of_interest()
    return [neighbour_forest(dtype, xs[i:i + 5], phase, **kw) for i in range(0, len(xs), 5) for phase in (0, 1)]


def ends_forests(dtype, **kw):
    pairs = [(single(63), single(63)), (single(32), single(32)), (ones(2), ones(2)), (single(31, 2), empty(0)),
             (empty(0), single(31)), (ones(33), empty(33))]
    return [ends_forest(dtype, a, b, i, **kw) for i, (a, b) in enumerate(pairs)]


def depth_forest(dtype, chain, full, **kw):
    """One tree per pilot depth; the sets alternate between a last-bit set, a first-bit-of-the-second-word set, ones and an empty
    set, the pairs run through all four."""
    sets = [single(31), single(32), ones(2), alternating(2, 1), empty(0), single(63)]
    trees = [Tree(sets[i % len(sets)], *PAIRS[i % 4], d=d, shape="chain") for i, d in enumerate(chain)]
    trees += [Tree(sets[(i + 1) % len(sets)], *PAIRS[(i + 2) % 4], d=d, shape="full") for i, d in enumerate(full)]
    return DecoderForest(dtype, _pad3(trees), name="depths", **kw)


def widest_forest(dtype, **kw):
    """The widest set between small ones, under all four pairs of its neighbours; its own pair is (members_left, default right)."""
    w = widest()
    trees = [Tree(ones(1), False, False), Tree(w, True, False), Tree(single(0), False, True), Tree(empty(0), True, True),
             Tree(single(31), False, True), Tree(ones(3), True, False)]
    return DecoderForest(dtype, trees, name="widest", **kw)


def first_mismatch(forest, data, want_leaf, got_leaf):
    bad = np.argwhere(np.asarray(want_leaf) != np.asarray(got_leaf))
    if bad.size == 0:
        return ""
    r, k = (int(v) for v in bad[0])
    t = forest.trees[k]
    x = data[r, forest.fid[k]]
    return (f"{forest.name}: {bad.shape[0]} wrong leaves; first at row {r}, tree {k} ({t.shape} {t.d}, set {t.cset.name}, members_left "
            f"{t.ml}, def_left {t.dl}): x = {x!r} (0x{int(np.float32(x).view(np.uint32)):08x}), expected {int(want_leaf[r, k])}, got "
            f"{int(got_leaf[r, k])}")


# ---- oblivious forests: the same sets as level splits ----
def tight(cset):
    """The set in as many words as its largest member needs: what the packer stores (an oblivious handle keeps a set of at most one
    word inline in the split record and a wider one in the pool)."""
    W = max(cset.members) // 32 + 1 if cset.members else 0
    return CatSet(W, cset.members, f"{cset.name}->W{W}")


class ObliviousDecoder:
    """Trees whose every level is a category-set split on a column of its own (column 0 is not read); leaf i of every tree holds
    float(i), so the leaf index -- bit l = the branch of level l -- is also the tree's value.  .forest(): the dict tests/
    oblivious_cat_ref.py reads; .handle_args(): what ObliviousForest takes."""

    def __init__(self, trees, name=""):
        self.trees, self.name = [[(tight(c), bool(ml), bool(dl)) for c, ml, dl in t] for t in trees], name
        self.levels = [lv for t in self.trees for lv in t]
        self.depths = np.array([len(t) for t in self.trees], np.int32)
        self.cols = 1 + len(self.levels)
        self.fids = np.arange(1, self.cols)
        self.def_left = np.array([dl for _, _, dl in self.levels], bool)
        self.leaves = np.concatenate([np.arange(1 << d, dtype=np.float32) for d in self.depths])
        self.cats = {s: sorted(c.members) for s, (c, _, _) in enumerate(self.levels)}
        self.members_left = [s for s, (_, ml, _) in enumerate(self.levels) if ml]

    def forest(self):
        return dict(depths=self.depths, fids=self.fids, thr=np.full(len(self.levels), np.nan, np.float32), def_left=self.def_left,
                    leaves=self.leaves, cols=self.cols, k=1, cats=self.cats, ml=frozenset(self.members_left))

    def expected_leaf(self, data, missing):
        data = np.ascontiguousarray(data, dtype=np.float32)
        out = np.zeros((data.shape[0], len(self.trees)), np.uint32)
        s = 0
        for t, tree in enumerate(self.trees):
            for l, (c, ml, dl) in enumerate(tree):
                x = data[:, self.fids[s]]
                member = np.array([is_member(float(v), c.members) for v in x], bool)
                right = np.where(is_missing(x, missing), not dl, member != ml)
                out[:, t] |= right.astype(np.uint32) << np.uint32(l)
                s += 1
        return out

    def expected_sums(self, leaf, init=None):
        acc = np.zeros(leaf.shape[0], np.float32) if init is None else np.array(init, np.float32)
        for t in range(leaf.shape[1]):
            acc = acc + leaf[:, t].astype(np.float32)
        return acc

    def rows(self, missing, min_rows=max(BATCHES)):
        vals = [edge_values(c, missing) for c, _, _ in self.levels]
        n = max(max(v.size for v in vals), min_rows)
        n += n % 64 == 0
        data = np.full((n, self.cols), 0.5, np.float32)
        for s, v in enumerate(vals):
            data[:, self.fids[s]] = np.roll(np.resize(v, n), 7 * s)
        return data


def oblivious_decoder():
    """Inline records (largest member <= 31) and pooled records (largest member >= 32) side by side on adjacent levels, in both
    orders, the pairs running through all four; the first pooled set opens the pool and an inline set follows the last."""
    inl = [single(31), ones(1), empty(0), single(0), ones_but(1, 31), alternating(1, 1), single(30)]
    pool = [single(32), CatSet(2, [0, 32], "0+32"), ones(2), single(63), single(33), alternating(2, 0), single(64), single(95)]
    a = [s for pair in zip(pool[:4], inl[:4]) for s in pair]           # pooled, inline, pooled, ...
    b = [s for pair in zip(inl[3:], pool[4:]) for s in pair]           # inline, pooled, ...
    c = [pool[0], pool[0], inl[0], inl[0], pool[3], inl[1]]            # equal neighbours
    trees = [[(s, *PAIRS[(i + j) % 4]) for i, s in enumerate(t)] for j, t in enumerate((a, b, c))]
    return ObliviousDecoder(trees, "oblivious")


# ---- the compact-node cut: handles of 2^14 - 1, 2^14 and 2^14 + 1 columns ----
def cut_forests(dtype, num_cols):
    """Two forests of num_cols columns: categorical nodes on the highest fid, on 0x3fff where that is another column, on 0x2000 and
    on 1 with the pilots on column 0; and the pilots -- numeric nodes -- on the highest fid with categorical nodes on 0x2000, on the
    column below the highest and on 2."""
    hi = num_cols - 1
    sets = [single(31), single(32), ones(2), alternating(2, 1), single(63), empty(0)]
    fa = list(dict.fromkeys([hi, 0x3fff if 0x3fff < num_cols else hi, 0x2000, 1]))
    fb = [0x2000, hi - 1, 2]
    a = DecoderForest(dtype, [Tree(sets[i], *PAIRS[i % 4], d=i % 3) for i in range(len(fa))], cols=num_cols, fids=fa,
                      name=f"cut{num_cols}a")
    b = DecoderForest(dtype, [Tree(sets[i + 2], *PAIRS[(i + 1) % 4], d=1 + i) for i in range(len(fb))], cols=num_cols, fids=fb,
                      pilot_fid=hi, name=f"cut{num_cols}b")
    return a, b


# ---- typed columns (predict_table) ----
TABLE_TYPES = ("uint8", "int16", "int32", "int64", "uint64", "float64")


def typed_values(cset, dtype, missing):
    """Elements of `dtype` around the set's edges: integers (negative ones, 2^24, 2^24 + 1 and 2^40 where the type has them, the
    sentinel where it is an integer), or float64 values that round to a float32 on the other side of a category's edge."""
    dtype = np.dtype(dtype)
    cats = edge_categories(cset) + [0, 5]
    if dtype.kind == "f":
        c = np.array(cats, np.float64)
        v = np.concatenate([c, c + 0.5, c + 0.999999999, c + 1 - 1e-4, FIXED.astype(np.float64),
                            [missing, 1e300, -1e300, 2.0 ** 24 - 1e-9, -1e-300]])
        return v.astype(dtype)
    info = np.iinfo(dtype)
    v = cats + [2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 40, info.max]
    if np.isfinite(missing):
        v.append(int(missing))
    if info.min < 0:
        v += [-1, -5, -32, -999, info.min]
    return np.array([x for x in v if info.min <= x <= info.max], dtype)
