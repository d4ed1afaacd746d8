"""Forests and grids of the partial-dependence tests (numpy only): random irregular forests with covers, classes and categorical
splits, grids that carry the special values, and the left-descending chains that fill the walk's stack."""
import numpy as np

SPARSE_NODE_DTYPE = np.dtype([("val", "<f4"), ("bits", "<i4"), ("left_idx", "<i4")])
LEAF = np.int32(-(1 << 31))
DEF_LEFT = 1 << 30
MISSING = -999.0


def pack_cats(categories, members_left):
    """(node, offset, words, ml) as tahoe_categorical_splits holds them -- the layout tahoe_amd.capi.pack_categorical builds: a
    split's bitset has as many words as its largest category needs (none for an empty set)."""
    keys = sorted(categories)
    node = np.array(keys, np.int32)
    offset = np.zeros(len(keys) + 1, np.int32)
    words = []
    for k, i in enumerate(keys):
        c = sorted(set(categories[i]))
        w = np.zeros(c[-1] // 32 + 1 if c else 0, np.uint32)
        for x in c:
            w[x // 32] |= np.uint32(1 << (x % 32))
        words += w.tolist()
        offset[k + 1] = len(words)
    ml = np.array([i in set(members_left) for i in keys], np.uint8)
    return node, offset, np.array(words, np.uint32), ml


def random_forest(seed, num_trees, num_cols, max_depth, leaf_prob, num_classes=1, cat_features=(), zero_cover_prob=0.05):
    """Irregular trees, children adjacent and after their parent.  Thresholds are multiples of 0.25 (a grid value can equal one),
    child covers split their parent's (non-integers; now and then one child gets cover 0), leaf values are normal."""
    rng = np.random.default_rng(seed)
    nodes, covers, roots, categories, members_left = [], [], [], {}, []
    for _ in range(num_trees):
        base = len(nodes)
        roots.append(base)
        nodes.append(None)
        covers.append(float(np.float32(rng.uniform(50, 500))))
        queue = [(0, 0)]
        while queue:
            pos, d = queue.pop(0)
            if d == max_depth or (d >= 2 and rng.random() < leaf_prob):
                nodes[base + pos] = (np.float32(rng.normal()), LEAF, 0)
                continue
            left = len(nodes) - base
            fid = int(rng.integers(num_cols))
            bits = fid | (DEF_LEFT if rng.random() < 0.5 else 0)
            nodes[base + pos] = (np.float32(np.round(rng.normal() * 4) / 4), np.int32(bits), left)
            if fid in cat_features:
                categories[base + pos] = [int(c) for c in np.flatnonzero(rng.random(40) < 0.4)]
                if rng.random() < 0.5:
                    members_left.append(base + pos)
            u = rng.random()
            share = 0.0 if u < zero_cover_prob / 2 else 1.0 if u < zero_cover_prob else rng.uniform(0.05, 0.95)
            cl = np.float32(covers[base + pos] * share)
            cr = np.float32(covers[base + pos] - float(cl))
            if covers[base + pos] == 0.0:  # below a zero-cover child: never visited, but create() wants a positive sum
                cl, cr = np.float32(1.0), np.float32(2.0)
            nodes += [None, None]
            covers += [float(cl), float(cr)]
            queue += [(left, d + 1), (left + 1, d + 1)]
    fo = dict(nodes=np.array(nodes, dtype=SPARSE_NODE_DTYPE), trees=np.array(roots, np.int32), covers=np.array(covers, np.float32),
              num_cols=num_cols, num_classes=num_classes, missing=MISSING, cats=None, categories=None, members_left=(),
              cat_features=tuple(cat_features))
    if cat_features:
        fo["categories"], fo["members_left"] = categories, members_left
        fo["cats"] = pack_cats(categories, members_left)
    return fo


SPECIALS = [MISSING, np.nan, -0.0, np.inf, -np.inf, 0.0, MISSING + 5e-7]


def random_grid(fo, feats, G, seed):
    """[G, len(feats)] float32: normal values, thresholds of the forest (exactly), the special values; category ids (and values
    that are no category) in the columns of categorical features."""
    rng = np.random.default_rng(seed)
    thr = fo["nodes"]["val"][fo["nodes"]["bits"] >= 0]
    grid = np.zeros((G, len(feats)), np.float32)
    for j, f in enumerate(feats):
        if f in fo["cat_features"]:
            col = rng.integers(0, 46, G).astype(np.float32) + np.where(rng.random(G) < 0.2, 0.7, 0.0).astype(np.float32)
            col[rng.random(G) < 0.1] = -1.0
        else:
            col = rng.normal(size=G).astype(np.float32)
            pick = rng.random(G) < 0.3
            col[pick] = rng.choice(thr, pick.sum())
        sp = rng.random(G) < 0.2
        col[sp] = rng.choice(np.array(SPECIALS, np.float32), sp.sum())
        grid[:, j] = col
    return grid


RANDOM_CASES = [
    dict(id="one_class", forest=dict(seed=11, num_trees=12, num_cols=8, max_depth=9, leaf_prob=0.25),
         targets=[[2], [0, 5], [1, 2, 3, 4, 6]]),
    dict(id="three_classes", forest=dict(seed=12, num_trees=12, num_cols=8, max_depth=9, leaf_prob=0.25, num_classes=3),
         targets=[[7], [3, 1], [6, 5, 4, 2, 0]]),
    dict(id="categorical", forest=dict(seed=13, num_trees=8, num_cols=8, max_depth=7, leaf_prob=0.2, num_classes=2,
                                       cat_features=(1, 6)),
         targets=[[1], [0], [6, 3, 1]]),
]


def chain(depth, num_cols=33):
    """One tree that descends `depth` edges through left children; every right child is a leaf, so a walk that takes both sides
    has `depth` right siblings pending at the bottom.  Node d splits on feature d % 32 at 0.0 (x >= 0 goes right); leaf values
    are distinct powers of two and small integers, covers halve to the left."""
    n = 2 * depth + 1
    sn = np.zeros(n, dtype=SPARSE_NODE_DTYPE)
    cv = np.zeros(n, np.float32)
    cv[0] = 1.0
    pos = 0
    for d in range(depth):
        left = 2 * d + 1
        sn[pos] = (0.0, d % 32, left)
        sn[left + 1] = (np.float32(d + 1), LEAF, 0)
        cv[left], cv[left + 1] = 3.0, 1.0 + (d % 3)
        pos = left
    sn[pos] = (np.float32(-7.5), LEAF, 0)
    return dict(nodes=sn, trees=np.array([0], np.int32), covers=cv, num_cols=num_cols, num_classes=1, missing=MISSING, cats=None,
                categories=None, members_left=(), cat_features=())
