"""Independent numpy restatement of the sparse walk with categorical splits (tahoe_sparse_forest_create_cat), for the tests.

Nodes as tahoe_sparse_node (val, bits = fid | def_left << 30 | is_leaf << 31, left_idx relative to the tree's root), root offsets
`trees`, and the categorical splits as the C struct holds them: node[k], offset[k], words, members_left[k] (None: members go
right everywhere).  At every node, with x the row's value of feature fid:
  missing (|x - missing| <= 1e-6 in float32): right iff not def_left;
  numeric node: right iff x >= val;
  split k: member = 0 <= x < 32 * nwords and bit trunc(x) of the split's words is set; right iff member != members_left[k].
Tree t belongs to class t % num_classes; each class's leaf values are added in float32 in increasing tree order, from 0.0f or
from `init`.  Leaf indices are relative to the tree's root."""
import numpy as np

LEAF = 1 << 31
DEF_LEFT = 1 << 30
FID_MASK = (1 << 30) - 1


def predict(nodes, trees, data, missing, node=(), offset=(0,), words=(), members_left=None, num_classes=1, init=None):
    """(sums, leaf): sums [rows] float32 (num_classes == 1) or [rows, num_classes]; leaf [rows, num_trees] uint32."""
    data = np.ascontiguousarray(data, dtype=np.float32)
    rows = data.shape[0]
    T = int(len(trees))
    val = np.ascontiguousarray(nodes["val"], dtype=np.float32)
    bits = np.ascontiguousarray(nodes["bits"]).view(np.uint32)
    left = np.ascontiguousarray(nodes["left_idx"], dtype=np.int64)
    split_of = np.full(len(nodes), -1, np.int64)  # node index -> split k
    split_of[np.asarray(node, dtype=np.int64)] = np.arange(len(node))
    offset = np.asarray(offset, dtype=np.int64)
    words = np.asarray(words, dtype=np.uint32)
    ml = np.zeros(len(node), bool) if members_left is None else np.asarray(members_left, dtype=np.uint8) != 0
    miss = np.float32(missing)
    leaf = np.zeros((rows, T), np.uint32)
    vals = np.zeros((rows, T), np.float32)
    r_all = np.arange(rows)
    for t in range(T):
        root = int(trees[t])
        curr = np.zeros(rows, np.int64)
        while True:
            g = root + curr
            inner = (bits[g] & LEAF) == 0
            if not inner.any():
                break
            r = r_all[inner]
            gi = g[inner]
            x = data[r, bits[gi] & FID_MASK]
            with np.errstate(invalid="ignore"):
                is_missing = np.abs(x - miss) <= np.float32(1e-6)
                right = x >= val[gi]
            k = split_of[gi]
            cat = k >= 0
            if cat.any():
                kc, xc = k[cat], x[cat]
                nw = offset[kc + 1] - offset[kc]
                with np.errstate(invalid="ignore"):
                    in_range = (xc >= np.float32(0.0)) & (xc < (32 * nw).astype(np.float32))
                c = np.where(in_range, xc, 0.0).astype(np.int64)  # truncation (x >= 0 here)
                w = words[np.where(in_range, offset[kc] + c // 32, 0)] if words.size else np.zeros(c.size, np.uint32)
                member = in_range & (((w >> (c % 32).astype(np.uint32)) & 1) == 1)
                right[cat] = member != ml[kc]
            right = np.where(is_missing, (bits[gi] & DEF_LEFT) == 0, right)
            curr[inner] = left[gi] + right.astype(np.int64)
        leaf[:, t] = curr
        vals[:, t] = val[root + curr]
    C = num_classes
    sums = np.zeros((rows, C), np.float32)
    if init is not None:
        sums[:] = np.asarray(init, np.float32).reshape(rows, C)
    for t in range(T):  # tree order, float32
        sums[:, t % C] = sums[:, t % C] + vals[:, t]
    return (sums[:, 0] if C == 1 else sums), leaf
