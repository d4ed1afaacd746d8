"""Independent numpy restatements of partial dependence on a sparse forest (tahoe_forest_predict_partial_dependence), for the tests.

Nodes as tahoe_sparse_node (val, bits = fid | def_left << 30 | is_leaf << 31, left_idx relative to the tree's root), root offsets
`trees`, covers[i] = the cover of nodes[i], and optionally the categorical splits as the C struct holds them: cats = (node, offset,
words, members_left or None).  A grid point gives values to the target columns only.  Per tree, from the root with weight 1:
  an internal node on a target takes predict's branch for the grid value (missing sentinel: right iff not def_left; NaN left;
    x >= val right; at split k: member = 0 <= x < 32 nwords and bit trunc(x) set, right iff member != members_left[k]);
  any other internal node sends the weight down both sides, left first: w * fl and w * fr with fl = cl / (cl + cr), fr = cr / (cl + cr)
    of the child covers; a side whose fraction is exactly 0 is not visited;
  a leaf adds w * val.
Tree t belongs to class t % num_classes.

pd_f32 is the specified arithmetic: every operation above one IEEE float32 operation, leaves added in depth-first order to an
accumulator that starts at +0.0f, the trees of a class added in increasing t from +0.0f.  pd_f64 evaluates the same definition in
float64 (fractions from the float32 covers, no intermediate rounding) and also returns A[g][c] = sum over the class's trees and
the reached leaves of w * |val|, the scale of the rounding bound `bound`."""
import numpy as np

LEAF = 1 << 31
DEF_LEFT = 1 << 30
FID_MASK = (1 << 30) - 1
F32 = np.float32


def _go_right(x, val, def_left, missing, split):
    """predict's branch for the float32 values x at one node (split: None, or (words of the split, members_left))."""
    with np.errstate(invalid="ignore"):
        is_missing = np.abs(x - F32(missing)) <= F32(1e-6)
        if split is None:
            right = x >= F32(val)
        else:
            w, ml = split
            in_range = (x >= F32(0.0)) & (x < F32(32 * len(w)))
            c = np.where(in_range, x, 0.0).astype(np.int64)
            word = w[np.where(in_range, c // 32, 0)] if len(w) else np.zeros(c.size, np.uint32)
            member = in_range & (((word >> (c % 32).astype(np.uint32)) & 1) == 1)
            right = member != ml
    return np.where(is_missing, not def_left, right)


def _walk(nodes, root, covers, targets, grid, missing, splits, dt):
    """(acc [G], absacc [G]) of one tree in dtype dt; float32: the specified operation order."""
    G = grid.shape[0]
    val = nodes["val"]
    bits = np.ascontiguousarray(nodes["bits"]).view(np.uint32)
    left = nodes["left_idx"]
    col = {int(f): j for j, f in enumerate(targets)}
    acc = np.zeros(G, dt)
    absacc = np.zeros(G, np.float64)

    def visit(i, idx, w):
        g = root + i
        if bits[g] & LEAF:
            acc[idx] = acc[idx] + w * dt(val[g])  # the product is rounded before the add (two numpy operations)
            absacc[idx] += w.astype(np.float64) * abs(float(val[g]))
            return
        fid = int(bits[g] & FID_MASK)
        l = int(left[g])
        if fid in col:
            r = _go_right(grid[idx, col[fid]], val[g], bool(bits[g] & DEF_LEFT), missing, splits.get(g))
            if (~r).any():
                visit(l, idx[~r], w[~r])
            if r.any():
                visit(l + 1, idx[r], w[r])
            return
        cl, cr = covers[root + l], covers[root + l + 1]
        if dt is F32:
            tot = F32(cl) + F32(cr)
            fl, fr = F32(cl) / tot, F32(cr) / tot
        else:
            tot = float(cl) + float(cr)
            fl, fr = np.float64(float(cl) / tot), np.float64(float(cr) / tot)
        if fl != 0:
            visit(l, idx, w * fl)
        if fr != 0:
            visit(l + 1, idx, w * fr)

    if G:
        visit(0, np.arange(G), np.ones(G, dt))
    return acc, absacc


def _prepare(nodes, trees, covers, targets, grid, cats):
    targets = [int(f) for f in np.asarray(targets, dtype=np.int64).reshape(-1)]
    assert len(set(targets)) == len(targets)
    grid = np.ascontiguousarray(grid, dtype=np.float32).reshape(-1, len(targets)) if len(targets) else \
        np.zeros((int(np.asarray(grid).shape[0]), 0), np.float32)
    covers = np.ascontiguousarray(covers, dtype=np.float32)
    splits = {}
    if cats is not None:
        node, offset, words, ml = cats
        words = np.asarray(words, dtype=np.uint32)
        for k, i in enumerate(np.asarray(node, dtype=np.int64)):
            splits[int(i)] = (words[int(offset[k]):int(offset[k + 1])], bool(ml[k]) if ml is not None else False)
    return targets, grid, covers, splits


def pd_f32(nodes, trees, covers, targets, grid, missing, num_classes=1, cats=None):
    """[G, num_classes] float32: the bits tahoe_forest_predict_partial_dependence must give."""
    targets, grid, covers, splits = _prepare(nodes, trees, covers, targets, grid, cats)
    out = np.zeros((grid.shape[0], num_classes), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(len(trees)):
            acc, _ = _walk(nodes, int(trees[t]), covers, targets, grid, missing, splits, F32)
            out[:, t % num_classes] = out[:, t % num_classes] + acc
    return out


def pd_f64(nodes, trees, covers, targets, grid, missing, num_classes=1, cats=None):
    """(pd [G, num_classes] float64, A [G, num_classes] float64)."""
    targets, grid, covers, splits = _prepare(nodes, trees, covers, targets, grid, cats)
    out = np.zeros((grid.shape[0], num_classes), np.float64)
    A = np.zeros((grid.shape[0], num_classes), np.float64)
    for t in range(len(trees)):
        acc, absacc = _walk(nodes, int(trees[t]), covers, targets, grid, missing, splits, np.float64)
        out[:, t % num_classes] += acc
        A[:, t % num_classes] += absacc
    return out, A


def shape_of(nodes, trees):
    """(D, L): the deepest leaf in edges, and the most leaves of one tree."""
    bits = np.ascontiguousarray(nodes["bits"]).view(np.uint32)
    D = L = 0
    for t in range(len(trees)):
        root = int(trees[t])
        stack, leaves = [(0, 0)], 0
        while stack:
            i, d = stack.pop()
            if bits[root + i] & LEAF:
                leaves += 1
                D = max(D, d)
            else:
                l = int(nodes["left_idx"][root + i])
                stack += [(l, d + 1), (l + 1, d + 1)]
        L = max(L, leaves)
    return D, L


def bound(nodes, trees, A):
    """The rounding bound of the specified float32 arithmetic against the exact value: per leaf term at most 2 D roundings of
    fractions and weight products and one of w * val, at most L adds per tree and T adds of trees, and one rounding of a leaf
    value folded to float32: 2^-23 (2 D + L + T + 1) A."""
    D, L = shape_of(nodes, trees)
    return 2.0 ** -23 * (2 * D + L + len(trees) + 1) * A
