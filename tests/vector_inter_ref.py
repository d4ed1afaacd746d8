"""Helpers of the tests of SHAP interaction values on vector-leaf handles (tahoe_vector_forest_create_ex with TAHOE_CREATE_CONTRIBS
| TAHOE_CREATE_VECTOR_INTERACTIONS): test infrastructure, not product.

  shape        the rule of vector_inter_build restated: the form (LDS triangles or in place), the class block KB, the rows R of a
               tile and the bytes of dynamic LDS, from num_cols, K and TAHOE_VECTOR_SHAP_KB
  tri_index    where the slab form keeps the unordered pair {a, b}: the strict upper triangle, row-major
  STEPS        the num_cols on both sides of every step of the rule at K = 9, with the (KB, R) the rule gives there
  interactions the float64 conditioned TreeSHAP recursion run once per (leaf path, conditioning element) with a unit leaf and
               scaled by the K leaf values: what the kernel does, in float64 and without its ordered sums
  two_col_rounds  21 depth-2 trees on the same two columns: one pair that adds in 21 rounds per bin"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_shap_ref as ssr  # noqa: E402
import vector_edges as ve  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

LDS_BUDGET = 80 * 1024   # kVecInterLdsBudget
LDS_DEVICE = 160 * 1024  # the LDS of a CDNA4 compute unit
MAX_ROWS = 32            # kVecInterMaxRows: one bit per row in the one-fraction mask
WAVES = 4

# num_cols -> (slab form, KB, R) at K = 9 under the automatic rule: both sides of every step
STEPS = {1: (True, 8, 32), 2: (True, 8, 32), 18: (True, 8, 4), 19: (True, 8, 2), 25: (True, 8, 2), 26: (True, 8, 1),
         36: (True, 8, 1), 37: (True, 4, 1), 51: (True, 4, 1), 52: (True, 2, 1), 71: (True, 2, 1), 72: (False, 8, 1)}


def pairs(F):
    return F * (F - 1) // 2


def tri_index(a, b, F):
    """(a, b), a < b < F -> [0, F (F - 1) / 2)"""
    return a * (2 * F - a - 1) // 2 + (b - a - 1)


def slab_row_bytes(F, kb):
    return (F + 4 * kb * pairs(F)) * 4


def shape(F, K, forced=None, lds=LDS_DEVICE):
    """-> (slab form, KB, R, bytes of dynamic LDS) of a handle of num_cols = F and K outputs; forced = TAHOE_VECTOR_SHAP_KB"""
    inter_row = (F + 4 * F * F) * 4  # the sparse handle's test: the form enters the bits
    slabs = inter_row <= LDS_BUDGET and inter_row <= lds
    budget = min(LDS_BUDGET, lds)

    def fits(c):
        return not slabs or slab_row_bytes(F, c) <= budget

    if forced in (1, 2, 4, 8):
        kb = forced if fits(forced) else 1
    else:
        kb = next((c for c in (8, 4, 2) if c < 2 * K and fits(c)), 1)
    if not slabs:
        return False, kb, 1, WAVES * F * 4
    R = MAX_ROWS
    while R > 1 and R * slab_row_bytes(F, kb) > budget:
        R //= 2
    return True, kb, R, R * slab_row_bytes(F, kb)


def batches(F, K, top=33):
    """Row counts around the tile of the handle: 1, R - 1, R, R + 1 and 33 for slabs; 1, 3, 4, 5 around the 4 waves in place"""
    slabs, _, R, _ = shape(F, K)
    if not slabs:
        return [1, 3, 4, 5]
    return sorted({r for r in (1, R - 1, R, R + 1, top) if 1 <= r <= top})


# ---- float64 conditioned TreeSHAP, once per path ----
def _extend(pw, z, o):
    """Lundberg's EXTEND on the weights of a path of len(pw) elements (the root's included): float64 [len + 1, rows]"""
    l = len(pw)
    new = np.zeros((l + 1,) + pw.shape[1:])
    for i in range(l):
        new[i + 1] += o * pw[i] * ((i + 1) / (l + 1))
        new[i] += z * pw[i] * ((l - i) / (l + 1))
    return new


def _unwound_sum(pw, z, o):
    """The sum of the weights of the path without the element (z, o): o is 0.0 or 1.0 per row"""
    l = len(pw) - 1
    one, zero = np.zeros(pw.shape[1:]), np.zeros(pw.shape[1:])
    nxt = pw[l].copy()
    for i in range(l - 1, -1, -1):
        tmp = nxt * ((l + 1) / (i + 1))
        one += tmp
        nxt = pw[i] - tmp * (z * ((l - i) / (l + 1)))
        if z > 0.0:
            zero += pw[i] / (z * ((l - i) / (l + 1)))
    return np.where(o > 0.0, one, zero)  # (z == 0 and o == 0: the element's term is (o - z) x ... = 0 whatever the sum)


def interactions(forest, covers, x, missing=vr.MISSING):
    """Off-diagonal interaction values of every output: float64 [rows, K, cols, cols], RAW (AVG only divides), diagonal 0.  Per
    leaf path with elements e_1 .. e_m, per conditioning element k and every other element j: (o_j - z_j) (o_k - z_k) / 2 x the
    unwound sum of j on the path without k, into [f_j][f_k] -- the recursion runs once with a unit leaf, and the K leaf values
    scale it."""
    x = np.ascontiguousarray(x, np.float32)
    K, F = forest["k"], forest["cols"]
    rows = x.shape[0]
    out = np.zeros((K, F, F, rows))
    for per_tree in ve.leaf_paths(forest, covers):
        for vec, elems in per_tree:
            if len(elems) < 2:
                continue
            z = [e[1] for e in elems]
            o = []
            for fid, _, edges in elems:
                follow = np.ones(rows, bool)
                for thr, def_left, right in edges:
                    follow &= ssr._go_right(x[:, fid], thr, def_left, missing) == right
                o.append(follow.astype(np.float64))
            leaf = forest["leaves"][vec].astype(np.float64)
            for k in range(len(elems)):
                pw = np.ones((1, rows))
                for j in range(len(elems)):
                    if j != k:
                        pw = _extend(pw, z[j], o[j])
                for j in range(len(elems)):
                    if j == k:
                        continue
                    unit = _unwound_sum(pw, z[j], o[j]) * (o[j] - z[j]) * ((o[k] - z[k]) * 0.5)
                    out[:, elems[j][0], elems[k][0], :] += leaf[:, None] * unit[None]
    return np.ascontiguousarray(out.transpose(3, 0, 1, 2))


# ---- forests ----
def _two_col_rounds():
    """21 trees, each x0 at the root and x1 under both children: 84 three-lane paths, 21 to a bin, all on the pair {0, 1}"""
    rng = np.random.default_rng(7100)

    def split(fid, left, right):
        return (fid, float(rng.choice(vr.GRID)), bool(rng.integers(0, 2)), left, right)

    specs = []
    for _ in range(21):
        v = [int(i) for i in rng.integers(0, 13, 4)]
        specs.append(split(0, split(1, v[0], v[1]), split(1, v[2], v[3])))
    forest = vr.make(specs, vr.mixed_leaves(rng, 13, 3), 3, 2)
    covers = {"consistent": vsr.consistent_covers(forest, 7101), "unrelated": vsr.unrelated_covers(forest, 7102)}
    return dict(forest=forest, covers=covers, data=vr.make_data(ve.ROWS, 2, seed=7103), missing=vr.MISSING)


_cases = {}


def case(name):
    """vector_edges.case, and two_col_rounds; computed once and read-only"""
    if name != "two_col_rounds":
        return ve.case(name)
    if name not in _cases:
        c = _cases[name] = _two_col_rounds()
        for a in (c["forest"]["nodes"], c["forest"]["trees"], c["forest"]["leaves"], c["data"], *c["covers"].values()):
            a.setflags(write=False)
    return _cases[name]
