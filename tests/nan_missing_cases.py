"""Forests, batches and CPU references of tests/test_nan_missing_gpu.py (TAHOE_CREATE_NAN_MISSING).  Test
infrastructure, not product; nothing here needs a GPU.

The reference for a handle created with the flag: for a batch x and a sentinel S whose band no value of x enters, the handle on x
must give the float32 bits of the existing CPU references (oracle.predict, oracle.sparse_predict, categorical_ref.predict) on
sub(x, S) -- x with every NaN replaced by S -- under missing = S.  not_vacuous() is the check every user makes on the CPU: that
reference differs from the one on x as it is (where a NaN goes left), in rows that hold a NaN and nowhere else."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref  # noqa: E402

S = -999.0  # the sentinel of every batch here; synth_data's values and the hand-made ones lie in [-1, 1)
NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)  # quiet, negative quiet, signalling, every bit set


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def sub(x, s=S):
    """x with every NaN replaced by s"""
    return np.where(np.isnan(x), np.float32(s), x).astype(np.float32)


def nan_rows(x):
    return np.isnan(x).any(axis=1)


def not_vacuous(want, left, x, what=""):
    """want: the reference on sub(x), left: the reference on x (NaN goes left).  They differ, and only in rows holding a NaN."""
    w, l = bits(want).reshape(len(x), -1), bits(left).reshape(len(x), -1)
    differ = (w != l).any(axis=1)
    assert differ.any(), f"{what}: treating NaN as missing changes no output bit -- the test shows nothing"
    assert not (differ & ~nan_rows(x)).any(), f"{what}: a row without a NaN depends on the rule"
    return differ


def first_row_differs(x, *refs):
    """Swaps row 0 of x and of every reference with the first row in which refs[0] and refs[1] differ, so that a batch of
    one row is not vacuous either (rows are independent: the references of the swapped batch are the swapped references)"""
    differ = not_vacuous(refs[0], refs[1], x)
    i = int(np.flatnonzero(differ)[0])
    for a in (x,) + refs:
        a[[0, i]] = a[[i, 0]]


def with_nan_patterns(x, seed=0):
    """The NaNs of x rewritten with the four bit patterns in turn (any NaN counts: quiet, signalling, either sign, any payload)"""
    u = x.view(np.uint32).copy()
    at = np.flatnonzero(np.isnan(x).reshape(-1))
    u.reshape(-1)[at] = np.array(NAN_BITS, np.uint32)[np.arange(at.size) % 4]
    out = u.view(np.float32)
    assert np.array_equal(np.isnan(out), np.isnan(x))
    return out


# ------------------------------------------------------------------------------------------------------------ forests
def hand_forest(ta, T, D, cols, seed, root_col=None, def_left="mixed", thr=(-0.5, 0.5)):
    """T perfect trees of depth D (test_missing_flag_of_the_right_quantise_chunk's construction): tree t's root splits on column
    root_col, or on t % cols, every other inner node on a random column.  def_left is one value per tree.  Both values are needed:
    in a def_left = 0 tree a missing value goes right where a NaN as a number goes left, which is what makes a test not vacuous;
    in a def_left = 1 tree a missing value goes left where the missing CODE read as a number -- the largest -- goes right, which
    is what shows a walk that took a "no missing value on this tile" form.  "mixed": trees t and t + cols, which share their
    root's column, get 0 and 1 (with root_col given: even and odd trees)."""
    rng = np.random.default_rng(seed)
    per = 2 ** (D + 1) - 1
    fid = np.concatenate([np.array([root_col if root_col is not None else t % cols] + list(rng.integers(0, cols, 2 ** D - 2)) + [0] * 2 ** D)
                          for t in range(T)])
    is_leaf = np.tile(np.arange(per) >= 2 ** D - 1, T)
    val = np.where(is_leaf, rng.uniform(-1, 1, T * per), rng.uniform(thr[0], thr[1], T * per)).astype(np.float32)
    if isinstance(def_left, str):
        assert def_left == "mixed"
        per_tree = np.arange(T) % 2 if root_col is not None else (np.arange(T) // cols) % 2
    else:
        per_tree = np.full(T, def_left)
    return ta.capi.encode_nodes(fid, val, np.repeat(per_tree, per), np.ones(T * per), is_leaf)


def dense_refs(oracle, nodes, T, D, x, C=1, missing=S, leaf=False, threads=8):
    """(margins of sub(x) [rows] or [rows, C], margins of x as it is) -- with leaf=True also the leaves of sub(x) [rows, T]"""
    per = nodes.size // T
    by_tree = nodes.reshape(T, per)

    def margins(data):
        if C == 1:
            return oracle.predict(nodes, T, D, data, missing, threads=threads)[0]
        return np.stack([oracle.predict(np.ascontiguousarray(by_tree[c::C]).reshape(-1), T // C, D, data, missing, threads=threads)[0]
                         for c in range(C)], axis=1)

    xs = sub(x, missing)
    out = (margins(xs), margins(x))
    if leaf:
        out += (oracle.predict(nodes, T, D, xs, missing, want_leaf=True, threads=threads)[1],)
    return out


def sparse_refs(oracle, sn, tr, x, C=1, missing=S, leaf=False, threads=8):
    def margins(data):
        if C == 1:
            return oracle.sparse_predict(sn, tr, data, missing, threads=threads)[0]
        return np.stack([oracle.sparse_predict(sn, np.ascontiguousarray(tr[c::C]), data, missing, threads=threads)[0] for c in range(C)],
                        axis=1)

    xs = sub(x, missing)
    out = (margins(xs), margins(x))
    if leaf:
        out += (oracle.sparse_predict(sn, tr, xs, missing, want_leaf=True, threads=threads)[1],)
    return out


def cat_forest(ta, T=60, cols=32, feats=(1, 5, 9, 17, 30), seed=11):
    """test_columns_gpu.py's categorical handle: the inner nodes on `feats` become category sets, a third with members_left"""
    sn, tr = ta.capi.synth_sparse_forest(T, cols, 4, 16, 0.32, 65535, seed)
    rng = np.random.default_rng(seed)
    b = sn["bits"].view(np.uint32)
    inner = np.flatnonzero((b >> 31) == 0)
    chosen = inner[np.isin(b[inner] & ((1 << 30) - 1), feats)]
    cats = {int(i): rng.choice(300, size=int(rng.integers(1, 200)), replace=False) for i in chosen}
    ml = {int(i) for i in chosen if rng.random() < 1 / 3}
    _, packed = ta.capi.pack_categorical(cats, ml)
    return dict(sn=sn, tr=tr, cols=cols, feats=feats, cats=cats, ml=ml, packed=packed)


def cat_batch(ta, cf, rows, seed):
    """categories, non-integers, -0.0 and NaN in the categorical columns; NaN at 1 % beside the sentinel at 3 % elsewhere"""
    rng = np.random.default_rng(seed)
    x = ta.synth_data(rows, cf["cols"], seed=seed, missing_prob=0.03, missing=S, nan_prob=0.01)
    for c in cf["feats"]:
        v = rng.integers(0, 320, rows).astype(np.float32)
        v[rng.random(rows) < 0.1] += np.float32(0.5)
        v[rng.random(rows) < 0.05] = np.float32(-0.0)
        v[rng.random(rows) < 0.05] = np.float32(np.nan)
        x[:, c] = np.where(x[:, c] == np.float32(S), x[:, c], v)
    return x


def cat_refs(cf, x, missing=S, leaf=False, trees=None, init=None):
    node, offset, words, mla = cf["packed"]
    tr = cf["tr"] if trees is None else trees

    def run(data):
        return categorical_ref.predict(cf["sn"], tr, data, missing, node, offset, words, mla, init=init)

    want, want_leaf = run(sub(x, missing))
    out = (np.ascontiguousarray(want, np.float32), np.ascontiguousarray(run(x)[0], np.float32))
    return out + (want_leaf,) if leaf else out


# --------------------------------------------------------------------------------------------------------- the definition
def definition_batch(m, cols, rows=200, seed=3):
    """Values in [-1, 1) with, scattered over every column: +-0, +-inf, subnormals, the values around both edges of the band of
    a finite sentinel m, the sentinel itself, and NaNs of the four bit patterns."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (rows, cols)).astype(np.float32)
    special = [0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, 5e-7, -5e-7, 2e-6, -2e-6]
    if np.isfinite(m):
        m32 = np.float32(m)
        for e in (np.float32(1e-6), np.float32(-1e-6)):
            edge = np.float32(m32 + e)
            special += [edge, np.nextafter(edge, np.float32(np.inf)), np.nextafter(edge, np.float32(-np.inf))]
        special += [m32]
    special = np.array(special, np.float32)
    at = rng.random(x.shape)
    x[at < 0.10] = special[rng.integers(0, special.size, int((at < 0.10).sum()))]
    x[(at >= 0.10) & (at < 0.15)] = np.nan
    return with_nan_patterns(x, seed)


def definition_refs(oracle, nodes, T, D, x, m):
    """(reference of the flagged handle under params.missing = m, reference of a handle without the flag).  A finite m is its own
    substitute: NaN -> m under missing = m is the definition.  For m = NaN or +-inf the band never matches, so the NaNs go to a
    finite S2 that no value enters, under missing = S2, and the infinities stay in place."""
    s2 = np.float32(m) if np.isfinite(m) else np.float32(-777.0)
    assert np.isfinite(m) or not (np.abs(x[np.isfinite(x)] - s2) <= 1.0).any()
    want = oracle.predict(nodes, T, D, sub(x, s2), float(s2), threads=4)[0]
    flagless = oracle.predict(nodes, T, D, x, float(m), threads=4)[0]
    return want, flagless
