"""Saabas contributions (TAHOE_CREATE_APPROX_CONTRIBS, tahoe_forest_predict_contribs_approx) without a GPU: the symbol and the flag,
the cover checks of the three create calls (they run before a device is touched), the NULL-handle refusal, and the numpy
reference of tests/approx_contribs_ref.py against contribs_ref's bias column, the oracle's margins and a direct float64 sum."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_contribs_ref as ref  # noqa: E402
import contribs_ref  # noqa: E402

INVALID_ARG, NO_DEVICE, INVALID_FOREST, UNSUPPORTED = 1, 4, 6, 7
APPROX, CONTRIBS = 0x10, 0x4
MISSING = -999.0
LEAF = -(1 << 31)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ta():
    lib = os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tahoe_amd", "csrc"), "-s", "-j4"], check=True)
    sys.path.insert(0, ROOT)
    import tahoe_amd

    return tahoe_amd


def _create(ta, nodes, T, D, cols, num_classes=1, flags=APPROX):
    params = ta.ForestParams(0, D, T, cols, 0, 0, 0.0, 0.0, 0, MISSING)
    h = C.c_void_p()
    if num_classes == 1:
        st = ta.lib.tahoe_forest_create_ex(C.byref(h), nodes.ctypes.data, C.byref(params), flags)
    else:
        st = ta.lib.tahoe_forest_create_multiclass(C.byref(h), nodes.ctypes.data, C.byref(params), num_classes, flags)
    if st != 0:
        assert not h.value
    else:
        ta.lib.tahoe_forest_destroy(h)
    return st


def _create_sparse(ta, sn, tr, cols, covers, num_classes=1, flags=APPROX):
    params = ta.ForestParams(int(sn.size), 0, int(tr.size), cols, 0, 0, 0.0, 0.0, 0, MISSING)
    h = C.c_void_p()
    cv = None if covers is None else np.ascontiguousarray(covers, dtype=np.float32)
    st = ta.lib.tahoe_sparse_forest_create_ex(C.byref(h), tr.ctypes.data, sn.ctypes.data, cv.ctypes.data if cv is not None else None,
                                              C.byref(params), num_classes, flags)
    if st != 0:
        assert not h.value
    else:
        ta.lib.tahoe_forest_destroy(h)
    return st


def vine(ta, depth, F):
    """One sparse tree `depth` inner nodes deep on features 0, 1, ..., depth - 1 (mod F): node 2k splits, 2k + 1 is a leaf."""
    sn = np.zeros(2 * depth + 1, dtype=ta.capi.SPARSE_NODE_DTYPE)
    for k in range(depth):
        sn[2 * k] = (np.float32(0.25 * (k % 5) - 0.5), k % F, 2 * k + 1)
        sn[2 * k + 1] = (np.float32(k), LEAF, 0)
    sn[-1] = (-1.0, LEAF, 0)
    return sn, np.zeros(1, np.int32)


def test_symbol_is_exported_and_bound(ta):
    assert ta.CREATE_APPROX_CONTRIBS == 0x10 and ta.capi.CREATE_APPROX_CONTRIBS == 0x10
    assert "tahoe_forest_predict_contribs_approx" in ta.capi.EXPORTED_SYMBOLS
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "tahoe_amd", "libtahoe_amd.so")],
                          capture_output=True, text=True).stdout
    assert " tahoe_forest_predict_contribs_approx" in syms
    assert ta.lib.tahoe_abi_version() == 2


def test_predict_on_null_handle(ta):
    assert ta.lib.tahoe_forest_predict_contribs_approx(None, None, None, 0, None) == INVALID_ARG
    assert ta.lib.tahoe_forest_predict_contribs_approx(None, None, None, 10, None) == INVALID_ARG


@pytest.mark.parametrize("flags", [APPROX, APPROX | CONTRIBS, APPROX | 0x1, APPROX | CONTRIBS | 0x1])
@pytest.mark.parametrize("num_classes", [1, 2])
def test_dense_creates_accept_the_flag(ta, flags, num_classes):
    nodes = ta.synth_forest(4, 3, 5, seed=3)
    nodes["weight"] = 1.0
    assert _create(ta, nodes, 4, 3, 5, num_classes, flags) not in (INVALID_ARG, INVALID_FOREST)


@pytest.mark.parametrize("flags", [APPROX, APPROX | CONTRIBS])
def test_sparse_create_accepts_the_flag(ta, flags):
    sn, tr = ta.capi.synth_sparse_forest(6, 8, 2, 6, 0.3, 200, 5)
    assert _create_sparse(ta, sn, tr, 8, np.ones(sn.size, np.float32), 1, flags) not in (INVALID_ARG, INVALID_FOREST)
    assert _create_sparse(ta, sn, tr, 8, np.ones(sn.size, np.float32), 2, flags) not in (INVALID_ARG, INVALID_FOREST)


@pytest.mark.parametrize("flags", [APPROX | 0x1, APPROX | 0x2, APPROX | 0x8])
def test_sparse_create_still_refuses_other_bits(ta, flags):
    sn, tr = ta.capi.synth_sparse_forest(6, 8, 2, 6, 0.3, 200, 5)
    assert _create_sparse(ta, sn, tr, 8, np.ones(sn.size, np.float32), 1, flags) == INVALID_ARG


def test_sparse_null_covers_are_refused(ta):
    sn, tr = ta.capi.synth_sparse_forest(6, 8, 2, 6, 0.3, 200, 5)
    assert _create_sparse(ta, sn, tr, 8, None, 1, APPROX) == INVALID_ARG
    assert "covers" in ta.lib.tahoe_last_error().decode()


@pytest.mark.parametrize("bad", [0.0, -0.5, float("nan"), float("inf")])
@pytest.mark.parametrize("num_classes", [1, 2])
def test_bad_dense_covers_are_refused(ta, bad, num_classes):
    T, D, cols = 4, 3, 5
    nodes = ta.synth_forest(T, D, cols, seed=3)
    per = ta.capi.tree_num_nodes(D)
    nodes["weight"] = 1.0
    if bad == 0.0:
        nodes["weight"][2 * per + 3] = 0.0
        nodes["weight"][2 * per + 4] = 0.0
    else:
        nodes["weight"][2 * per + 4] = bad
    assert _create(ta, nodes, T, D, cols, num_classes, APPROX) == INVALID_FOREST
    msg = ta.lib.tahoe_last_error().decode()
    assert "tree 2 node 1" in msg, msg
    # the same refusal and message as TAHOE_CREATE_CONTRIBS
    assert _create(ta, nodes, T, D, cols, num_classes, CONTRIBS) == INVALID_FOREST
    assert ta.lib.tahoe_last_error().decode() == msg


def test_bad_sparse_covers_are_refused(ta):
    sn, tr = vine(ta, 3, 3)
    covers = np.ones(sn.size, np.float32)
    covers[3], covers[4] = 0.0, 0.0  # the children of inner node 2
    assert _create_sparse(ta, sn, tr, 3, covers, 1, APPROX) == INVALID_FOREST
    msg = ta.lib.tahoe_last_error().decode()
    assert "tree 0 node 2" in msg, msg
    assert _create_sparse(ta, sn, tr, 3, covers, 1, CONTRIBS) == INVALID_FOREST
    assert ta.lib.tahoe_last_error().decode() == msg


def test_deep_sparse_paths_need_only_the_exact_flag_limit(ta):
    sn, tr = vine(ta, 40, 40)  # 40 distinct features on one path: beyond TAHOE_CREATE_CONTRIBS's 31
    covers = np.ones(sn.size, np.float32)
    assert _create_sparse(ta, sn, tr, 40, covers, 1, APPROX) not in (INVALID_ARG, INVALID_FOREST, UNSUPPORTED)
    assert _create_sparse(ta, sn, tr, 40, covers, 1, APPROX | CONTRIBS) == UNSUPPORTED


def test_python_forest_raises_on_bad_covers(ta):
    nodes = ta.synth_forest(3, 2, 4, seed=5)
    nodes["weight"] = -1.0
    with pytest.raises(ta.TahoeError) as e:
        ta.Forest(nodes, 3, 2, 4, approx_contribs=True)
    assert e.value.status == INVALID_FOREST
    sn, tr = vine(ta, 3, 3)
    with pytest.raises(ta.TahoeError) as e:
        ta.capi.SparseForest(sn, tr, 3, covers=np.full(sn.size, -1.0, np.float32), approx_contribs=True)
    assert e.value.status == INVALID_FOREST


# ---- the reference ----
def random_forest(ta, rng, T, D, cols, nan_thr=0.05):
    """synth_forest with random covers, early leaves, a root-leaf tree and some NaN thresholds."""
    nodes = ta.synth_forest(T, D, cols, seed=int(rng.integers(1 << 30)), leaf_prob=0.15)
    nodes["weight"] = rng.uniform(0.05, 1.0, nodes.size).astype(np.float32)
    internal = (nodes["bits"].view(np.uint32) >> 31) == 0
    nodes["val"][internal & (rng.random(nodes.size) < nan_thr)] = np.nan
    nodes["bits"][0] = nodes["bits"][0] | np.int32(LEAF)  # tree 0 is a single leaf
    return nodes


def random_rows(ta, rng, rows, cols):
    return ta.synth_data(rows, cols, seed=int(rng.integers(1 << 30)), missing_prob=0.1, missing=MISSING, nan_prob=0.05)


@pytest.mark.parametrize("C_, avg, bias", [(1, False, 0.0), (1, True, 0.5), (3, True, -0.25)])
def test_reference_bias_is_contribs_ref_bias(ta, C_, avg, bias):
    rng = np.random.default_rng(1)
    T, D, cols = 6, 4, 5
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 8, cols)
    phi = ref.dense(nodes, T, D, cols, x, MISSING, num_classes=C_, avg=avg, global_bias=bias)
    want = contribs_ref.bias_f32(nodes, T, D, C_, avg, bias)
    assert np.array_equal(phi[:, :, cols].view(np.uint32), np.broadcast_to(want, (8, C_)).view(np.uint32))


@pytest.mark.parametrize("seed", range(4))
def test_reference_additivity_against_oracle(ta, seed):
    from oracle import oracle

    rng = np.random.default_rng(20 + seed)
    T, D, cols = 12, int(rng.integers(1, 7)), int(rng.integers(2, 6))
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 64, cols)
    margin = oracle.predict(nodes, T, D, x, MISSING)[0].astype(np.float64)  # float32 sums in tree order
    phi, S, N = ref.dense(nodes, T, D, cols, x, MISSING, scale=True)
    got = phi[:, 0, :].astype(np.float64).sum(axis=1)
    leaf_abs = oracle.abs_leaf_sum(nodes, T, D, x, MISSING)
    # float32: a rounded delta and a rounded add per step, the margin's own sum, the bias rounding, the final float64 sum of F + 1
    tol = (2 * N[:, 0] + 4) * U * (S[:, 0] + np.abs(phi[:, 0, cols])) + (T + 2) * U * leaf_abs + 1e-300
    assert np.all(np.abs(got - margin) <= tol), np.max(np.abs(got - margin) / tol)


@pytest.mark.parametrize("seed", range(4))
def test_reference_matches_a_direct_float64_sum(ta, seed):
    rng = np.random.default_rng(40 + seed)
    T, D, cols = 6, int(rng.integers(1, 5)), int(rng.integers(2, 6))
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 30, cols)
    for C_, avg, bias in ((1, False, 0.0), (3, True, 0.125)):
        phi, S, N = ref.dense(nodes, T, D, cols, x, MISSING, num_classes=C_, avg=avg, global_bias=bias, scale=True)
        want = ref.direct64(nodes, T, D, cols, x, MISSING, num_classes=C_, avg=avg, global_bias=bias)
        tol = (2 * N + 2)[:, :, None] * U * (S[:, :, None] + np.abs(want)) + 1e-300
        assert np.all(np.abs(phi.astype(np.float64) - want) <= tol)


def test_reference_sparse_conversion_gives_the_dense_bits(ta):
    rng = np.random.default_rng(7)
    T, D, cols = 8, 5, 4
    nodes = random_forest(ta, rng, T, D, cols)
    x = random_rows(ta, rng, 50, cols)
    sn, tr, cv = ta.capi.dense_to_sparse(nodes, T, D, covers=True)
    for C_, avg, bias in ((1, False, 0.0), (2, True, 0.75)):
        a = ref.dense(nodes, T, D, cols, x, MISSING, num_classes=C_, avg=avg, global_bias=bias)
        b = ref.sparse(sn, tr, cv, cols, x, MISSING, num_classes=C_, avg=avg, global_bias=bias)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
