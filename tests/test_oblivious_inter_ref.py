"""tests/oblivious_inter_ref.py against the definition, against the project's other references and against itself; no GPU.

Bounds.  Two float64 evaluations of one entry differ by rounding only: 1e-12 (sum |M| + 1) per (row, class) is some 10^3 float64
roundings of the largest magnitudes involved.  emulate against poly takes the bar of tests/test_oblivious_inter_gpu.py, since it
states the GPU's bits: |emulate - poly| <= (N + 6 (D + 2)) 2^-24 A per off-diagonal entry.  A row of emulate sums to phi_i up to
the rounding of S_i (at most F - 1 float32 adds of the row's off-diagonals) and of the one subtraction: (F + 1) 2^-24 sum_j |M_ij|."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interactions_ref  # noqa: E402
import oblivious_inter_ref as oir  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402

MIXED = [0, 1, 2, 6, 3, 6, 4]  # depths; on 5 columns the features repeat within a tree
KINDS = ["int", "half", "most", "zero"]
U = 2.0 ** -24
_cache = {}


def case(kind, k=3, avg=False, bias=0.0):
    key = (kind, k, avg, bias)
    if key not in _cache:
        forest = obr.make_forest(MIXED, 5, k, seed=11)
        covers = osr.make_covers(forest, kind, seed=3)
        data = obr.make_data(9, 5, seed=4)
        poly = oir.poly(forest, covers, data, avg=avg, global_bias=bias)
        for a in (covers, data) + poly:
            a.setflags(write=False)
        _cache[key] = (forest, covers, data, poly)
    return _cache[key]


@pytest.mark.parametrize("kind", KINDS)
def test_poly_equals_the_interaction_index_from_its_definition(kind):
    forest, covers, data, (got, A, N) = case(kind)
    assert kind == "int" or (covers == 0).any()
    want = oir.brute(forest, covers, data)
    tol = 1e-12 * (np.abs(want).sum(axis=(-1, -2), keepdims=True) + 1.0)
    assert np.all(np.abs(got - want) <= tol), np.abs(got - want).max()
    assert np.array_equal(got, got.swapaxes(-1, -2)) and N.max() > 0 and np.abs(got).max() > 1.0


def test_poly_equals_the_definition_on_two_trees_of_distinct_features_with_avg():
    forest = obr.make_forest([6, 5], 8, 1, seed=5)
    forest["fids"][:] = [0, 1, 2, 3, 4, 5, 7, 6, 5, 4, 3]
    covers = osr.make_covers(forest, "half", seed=3)
    data = obr.make_data(7, 8, seed=4)
    want = oir.brute(forest, covers, data, avg=True, global_bias=0.25)
    got, _, _ = oir.poly(forest, covers, data, avg=True, global_bias=0.25)
    assert np.all(np.abs(got - want) <= 1e-12 * (np.abs(want).sum(axis=(-1, -2), keepdims=True) + 1.0))


@pytest.mark.parametrize("k", [1, 3])
def test_poly_equals_the_dense_reference_on_the_expansion(k):
    forest, covers, data, (got, A, N) = case("int", k=k, avg=True, bias=-0.5)
    T = len(forest["depths"])
    per_class = [oir.expand(forest, covers, c) for c in range(k)]
    nodes = np.stack([n.reshape(T, -1) for n, _ in per_class], axis=1).reshape(-1)
    want, _, _ = interactions_ref.poly(nodes, T * k, per_class[0][1], forest["cols"], data, obr.MISSING, num_classes=k, avg=True,
                                       global_bias=-0.5)
    tol = 1e-12 * (np.abs(want).sum(axis=(-1, -2), keepdims=True) + 1.0)
    assert np.all(np.abs(got - want) <= tol), np.abs(got - want).max()
    assert np.array_equal(got[:, :, -1, -1].astype(np.float32).view(np.uint32), want[:, :, -1, -1].astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
def test_emulate_is_within_the_gpu_bound_symmetric_and_its_rows_sum_to_phi(kind):
    forest, covers, data, (want, A, N) = case(kind, avg=(kind == "half"), bias=0.125)
    got = oir.emulate(forest, covers, data, avg=(kind == "half"), global_bias=0.125)
    assert got.dtype == np.float32 and got.shape == want.shape
    F, D = forest["cols"], max(MIXED)
    off = ~np.eye(F + 1, dtype=bool)
    err, bound = np.abs(got.astype(np.float64) - want), (N + 6 * (D + 2)) * U * A
    assert np.all(err[..., off] <= bound[..., off]), (err[..., off] / np.where(bound > 0, bound, 1.0)[..., off]).max()
    assert np.array_equal(got.view(np.uint32), got.swapaxes(-1, -2).copy().view(np.uint32))
    phi = osr.emulate(forest, covers, data, avg=(kind == "half"), global_bias=0.125)
    g64 = got.astype(np.float64)
    assert np.all(np.abs(g64[:, :, :F, :F].sum(axis=-1) - phi[:, :, :F]) <= (F + 1) * U * np.abs(g64[:, :, :F, :F]).sum(axis=-1))
    assert np.array_equal(got[:, :, F, F].view(np.uint32), phi[:, :, F].view(np.uint32))
    assert not got[:, :, F, :F].view(np.uint32).any() and not got[:, :, :F, F].view(np.uint32).any()


def test_a_dead_leaf_of_infinite_value_makes_no_nan():
    forest = obr.make_forest([3], 3, 1, seed=2)
    forest["fids"][:] = [0, 1, 2]
    forest["thr"][:] = 0.0
    covers = np.array([3, 1, 2, 2, 0, 5, 1, 4], np.float32)  # leaf 4 is empty: z = 0 for level 2's feature on its path
    forest["leaves"] = np.asarray(forest["leaves"], np.float32).copy()
    forest["leaves"][4] = np.inf
    data = np.array([[-9.0, -9.0, -9.0]], np.float32)  # leaf 0: it leaves leaf 4's path at that feature
    off = ~np.eye(4, dtype=bool)
    off[3, :] = off[:, 3] = False  # (the bias is the mean over every leaf and is not finite; oblivious_shap_ref.poly multiplies)
    with np.errstate(invalid="ignore"):
        got, want = oir.emulate(forest, covers, data), oir.poly(forest, covers, data)[0]
        assert np.isfinite(got[:, :, :3, :3]).all() and np.isfinite(want[..., off]).all() and np.abs(got[..., off]).max() > 0
        # (leaf 7 does weigh leaf 4: level 2's feature agrees)
        assert not np.isfinite(oir.emulate(forest, covers, -data)[..., off]).all()
