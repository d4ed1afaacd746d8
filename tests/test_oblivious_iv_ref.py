"""tests/oblivious_iv_ref.py against the definition and against the project's dense interventional reference; no GPU.

Bound.  Two float64 evaluations of one value differ by rounding only: 1e-12 (sum |phi| + 1) per (row, output) is some 10^3 float64
roundings of the largest magnitudes involved."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interventional_ref as ivr  # noqa: E402
import oblivious_iv_ref as oiv  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402

# (depths, columns, K, background rows, AVG, global bias): depth 0 trees, features that repeat within a tree (5 columns under
# depth 6), K > 1
CASES = {
    "mixed_k3": ([0, 1, 2, 6, 3, 6, 4], 5, 3, 7, False, 0.0),
    "mixed_k1_avg": ([3, 0, 5, 1, 0, 4], 6, 1, 40, True, 0.25),
    "deep_k2_avg": ([6, 6, 2, 5], 8, 2, 19, True, -0.5),
}
_cache = {}


def case(name):
    if name not in _cache:
        depths, cols, k, B, avg, gb = CASES[name]
        forest = obr.make_forest(depths, cols, k, seed=11)
        data = obr.make_data(9, cols, seed=4)
        bg = obr.make_data(B, cols, seed=5)
        got = oiv.paths(forest, data, bg, avg=avg, global_bias=gb)
        for a in (data, bg) + got:
            a.setflags(write=False)
        _cache[name] = (forest, data, bg, avg, gb, got)
    return _cache[name]


def close(got, want):
    tol = 1e-12 * (np.abs(want).sum(axis=-1, keepdims=True) + 1.0)
    return bool(np.all(np.abs(got - want) <= tol)), float(np.abs(got - want).max())


@pytest.mark.parametrize("name", list(CASES))
def test_paths_equals_the_shapley_values_from_their_definition(name):
    forest, data, bg, avg, gb, (got, A, N) = case(name)
    want = oiv.brute(forest, data, bg, avg=avg, global_bias=gb)
    ok, worst = close(got, want)
    assert ok, worst
    F = forest["cols"]
    assert np.abs(got[:, :, :F]).max() > 1.0 and N.max() > 0
    assert np.all(np.abs(got[:, :, :F]) <= A[:, :, :F] * (1 + 1e-12))


def test_the_cases_carry_every_kind_of_value_the_branch_rule_tells_apart():
    for which in (1, 2):  # the rows, the background
        v = np.concatenate([case(name)[which].ravel() for name in CASES])
        assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() and (v == np.float32(obr.MISSING)).any()
        assert (v == np.nextafter(np.float32(obr.MISSING), np.float32(0))).any()  # the sentinel's neighbour: not missing
        assert np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()


@pytest.mark.parametrize("name", list(CASES))
def test_paths_and_brute_equal_the_dense_reference_on_the_heap_expansion(name, built):
    forest, data, bg, avg, gb, (got, A, N) = case(name)
    ones = np.ones(int((1 << np.asarray(forest["depths"], np.int64)).sum()), np.float32)
    T, F = len(forest["depths"]), forest["cols"]
    want = np.empty_like(got)
    for k in range(forest["k"]):
        nodes, D = osr.expand_with_covers(forest, ones, k)
        want[:, k] = ivr.paths(nodes, T, D, F, data, bg, obr.MISSING, 1, avg, gb)[0][:, 0]
    ok, worst = close(got, want)
    assert ok, worst
    ok, worst = close(oiv.brute(forest, data, bg, avg=avg, global_bias=gb), want)
    assert ok, worst
    assert np.array_equal(got[:, :, F].astype(np.float32).view(np.uint32), want[:, :, F].astype(np.float32).view(np.uint32))


def test_the_histogram_is_smaller_than_the_background_and_counts_every_row():
    forest, data, bg, *_ = case("mixed_k1_avg")
    occ = oiv.occupancy(forest, bg)
    assert all(int(c.sum()) == bg.shape[0] and np.all(np.diff(l) > 0) for l, c in occ)
    assert sum(l.size for l, _ in occ) < bg.shape[0] * len(occ) and max(int(c.max()) for _, c in occ) > 1


def test_a_row_against_itself_has_no_players():
    forest, data, *_ = case("mixed_k3")
    phi, A, N = oiv.paths(forest, data[:1], data[:1])
    F = forest["cols"]
    assert not phi[:, :, :F].any() and not N.any()
