"""tests/oblivious_ref.py without a GPU: the numpy rule of tahoe_oblivious_forest_create against the CPU oracle run on the heap
expansion of the same forest -- equal bits in the sums and, through the bit reversal, equal leaf indices -- and the identity
behind strict_borders."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oblivious_ref as obr  # noqa: E402


@pytest.fixture(scope="module")
def env(built):
    import tahoe_amd as ta
    from oracle import oracle

    return ta, oracle


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("depths,cols,k", [([0, 1, 2, 6, 2, 0, 6, 1, 6], 5, 1), ([6, 2, 1, 0, 6], 3, 3), ([0, 0, 0], 1, 2),
                                          ([6] * 7, 40, 1), ([1], 1, 1)])
def test_reference_equals_the_oracle_on_the_expansion(env, depths, cols, k):
    _, oracle = env
    forest = obr.make_forest(depths, cols, k, seed=11 + cols)
    data = obr.make_data(130, cols, seed=5)
    assert np.isnan(data).any() and np.isinf(data).any() and (data == obr.MISSING).any()
    sums, leaf = obr.ref_of(forest, data)
    for c in range(k):
        nodes, D = obr.dense_of(forest, c)
        want, heap_leaf = oracle.predict(nodes, len(depths), D, data, obr.MISSING, want_leaf=True)
        assert same_bits(sums[:, c], want), c
        assert np.array_equal(obr.heap_leaf_to_oblivious(heap_leaf, depths), leaf)
    if max(depths) > 0:
        assert len(np.unique(leaf)) > 1


def test_reference_known_answer():
    # one tree of depth 2: level 0 on x0 >= 0.5 (default left), level 1 on x1 >= 0.0 (default right); leaves 1, 2, 4, 8
    m = obr.MISSING
    data = np.array([[0.5, -0.0], [0.25, 0.0], [np.nan, np.nan], [m, m], [np.inf, -np.inf]], np.float32)
    sums, leaf = obr.oblivious_ref([2], [0, 1], [0.5, 0.0], [1, 0], [1.0, 2.0, 4.0, 8.0], 1, data, m)
    assert leaf[:, 0].tolist() == [3, 2, 0, 2, 1]
    assert sums[:, 0].tolist() == [8.0, 4.0, 1.0, 4.0, 2.0]
    init = np.full(5, 0.5, np.float32)
    acc, _ = obr.oblivious_ref([2], [0, 1], [0.5, 0.0], [1, 0], [1.0, 2.0, 4.0, 8.0], 1, data, m, init=init)
    assert acc[:, 0].tolist() == [8.5, 4.5, 1.5, 4.5, 2.5]


def test_strict_borders_identity(env):
    ta, _ = env
    fmax, tiny = np.float32(3.4028235e38), np.float32(1e-45)
    grid = np.array([-np.inf, -fmax, -2.0, -1.0000001, -1.0, -1.17549435e-38, -tiny, -0.0, 0.0, tiny, 5e-45, 1.17549435e-38,
                     0.99999994, 1.0, 1.0000001, 2.0, fmax, np.inf], np.float32)
    borders = grid[np.isfinite(grid)]
    thr = ta.strict_borders(borders)
    assert thr.dtype == np.float32 and thr[borders == fmax] == np.inf
    assert thr[np.flatnonzero(borders == 0.0)].tolist() == [float(tiny)] * 2  # +-0.0 -> the smallest subnormal
    x = grid[:, None]
    assert np.array_equal(x > borders[None, :], x >= thr[None, :])
    with np.errstate(invalid="ignore"):  # NaN: left under both rules
        assert not (np.float32(np.nan) > borders).any() and not (np.float32(np.nan) >= thr).any()
