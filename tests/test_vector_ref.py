"""tests/vector_ref.py without a GPU: the numpy rule of tahoe_vector_forest_create against the CPU oracle run per class on the
K-fold expansion of a forest of complete depth-3 trees, against tests/oblivious_ref.py on an oblivious forest written as
vector-leaf trees, and what the named forests of the GPU tests are said to contain."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oblivious_ref as obr  # noqa: E402
import vector_ref as vr  # noqa: E402

NODE_DTYPE = np.dtype([("weight", "<f4"), ("val", "<f4"), ("bits", "<i4")])


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("trees,cols,k", [(5, 5, 3), (9, 8, 1), (1, 1, 9)])
def test_reference_equals_the_oracle_on_the_expansion(built, trees, cols, k):
    from oracle import oracle

    rng = np.random.default_rng(31 + k)
    forest = vr.make([vr.random_tree(rng, cols, 13, 3, 0.0) for _ in range(trees)], vr.mixed_leaves(rng, 13, k), k, cols)
    data = vr.make_data(130, cols, seed=5)
    assert np.isnan(data).any() and np.isinf(data).any() and (data == vr.MISSING).any()
    sums, leaf, steps = vr.vector_ref(forest, data)
    assert (steps == 3).all()
    exp_nodes, exp_trees = vr.expand(forest)
    assert exp_trees.size == trees * k and exp_nodes.size == trees * k * 15
    # a complete depth-3 tree laid out breadth-first with adjacent children is the heap: children of i at 2i + 1, 2i + 2
    tree0 = exp_nodes[:15]
    assert (tree0["left_idx"][:7] == 2 * np.arange(7) + 1).all()
    for c in range(k):
        dense = np.zeros(trees * 15, NODE_DTYPE)
        for t in range(trees):
            src = exp_nodes[exp_trees[t * k + c]:exp_trees[t * k + c] + 15]
            dense["val"][t * 15:(t + 1) * 15] = src["val"]
            dense["bits"][t * 15:(t + 1) * 15] = src["bits"]
        want, heap_leaf = oracle.predict(dense, trees, 3, data, vr.MISSING, want_leaf=True)
        assert same_bits(sums[:, c], want), c
        assert np.array_equal(heap_leaf.astype(np.uint32), leaf)
    assert len(np.unique(leaf)) > 1


@pytest.mark.parametrize("depths,cols,k", [([0, 1, 2, 6, 2, 0, 6, 1, 6], 5, 1), ([6, 2, 1, 0, 6], 3, 3), ([0, 0, 0], 1, 2)])
def test_reference_equals_the_oblivious_reference(depths, cols, k):
    ob = obr.make_forest(depths, cols, k, seed=11 + cols)
    data = obr.make_data(130, cols, seed=5)
    want, want_leaf = obr.ref_of(ob, data)
    sums, leaf, _ = vr.vector_ref(vr.from_oblivious(ob), data)
    assert same_bits(sums, want)
    assert np.array_equal(obr.heap_leaf_to_oblivious(leaf, depths), want_leaf)


def test_reference_known_answer():
    # x0 >= 0.5 (default left) ? (x1 >= 0.0 (default right) ? vector 0 : vector 2) : vector 2 -- the two leaves share a vector
    m = vr.MISSING
    forest = vr.make([(0, 0.5, True, 2, (1, 0.0, False, 2, 0))], [[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]], 2, 2)
    assert forest["nodes"]["left_idx"].tolist() == [1, 2, 3, 2, 0]
    data = np.array([[0.5, -0.0], [0.25, 0.0], [np.nan, np.nan], [m, m], [np.inf, -np.inf], [0.5, m]], np.float32)
    sums, leaf, steps = vr.vector_ref(forest, data, m)
    assert leaf[:, 0].tolist() == [4, 1, 1, 1, 3, 4]
    assert sums.tolist() == [[1.0, 10.0], [4.0, 40.0], [4.0, 40.0], [4.0, 40.0], [4.0, 40.0], [1.0, 10.0]]
    assert steps[:, 0].tolist() == [2, 1, 1, 1, 2, 2]
    nodes, trees = vr.expand(forest)
    assert trees.tolist() == [0, 5] and nodes["val"][[1, 3, 4]].tolist() == [4.0, 4.0, 1.0]
    assert nodes["val"][[6, 8, 9]].tolist() == [40.0, 40.0, 10.0]


def test_the_named_forests_hold_what_the_gpu_tests_need():
    assert sorted({len(v[0]) for v in vr.FORESTS.values()}) == [0, 1, 3, 4, 5, 9]
    assert sorted({v[2] for v in vr.FORESTS.values()}) == [1, 3, 8, 9, 17]
    assert sorted({v[1] for v in vr.FORESTS.values()}) == [1, 5, 8]
    both_defaults, ties, shared = set(), False, False
    for name, (kinds, cols, k) in vr.FORESTS.items():
        forest, data, sums, leaf, steps = vr.case(name)
        nodes = forest["nodes"]
        assert sums.shape == (vr.ROWS, k) and leaf.shape == (vr.ROWS, len(kinds))
        internal = nodes[nodes["bits"] >= 0]
        both_defaults |= set(((internal["bits"] >> 30) & 1).tolist())
        leaves_of = nodes["left_idx"][nodes["bits"] < 0]
        shared |= len(np.unique(leaves_of)) < leaves_of.size
        if leaves_of.size > 2:
            assert (np.diff(leaves_of) < 0).any() and (np.diff(leaves_of) > 0).any()  # no relation to the node order
        if internal.size:
            fid = internal["bits"] & vr.FID_MASK
            ties |= bool((data[:, fid] == internal["val"][None, :]).any())
        for t, kind in enumerate(kinds):
            if kind == "leaf":
                assert (steps[:, t] == 0).all() and (leaf[:, t] == 0).all()
            elif kind == "stump":
                assert (steps[:, t] == 1).all() and set(leaf[:, t].tolist()) == {1, 2}
            elif kind == "chain":  # rows leave at different steps, some at the first and some at the last
                assert steps[:, t].min() == 1 and steps[:, t].max() == 24 and len(np.unique(steps[:64, t])) > 4
        assert np.isnan(data).any() and np.isinf(data).any() and (data == vr.MISSING).any()
        assert (np.signbit(data) & (data == 0)).any()
    assert both_defaults == {0, 1} and ties and shared
