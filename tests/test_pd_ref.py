"""The float32 restatement of partial dependence (tests/pd_ref.py) without a GPU: against scikit-learn's recursion method on the
recorded fixture (tests/golden/pd_sklearn.npz), against the float64 evaluation of the same definition on random irregular forests
with classes and categorical splits, and the all-targets identity with the tree-order prediction sum.  The bound is derived
(pd_ref.bound), not measured."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import categorical_ref  # noqa: E402
import pd_cases  # noqa: E402
import pd_ref  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "pd_sklearn.npz"))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_restatement_matches_scikit_learn(golden, name):
    z = golden
    nodes, trees, covers = z["nodes"], z["trees"], z["covers"]
    assert len(trees) == 12 and pd_ref.shape_of(nodes, trees)[0] <= 4
    feats, grid, want, A = z[f"{name}_features"], z[f"{name}_grid"], z[f"{name}_sklearn"], z[f"{name}_A"]
    assert grid.shape[0] <= 200 and grid.shape[1] == len(feats)
    got = pd_ref.pd_f32(nodes, trees, covers, feats, grid, float(z["missing"]))[:, 0]
    _, A_now = pd_ref.pd_f64(nodes, trees, covers, feats, grid, float(z["missing"]))
    assert np.allclose(A_now[:, 0], A, rtol=1e-12)
    tol = pd_ref.bound(nodes, trees, A)
    err = np.abs(got.astype(np.float64) - want)
    print(f"targets {feats.tolist()}: max error {err.max():.3g}, bound at that point {tol[err.argmax()]:.3g}, scale {np.abs(want).max():.3g}")
    assert (err <= tol).all()
    assert np.ptp(want) > 0.05  # the curve is not flat: the check above compares something


@pytest.mark.parametrize("case", pd_cases.RANDOM_CASES, ids=lambda c: c["id"])
def test_restatement_matches_float64(case):
    fo = pd_cases.random_forest(**case["forest"])
    for feats in case["targets"]:
        grid = pd_cases.random_grid(fo, feats, 40, seed=len(feats))
        got = pd_ref.pd_f32(fo["nodes"], fo["trees"], fo["covers"], feats, grid, fo["missing"], fo["num_classes"], fo["cats"])
        want, A = pd_ref.pd_f64(fo["nodes"], fo["trees"], fo["covers"], feats, grid, fo["missing"], fo["num_classes"], fo["cats"])
        tol = pd_ref.bound(fo["nodes"], fo["trees"], A)
        assert (np.abs(got.astype(np.float64) - want) <= tol).all()
        assert (A > 0).all()


@pytest.mark.parametrize("case", pd_cases.RANDOM_CASES, ids=lambda c: c["id"])
def test_all_targets_is_the_tree_order_sum(case):
    fo = pd_cases.random_forest(**case["forest"])
    F = fo["num_cols"]
    rows = pd_cases.random_grid(fo, list(range(F)), 50, seed=9)
    node, offset, words, ml = fo["cats"] if fo["cats"] is not None else ((), (0,), (), None)
    want, _ = categorical_ref.predict(fo["nodes"], fo["trees"], rows, fo["missing"], node, offset, words, ml, fo["num_classes"])
    want = want.reshape(rows.shape[0], fo["num_classes"])
    perm = np.random.default_rng(3).permutation(F)  # the targets in any order: column j is feature perm[j]
    got = pd_ref.pd_f32(fo["nodes"], fo["trees"], fo["covers"], perm, rows[:, perm], fo["missing"], fo["num_classes"], fo["cats"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_no_targets_is_the_cover_weighted_mean():
    fo = pd_cases.random_forest(**pd_cases.RANDOM_CASES[0]["forest"])
    got = pd_ref.pd_f32(fo["nodes"], fo["trees"], fo["covers"], [], np.zeros((3, 0), np.float32), fo["missing"], fo["num_classes"])
    assert got.shape == (3, fo["num_classes"]) and (got == got[0]).all()
    # the mean by another route: leaf value times the product of the fractions on its path, float64
    nodes, trees, covers = fo["nodes"], fo["trees"], fo["covers"].astype(np.float64)
    mean = np.zeros(fo["num_classes"])
    for t in range(len(trees)):
        root = int(trees[t])
        stack = [(0, 1.0)]
        while stack:
            i, w = stack.pop()
            if nodes["bits"][root + i] < 0:
                mean[t % fo["num_classes"]] += w * float(nodes["val"][root + i])
                continue
            l = int(nodes["left_idx"][root + i])
            tot = covers[root + l] + covers[root + l + 1]
            stack += [(c, w * covers[root + c] / tot) for c in (l, l + 1) if covers[root + c] > 0]
    assert np.allclose(got[0], mean, rtol=1e-5, atol=1e-6)


def test_known_answer_by_hand():
    """One tree: root on x0 (>= 0.5 right), left child a leaf 1.0, right child splits on x1 into leaves 10.0 (cover 1) and 20.0
    (cover 3).  Target x0: left of 0.5 the value is 1.0, right of it 0.25 * 10 + 0.75 * 20 = 17.5.  Target x1: 0.5 * 1 + 0.5 * leaf."""
    LEAF = np.int32(-(1 << 31))
    sn = np.zeros(5, dtype=pd_cases.SPARSE_NODE_DTYPE)
    sn[0] = (0.5, 0, 1)
    sn[1] = (1.0, LEAF, 0)
    sn[2] = (2.0, 1, 3)
    sn[3] = (10.0, LEAF, 0)
    sn[4] = (20.0, LEAF, 0)
    tr = np.array([0], np.int32)
    cv = np.array([8, 4, 4, 1, 3], np.float32)
    got = pd_ref.pd_f32(sn, tr, cv, [0], np.array([[0.0], [0.5], [np.nan], [-999.0]], np.float32), -999.0)[:, 0]
    assert got.tolist() == [1.0, 17.5, 1.0, 17.5]  # NaN goes left; the sentinel takes the default branch, right without def_left
    got = pd_ref.pd_f32(sn, tr, cv, [1], np.array([[1.0], [2.0]], np.float32), -999.0)[:, 0]
    assert got.tolist() == [5.5, 10.5]
    got = pd_ref.pd_f32(sn, tr, cv, [], np.zeros((1, 0), np.float32), -999.0)[:, 0]
    assert got.tolist() == [0.5 * 1.0 + 0.5 * 17.5]
