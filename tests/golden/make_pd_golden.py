"""Writes tests/golden/pd_sklearn.npz: a small scikit-learn GradientBoostingRegressor as a sparse forest with covers, and what
scikit-learn's partial_dependence(method="recursion") gives for three target sets.  Needs scikit-learn (1.7.2 wrote the committed
file); the tests read the file and never import scikit-learn.

The forest: 12 trees of depth <= 4 on 6 features, children renumbered so that the two children of a node are adjacent (left_idx,
left_idx + 1) and lie after their parent; the learning rate folded into the float32 leaf values; covers = tree_.weighted_n_node_samples.
scikit-learn's `x <= thr goes left` (x a float32, thr a float64) becomes this library's `x >= val goes right` with
val = nextafter(thr rounded down to float32, +inf).  The recursion method leaves out the init estimator, as the raw sums here do.

Run from the repository root:  python tests/golden/make_pd_golden.py"""
import os
import sys

import numpy as np
from sklearn.ensemble import GradientBoostingRegressor
from sklearn.inspection import partial_dependence

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pd_ref  # noqa: E402

SPARSE_NODE_DTYPE = np.dtype([("val", "<f4"), ("bits", "<i4"), ("left_idx", "<i4")])
TARGET_SETS = {"a": ([0], 30), "b": ([0, 1], 12), "c": ([2, 4, 5], 5)}  # name -> (features, grid resolution per axis)


def f32_down(x):
    y = np.float32(x)
    return y if float(y) <= float(x) else np.nextafter(y, np.float32(-np.inf))


def convert(est):
    nodes, covers, roots = [], [], []
    for stage in est.estimators_[:, 0]:
        tr = stage.tree_
        base = len(nodes)
        roots.append(base)
        nodes.append(None)
        covers.append(0.0)
        queue = [(0, 0)]  # (scikit-learn node, position relative to the root)
        while queue:
            i, pos = queue.pop(0)
            covers[base + pos] = np.float32(tr.weighted_n_node_samples[i])
            if tr.children_left[i] < 0:
                nodes[base + pos] = (np.float32(tr.value[i, 0, 0] * est.learning_rate), np.int32(-(1 << 31)), 0)
                continue
            left = len(nodes) - base
            nodes += [None, None]
            covers += [0.0, 0.0]
            val = np.nextafter(f32_down(tr.threshold[i]), np.float32(np.inf))
            nodes[base + pos] = (val, np.int32(tr.feature[i]), left)
            queue += [(tr.children_left[i], left), (tr.children_right[i], left + 1)]
    return (np.array(nodes, dtype=SPARSE_NODE_DTYPE), np.array(roots, np.int32), np.array(covers, np.float32))


def main():
    rng = np.random.default_rng(20240607)
    X = rng.normal(size=(400, 6)).astype(np.float32)
    X[:, 3] = np.round(X[:, 3] * 2) / 2  # a feature with few distinct values: grid points equal to thresholds' neighbours
    y = np.sin(X[:, 0]) + X[:, 1] * X[:, 2] + 0.5 * (X[:, 4] > 0) - 0.3 * X[:, 5] ** 2 + 0.1 * rng.normal(size=400)
    est = GradientBoostingRegressor(n_estimators=12, max_depth=4, learning_rate=0.3, random_state=0).fit(X, y)
    nodes, trees, covers = convert(est)
    out = {"nodes": nodes, "trees": trees, "covers": covers, "num_cols": np.int32(6), "missing": np.float32(-999.0)}
    for name, (feats, res) in TARGET_SETS.items():
        r = partial_dependence(est, X, features=feats, method="recursion", kind="average", grid_resolution=res)
        axes = [np.asarray(a, dtype=np.float32) for a in r["grid_values"]]
        grid = np.stack([m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij")], axis=1).astype(np.float32)
        want = np.asarray(r["average"], dtype=np.float64).reshape(-1)
        _, A = pd_ref.pd_f64(nodes, trees, covers, feats, grid, -999.0)
        out[f"{name}_features"] = np.array(feats, np.int32)
        out[f"{name}_grid"] = grid
        out[f"{name}_sklearn"] = want
        out[f"{name}_A"] = A[:, 0]
    np.savez_compressed(os.path.join(HERE, "pd_sklearn.npz"), **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
