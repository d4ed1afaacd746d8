"""The float64 references that tests/test_shap_edges_gpu.py compares the kernels with (contribs_ref.poly,
interactions_ref.poly, interventional_ref.paths), checked against their subset brute force on the adversarial pools of
tests/shap_edges.py: extreme covers (zero, 1e-30 .. 1e30, within 1e-8 of 1, float32 subnormals, a float32 sum that overflows,
ratios down to 1e-300), branch-rule edges (+-0, +-inf, NaN and subnormal thresholds and data, the missing band, contradictory
bounds on a repeated feature) and long paths.  Bar: within 1e-12 of sum |phi| per row (bias column included).

The Saabas reference (approx_contribs_ref.dense, which tests/test_approx_edges_gpu.py compares approx_kernel with bit for bit) on
the same pools: against its float64 restatement direct64 within (N + 1) 2^-24 S per row and class (N float32 adds of deltas
rounded once, S the sum of |delta|), the float64 deltas of every (row, tree) path telescoping to leaf - E(root), and the
preconditions that keep the GPU cases from passing vacuously.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_contribs_ref as aref  # noqa: E402
import contribs_ref  # noqa: E402
import interactions_ref  # noqa: E402
import interventional_ref as ivr  # noqa: E402
import shap_edges as se  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module")
def lib(built):
    import tahoe_amd  # noqa: F401  (encode_nodes; the oracle for interventional brute force)

    return True


def agree(want, got, label):
    scale = np.abs(want).reshape(want.shape[0], -1).sum(axis=-1)
    err = np.abs(want - got).reshape(want.shape[0], -1).max(axis=-1)
    assert np.all(np.isfinite(got)), label
    assert np.all(err <= 1e-12 * scale), f"{label}: max err / sum|phi| = {np.max(err / np.maximum(scale, 1e-300)):.3e}"


def all_three(nodes, T, D, F, x, bg, missing, label, interactions=True, interventional=True):
    p, _, _ = contribs_ref.poly(nodes, T, D, F, x, missing)
    agree(contribs_ref.brute(nodes, T, D, F, x, missing), p, f"{label} contribs")
    if interactions:
        pi, _, _ = interactions_ref.poly(nodes, T, D, F, x, missing)
        agree(interactions_ref.brute(nodes, T, D, F, x, missing), pi, f"{label} interactions")
    if interventional:
        pv, _, _ = ivr.paths(nodes, T, D, F, x, bg, missing)
        agree(ivr.brute(nodes, T, D, F, x, bg, missing), pv, f"{label} interventional")


@pytest.mark.parametrize("mode", se.COVER_MODES)
def test_cover_pools(lib, mode):
    for seed in range(3):
        nodes, T, D, F, x, bg, missing = se.edge_case(f"covers:{mode}", 10 * seed + len(mode))
        all_three(nodes, T, D, F, x, bg, missing, f"covers {mode} seed {seed}", interventional=False)


@pytest.mark.parametrize("zero_on_path", [False, True])
def test_tiny_stump(lib, zero_on_path):
    nodes, T, D, F, x = se.tiny_stump_case(zero_on_path)
    assert se.min_zero_fraction_not_followed(nodes, T, x, -999.0) < se.Z_MIN  # a row does not follow a tiny-ratio element
    all_three(nodes, T, D, F, x, x[:2], -999.0, "tiny stump", interactions=zero_on_path)


@pytest.mark.parametrize("ratio_edges", [1, 2, 4])
def test_ratios_down_to_1e_300(lib, ratio_edges):
    """A spine whose deep path takes the small child k times at ratio 1e-75 (covers 1e-37 and 1e38): z down to 1e-300 on one
    merged element (feature 0 repeated) and tiny ratios on others."""
    D = 6
    fids = [0] * ratio_edges + [1, 2, 3, 1, 2, 3][: D - ratio_edges]
    thr = [F32(v) for v in (0.5, -0.5, 0.25, 1.0, 2.0, 0.0)]
    right = [True, False, True, False, True, True]
    nodes = se.spine(D, fids, thr, covers=(F32(1e38), F32(1e-37)), right=right)
    rng = np.random.default_rng(ratio_edges)
    x = se.random_data(rng, 40, 4, -999.0, pool=np.array([-1.0, -0.4, 0.0, 0.3, 0.6, 1.5, 3.0, -999.0, np.nan], F32))
    z = min(e[1] for _, el in contribs_ref._paths(nodes) for e in el)
    assert z < 1e-70 ** ratio_edges
    all_three(nodes, 1, D, 4, x, x[:3], -999.0, f"1e-300 spine ({ratio_edges} edges)")


@pytest.mark.parametrize("missing", list(se.MISSINGS))
def test_branch_rule_pools(lib, missing):
    for seed in range(3):
        nodes, T, D, F, x, bg, m = se.edge_case(f"branch:{missing}", 100 + seed)
        all_three(nodes, T, D, F, x, bg, m, f"branch missing={missing} seed {seed}")


@pytest.mark.parametrize("missing", list(se.MISSINGS))
def test_contradictory_bounds(lib, missing):
    nodes, T, D, F, x, bg, m = se.edge_case(f"contradictory:{missing}", 7)
    x = np.concatenate([x, np.array([[6.0, 0.0], [4.0, 1.0], [F32(m), 0.0], [np.nan, F32(m)]], F32)])
    all_three(nodes, T, D, F, x, bg, m, f"contradictory missing={missing}")


def test_spine_depth_12_distinct_features(lib):
    D = 12
    nodes = se.spine(D, list(range(D)), [F32(0.5)] * D)
    rng = np.random.default_rng(12)
    x = se.random_data(rng, 6, D, -999.0, pool=np.array([0.0, 1.0, -999.0, np.nan, 0.5], F32))
    assert max(se.path_lengths(nodes, 1)) == D + 1
    all_three(nodes, 1, D, D, x, x[:2], -999.0, "spine 12")


def test_f1_stumps(lib):
    rng = np.random.default_rng(1)
    T = 64
    nodes = np.concatenate([se.stump(*se.cover_pair(rng, "mixed"), thr=F32(rng.choice(se.threshold_pool(0.5))),
                                     leaves=(rng.uniform(-2, 2), rng.uniform(-2, 2))) for _ in range(T)])
    x = se.random_data(rng, 40, 1, 0.5)
    assert all(se.bin_rounds(b) == 32 for b in se.pack_bins(nodes, T))
    all_three(nodes, T, 1, 1, x, x[:4], 0.5, "F=1 stumps", interactions=False)


@pytest.mark.parametrize("seed", range(30))
def test_seeded_sweep(lib, seed):
    nodes, T, D, F, x, bg, m = se.edge_case("sweep", 1000 + seed)
    all_three(nodes, T, D, F, x, bg, m, f"sweep {seed}")


@pytest.mark.parametrize("D", [4, 12])
def test_interactions_absolute_magnitude(lib, D):
    """interactions_ref.poly(cond=True): the same Phi, A and N as without it, and Aabs (the unwind with its subtraction made an
    addition) >= A everywhere, far above A on a long spine (the cancellation the GPU bar covers)."""
    nodes = se.spine(D, list(range(D)), [F32(0.5)] * D)
    rng = np.random.default_rng(D)
    x = se.random_data(rng, 12, D, -999.0, pool=np.array([0.0, 1.0, -999.0, np.nan], F32))
    want, A, N, Aabs = interactions_ref.poly(nodes, 1, D, D, x, -999.0, cond=True)
    w2, A2, N2 = interactions_ref.poly(nodes, 1, D, D, x, -999.0)
    assert np.array_equal(want, w2) and np.array_equal(A, A2) and np.array_equal(N, N2)
    assert np.all(Aabs >= A * (1 - 1e-12))
    if D == 12:
        assert np.max(Aabs[A > 0] / A[A > 0]) > 10


# ---- the Saabas reference on the same pools ----
U = 2.0 ** -24
APPROX_CASES = ([(f"covers:{m}", 10 * s + len(m)) for m in se.COVER_MODES for s in range(2)]
                + [(f"branch:{m}", 100 + s) for m in se.MISSINGS for s in range(2)]
                + [(f"contradictory:{m}", 7) for m in se.MISSINGS] + [("sweep", 1000 + s) for s in range(6)])


def stored_deltas(nodes, T, D):
    """[(E(n), float32 d(left), float32 d(right))] over the reachable internal nodes of every tree."""
    per = (1 << (D + 1)) - 1
    left = 2 * np.arange(per, dtype=np.int64) + 1
    out = []
    for tree in nodes.reshape(T, per):
        fid, dl, leaf, val, w = contribs_ref._decode(tree)
        E = aref._means(val.astype(F32), leaf, left, w, True)
        for n in se.reachable(tree):
            if not leaf[n]:
                out.append((E[n], F32(E[2 * n + 1] - E[n]), F32(E[2 * n + 2] - E[n])))
    return out


@pytest.mark.parametrize("kind, seed", APPROX_CASES)
def test_approx_reference_telescopes(lib, kind, seed):
    nodes, T, D, F, x, bg, m = se.edge_case(kind, seed)
    label = f"{kind} seed {seed}"
    phi, S, N = aref.dense(nodes, T, D, F, x, m, scale=True)
    assert np.all(np.isfinite(phi)), f"{label}: the reference is finite on this case"
    want = aref.direct64(nodes, T, D, F, x, m)
    err = np.abs(phi.astype(np.float64) - want)[..., :F]
    tol = ((N + 1) * U * S)[:, :, None]
    assert np.all(err <= tol), f"{label}: dense vs direct64, worst {np.max(err / np.maximum(tol, 1e-300)):.3g} of the bound"
    for t, (E, path) in enumerate(se.approx_walks(nodes, T, D, x, m)):
        for r in range(x.shape[0]):
            p = path[r][path[r] >= 0]
            total = 0.0
            for a, b in zip(p[:-1], p[1:]):
                total += E[b] - E[a]
            bound = D * 2.0 ** -52 * np.max(np.abs(E[p]))
            assert abs(total - (E[p[-1]] - E[0])) <= bound, f"{label}: row {r} tree {t} does not telescope"


@pytest.mark.parametrize("seed", range(2))
def test_approx_zero_cover_children_taken_and_not(lib, seed):
    nodes, T, D, F, x, bg, m = se.edge_case("covers:zero", 10 * seed + len("zero"))
    taken, avoided = se.zero_cover_visits(nodes, T, D, x, m)
    assert taken > 0 and avoided > 0, "at splits with a zero-cover child, rows take that child and rows take its sibling"


@pytest.mark.parametrize("seed", range(2))
def test_approx_near_one_cancels(lib, seed):
    nodes, T, D, F, x, bg, m = se.edge_case("covers:near_one", 10 * seed + len("near_one"))
    small = [d for E, a, b in stored_deltas(nodes, T, D) for d in (a, b) if 0 < abs(float(d)) < 2.0 ** -20 * abs(E)]
    assert small, "a stored delta below 2^-20 |E(n)|: the difference of the means cancels almost completely"


def test_approx_leaf_pools(lib):
    """The leaf-magnitude cases of tests/test_approx_edges_gpu.py: subnormal deltas and sums that stay nonzero, large leaves
    with a finite reference, and leaves near FLT_MAX with between 1 % and 99 % of the feature outputs non-finite."""
    nodes, T, D, F, x, m = se.leaf_case("subnormal")
    d = np.array([float(v) for _, a, b in stored_deltas(nodes, T, D) for v in (a, b)])
    assert np.any((d != 0) & (np.abs(d) < se.FLT_MIN)), "subnormal stored deltas"
    for avg in (False, True):
        phi = aref.dense(nodes, T, D, F, x, m, avg=avg)[..., :F]
        assert np.all(np.isfinite(phi)) and np.any((phi != 0) & (np.abs(phi) < se.FLT_MIN)), "subnormal outputs"
    nodes, T, D, F, x, m = se.leaf_case("large")
    assert 2 * T * D * float(np.max(np.abs(se.reachable_leaves(nodes, T)))) < se.FLT_MAX
    assert np.all(np.isfinite(aref.dense(nodes, T, D, F, x, m)))
    nodes, T, D, F, x, m = se.leaf_case("overflow")
    bad = ~np.isfinite(aref.dense(nodes, T, D, F, x, m)[..., :F])
    assert 0.01 <= bad.mean() <= 0.99, f"{bad.mean():.3f} of the feature outputs are non-finite"
    assert np.any(np.isnan(aref.dense(nodes, T, D, F, x, m)[..., :F])), "inf - inf on some row"
