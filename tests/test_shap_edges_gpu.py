"""The three SHAP entry points (predict_contribs, predict_interactions, predict_contribs_interventional) at their edges, on the
GPU, against the float64 references (checked against their brute force by tests/test_shap_edges_capi.py).  Needs an MI355X.

Cases: extreme covers (zero, 1e-30 .. 1e30, within 1e-8 of 1, float32 subnormals, a float32 sum that overflows, the stump with
covers (1e-39, 1) with and without a zero-cover element on the path); branch-rule edges (+-0, +-inf, NaN, subnormals, float32
neighbours of thresholds, the missing band, a sentinel equal to a threshold, missing = NaN, contradictory bounds, NaN
thresholds); path and bin structure (F = 1 stumps: 32 rounds in a bin; spines of depth 20-22; root leaves only, T = 0, a class
without bins); the LDS forms at their boundaries; interventional background sizes around the 8-way unroll; a seeded sweep.

Bars (tests/shap_edges.py): every output finite; |phi - phi64| <= gamma A + floor with the gamma of the entry point's own GPU
file and floor = (N + k (D + 2)) 2^-121 max|leaf| (<= 1e-30 here: it covers create's cut of zero fractions below 2^-121 and
subnormal roundings, never a normal-range error); the bias column bit for bit; for interactions symmetry, diagonal, bias corner
and zero row / column F bit for bit; additivity against the library's margin; each checked row alone bitwise equal to its row
of the full batch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contribs_ref  # noqa: E402
import interventional_ref as ivr  # noqa: E402
import shap_edges as se  # noqa: E402
from shap_edges import bits, check_contribs, check_interactions, check_interventional  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
M = -999.0
UNSUPPORTED = 7


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


# ---- a. covers ----
@pytest.mark.parametrize("mode", se.COVER_MODES)
def test_covers_contribs_and_interactions(env, mode):
    for seed in range(2):
        nodes, T, D, F, x, bg, missing = se.edge_case(f"covers:{mode}", 10 * seed + len(mode))
        label = f"covers {mode} seed {seed}"
        check_contribs(env, nodes, T, D, F, x, missing, label=label, brute=True)
        check_interactions(env, nodes, T, D, F, x, missing, label=label, brute=True)


@pytest.mark.parametrize("zero_on_path", [False, True])
def test_tiny_cover_stump(env, zero_on_path):
    """Covers (1e-39, 1): the kernels' pre = (ud - i) z / (ud + 1) would be subnormal and rcp(pre) +inf (phi = -inf, or NaN
    next to a zero-cover element) had create kept z = 1e-39; it stores 0 below 2^-121."""
    nodes, T, D, F, x = se.tiny_stump_case(zero_on_path)
    assert se.min_zero_fraction_not_followed(nodes, T, x, M) < se.Z_MIN, "some row does not follow an element with z < 2^-121"
    check_contribs(env, nodes, T, D, F, x, M, label="tiny stump", brute=True)
    if zero_on_path:
        check_interactions(env, nodes, T, D, F, x, M, label="tiny stump + zero cover", brute=True)


def test_zero_cover_followed_and_not(env):
    """A zero-cover child on every split, rows on both sides of it."""
    rng = np.random.default_rng(5)
    nodes = se.random_forest(rng, 3, 3, 4, M, covers="zero", leaf_prob=0.0, thresholds=np.array([0.5], F32))
    x = se.random_data(rng, 33, 4, M, pool=np.array([0.0, 1.0], F32))
    w = nodes["weight"].reshape(3, 15)[:, 1:]
    assert np.any(w == 0)
    per = 15
    followed, not_followed = False, False
    for t in range(3):
        for _, elems in contribs_ref._paths(nodes.reshape(3, per)[t]):
            for f, z, edges in elems:
                if z == 0:
                    o = np.ones(x.shape[0], bool)
                    for thr, dl, right in edges:
                        o &= contribs_ref.go_right(x[:, f], thr, dl, M) == right
                    followed |= bool(o.any())
                    not_followed |= bool((~o).any())
    assert followed and not_followed, "rows follow and do not follow a zero-cover element"
    check_contribs(env, nodes, 3, 3, 4, x, M, label="zero covers", brute=True)
    check_interactions(env, nodes, 3, 3, 4, x, M, label="zero covers", brute=True)


# ---- b. branch-rule edges ----
@pytest.mark.parametrize("missing", list(se.MISSINGS))
def test_branch_rule_edges(env, missing):
    for seed in range(2):
        nodes, T, D, F, x, bg, m = se.edge_case(f"branch:{missing}", 100 + seed)
        label = f"branch missing={missing} seed {seed}"
        internal = (nodes["bits"].view(np.uint32) >> 31) == 0
        thr = nodes["val"][internal]
        assert np.any(~np.isfinite(thr)), "NaN or infinite thresholds"
        check_contribs(env, nodes, T, D, F, x, m, label=label, brute=True)
        check_interactions(env, nodes, T, D, F, x, m, label=label, brute=True, need_pairs=False)
        check_interventional(env, nodes, T, D, F, x, bg, m, label=label, brute=True)
        check_interventional(env, nodes, T, D, F, x, x[:7], m, label=label + " (x as background)", brute=True)


@pytest.mark.parametrize("missing", list(se.MISSINGS))
def test_contradictory_bounds_and_nan_thresholds(env, missing):
    nodes, T, D, F, x, bg, m = se.edge_case(f"contradictory:{missing}", 7)
    x = np.concatenate([x, np.array([[6.0, 0.0], [4.0, 1.0], [F32(m), 0.0], [np.nan, F32(m)]], F32)])
    label = f"contradictory missing={missing}"
    check_contribs(env, nodes, T, D, F, x, m, label=label, brute=True)
    check_interactions(env, nodes, T, D, F, x, m, label=label, brute=True)
    check_interventional(env, nodes, T, D, F, x, bg, m, label=label, brute=True)


# ---- c. path and bin structure ----
def test_f1_stumps_32_rounds(env):
    rng = np.random.default_rng(1)
    T = 64
    nodes = np.concatenate([se.stump(*se.cover_pair(rng, "mixed"), thr=F32(rng.choice(se.threshold_pool(0.5))),
                                     leaves=(rng.uniform(-2, 2), rng.uniform(-2, 2))) for _ in range(T)])
    x = se.random_data(rng, 70, 1, 0.5)
    bins = se.pack_bins(nodes, T)
    assert len(bins) == 4 and all(se.bin_rounds(b) == 32 for b in bins), "a bin has 32 rounds (round field 31)"
    check_contribs(env, nodes, T, 1, 1, x, 0.5, label="F=1 stumps", brute=True)
    check_interactions(env, nodes, T, 1, 1, x, 0.5, label="F=1 stumps", need_pairs=False)
    check_interventional(env, nodes, T, 1, 1, x, x[:9], 0.5, label="F=1 stumps", brute=True)


def _spines(D):
    """Two spines of depth D on D distinct features of 24 (paths of 2 .. D + 1 elements), and rows from a small pool."""
    F = 24
    rng = np.random.default_rng(D)
    fids = list(rng.permutation(F)[:D])
    nodes = se.spine(D, fids, [F32(0.5)] * D)
    assert max(se.path_lengths(nodes, 1)) == D + 1, f"a path has {D + 1} elements"
    nodes2 = np.concatenate([nodes, se.spine(D, fids[::-1], [F32(0.25)] * D, leaf0=-1.0)])
    bins = se.pack_bins(nodes2, 2)
    assert any(sorted(L for L, _ in b)[-2:] == [D + 1, D + 1] for b in bins), "two longest paths in one bin"
    x = se.random_data(rng, 20, F, M, pool=np.array([0.0, 0.3, 0.6, 1.0, M, np.nan], F32))
    bg = se.random_data(rng, 9, F, M, pool=np.array([0.0, 0.3, 0.6, 1.0, M, np.nan], F32))
    return nodes, nodes2, fids, F, x, bg


@pytest.mark.parametrize("D", [20, 21, 22])
def test_spine_distinct_features(env, D):
    nodes, nodes2, fids, F, x, bg = _spines(D)
    check_contribs(env, nodes2, 2, D, F, x, M, label=f"spine {D}")
    check_interactions(env, nodes2, 2, D, F, x, M, label=f"spine {D}")
    check_interventional(env, nodes2, 2, D, F, x, bg, M, label=f"spine {D}")
    if D == 22:  # interventional reads W[p][q] up to p + q = 22: x and its background differ on every spine feature
        xa = np.full((1, F), 1.0, F32)
        xa[0, fids] = np.where(np.arange(D) % 2 == 0, 1.0, 0.0)  # the deep path: right at even k, left at odd k
        ba = xa.copy()
        ba[0, fids] = 1.0 - xa[0, fids]
        check_interventional(env, nodes2[: nodes.size], 1, D, F, xa, ba, M, label="spine 22 p + q = 22")


def test_spine_three_features_long_merged_paths(env):
    D = 21
    nodes = se.spine(D, [k % 3 for k in range(D)], [F32(v) for v in np.linspace(-1, 1, D)])
    assert max(se.path_lengths(nodes, 1)) == 4
    rng = np.random.default_rng(3)
    x = se.random_data(rng, 40, 3, M, pool=np.concatenate([np.linspace(-1.1, 1.1, 23), [M, np.nan]]).astype(F32))
    check_contribs(env, nodes, 1, D, 3, x, M, label="spine 3 features")
    check_interactions(env, nodes, 1, D, 3, x, M, label="spine 3 features")
    check_interventional(env, nodes, 1, D, 3, x, x[:5], M, label="spine 3 features", brute=True)


def test_spine_depth_12_brute_force(env):
    D = 12
    nodes = se.spine(D, list(range(D)), [F32(0.5)] * D)
    rng = np.random.default_rng(12)
    x = se.random_data(rng, 6, D, M, pool=np.array([0.0, 1.0, M, np.nan, 0.5], F32))
    check_contribs(env, nodes, 1, D, D, x, M, label="spine 12", brute=True)
    check_interactions(env, nodes, 1, D, D, x, M, label="spine 12", brute=True)
    check_interventional(env, nodes, 1, D, D, x, x[:2], M, label="spine 12", brute=True)


def _all_plus_zero(a):
    return not np.any(bits(a))


@pytest.mark.parametrize("T", [0, 5])
def test_no_bins(env, T):
    """Only root leaves (T = 5), or no trees: +0.0 contributions, the exact bias."""
    ta, torch = env
    D, F = 2, 3
    per = 2 ** (D + 1) - 1
    nodes = np.concatenate([se.encode(np.zeros(per), [F32(0.5 + t)] + [F32(9.0)] * (per - 1), np.zeros(per),
                                      np.full(per, F32(np.nan)), np.ones(per)) for t in range(T)]) if T else \
        np.empty(0, ta.capi.NODE_DTYPE)
    assert se.pack_bins(nodes, T) == []
    x = se.random_data(np.random.default_rng(T), 9, F, M)
    _, got = check_contribs(env, nodes, T, D, F, x, M, bias=0.25, label=f"no bins T={T}")
    assert _all_plus_zero(got[..., :-1])
    _, gi = check_interactions(env, nodes, T, D, F, x, M, bias=0.25, label=f"no bins T={T}", need_pairs=False)
    idx = np.arange(F + 1)
    assert _all_plus_zero(gi[..., idx[:, None] != idx[None, :]]) and _all_plus_zero(gi[..., idx[:F], idx[:F]])
    _, gv = check_interventional(env, nodes, T, D, F, x, x[:3], M, bias=0.25, label=f"no bins T={T}")
    assert _all_plus_zero(gv[..., :-1])


def test_multiclass_with_a_class_without_bins(env):
    ta, torch = env
    C, D, F = 3, 4, 5
    rng = np.random.default_rng(33)
    per = 2 ** (D + 1) - 1
    trees = []
    for t in range(6):
        if t % C == 1:  # class 1: root leaves only
            trees.append(se.encode(np.zeros(per), [F32(1.5)] + [F32(0)] * (per - 1), np.zeros(per), np.ones(per),
                                   np.ones(per)))
        else:
            trees.append(se.random_forest(rng, 1, D, F, M, covers="mixed", leaf_prob=0.1))
    nodes = np.concatenate(trees)
    x = se.random_data(rng, 21, F, M)
    out = ta.OUT_AVG | ta.OUT_SOFTMAX
    _, got = check_contribs(env, nodes, 6, D, F, x, M, num_classes=C, output=out, bias=0.375, label="C=3, class 1 empty",
                            brute=True)
    assert _all_plus_zero(got[:, 1, :-1])
    check_interactions(env, nodes, 6, D, F, x, M, num_classes=C, output=out, bias=0.375, label="C=3, class 1 empty")
    _, gv = check_interventional(env, nodes, 6, D, F, x, x[:4], M, num_classes=C, output=out, bias=0.375,
                                 label="C=3, class 1 empty", brute=True)
    assert _all_plus_zero(gv[:, 1, :-1])


# ---- d. LDS form boundaries ----
def _rows_for(R):
    return sorted({2 * R + 1, max(R - 1, 1)})


def _forest(env, F, seed):
    ta, _ = env
    rng = np.random.default_rng(seed)
    T = int(rng.integers(10, 21))
    D = int(rng.integers(6, 8))
    nodes = ta.synth_forest(T, D, F, seed=seed, leaf_prob=0.05)
    nodes["weight"] = rng.uniform(0.05, 1.0, nodes.size).astype(F32)
    return nodes, T, D


# The library does not report the tile rows it picks, so these preconditions check tests/shap_edges.py's restatement of the
# rules in contribs_build / iv_shape against the expected table, not the library itself: a later change to those rules must
# update the restatements, or these cases drift off the boundaries without failing.
CONTRIBS_FORMS = {65: 32, 129: 16, 513: 4, 2049: 1, 4096: 1, 4097: 1, 8192: 1}


@pytest.mark.parametrize("F", list(CONTRIBS_FORMS))
def test_contribs_form_boundaries(env, F):
    ta, _ = env
    R = se.contribs_tile_rows(F)
    assert R == CONTRIBS_FORMS[F], f"F={F} gives tile rows {CONTRIBS_FORMS[F]} by the rule in contribs_build"
    assert (20 * R * F > 80 * 1024) == (F == 4097 or F == 8192)
    nodes, T, D = _forest(env, F, F)
    for n in _rows_for(R):
        x = ta.synth_data(n, F, seed=F + n, missing_prob=0.02, missing=M, nan_prob=0.01)
        check_contribs(env, nodes, T, D, F, x, M, label=f"contribs F={F} rows={n}")


def test_contribs_widest_plus_one_is_refused(env):
    ta, _ = env
    nodes, T, D = _forest(env, 8193, 8193)
    with pytest.raises(ta.capi.TahoeError) as e:
        ta.Forest(nodes, T, D, 8193, missing=M, contribs=True)
    assert e.value.status == UNSUPPORTED


def test_multiclass_at_a_form_boundary(env):
    ta, _ = env
    C, F, T, D = 3, 4097, 12, 6
    nodes = ta.synth_forest(T, D, F, seed=41, leaf_prob=0.05)
    nodes["weight"] = np.random.default_rng(41).uniform(0.05, 1.0, nodes.size).astype(F32)
    x = ta.synth_data(3, F, seed=42, missing_prob=0.02, missing=M, nan_prob=0.01)
    _, got = check_contribs(env, nodes, T, D, F, x, M, num_classes=C, label="C=3 F=4097")
    for c in range(C):
        g = ta.Forest(ivr.sub_forest(nodes, T, C, c), T // C, D, F, missing=M, contribs=True)
        assert np.array_equal(bits(se.gpu_phi(env, g, x)[:, 0]), bits(got[:, c])), c
        g.close()


INTER_FORMS = {13: (True, 16), 18: (True, 8), 26: (True, 4), 36: (True, 2), 50: (True, 2), 51: (True, 1), 71: (True, 1),
               72: (False, 1)}


@pytest.mark.parametrize("F", list(INTER_FORMS))
def test_interactions_form_boundaries(env, F):
    ta, _ = env
    slabs, RI = se.interactions_tile_rows(F)
    assert (slabs, RI) == INTER_FORMS[F], f"F={F} gives the form {INTER_FORMS[F]} by the rule in contribs_build"
    nodes, T, D = _forest(env, F, 500 + F)
    for n in _rows_for(RI if slabs else 4):
        x = ta.synth_data(n, F, seed=F + n, missing_prob=0.02, missing=M, nan_prob=0.01)
        check_interactions(env, nodes, T, D, F, x, M, label=f"interactions F={F} rows={n}")


def test_interactions_in_place_above_4096(env):
    ta, _ = env
    F = 4100
    assert se.interactions_tile_rows(F) == (False, 1)
    nodes, T, D = _forest(env, F, 4100)
    x = ta.synth_data(2, F, seed=4101, missing_prob=0.02, missing=M, nan_prob=0.01)
    check_interactions(env, nodes, T, D, F, x, M, label="interactions F=4100")


IV_FORMS = {486: (8, True), 487: (4, True), 973: (2, True), 1946: (1, True), 3891: (1, True), 3892: (1, True),
            7987: (1, True), 7988: (1, False)}


@pytest.mark.parametrize("F", list(IV_FORMS))
def test_interventional_form_boundaries(env, F):
    ta, _ = env
    R, wlds = se.interventional_shape(F)
    assert (R, wlds) == IV_FORMS[F], f"F={F} gives {IV_FORMS[F]} by the rule in iv_shape"
    nodes, T, D = _forest(env, F, 900 + F)
    bg = ta.synth_data(9, F, seed=F + 3, missing_prob=0.02, missing=M, nan_prob=0.01)
    for n in _rows_for(R):
        x = ta.synth_data(n, F, seed=F + n, missing_prob=0.02, missing=M, nan_prob=0.01)
        check_interventional(env, nodes, T, D, F, x, bg, M, label=f"interventional F={F} rows={n}")


# ---- e. interventional background sizes ----
@pytest.fixture(scope="module")
def bg_forest(env):
    rng = np.random.default_rng(77)
    T, D, F = 8, 5, 6
    nodes = se.random_forest(rng, T, D, F, 0.5, leaf_prob=0.1)
    x = se.random_data(rng, 19, F, 0.5)
    return nodes, T, D, F, x, rng


@pytest.mark.parametrize("B", [1, 7, 8, 9, 17, 1000])
def test_background_sizes(env, bg_forest, B):
    nodes, T, D, F, x, rng = bg_forest
    bg = se.random_data(np.random.default_rng(B), B, F, 0.5)
    check_interventional(env, nodes, T, D, F, x, bg, 0.5, label=f"B={B}", brute=B <= 17)


@pytest.mark.parametrize("kind", ["identical", "all_missing", "all_nan"])
def test_degenerate_backgrounds(env, bg_forest, kind):
    nodes, T, D, F, x, rng = bg_forest
    row = {"identical": x[3], "all_missing": np.full(F, 0.5, F32), "all_nan": np.full(F, np.nan, F32)}[kind]
    bg = np.repeat(row[None, :], 9, axis=0)
    check_interventional(env, nodes, T, D, F, x, bg, 0.5, label=f"background {kind}", brute=True)


# ---- f. seeded sweep ----
@pytest.mark.parametrize("seed", range(30))
def test_seeded_sweep(env, seed):
    nodes, T, D, F, x, bg, m = se.edge_case("sweep", 1000 + seed)
    label = f"sweep {seed}"
    check_contribs(env, nodes, T, D, F, x, m, label=label, brute=True)
    check_interactions(env, nodes, T, D, F, x, m, label=label, brute=True, need_pairs=False)
    check_interventional(env, nodes, T, D, F, x, bg, m, label=label, brute=True)
