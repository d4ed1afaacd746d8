"""Saabas contributions (tahoe_forest_predict_contribs_approx) at their edges, on the GPU, against tests/approx_contribs_ref.py
(checked against its float64 restatement on the same cases by tests/test_shap_edges_capi.py).  Needs an MI355X.

Cases: extreme covers (zero, 1e-30 .. 1e30, within 1e-8 of 1, float32 subnormals, a float32 sum that overflows, the stump with
covers (1e-39, 1)); leaves whose deltas are subnormal, near FLT_MAX / (2 T D), or overflow to +-inf; branch-rule edges (every
sentinel of MISSINGS, +-0, +-inf, NaN and subnormal thresholds and data, the missing band, contradictory bounds); structure
(F = 1 stumps, spines of depth 20-22, no trees, root leaves only, a class of root leaves); every kernel form at its
boundaries (4, 3, 2 and 1 waves of LDS slab, in place, TAHOE_APPROX_FORM); irregular sparse forests with extreme covers; a
seeded sweep.

Bars (shap_edges.check_approx): every output bit for bit the reference's (a NaN for a NaN); the bias column bit for bit
predict_contribs'; additivity against predict_raw within the bound of tests/test_approx_contribs_gpu.py on rows without an
overflow; each checked row alone bitwise equal to its row of the batch; the converted sparse handle bit for bit the dense one
under every strategy, the re-laid-out handle (exchange bits) bit for bit the plain one; no call writes past its rows."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_contribs_ref as ref  # noqa: E402
import shap_edges as se  # noqa: E402
from shap_edges import assert_same_bits, bits, check_approx, gpu_approx  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
M = -999.0


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


@pytest.fixture(autouse=True)
def no_forced_form(monkeypatch):
    monkeypatch.delenv("TAHOE_APPROX_FORM", raising=False)
    return monkeypatch


def _all_plus_zero(a):
    return not np.any(bits(a))


# ---- a. covers ----
@pytest.mark.parametrize("mode", se.COVER_MODES)
def test_covers(env, mode):
    for seed in range(2):
        nodes, T, D, F, x, bg, missing = se.edge_case(f"covers:{mode}", 10 * seed + len(mode))
        _, got = check_approx(env, nodes, T, D, F, x, missing, label=f"covers {mode} seed {seed}")
        assert np.all(np.isfinite(got))


@pytest.mark.parametrize("zero_on_path", [False, True])
def test_tiny_cover_stump(env, zero_on_path):
    """Covers (1e-39, 1): E(n) is the right leaf up to 1e-39, so d(right) rounds to a float32 subnormal or zero and d(left) to
    the whole difference of the leaves."""
    nodes, T, D, F, x = se.tiny_stump_case(zero_on_path)
    _, got = check_approx(env, nodes, T, D, F, x, M, label="tiny stump")
    assert np.all(np.isfinite(got))


def test_zero_cover_taken_and_not(env):
    """A zero-cover child on every split, rows on both sides of it: E(n) is the other child's mean, never 0 x E = NaN."""
    rng = np.random.default_rng(5)
    nodes = se.random_forest(rng, 3, 3, 4, M, covers="zero", leaf_prob=0.0, thresholds=np.array([0.5], F32))
    x = se.random_data(rng, 33, 4, M, pool=np.array([0.0, 1.0], F32))
    assert np.any(nodes["weight"].reshape(3, 15)[:, 1:] == 0)
    taken, avoided = se.zero_cover_visits(nodes, 3, 3, x, M)
    assert taken > 0 and avoided > 0, "rows take and do not take a zero-cover child"
    _, got = check_approx(env, nodes, 3, 3, 4, x, M, label="zero covers")
    assert np.all(np.isfinite(got))


# ---- b. leaf magnitude ----
def test_subnormal_deltas_are_not_flushed(env):
    ta, _ = env
    nodes, T, D, F, x, missing = se.leaf_case("subnormal")
    for output, bias in ((0, 0.0), (ta.OUT_AVG, 0.0)):
        want = ref.dense(nodes, T, D, F, x, missing, avg=output != 0)[..., :F]
        tiny = (want != 0) & (np.abs(want) < se.FLT_MIN)
        assert tiny.any(), "subnormal outputs in the reference"
        _, got = check_approx(env, nodes, T, D, F, x, missing, output=output, bias=bias, label=f"subnormal leaves out={output}")
        assert np.all(np.isfinite(got))
        assert np.all(got[..., :F][tiny] != 0), "a subnormal sum was flushed to zero"


def test_large_finite_leaves(env):
    nodes, T, D, F, x, missing = se.leaf_case("large")
    assert 2 * T * D * float(np.max(np.abs(se.reachable_leaves(nodes, T)))) < se.FLT_MAX
    _, got = check_approx(env, nodes, T, D, F, x, missing, label="leaves up to 1e37")
    assert np.all(np.isfinite(got))


def test_overflowing_deltas_are_ieee_results(env):
    """Leaves of +-3e38 and +-FLT_MAX: deltas round to +-inf, a row's sum to +-inf or NaN, exactly where the reference's do;
    the handle reports no error and serves the next call."""
    nodes, T, D, F, x, missing = se.leaf_case("overflow")
    want = ref.dense(nodes, T, D, F, x, missing)
    bad = ~np.isfinite(want[..., :F])
    assert 0.01 <= bad.mean() <= 0.99 and np.isnan(want).any()
    f, got = check_approx(env, nodes, T, D, F, x, missing, label="leaves up to FLT_MAX")
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    f.check()
    fin = np.isfinite(want).all(axis=(1, 2))
    assert fin.any(), "a row whose reference is finite, for the call that follows"
    after = gpu_approx(env, f, x[fin])
    assert np.all(np.isfinite(after)) and np.array_equal(bits(after), bits(want[fin]))
    f.check()


# ---- c. branch rule ----
@pytest.mark.parametrize("missing", list(se.MISSINGS))
def test_branch_rule_edges(env, missing):
    for seed in range(2):
        nodes, T, D, F, x, bg, m = se.edge_case(f"branch:{missing}", 100 + seed)
        internal = (nodes["bits"].view(np.uint32) >> 31) == 0
        assert np.any(~np.isfinite(nodes["val"][internal])), "NaN or infinite thresholds"
        _, got = check_approx(env, nodes, T, D, F, x, m, label=f"branch missing={missing} seed {seed}")
        assert np.all(np.isfinite(got))


@pytest.mark.parametrize("missing", list(se.MISSINGS))
def test_contradictory_bounds_and_nan_thresholds(env, missing):
    for seed in range(2):
        nodes, T, D, F, x, bg, m = se.edge_case(f"contradictory:{missing}", 7 + seed)
        x = np.concatenate([x, np.array([[6.0, 0.0], [4.0, 1.0], [F32(m), 0.0], [np.nan, F32(m)]], F32)])
        _, got = check_approx(env, nodes, T, D, F, x, m, label=f"contradictory missing={missing} seed {seed}")
        assert np.all(np.isfinite(got))


# ---- d. structure ----
def test_f1_stumps_one_accumulator(env):
    rng = np.random.default_rng(1)
    T = 64
    nodes = np.concatenate([se.stump(*se.cover_pair(rng, "mixed"), thr=F32(rng.choice(se.threshold_pool(0.5))),
                                     leaves=(rng.uniform(-2, 2), rng.uniform(-2, 2))) for _ in range(T)])
    x = se.random_data(rng, 70, 1, 0.5)
    check_approx(env, nodes, T, 1, 1, x, 0.5, label="F=1 stumps")


@pytest.mark.parametrize("D", [20, 21, 22])
def test_spine_distinct_features(env, D):
    F = 24
    rng = np.random.default_rng(D)
    fids = list(rng.permutation(F)[:D])
    nodes = np.concatenate([se.spine(D, fids, [F32(0.5)] * D), se.spine(D, fids[::-1], [F32(0.25)] * D, leaf0=-1.0)])
    x = se.random_data(rng, 20, F, M, pool=np.array([0.0, 0.3, 0.6, 1.0, M, np.nan], F32))
    turns = np.where(np.arange(D) % 2 == 0, 1.0, 0.0).astype(F32)  # the deep path: right at even levels, left at odd ones
    x[0, fids], x[1, fids[::-1]] = turns, turns
    _, S, N = ref.dense(nodes, 2, D, F, x, M, scale=True)
    assert N[0, 0] > D and N[1, 0] > D, f"rows 0 and 1 walk all {D} levels of one spine each"
    check_approx(env, nodes, 2, D, F, x, M, label=f"spine {D}")


def test_spine_three_features_merged(env):
    D = 21
    nodes = se.spine(D, [k % 3 for k in range(D)], [F32(v) for v in np.linspace(-1, 1, D)])
    rng = np.random.default_rng(3)
    x = se.random_data(rng, 40, 3, M, pool=np.concatenate([np.linspace(-1.1, 1.1, 23), [M, np.nan]]).astype(F32))
    check_approx(env, nodes, 1, D, 3, x, M, label="spine 3 features")


@pytest.mark.parametrize("T", [0, 5])
def test_no_walks(env, T):
    """Only root leaves (T = 5), or no trees: +0.0 contributions, the exact bias."""
    ta, _ = env
    D, F = 2, 3
    per = 2 ** (D + 1) - 1
    nodes = np.concatenate([se.encode(np.zeros(per), [F32(0.5 + t)] + [F32(9.0)] * (per - 1), np.zeros(per),
                                      np.full(per, F32(np.nan)), np.ones(per)) for t in range(T)]) if T else \
        np.empty(0, ta.capi.NODE_DTYPE)
    x = se.random_data(np.random.default_rng(T), 9, F, M)
    _, got = check_approx(env, nodes, T, D, F, x, M, bias=0.25, label=f"no walks T={T}")
    assert _all_plus_zero(got[..., :-1])


def test_multiclass_with_a_class_of_root_leaves(env):
    ta, _ = env
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
    _, got = check_approx(env, nodes, 6, D, F, x, M, num_classes=C, output=ta.OUT_AVG | ta.OUT_SOFTMAX, bias=0.375,
                          label="C=3, class 1 root leaves")
    assert _all_plus_zero(got[:, 1, :-1]) and np.any(got[:, 0, :-1] != 0) and np.any(got[:, 2, :-1] != 0)


# ---- e. form boundaries ----
# (LDS slab form?, waves per workgroup) at 160 KiB of LDS; see the comment on shap_edges.approx_form
APPROX_FORMS = {62: (True, 4), 63: (True, 3), 84: (True, 3), 85: (True, 2), 126: (True, 2), 127: (True, 1), 318: (True, 1),
                319: (False, 4)}


def _lds_bytes(env):
    n = ctypes.c_int()
    assert env[0].lib.tahoe_device_lds_bytes(ctypes.byref(n)) == 0
    return n.value


def _forest(env, F, seed, T=None):
    ta, _ = env
    rng = np.random.default_rng(seed)
    T = int(rng.integers(10, 21)) if T is None else T
    D = int(rng.integers(6, 8))
    nodes = ta.synth_forest(T, D, F, seed=seed, leaf_prob=0.05)
    nodes["weight"] = rng.uniform(0.05, 1.0, nodes.size).astype(F32)
    return nodes, T, D


def _rows(env, n, F):
    return env[0].synth_data(n, F, seed=F + n, missing_prob=0.02, missing=M, nan_prob=0.01)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("F", list(APPROX_FORMS))
def test_form_boundaries(env, F, C):
    ta, _ = env
    lds = _lds_bytes(env)
    assert lds == 160 * 1024
    slab, waves = se.approx_form(F, lds)
    assert (slab, waves) == APPROX_FORMS[F], f"F={F} gives the form {APPROX_FORMS[F]} by the rule in finish_build"
    nodes, T, D = _forest(env, F, 1300 + F, T=None if C == 1 else 12)
    output, bias = (0, 0.0) if C == 1 else (ta.OUT_AVG, 0.625)
    h = se.approx_handles(env, nodes, T, D, F, M, C, output, bias)
    assert all(f is not None for f in h.values())
    for n in (1, 64 * waves - 1, 64 * waves + 1, 128 * waves + 1):
        se.check_approx_batch(env, h, nodes, T, D, F, _rows(env, n, F), M, C, output, bias, label=f"F={F} C={C} rows={n}")
    for f in h.values():
        f.close()


# F: (TAHOE_APPROX_FORM, the form it gives, the unforced form); at 639 one wave's slab no longer fits and = 1 stays in place
FORCED_FORMS = {319: (1, (True, 1), (False, 4)), 638: (1, (True, 1), (False, 4)), 639: (1, (False, 4), (False, 4)),
                5: (2, (False, 4), (True, 4)), 62: (2, (False, 4), (True, 4))}


@pytest.mark.parametrize("F", list(FORCED_FORMS))
def test_forced_forms(env, no_forced_form, F):
    """TAHOE_APPROX_FORM at create: the bits of the unforced handle of the same forest, and the reference's."""
    ta, _ = env
    lds = _lds_bytes(env)
    forced, form, unforced = FORCED_FORMS[F]
    assert se.approx_form(F, lds, forced) == form and se.approx_form(F, lds) == unforced
    nodes, T, D = _forest(env, F, 1700 + F, T=12)
    for C, output, bias in ((1, 0, 0.0), (3, ta.OUT_AVG, -0.5)):
        kw = dict(missing=M, output=output, global_bias=bias, num_classes=C, approx_contribs=True)
        plain = ta.Forest(nodes, T, D, F, **kw)
        no_forced_form.setenv("TAHOE_APPROX_FORM", str(forced))
        pushed = ta.Forest(nodes, T, D, F, **kw)
        no_forced_form.delenv("TAHOE_APPROX_FORM")
        for n in (1, 63, 65, 257):
            x = _rows(env, n, F)
            got = gpu_approx(env, pushed, x)
            assert np.array_equal(bits(got), bits(gpu_approx(env, plain, x))), f"F={F} forced={forced} C={C} rows={n}"
            assert_same_bits(got, ref.dense(nodes, T, D, F, x, M, num_classes=C, avg=output != 0, global_bias=bias),
                             f"F={F} forced={forced} C={C} rows={n}: against the reference")
        plain.close()
        pushed.close()


# ---- f. sparse records ----
@pytest.mark.parametrize("mode", ["zero", "span", "subnormal", "mixed"])
def test_irregular_sparse_forests_with_extreme_covers(env, mode):
    ta, _ = env
    F, T = 24, 12
    rng = np.random.default_rng(len(mode))
    sn, tr = ta.capi.synth_sparse_forest(T, F, 4, 24, 0.3, 600, 800 + len(mode))
    ends = np.append(tr[1:], sn.size)
    cv = np.ones(sn.size, F32)
    for a, b in zip(tr, ends):
        for i in range(a, b):
            if sn["bits"][i] >= 0:  # an internal node: its children are a + left_idx and the node after it
                l = a + int(sn["left_idx"][i])
                cv[l], cv[l + 1] = se.cover_pair(rng, mode)
    assert int(np.max(ends - tr)) > 63, "trees of more than 63 nodes (deeper than a dense depth-5 tree)"
    x = ta.synth_data(150, F, seed=len(mode), missing_prob=0.05, missing=M, nan_prob=0.02)
    for C, out, bias in ((1, 0, 0.0), (3, ta.OUT_AVG, 0.125)):
        f = ta.capi.SparseForest(sn, tr, F, missing=M, covers=cv, num_classes=C, output=out, global_bias=bias,
                                 approx_contribs=True)
        want = ref.sparse(sn, tr, cv, F, x, M, num_classes=C, avg=bool(out), global_bias=bias)
        assert np.all(np.isfinite(want))
        got = gpu_approx(env, f, x)
        assert_same_bits(got, want, f"irregular covers={mode} C={C}")
        se.single_rows_match(lambda g, xx: gpu_approx(env, g, xx), f, x, got)
        f.close()


# ---- g. seeded sweep ----
@pytest.mark.parametrize("seed", range(30))
def test_seeded_sweep(env, seed):
    nodes, T, D, F, x, bg, m = se.edge_case("sweep", 1000 + seed)
    _, got = check_approx(env, nodes, T, D, F, x, m, label=f"sweep {seed}")
    assert np.all(np.isfinite(got))
