"""Oblivious handles at the edges (tests/oblivious_edges.py): every ob_shap_tree<M, KB, INPLACE> of oblivious_shap.hip, extreme
leaf covers, the branch rule on IEEE thresholds and data under every `missing`, and Saabas deltas that overflow.  Needs an MI355X.

TreeSHAP is compared bit for bit with oblivious_shap_ref.emulate, a float32 restatement of the kernel's tables and recursion.
That the GPU gives those bits rests on how the library is built, not on a tolerance: no contraction (-ffp-contract=off in
tahoe_amd/csrc/Makefile, so a product and the sum that takes it round separately), float32 subnormals kept (the kernels' denorm
mode), a correctly rounded float division (hipcc's default, the one AVG division), no fast-math flag, and the sum order the
kernel's header fixes.  Under it the bar of tests/test_oblivious_shap_gpu.py against the float64 poly stays in force,
(N + 4 (D + 2)) 2^-24 A, with the floor of shap_edges.floor_term where covers reach the 2^-121 cut; the restatement alone uses
at most 0.14 of it (tests/test_oblivious_edges_capi.py prints the ratios), so the bar cannot see what the bits do.  Saabas, the
bias column, the walks and everything said to be bitwise compare bits (shap_edges.assert_same_bits: a NaN need only be a NaN
at the same place).  Every explanation call writes into the head of a buffer 256 rows longer whose tail must come back
untouched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_contribs_ref  # noqa: E402
import oblivious_edges as oe  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402
import shap_edges as se  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TAIL = 256
SENTINEL = 7.0
FORMS = [False, True]  # TAHOE_OBLIVIOUS_SHAP_INPLACE forced at create?


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


@pytest.fixture
def unforced(monkeypatch):
    monkeypatch.delenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", raising=False)
    return monkeypatch


def handle(env, c, knob=None, forced=False, **kw):
    """The case's oblivious handle; forced: created with TAHOE_OBLIVIOUS_SHAP_INPLACE=1 (knob = the unforced fixture)"""
    ta, _ = env
    forest = c["forest"]
    if forced:
        knob.setenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", "1")
    try:
        return ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"],
                                  forest["cols"], leaf_dim=forest["k"], missing=c["missing"], leaf_covers=c["covers"],
                                  output=ta.OUT_AVG if c["avg"] else 0, global_bias=c["bias"], **kw)
    finally:
        if forced:
            knob.delenv("TAHOE_OBLIVIOUS_SHAP_INPLACE", raising=False)


def expansion_nodes(c, covers=True):
    """-> (nodes, D) of the heap expansion: tree t * K + k carries class k's leaves; covers: the subtree covers as node weights"""
    forest = c["forest"]
    k, T = forest["k"], len(forest["depths"])
    per_class = [osr.expand_with_covers(forest, c["covers"], cls) if covers else obr.dense_of(forest, cls) for cls in range(k)]
    return np.stack([n.reshape(T, -1) for n, _ in per_class], axis=1).reshape(-1), per_class[0][1]


def expansion_handle(env, c, covers=True, **kw):
    ta, _ = env
    forest = c["forest"]
    nodes, D = expansion_nodes(c, covers)
    return ta.Forest(nodes, len(forest["depths"]) * forest["k"], D, forest["cols"], missing=c["missing"], num_classes=forest["k"],
                     output=ta.OUT_AVG if c["avg"] else 0, global_bias=c["bias"], **kw)


def run(env, f, call, x):
    """f.<call>(x) into the head of a longer buffer -> numpy [rows, K, F + 1]; the tail must stay as it was"""
    ta, torch = env
    rows, k, F1 = x.shape[0], f.num_classes, f.num_cols + 1
    shape = (rows + TAIL,) + ((k,) if k > 1 else ()) + (F1,)
    buf = torch.full(shape, SENTINEL, device="cuda")
    getattr(f, call)(x, out=buf[:rows])
    torch.cuda.synchronize()
    assert bool((buf[rows:] == SENTINEL).all()), f"{call} wrote past its {rows} rows"
    return buf[:rows].cpu().numpy().reshape(rows, k, F1)


def check_shap(env, knob, name, forced, batches=(1, 64), additive=False):
    """predict_contribs on the case in one form: the bits of emulate, the bar against poly (every output finite), the bias bits,
    the listed batch sizes against the head of the full batch, and with additive the sum against predict_raw"""
    ta, torch = env
    c = oe.reference(name)
    forest, data = c["forest"], c["data"]
    want, A, N = c["poly"]
    label = f"{name} {'in place' if forced else 'unforced'}"
    f = handle(env, c, knob, forced, contribs=True)
    x = torch.from_numpy(data.copy()).cuda()
    got32 = run(env, f, "predict_contribs", x)
    got = got32.astype(np.float64)
    assert np.all(np.isfinite(got32)), f"{label}: non-finite outputs at {np.argwhere(~np.isfinite(got32))[:5]}"
    bound, floor = oe.bar(c, A, N)
    assert np.all(floor <= 1e-30), f"{label}: the floor {floor.max():.3e} could mask a normal-range error"
    err, bound = np.abs(got - want)[:, :, :-1], bound[:, :, :-1]
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    differ = int((se.bits(got32) != se.bits(c["emulate"])).sum())
    print(f"{label}: max err / bound = {worst:.4f}; {differ} of {got32.size} outputs differ from emulate")
    se.assert_same_bits(got32, c["emulate"], f"{label}: against emulate")
    assert np.all(err <= bound), f"{label}: bound exceeded {worst:.3f}x at {np.argwhere(err > bound)[:5]}"
    b = osr.bias_f32(forest, c["covers"], c["avg"], c["bias"])
    assert np.array_equal(se.bits(got32[:, :, -1]), se.bits(np.broadcast_to(b, got32[:, :, -1].shape))), f"{label}: bias column"
    for r in batches:
        if r < data.shape[0]:
            assert np.array_equal(se.bits(run(env, f, "predict_contribs", x[:r].contiguous())), se.bits(got32[:r])), (label, r)
    if additive:
        T, F = len(forest["depths"]), forest["cols"]
        raw = f.predict_raw(x).cpu().numpy().astype(np.float64).reshape(data.shape[0], forest["k"])
        margin = (raw / T if c["avg"] and T else raw) + float(np.float32(c["bias"]))
        tol = bound.sum(axis=-1) + (T + 4) * U * (A.sum(axis=-1) + np.abs(margin)) + F * U * np.abs(got).sum(-1)
        assert np.all(np.abs(got.sum(axis=-1) - margin) <= tol), f"{label}: additivity"
    f.close()
    return got32, bound


# ------------------------------------------------------------------------------------------------ a: every element count
@pytest.mark.parametrize("forced", FORMS)
@pytest.mark.parametrize("name", oe.ELEMENT_CASES)
def test_treeshap_bits_for_every_element_count(env, unforced, name, forced):
    check_shap(env, unforced, name, forced)


@pytest.mark.parametrize("forced", FORMS)
@pytest.mark.parametrize("name", oe.MERGED_CASES)
def test_treeshap_bits_at_depth_16_on_repeated_features(env, unforced, name, forced):
    check_shap(env, unforced, name, forced, batches=(1,))


@pytest.mark.parametrize("forced", FORMS)
@pytest.mark.parametrize("name", oe.MULTI_CASES)
def test_treeshap_bits_across_trees_that_share_columns(env, unforced, name, forced):
    check_shap(env, unforced, name, forced, additive=True)


# ------------------------------------------------------------------------------------------------ b: covers
@pytest.mark.parametrize("forced", FORMS)
@pytest.mark.parametrize("name", oe.COVER_CASES)
def test_extreme_covers(env, unforced, name, forced):
    """Create accepts every pool (float32 subnormals, a float32 sum that overflows); TreeSHAP gives emulate's bits inside the bar
    with the floor, every output finite, and adds up to predict_raw; Saabas gives osr.saabas' bits; one bias for both"""
    ta, torch = env
    shap, _ = check_shap(env, unforced, name, forced, additive=True)
    c = oe.reference(name)
    f = handle(env, c, unforced, forced, approx_contribs=True)
    got = run(env, f, "predict_contribs_approx", torch.from_numpy(c["data"].copy()).cuda())
    se.assert_same_bits(got, c["saabas"], f"{name}: Saabas")
    assert np.array_equal(se.bits(got[:, :, -1]), se.bits(shap[:, :, -1])), f"{name}: the two bias columns"
    f.close()


@pytest.mark.parametrize("pool", oe.EXPANSION_POOLS)
def test_extreme_covers_against_the_heap_expansion(env, unforced, pool):
    """The dense handle on the heap expansion, its node weights the subtree covers.  Only oblivious_edges.EXPANSION_POOLS: in
    zero, most, subnormal, f32_overflow, cut and mixed a subtree cover is 0, subnormal or past FLT_MAX, and the expansion takes
    float32 node weights -- it cannot hold an overflowing sum, and a node of weight 0 does not mean there what a cover of 0 means
    here.  TreeSHAP: |native - expansion| <= the sum of the two handles' bars; the bias column bit for bit.

    Saabas bit for bit where the float32 node weights are the float64 subtree covers (int: sums below 2^24).  In span and
    near_one a subtree cover is rounded once more on its way into a float32 node weight, so the two handles are given different
    covers: each equals its own reference bit for bit (approx_contribs_ref.dense on the expansion; osr.saabas here), the two
    references differ in 193 and 201 of 1755 outputs, and the handles are held to what the rounding can do.  A node mean is
    nested weighted means of the leaves, D levels deep; a relative change of 2^-24 in every weight moves a level's mix by at
    most 2 2^-24 of the spread 2 L of its operands (L = max |leaf|), a node mean by 4 D 2^-24 L, a delta by twice that plus its
    own rounding 2 2^-24 L; a column sums n = sum of the depths such deltas at most, with (n + 1) 2^-24 of the sum of their
    magnitudes, <= 2 n L, as summation error on either side: |native - expansion| <= n (8 D + 2 + 4 (n + 1)) 2^-24 L."""
    ta, torch = env
    name = f"covers:{pool}"
    c = oe.reference(name)
    forest = c["forest"]
    D, F = oe.depth_of(forest), forest["cols"]
    want, A, N = c["poly"]
    x = torch.from_numpy(c["data"].copy()).cuda()
    f = handle(env, c, contribs=True, approx_contribs=True)
    g = expansion_handle(env, c, contribs=True, approx_contribs=True)
    mine, theirs = run(env, f, "predict_contribs", x), run(env, g, "predict_contribs", x)
    bound, _ = oe.bar(c, A, N)
    diff = np.abs(mine.astype(np.float64) - theirs)[:, :, :-1]
    print(f"{name}: max |native - expansion| / (2 bars) = {float((diff / np.where(bound > 0, 2 * bound, 1.0)[:, :, :-1]).max()):.4f}")
    assert np.all(diff <= 2 * bound[:, :, :-1]), f"{name}: TreeSHAP against the expansion"
    assert np.array_equal(se.bits(mine[:, :, -1]), se.bits(theirs[:, :, -1])), f"{name}: bias column against the expansion"
    mine, theirs = run(env, f, "predict_contribs_approx", x), run(env, g, "predict_contribs_approx", x)
    se.assert_same_bits(mine, c["saabas"], f"{name}: Saabas")
    assert np.array_equal(se.bits(mine[:, :, -1]), se.bits(theirs[:, :, -1])), f"{name}: Saabas bias column against the expansion"
    if pool == "int":
        se.assert_same_bits(mine, theirs, f"{name}: Saabas against the expansion")
    else:
        nodes, _ = expansion_nodes(c)
        own = approx_contribs_ref.dense(nodes, len(forest["depths"]) * forest["k"], D, F, c["data"], c["missing"], num_classes=forest["k"])
        se.assert_same_bits(theirs, own, f"{name}: the expansion's Saabas against its own reference")
        n, L = int(np.sum(forest["depths"])), float(np.abs(forest["leaves"]).max())
        tol = n * (8 * D + 2 + 4 * (n + 1)) * U * L
        diff = np.abs(mine.astype(np.float64) - theirs)[:, :, :F]
        print(f"{name}: Saabas, {int((se.bits(mine) != se.bits(theirs)).sum())} of {mine.size} outputs differ from the expansion's, "
              f"max {diff.max():.3e} of {tol:.3e}")
        assert np.all(diff <= tol), f"{name}: Saabas against the expansion"
    f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ c: the branch rule
@pytest.mark.parametrize("name", oe.BRANCH_CASES)
def test_the_branch_rule_in_every_walk(env, unforced, name):
    """oblivious_walk under DIRECT and ROWTILE, the dense walk on the expansion, the Saabas walk and ob_shap_leaf_index with its
    remapped split table (LDS form) and its plain one (in place): one rule, the reference's"""
    ta, torch = env
    c = oe.reference(name)
    forest, data, missing = c["forest"], c["data"], c["missing"]
    rows, k, T = data.shape[0], forest["k"], len(forest["depths"])
    want, want_leaf = obr.ref_of(forest, data, missing=missing)
    x = torch.from_numpy(data.copy()).cuda()
    f = handle(env, c, contribs=True, approx_contribs=True)
    for strat in ("DIRECT", "ROWTILE"):
        f.set_strategy(getattr(ta, "STRATEGY_" + strat))
        assert f.kernel_form(rows) == ("oblivious_direct" if strat == "DIRECT" else "oblivious_tile")
        leaf, sums = f.predict_leaf_idx(x)
        se.assert_same_bits(f.predict_raw(x).cpu().numpy(), want, f"{name} {strat}: predict_raw")
        se.assert_same_bits(sums.cpu().numpy(), want, f"{name} {strat}: predict_leaf_idx sums")
        assert np.array_equal(leaf.cpu().numpy().view(np.uint32), want_leaf), f"{name} {strat}: leaf indices"
    g = expansion_handle(env, c, covers=False)
    leaf, sums = g.predict_leaf_idx(x)
    se.assert_same_bits(g.predict_raw(x).cpu().numpy(), want, f"{name}: the expansion's predict_raw")
    se.assert_same_bits(sums.cpu().numpy(), want, f"{name}: the expansion's predict_leaf_idx sums")
    heap_leaf = leaf.cpu().numpy().view(np.uint32).reshape(rows, T, k)
    for cls in range(k):
        assert np.array_equal(obr.heap_leaf_to_oblivious(heap_leaf[:, :, cls], forest["depths"]), want_leaf), (name, cls)
    g.close()
    se.assert_same_bits(run(env, f, "predict_contribs_approx", x), c["saabas"], f"{name}: Saabas")
    f.close()
    for forced in FORMS:
        check_shap(env, unforced, name, forced, batches=(1, 64), additive=True)


# ------------------------------------------------------------------------------------------------ d: Saabas overflow
@pytest.mark.parametrize("forced", FORMS)
def test_saabas_deltas_that_overflow(env, unforced, forced):
    """Leaves of +-3e38 and +-1e38: a float32 delta is +-inf, a column that adds both signs is NaN -- where the reference's is"""
    ta, torch = env
    c = oe.reference(oe.LEAF_CASE, shap=False)
    want = c["saabas"]
    assert np.isinf(want).any() and np.isnan(want).any()
    f = handle(env, c, unforced, forced, approx_contribs=True)
    x = torch.from_numpy(c["data"].copy()).cuda()
    got = run(env, f, "predict_contribs_approx", x)
    se.assert_same_bits(got, want, "overflowing leaves: Saabas")
    se.assert_same_bits(got[:, :, -1], np.broadcast_to(osr.bias_f32(c["forest"], c["covers"]), got[:, :, -1].shape),
                        "overflowing leaves: bias column")
    for r in (1, 64):
        se.assert_same_bits(run(env, f, "predict_contribs_approx", x[:r].contiguous()), want[:r], f"overflowing leaves: {r} rows")
    f.close()
