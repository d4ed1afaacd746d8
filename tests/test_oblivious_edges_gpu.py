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
untouched.

SHAP interaction values (oblivious_inter_kernel, ob_inter_tree<M, KB>) on the same cases and on the inter:* ones: check_inter
holds predict_interactions to the bits of oblivious_inter_ref.emulate, to oblivious_edges.inter_bar of the float64 poly off the
diagonal, to the matrix's structure, and to oblivious_shap_ref.poly's phi in its row sums."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import approx_contribs_ref  # noqa: E402
import interactions_ref  # noqa: E402
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


def run(env, f, call, x, dims=1, shift=0):
    """f.<call>(x) into the head of a longer buffer -> numpy [rows, K, (F + 1) x dims]; the tail must stay as it was.  shift: the
    output starts that many floats past the buffer's (16-byte aligned) start, and the floats before it must stay too"""
    ta, torch = env
    rows, k, F1 = x.shape[0], f.num_classes, f.num_cols + 1
    shape = (rows,) + ((k,) if k > 1 else ()) + (F1,) * dims
    n = int(np.prod(shape))
    buf = torch.full((shift + (n // max(rows, 1)) * (rows + TAIL),), SENTINEL, device="cuda")
    assert buf.data_ptr() % 16 == 0
    getattr(f, call)(x, out=buf[shift:shift + n].view(shape))
    torch.cuda.synchronize()
    assert bool((buf[shift + n:] == SENTINEL).all()) and bool((buf[:shift] == SENTINEL).all()), f"{call} wrote past its {rows} rows"
    return buf[shift:shift + n].cpu().numpy().reshape((rows, k) + (F1,) * dims)


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


def check_inter(env, knob, name, forced=False):
    """predict_interactions on the case (its first oe.inter_rows rows), the handle created in one form:
      bits       emulate's; where leaves overflow a NaN need only be a NaN at the same place, and everywhere else no entry is
                 non-finite
      bar        inside oe.inter_bar of poly off the diagonal, where the case has a poly (on the finite entries)
      structure  bitwise symmetric; row and column F zero but for [F][F], the bias bits; unused columns all-zero bits; the
                 diagonal = predict_contribs of a contribs=True handle minus the float32 sum of the row's off-diagonals, j
                 ascending from +0.0f
      row sums   sum_j Phi[i][j] in float64 against oblivious_shap_ref.poly's phi_i within the sum of the two bars: the
                 off-diagonals cancel against the diagonal up to the float32 sum and the subtraction that made it (at most U u
                 sum_j |Phi_ij| for U used columns, inside the interaction bars of the row, whose n >= 6 (D + 2) exceeds U in
                 every case here), which leaves the error of phi_i itself, TreeSHAP's bar.  It leans on neither emulate nor the
                 kernel's order.
    -> (got, worst err / bound or None)"""
    ta, torch = env
    c = oe.inter_reference(name)
    forest, data, emu = c["forest"], c["data"], c["emulate"]
    rows, F = data.shape[0], forest["cols"]
    overflow = name == oe.LEAF_CASE
    label = f"{name} interactions{' in place' if forced else ''}"
    f = handle(env, c, knob, forced, interactions=True)
    x = torch.from_numpy(data.copy()).cuda()
    got = run(env, f, "predict_interactions", x, dims=2)
    f.close()
    finite = np.isfinite(got)
    assert overflow or finite.all(), f"{label}: non-finite outputs at {np.argwhere(~finite)[:5]}"
    differ = int(((se.bits(got) != se.bits(emu)) & ~(np.isnan(got) & np.isnan(emu))).sum())
    eye = np.eye(F + 1, dtype=bool)
    worst = None
    if c["poly"] is not None:
        want, A, N = c["poly"]
        bound, floor = oe.inter_bar(c, A, N)
        assert np.all(floor <= 1e-30), f"{label}: the floor {floor.max():.3e} could mask a normal-range error"
        err, off = np.abs(got.astype(np.float64) - want), ~eye & finite
        worst = float((err / np.where(bound > 0, bound, 1.0))[off].max()) if off.any() else 0.0
    print(f"{label}: max err / bound = {'none' if worst is None else format(worst, '.4f')}; {differ} of {got.size} outputs differ "
          f"from emulate")
    se.assert_same_bits(got, emu, f"{label}: against emulate")
    if worst is not None:
        assert np.all(err[off] <= bound[off]), f"{label}: bound exceeded {worst:.3f}x at {np.argwhere(off & (err > bound))[:5]}"
    # structure
    assert np.array_equal(se.bits(got), se.bits(got.swapaxes(-1, -2))), f"{label}: not symmetric"
    b = osr.bias_f32(forest, c["covers"], c["avg"], c["bias"])
    assert np.array_equal(se.bits(got[:, :, F, F]), se.bits(np.broadcast_to(b, got.shape[:2]))), f"{label}: bias corner"
    assert not se.bits(got[:, :, F, :F]).any() and not se.bits(got[:, :, :F, F]).any(), f"{label}: row / column F"
    used = np.unique(forest["fids"]).astype(np.int64)
    unused = np.setdiff1d(np.arange(F), used)
    assert not se.bits(got[:, :, unused, :]).any() and not se.bits(got[:, :, :, unused]).any(), f"{label}: unused columns"
    g = handle(env, c, knob, forced, contribs=True)
    phi = run(env, g, "predict_contribs", x)
    g.close()
    diag = np.zeros(got.shape[:2] + (F,), np.float32)
    with np.errstate(all="ignore"):
        for i in used:
            s = np.zeros(got.shape[:2], np.float32)
            for j in range(F):
                if j != i:
                    s = s + got[:, :, i, j]
            diag[:, :, i] = phi[:, :, i] - s
    idx = np.arange(F)
    se.assert_same_bits(got[:, :, idx, idx], diag, f"{label}: diagonal")
    # row sums
    if worst is not None:
        with np.errstate(all="ignore"):
            shap = oe.reference(name)
        want_phi, A1, N1 = (a[:rows] for a in shap["poly"])
        tol = oe.bar(c, A1, N1)[0][:, :, :F] + np.where(eye, 0.0, bound)[:, :, :F, :F].sum(axis=-1)
        whole = finite[:, :, :F, :F].all(axis=-1)
        with np.errstate(invalid="ignore"):
            miss = np.abs(got.astype(np.float64)[:, :, :F, :F].sum(axis=-1) - want_phi[:, :, :F])
        assert np.all(miss[whole] <= tol[whole]), f"{label}: row sums, {float((miss / np.where(tol > 0, tol, 1.0))[whole].max()):.3f}x"
    return got, worst


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
    remapped split table (LDS form), its plain one (in place) and the interaction kernel's copy: one rule, the reference's"""
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
    check_inter(env, unforced, name)  # ob_shap_leaf_index on the column split table of oblivious_inter_kernel


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


# ------------------------------------------------------------------------------------------------ e: interaction values
@pytest.mark.parametrize("name", oe.ELEMENT_CASES)
def test_interaction_bits_for_every_element_count(env, unforced, name):
    """ob_inter_tree<M, 1> and <M, 4> for M = 2 .. 16 (M = 1: no pair), with a full and a partial class block"""
    check_inter(env, unforced, name)


@pytest.mark.parametrize("name", oe.MERGED_CASES)
def test_interaction_bits_at_depth_16_on_repeated_features(env, unforced, name):
    check_inter(env, unforced, name)


@pytest.mark.parametrize("name", oe.MULTI_CASES + ["inter:k4"])
def test_interaction_bits_across_trees_that_share_columns(env, unforced, name):
    got, _ = check_inter(env, unforced, name)
    assert np.abs(got[:, :, :-1, :-1]).max() > 0


@pytest.mark.parametrize("name", oe.COVER_CASES)
def test_interactions_under_extreme_covers(env, unforced, name):
    check_inter(env, unforced, name)


@pytest.mark.parametrize("pool", oe.EXPANSION_POOLS)
def test_interactions_against_the_heap_expansion(env, unforced, pool):
    """The dense handle on the heap expansion with the subtree covers as node weights (the pools that allow it): the two
    handles' off-diagonals within the sum of their bars -- inter_bar here, tests/test_interactions_gpu.py's
    (N + 6 (D + 2)) 2^-24 A of interactions_ref.poly there -- and the bias corner bit for bit"""
    ta, torch = env
    name = f"covers:{pool}"
    c = oe.inter_reference(name)
    forest = c["forest"]
    F, k, T = forest["cols"], forest["k"], len(forest["depths"])
    nodes, D = expansion_nodes(c)
    _, Ad, Nd = interactions_ref.poly(nodes, T * k, D, F, c["data"], c["missing"], num_classes=k)
    f = handle(env, c, interactions=True)
    g = expansion_handle(env, c, contribs=True)
    x = torch.from_numpy(c["data"].copy()).cuda()
    mine, theirs = run(env, f, "predict_interactions", x, dims=2), run(env, g, "predict_interactions", x, dims=2)
    f.close()
    g.close()
    _, A, N = c["poly"]
    bound = oe.inter_bar(c, A, N)[0] + (Nd[None] + 6 * (D + 2)) * U * Ad
    off = ~np.eye(F + 1, dtype=bool)
    err = np.abs(mine.astype(np.float64) - theirs.astype(np.float64))
    worst = float((err / np.where(bound > 0, bound, 1.0))[..., off].max())
    print(f"{name}: max |native - expansion| / (the two bars) = {worst:.4f}")
    assert np.abs(theirs[..., off]).max() > 0 and np.all(err[..., off] <= bound[..., off]), f"{name}: {worst:.3f}x"
    assert np.array_equal(se.bits(mine[:, :, F, F]), se.bits(theirs[:, :, F, F])), f"{name}: bias corner against the expansion"


def test_interactions_with_leaves_near_flt_max(env, unforced):
    """Terms and sums that overflow: +-inf with emulate's bits, NaN where emulate's is, the rest inside the bar"""
    got, _ = check_inter(env, unforced, oe.LEAF_CASE)
    assert np.isnan(got).any() or np.isinf(got).any()
    assert np.isfinite(got[:, :, :-1, :-1]).any()


@pytest.mark.parametrize("name", oe.INTER_ONLY_CASES)
def test_interaction_only_cases(env, unforced, name):
    """No tree, no used feature, 3 used columns of 300 (K 301^2 floats zeroed per row, size_t indexing), a single column, one
    full class block.  The wide cases also as one row and as a 64-row batch, and with output and data both starting one float
    past a 16-byte boundary: the same bits"""
    ta, torch = env
    got, _ = check_inter(env, unforced, name)
    c = oe.inter_reference(name)
    F = c["forest"]["cols"]
    if name.startswith("inter:none") or name == "inter:one_col":
        rest = got.copy()
        rest[:, :, F, F] = 0
        rest[:, :, np.arange(F), np.arange(F)] = 0
        assert not se.bits(rest).any(), f"{name}: an off-diagonal entry is set"
        assert name == "inter:one_col" or not se.bits(got[:, :, :F, :F]).any()
    if name.startswith("inter:wide"):
        f = handle(env, c, interactions=True)
        x = torch.from_numpy(c["data"].copy()).cuda()
        for r in (1, 64):
            part = run(env, f, "predict_interactions", x[:r].contiguous(), dims=2)
            assert np.array_equal(se.bits(part), se.bits(got[:r])), (name, r)
        assert np.array_equal(se.bits(run(env, f, "predict_interactions", x[64:65].clone(), dims=2)), se.bits(got[64:65])), name
        flat = torch.full((x.numel() + 1,), SENTINEL, device="cuda")
        assert flat.data_ptr() % 16 == 0
        flat[1:] = x.reshape(-1)
        shifted = run(env, f, "predict_interactions", flat[1:].view(x.shape), dims=2, shift=1)
        assert np.array_equal(se.bits(shifted), se.bits(got)), f"{name}: misaligned output and data"
        f.close()


@pytest.mark.parametrize("name", ["multi:sum", "covers:mixed"])
def test_one_handle_serves_contribs_and_interactions_in_both_forms(env, unforced, name):
    """contribs=True, interactions=True: TreeSHAP reads compact ids (LDS form) or columns (in place), the interaction kernel its
    own column tables in either.  predict_interactions gives emulate's bits in both forms, those of the interactions-only
    handle; predict_contribs on the same handle keeps the bits of the contribs-only handle of its form"""
    ta, torch = env
    c = oe.inter_reference(name)
    shap = oe.reference(name)
    x = torch.from_numpy(c["data"].copy()).cuda()
    only = handle(env, c, interactions=True)
    want = run(env, only, "predict_interactions", x, dims=2)
    only.close()
    se.assert_same_bits(want, c["emulate"], f"{name}: the interactions-only handle against emulate")
    for forced in FORMS:
        label = f"{name} {'in place' if forced else 'unforced'}"
        both = handle(env, c, unforced, forced, contribs=True, interactions=True)
        alone = handle(env, c, unforced, forced, contribs=True)
        for _ in range(2):  # (the two calls do not disturb each other's tables)
            assert np.array_equal(se.bits(run(env, both, "predict_interactions", x, dims=2)), se.bits(want)), f"{label}: interactions"
            phi = run(env, both, "predict_contribs", x)
            assert np.array_equal(se.bits(phi), se.bits(run(env, alone, "predict_contribs", x))), f"{label}: contribs"
            se.assert_same_bits(phi, shap["emulate"], f"{label}: contribs against emulate")
        both.close()
        alone.close()
