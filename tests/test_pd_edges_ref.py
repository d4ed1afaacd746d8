"""The conditions tests/test_pd_edges_gpu.py leans on, without a GPU: every ORDER_CASES forest is sensitive to the order of the
adds pd_sum_kernel makes, the hand-derived IEEE expectations are the bits of the float32 restatement (tests/pd_ref.py), the
restatement is within its bound of float64 on every finite case, and the structure cases give the bits of their plain twins.
An edit of tests/pd_edges.py that removes an edge fails here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pd_cases  # noqa: E402
import pd_edges as pe  # noqa: E402
import pd_ref  # noqa: E402

F32 = np.float32


def test_the_order_cases_reach_every_path_of_the_two_kernels():
    ct = sorted({T // C for T, C in pe.ORDER_CASES})
    assert {c // 16 for c in ct} == {0, 1, 2, 3}  # the block of 16 not at all, once, twice, three times
    assert {16, 32} <= set(ct)  # once and twice without a tail
    assert all(any(c // 16 == k and c % 16 for c in ct) for k in (1, 2, 3))  # once, twice and three times with one
    assert {T % 4 for T, _ in pe.ORDER_CASES} == {0, 1, 2, 3}  # the walk's last workgroup of four waves, full and partly filled
    assert {C for _, C in pe.ORDER_CASES} == {1, 3}
    assert pe.ORDER_G == 130  # three tiles of 64, the last partly filled
    assert all(T <= 100 for T, _ in pe.ORDER_CASES)


@pytest.mark.parametrize("T,C", pe.ORDER_CASES)
def test_order_sensitivity(T, C):
    """The float32 sum over a class's trees changes bits in at least a quarter of the outputs when the trees are added in
    reversed order; when the first two blocks of 16 are swapped (class_trees >= 32); when the tail is added before the blocks
    (class_trees % 16 != 0).  A kernel that gets the order wrong in one of these ways cannot match the restatement."""
    fo = pe.order_case(T, C)
    Tc = T // C
    assert pd_ref.shape_of(fo["nodes"], fo["trees"])[0] <= 3 and fo["grid"].shape == (130, 2)
    vals = pe.tree_values(fo, fo["targets"], fo["grid"])
    want = pe.want_f32(fo, fo["targets"], fo["grid"])
    nb = Tc // 16 * 16
    orders = {"reversed": list(range(Tc))[::-1]}
    if Tc >= 32:
        orders["blocks swapped"] = list(range(16, 32)) + list(range(16)) + list(range(32, Tc))
    if Tc % 16 and nb:  # (class_trees < 16 has no block: tail first is the specified order itself)
        orders["tail first"] = list(range(nb, Tc)) + list(range(nb))
    for name, order in orders.items():
        assert sorted(order) == list(range(Tc))
        changed = total = 0
        for c in range(C):
            cls = vals[c::C]
            assert np.array_equal(pe.bits(pe.ordered_sum(cls, range(Tc))), pe.bits(want[:, c]))  # the specified order
            changed += int((pe.bits(pe.ordered_sum(cls, order)) != pe.bits(want[:, c])).sum())
            total += cls.shape[1]
        print(f"T={T} C={C} {name}: {changed} of {total} outputs change bits ({100.0 * changed / total:.1f} %)")
        assert 4 * changed >= total, (name, changed, total)


def finite_cases():
    for T, C in pe.ORDER_CASES:
        yield pe.order_case(T, C)
    for name in pe.FINITE_IEEE:
        yield pe.IEEE_CASES[name]()
    for make in pe.STRUCTURE_CASES.values():
        yield make()
    yield pe.no_trees(1)
    yield pe.no_trees(3)


def test_restatement_matches_float64_on_every_finite_case():
    for case in finite_cases():
        for run, feats, grid in pe.runs(case):
            got = pe.want_f32(case, feats, grid)
            want, tol = pe.want_f64(case, feats, grid)
            assert np.isfinite(got).all() and (np.abs(got.astype(np.float64) - want) <= tol).all(), (case.get("id"), run)
    hf = pe.high_fid()
    for feats in hf["target_lists"]:
        got = pe.want_f32(hf, feats, hf["grid"])
        want, tol = pe.want_f64(hf, feats, hf["grid"])
        assert (np.abs(got.astype(np.float64) - want) <= tol).all()


@pytest.mark.parametrize("name", ["tiny_fraction", "subnormal_sum", "minus_zero"])
def test_hand_derived_bits_are_the_reference(name):
    case = pe.IEEE_CASES[name]()
    seen = 0
    for run, feats, grid in pe.runs(case):
        if run in case["expect"]:
            got = pe.bits(pe.want_f32(case, feats, grid))
            assert (got == case["expect"][run]).all(), (name, run, got)
            seen += 1
    assert seen >= 2


def test_tiny_fraction_is_subnormal():
    case = pe.tiny_fraction()
    cl, cr = case["covers"][1], case["covers"][2]
    fl = F32(cl) / (F32(cl) + F32(cr))
    assert fl != 0 and fl < F32(2.0 ** -126) and fl == F32(2.0 ** -140)
    assert pe.bits(F32(3.0 + 2.0 ** -20)) != pe.bits(F32(3.0))
    assert F32(2.0 ** -132) + F32(3 * 2.0 ** -142) == F32(131456 * 2.0 ** -149)  # subnormal_sum's arithmetic


def test_weight_underflow_by_hand():
    """Exactly 0.0f at level 30, nonzero at level 29; NaN with no split a target, +inf down the left spine."""
    case = pe.weight_underflow()
    nd, cv = case["nodes"], case["covers"]
    w, pos, ws = F32(1.0), 0, [F32(1.0)]
    for d in range(pe.UNDERFLOW_DEPTH):
        l = int(nd["left_idx"][pos])
        fl = cv[l] / (cv[l] + cv[l + 1])
        assert fl == F32(2.0 ** -5)
        w = w * fl
        ws.append(w)
        pos = l
    assert np.isposinf(nd["val"][pos]) and nd["bits"][pos] < 0
    assert ws[29] == F32(2.0 ** -145) and ws[29] != 0 and ws[30] == 0 and ws[32] == 0
    assert pd_ref.shape_of(nd, case["trees"])[0] == 32
    got = {run: pe.want_f32(case, feats, grid) for run, feats, grid in pe.runs(case)}
    assert np.isnan(got["none"]).all() and np.isnan(got["listed"]).all()
    assert np.isposinf(got["all"][0, 0]) and np.isfinite(got["all"][1:]).any()
    # the walk up to level 29 alone is finite: the NaN is the underflowed weight's, not an overflow's
    nd["val"][pos] = 1.0
    assert np.isfinite(pe.want_f32(case, [32], case["grid"])).all()


def test_inf_trees_and_the_mix():
    case = pe.inf_trees()
    got = pe.want_f32(case, [], np.zeros((2, 0), F32))
    assert np.isnan(got[:, 0]).all() and np.isposinf(got[:, 1]).all()
    mix = pe.ieee_mix()
    leaves = mix["nodes"]["val"][mix["nodes"]["bits"] < 0]
    for v in pe.MIX_LEAVES[:8]:  # every special value is some leaf
        assert (pe.bits(leaves) == pe.bits(v)).any(), v
    inner = mix["nodes"][mix["nodes"]["bits"] >= 0]
    assert pd_ref.shape_of(mix["nodes"], mix["trees"])[0] <= 3 and len(mix["trees"]) == 8
    cv = mix["covers"]
    assert np.isfinite(cv).all() and (cv >= 0).all() and inner.size
    sub = (cv > 0) & (cv < F32(2.0 ** -126))
    assert sub.any() and (cv == 0).any() and (cv > 1e30).any()  # subnormal, zero and huge covers are all there
    for run, feats, grid in pe.runs(mix):
        got = pe.want_f32(mix, feats, grid)
        print(run, "NaN", np.isnan(got).sum(0), "inf", np.isinf(got).sum(0), "0 < |v| < 2^-126", ((got != 0) & (np.abs(got) < 2.0 ** -126)).sum(0))
        assert (np.isnan(got) | np.isinf(got)).any()  # the special values arrive ...
        assert np.isfinite(got).any(0).sum() >= 2 and np.isfinite(got[:, 2]).all()  # ... and do not drown every class
        assert ((got[:, 2] != 0) & (np.abs(got[:, 2]) < 2.0 ** -125)).any()  # class 2 stays around the smallest normal number


@pytest.mark.parametrize("name", sorted(pe.TWINS))
def test_structure_cases_give_the_bits_of_their_twins(name):
    case, twin = pe.STRUCTURE_CASES[name](), pe.TWINS[name]()
    assert case["nodes"].size != twin["nodes"].size or not np.array_equal(case["nodes"], twin["nodes"])
    for (run, feats, grid), (_, feats2, grid2) in zip(pe.runs(case), pe.runs(twin)):
        if run == "all":  # the unreachable split's feature is no split of the twin: use the case's list on both
            feats2, grid2 = feats, grid
        assert np.array_equal(pe.bits(pe.want_f32(case, feats, grid)), pe.bits(pe.want_f32(twin, feats2, grid2))), (name, run)
    if name.startswith("prefix"):
        assert case["trees"][0] == 3 and np.isnan(case["covers"][:3]).all()
    else:
        n = case["nodes"][3]
        assert n["bits"] >= 0 and np.isnan(case["covers"][6]) and case["covers"][7] == -1
        assert 3 not in {int(case["nodes"]["left_idx"][i]) + k for i in (0, 1) for k in (0, 1)}  # nothing points to node 3


def test_the_other_structure_cases():
    for C in (1, 3):
        fo = pe.no_trees(C)
        got = pe.want_f32(fo, fo["targets"], fo["grid"])
        assert got.shape == (70, C) and not pe.bits(got).any()
    rl = pe.root_leaves()
    assert pe.want_f32(rl, [], np.zeros((1, 0), F32))[0, 0] == F32(0.5 + 1.5 + 2.5 + 3.5 + 4.5)
    sl = pe.stumps_and_leaves()
    depth = [int(sl["nodes"]["bits"][r] >= 0) for r in sl["trees"]]
    assert depth == [0, 1, 1, 0, 0, 1] and sl["num_classes"] == 2
    hf = pe.high_fid()
    assert hf["num_cols"] == 2 ** 29 + 2 and hf["nodes"]["bits"][0] == 2 ** 29 + 1
    for feats in hf["target_lists"]:
        assert np.array_equal(pe.bits(pe.want_f32(hf, feats, hf["grid"]))[:, 0], hf["expect"][tuple(feats)])


def test_same():
    a = np.array([1.0, np.nan, -0.0], F32)
    pos_nan = np.array([1.0, 0, -0.0], F32)
    pos_nan.view(np.uint32)[1] = 0x7FC00000
    assert pe.same(pos_nan, a) and pe.same(a, a)
    assert not pe.same(np.array([1.0, np.nan, 0.0], F32), a)  # the sign of zero counts
    assert not pe.same(np.array([1.0, 2.0, -0.0], F32), a)  # a number where a NaN belongs
    assert not pe.same(np.array([np.nan, np.nan, -0.0], F32), a)  # a NaN where a number belongs
    assert not pe.same(a[:2], a)
