"""The references of the vector-leaf TreeSHAP tests agree with each other (no GPU): the float64 brute force of
tests/sparse_shap_ref.py on the K-fold expansion, class k, against the direct evaluation of tests/vector_shap_ref.py on the vector
forest, bias column included -- so the GPU tests may use either -- and the named forests have the shapes the GPU tests rely on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sparse_shap_ref as ssr  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402

X_ROWS = 5  # both routes are vectorised over the rows; the expansion route costs 2^cols x T x K tree walks whatever their number


@pytest.mark.parametrize("name", vsr.SMALL)
def test_expansion_route_equals_the_direct_route(name):
    forest, data, covers = vsr.case(name)
    K, F = forest["k"], forest["cols"]
    assert F <= 8
    x = data[:X_ROWS]
    sn, tr = vr.expand(forest)
    for label, cv in covers.items():
        tiled = vsr.tile_covers(forest, cv)
        assert tiled.size == sn.size
        # (AVG and the bias only scale and shift what both routes computed: one evaluation each, with both set)
        want = ssr.contribs(sn, tr, tiled, x, F, vsr.MISSING, K, True, 0.375)
        got = vsr.contribs(forest, cv, x, avg=True, global_bias=0.375)
        assert got.shape == want.shape == (X_ROWS, K, F + 1)
        scale = np.abs(want).max() if want.size else 0.0
        assert np.all(np.abs(got - want) <= 1e-12 * scale), (name, label)
        for avg, bias in ((False, 0.0), (True, 0.375)):
            b_exp = ssr.bias_column(sn, tr, tiled, K, avg, bias)
            b_vec = vsr.bias_column(forest, cv, avg, bias)
            assert np.array_equal(b_exp.view(np.uint32), b_vec.view(np.uint32)), (name, label, avg)
        if forest["trees"].size:  # the float32 bias column is the brute force's, rounded
            assert np.allclose(b_vec, got[0, :, F], rtol=1e-6, atol=1e-6 * (scale + 1.0)), (name, label)


def test_covers_are_what_their_names_say():
    forest, _, covers = vsr.case("nine_k17")
    nodes, trees = forest["nodes"], forest["trees"]
    bounds = list(trees) + [nodes.size]
    cons, unrel = covers["consistent"], covers["unrelated"]
    assert (cons > 0).all() and (unrel > 0).all() and cons.dtype == unrel.dtype == np.float32
    off = 0
    for t in range(trees.size):
        lo, hi = int(bounds[t]), int(bounds[t + 1])
        for i in range(lo, hi):
            if nodes["bits"][i] >= 0:
                li = lo + int(nodes["left_idx"][i])
                assert cons[i] == np.float32(float(cons[li]) + float(cons[li + 1])) or abs(
                    float(cons[i]) - float(cons[li]) - float(cons[li + 1])) <= 2e-7 * float(cons[i])
                off += abs(float(unrel[i]) - float(unrel[li]) - float(unrel[li + 1])) > 1e-3
    assert off > 0  # the second generator is not consistent
    tiled = vsr.tile_covers(forest, cons)
    sn, tr = vr.expand(forest)
    assert tiled.size == sn.size
    k = forest["k"]
    for t in (0, trees.size - 1):
        for c in (0, k - 1):
            r = int(tr[t * k + c])
            assert np.array_equal(tiled[r:r + int(bounds[t + 1]) - int(bounds[t])], cons[int(bounds[t]):int(bounds[t + 1])])


def test_named_forests_have_the_shapes_the_gpu_tests_rely_on():
    # repeat_k3: repeated features merged (no path longer than its 5 features), several paths per bin, rounds > 1
    forest, _, _ = vsr.case("repeat_k3")
    assert forest["cols"] == 5 and forest["k"] == 3 and forest["trees"].size == 1
    ps, bs = vsr.paths(forest), vsr.bins(forest)
    assert len(ps) >= 20 and max(len(p) for p in ps) <= 5 and all(len(set(p)) == len(p) for p in ps)
    assert any(rounds > 1 for _, rounds in bs)
    assert any(len(b) >= 2 and any(len(p) >= 2 for p in b) for b, _ in bs)  # a path of >= 2 elements shares its bin
    # more than one bin per wave somewhere: more than 4 bins in a forest of the plain list
    assert max(len(vsr.bins(vsr.case(n)[0])) for n in vsr.NAMES) > 4
    # K on both sides of the 8-class block, and K == 1
    ks = {vsr.case(n)[0]["k"] for n in vsr.NAMES}
    assert 1 in ks and any(1 < k < 8 for k in ks) and 8 in ks and any(8 < k <= 16 for k in ks) and any(k > 16 for k in ks)
    # wide_k9: 700 columns, K = 9
    forest, data, _ = vsr.case("wide_k9")
    assert forest["cols"] == 700 and forest["k"] == 9 and forest["trees"].size == 3 and data.shape == (vsr.ROWS, 700)
    # zero_side_k3 / tiny_ratio_k3: the covers the issue names
    forest, _, covers = vsr.case("zero_side_k3")
    assert list(covers["fixed"]) == [1.0, 0.0, 1.0] and forest["nodes"]["bits"][0] >= 0 and (forest["nodes"]["bits"][1:] < 0).all()
    forest, _, covers = vsr.case("tiny_ratio_k3")
    cv = covers["fixed"].astype(np.float64)
    assert 0 < cv[1] / (cv[1] + cv[2]) < 2.0 ** -121 and 0 < cv[3] / (cv[3] + cv[4]) < 2.0 ** -121
    # a root-leaf tree is in the list
    assert any((vsr.case(n)[0]["nodes"]["bits"][vsr.case(n)[0]["trees"]] < 0).any() for n in vsr.NAMES if vsr.case(n)[0]["trees"].size)
