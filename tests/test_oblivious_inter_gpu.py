"""SHAP interaction values on oblivious handles (tahoe_oblivious_forest_create_ex with TAHOE_CREATE_INTERACTIONS) against
tests/oblivious_inter_ref.py and against the heap expansion on dense handles.  Needs an MI355X.

The bits are specified: every result equals oblivious_inter_ref.emulate, the kernel restated in float32.  Beside that the
off-diagonal bar of tests/test_interactions_gpu.py for the same recursions: |got - poly| <= (N + 6 (D + 2)) 2^-24 A per entry,
N float32 adds of terms whose absolute values sum to A, each term carrying the rounding of a conditioned extend / unwind of at
most D + 1 steps.  Every call writes into the head of a buffer 256 rows longer whose tail must come back untouched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interactions_ref  # noqa: E402
import oblivious_inter_ref as oir  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = obr.MISSING
INVALID_ARG, UNSUPPORTED = 1, 7
U = 2.0 ** -24
ROWS = 129
TAIL = 256
SENTINEL = 7.0
MIXED = [0, 1, 2, 6, 3, 6, 4]  # depths; on 5 columns the features repeat within a tree
_cache = {}


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def handle(ta, forest, covers=None, **kw):
    return ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], forest["cols"],
                              leaf_dim=forest["k"], missing=MISSING, leaf_covers=covers, **kw)


def run(env, f, x, call="predict_interactions", dims=2):
    """f.<call>(x) into the head of a longer buffer -> numpy [rows, K, (F + 1) x dims]; the tail must stay as it was"""
    ta, torch = env
    rows, k, F1 = x.shape[0], f.num_classes, f.num_cols + 1
    shape = (rows + TAIL,) + ((k,) if k > 1 else ()) + (F1,) * dims
    buf = torch.full(shape, SENTINEL, device="cuda")
    getattr(f, call)(x, out=buf[:rows])
    torch.cuda.synchronize()
    assert bool((buf[rows:] == SENTINEL).all()), f"{call} wrote past its {rows} rows"
    return buf[:rows].cpu().numpy().reshape((rows, k) + (F1,) * dims)


def case(name, depths, cols, k, kind, rows=ROWS, avg=False, bias=0.0, fids=None, spread=None, poly=True):
    """(forest, covers, data, poly's (Phi, A, N) or None, emulate's Phi), computed once and read-only.  spread: the forest is made
    on len(spread) columns and its feature c becomes column spread[c] of `cols`, so that some columns stay unused."""
    if name not in _cache:
        forest = obr.make_forest(depths, cols if spread is None else len(spread), k, seed=3000 + len(name))
        if fids is not None:
            forest["fids"][:] = fids
        if spread is not None:
            forest["fids"][:] = np.asarray(spread)[np.asarray(forest["fids"])]
            forest["cols"] = cols
        covers = osr.make_covers(forest, kind, seed=41 + len(name))
        data = obr.make_data(rows, cols, seed=19 + cols)
        ref = oir.poly(forest, covers, data, avg=avg, global_bias=bias) if poly else None
        emu = oir.emulate(forest, covers, data, avg=avg, global_bias=bias)
        for a in (covers, data, emu) + (ref or ()):
            a.setflags(write=False)
        _cache[name] = (forest, covers, data, ref, emu)
    return _cache[name]


def check(env, name, **spec):
    """predict_interactions on the case: emulate's bits, the bar, symmetry, the diagonal from predict_contribs, corner and zeroes"""
    ta, torch = env
    avg, bias = spec.get("avg", False), spec.get("bias", 0.0)
    forest, covers, data, ref, emu = case(name, **spec)
    D, F = int(max(forest["depths"], default=0)), forest["cols"]
    kw = dict(output=ta.OUT_AVG if avg else 0, global_bias=bias)
    f = handle(ta, forest, covers, interactions=True, **kw)
    x = torch.from_numpy(data.copy()).cuda()
    got = run(env, f, x)
    f.close()
    off = ~np.eye(F + 1, dtype=bool)
    if ref is not None:
        want, A, N = ref
        err, bound = np.abs(got.astype(np.float64) - want)[..., off], ((N + 6 * (D + 2)) * U * A)[..., off]
        worst = float((err / np.where(bound > 0, bound, 1.0)).max())
        print(f"{name}: max err / bound = {worst:.3f}")
        assert np.all(err <= bound), f"{name}: bound exceeded {worst:.3f}x at {np.argwhere(err > bound)[:5]}"
    diff = np.argwhere(bits(got) != bits(emu))
    assert diff.size == 0, f"{name}: {len(diff)} entries differ from emulate, first {diff[:5]}"
    assert np.array_equal(bits(got), bits(got.swapaxes(-1, -2))), f"{name}: not symmetric"
    # the diagonal: phi_i of a CONTRIBS handle minus the float32 sum of the row's off-diagonals, j ascending from +0.0f
    g = handle(ta, forest, covers, contribs=True, **kw)
    phi = run(env, g, x, "predict_contribs", dims=1)
    g.close()
    used = np.unique(forest["fids"])
    diag = np.zeros(got.shape[:2] + (F,), np.float32)
    for i in used:
        s = np.zeros(got.shape[:2], np.float32)
        for j in range(F):
            if j != i:
                s = s + got[:, :, i, j]
        diag[:, :, i] = phi[:, :, i] - s
    idx = np.arange(F)
    assert np.array_equal(bits(got[:, :, idx, idx]), bits(diag)), f"{name}: diagonal"
    b = emu[0, :, F, F]  # oblivious_shap_ref.bias_f32, which emulate puts there (computed once: it walks the leaves one by one)
    assert np.array_equal(bits(got[:, :, F, F]), bits(np.broadcast_to(b, got.shape[:2]))), f"{name}: bias corner"
    assert not bits(got[:, :, F, :F]).any() and not bits(got[:, :, :F, F]).any(), f"{name}: row / column F"
    unused = np.setdiff1d(np.arange(F), used)
    assert not bits(got[:, :, unused, :]).any() and not bits(got[:, :, :, unused]).any(), f"{name}: unused columns"
    return got


# ------------------------------------------------------------------------------------------------ against emulate and poly
@pytest.mark.parametrize("kind", ["int", "half", "most", "zero"])
@pytest.mark.parametrize("k", [1, 3, 9])
def test_mixed_depths(env, k, kind):
    check(env, f"mixed_{kind}_k{k}", depths=MIXED, cols=5, k=k, kind=kind)


def test_avg_global_bias_and_unused_columns(env):
    got = check(env, "mixed_avg", depths=MIXED, cols=7, k=3, kind="half", avg=True, bias=-0.375, spread=[6, 0, 3, 4, 2])
    assert np.abs(got[:, :, :7, :7]).max() > 0


def test_every_number_of_distinct_features_once(env):
    """Trees of depths 1 .. 16, tree d on d distinct features of 16 columns: m = 1 .. 16, every instantiation"""
    rng = np.random.default_rng(16)
    fids = np.concatenate([rng.permutation(16)[:d] for d in range(1, 17)])
    check(env, "every_m", depths=list(range(1, 17)), cols=16, k=1, kind="half", rows=3, fids=fids, poly=False)


def test_depth_16_on_four_repeated_features(env):
    check(env, "deep16", depths=[16], cols=4, k=1, kind="half", rows=5, fids=np.arange(16) % 4, poly=False)


# ------------------------------------------------------------------------------------------------ bitwise
def test_repeats_batches_rows_alone_and_permutations_give_the_same_bits(env):
    ta, torch = env
    forest, covers, data, _, emu = case("mixed_int_k3", depths=MIXED, cols=5, k=3, kind="int")
    f = handle(ta, forest, covers, interactions=True)
    x = torch.from_numpy(data.copy()).cuda()
    first = run(env, f, x)
    assert np.array_equal(bits(first), bits(emu))
    assert np.array_equal(bits(first), bits(run(env, f, x)))
    for r in (1, 63, 64, 65):
        assert np.array_equal(bits(run(env, f, x[:r].contiguous())), bits(first[:r])), r
    for r in (0, 63, 64, ROWS - 1):
        assert np.array_equal(bits(run(env, f, x[r:r + 1].clone())), bits(first[r:r + 1])), r
    perm = np.random.default_rng(5).permutation(ROWS)
    assert np.array_equal(bits(run(env, f, x[torch.from_numpy(perm).cuda()].contiguous())), bits(first[perm]))
    f.close()


# ------------------------------------------------------------------------------------------------ against the library
@pytest.mark.parametrize("k", [1, 3])
def test_the_heap_expansion_on_a_dense_handle_agrees(env, k):
    ta, torch = env
    forest, covers, data, (want, A, N), _ = case(f"mixed_int_k{k}", depths=MIXED, cols=5, k=k, kind="int")
    T, D, F = len(forest["depths"]), max(MIXED), forest["cols"]
    per_class = [oir.expand(forest, covers, c) for c in range(k)]
    nodes = np.stack([n.reshape(T, -1) for n, _ in per_class], axis=1).reshape(-1)
    _, Ad, Nd = interactions_ref.poly(nodes, T * k, D, F, data, MISSING, num_classes=k)
    f = handle(ta, forest, covers, interactions=True)
    g = ta.Forest(nodes, T * k, D, F, missing=MISSING, num_classes=k, contribs=True)
    x = torch.from_numpy(data.copy()).cuda()
    mine, theirs = run(env, f, x), run(env, g, x)
    off = ~np.eye(F + 1, dtype=bool)
    bound = (N + 6 * (D + 2)) * U * A + (Nd[None] + 6 * (D + 2)) * U * Ad
    err = np.abs(mine.astype(np.float64) - theirs.astype(np.float64))
    assert np.all(err[..., off] <= bound[..., off]), (err[..., off] / np.where(bound > 0, bound, 1.0)[..., off]).max()
    assert np.array_equal(bits(mine[:, :, F, F]), bits(theirs[:, :, F, F]))
    f.close()
    g.close()


# ------------------------------------------------------------------------------------------------ the interface
def test_refusals_null_arguments_and_zero_rows(env):
    ta, torch = env
    forest, covers, data, _, _ = case("mixed_int_k3", depths=MIXED, cols=5, k=3, kind="int")
    x = torch.from_numpy(data.copy()).cuda()
    out = torch.full((ROWS * 3 * 6 * 6,), SENTINEL, device="cuda")
    lib = ta.lib

    def refused(f, names):
        for name in names:
            fn = getattr(lib, name)
            st = fn(f._h, x.data_ptr(), ROWS, None) if name == "tahoe_forest_set_background" else \
                fn(f._h, out.data_ptr(), x.data_ptr(), ROWS, None)
            msg = lib.tahoe_last_error().decode()
            assert st == UNSUPPORTED and "oblivious" in msg and name in msg, (name, st, msg)

    only_shap = handle(ta, forest, covers, contribs=True)
    refused(only_shap, ["tahoe_forest_predict_interactions"])
    only_inter = handle(ta, forest, covers, interactions=True)
    refused(only_inter, ["tahoe_forest_predict_contribs", "tahoe_forest_predict_contribs_approx", "tahoe_forest_set_background",
                         "tahoe_forest_predict_contribs_interventional"])
    assert lib.tahoe_forest_predict_interactions(only_inter._h, None, x.data_ptr(), ROWS, None) == INVALID_ARG
    assert lib.tahoe_forest_predict_interactions(only_inter._h, out.data_ptr(), None, ROWS, None) == INVALID_ARG
    assert lib.tahoe_forest_predict_interactions(only_inter._h, out.data_ptr(), x.data_ptr(), 0, None) == 0
    assert lib.tahoe_forest_predict_interactions(only_inter._h, None, None, 0, None) == 0
    assert tuple(only_inter.predict_interactions(x[:0].contiguous()).shape) == (0, 3, 6, 6)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    for f in (only_shap, only_inter):
        f.check()
        f.close()


def test_all_three_flags_serve_their_calls_and_the_tables_count_in_device_bytes(env):
    ta, torch = env
    forest, covers, data, _, emu = case("mixed_int_k3", depths=MIXED, cols=5, k=3, kind="int")
    x = torch.from_numpy(data.copy()).cuda()
    shap, inter = handle(ta, forest, covers, contribs=True), handle(ta, forest, covers, interactions=True)
    both = handle(ta, forest, covers, contribs=True, interactions=True)
    three = handle(ta, forest, covers, contribs=True, approx_contribs=True, interactions=True)
    depths = np.asarray(forest["depths"], np.int64)
    elems = sum(np.unique(forest["fids"][s:s + int(d)]).size for d, s in zip(depths, np.concatenate([[0], np.cumsum(depths)])))
    copies = 8 * int(depths.sum()) + 8 * elems  # splits and elems with columns
    assert inter.info().device_bytes >= shap.info().device_bytes + copies
    assert both.info().device_bytes - inter.info().device_bytes < 64  # the TreeSHAP tables are shared
    assert np.array_equal(bits(run(env, three, x)), bits(emu)) and np.array_equal(bits(run(env, both, x)), bits(emu))
    want = run(env, shap, x, "predict_contribs", dims=1)
    assert np.array_equal(bits(run(env, three, x, "predict_contribs", dims=1)), bits(want))
    assert np.array_equal(bits(run(env, three, x, "predict_contribs_approx", dims=1)), bits(osr.saabas(forest, covers, data)))
    for f in (shap, inter, both, three):
        f.close()


def test_the_call_can_be_captured_on_a_side_stream(env):
    ta, torch = env
    forest, covers, data, _, emu = case("mixed_int_k3", depths=MIXED, cols=5, k=3, kind="int")
    f = handle(ta, forest, covers, interactions=True)
    x = torch.from_numpy(data.copy()).cuda()
    want = run(env, f, x)
    out = torch.zeros((ROWS, 3, 6, 6), device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        f.predict_interactions(x, out=out, stream=side)
    for _ in range(2):
        out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(want))
    f.close()
