"""The output epilogues on the GPU at the edges (transform_kernel / tahoe_transform_preds, transform_mc_kernel,
transform_staged_kernel) against tests/epilogue_ref.py: AVG, bias and THRESHOLD bit for bit, SIGMOID and SOFTMAX against float64
under the bars derived there, NaN / +-inf / saturated tails exactly, and the same bits from every entry point that serves a
configuration.  The margins are exact: lookup forests (tests/epilogue_ref.py: lookup_forest) whose raw sum of row i is
0.0f + table[i], proven against the CPU oracle before any GPU call; -0.0, which no sum from 0.0f keeps, goes in through
tahoe_transform_preds.  Every test prints its maximum error in units of u = 2^-24.

Measured on an MI355X over the whole table, all configurations, in units of u (every bar holds, none was widened):
sigmoid 1.84 u (bar 4 u) and 1.0 x 2^-149 in the subnormal tail; softmax 2.77 u at C = 3 (bar 7 u) and 4.01 u at C = 10
(bar 14 u), 0.72 x 2^-149 in the tail; AVG, bias and THRESHOLD 0 (bit for bit).  Needs an MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
AVG, SIG, THR, SMX = er.OUT_AVG, er.OUT_SIGMOID, er.OUT_THRESHOLD, er.OUT_SOFTMAX
C1_OUTPUTS = (0, AVG, SIG, AVG | SIG, THR, SIG | THR, AVG | THR)
MC_OUTPUTS = (0, AVG, AVG | SIG, SMX, AVG | SMX)
BIASES = (0.0, 0.25, -88.0, 1e30)
THR_LINEAR, THR_SIGMOID = 1.0, 0.3
ZERO_TREES = 2  # per class: T = 3 or 3C, the sum unchanged and the divisor visible
OTHER_TOTAL = 7  # a num_trees_total for tahoe_transform_preds that no handle here has
_cache = {}


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta
    from oracle import oracle

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch, oracle


def host(t):
    return np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t)


def report(what, in_u, in_tiny):
    print(f"{what}: max error {in_u:.3f} u, {in_tiny:.3f} x 2^-149 in the subnormal tail")


def case(oracle, key, columns, depth, zeros_first=False):
    """A lookup forest of `columns` [n, C] with its rows, its margins and the CPU proof that the oracle's raw sums are the
    margins (the fixture, not the library); built once."""
    k = (key, depth, zeros_first)
    if k not in _cache:
        nodes, T, data, margins = er.lookup_forest(columns, depth, zero_trees=ZERO_TREES, zeros_first=zeros_first)
        Cn = columns.shape[1]
        assert er.same_bits(er.oracle_margins(oracle, nodes, T, depth, data, Cn), margins), k
        for a in (nodes, data, margins):
            a.setflags(write=False)
        _cache[k] = (nodes, T, data, margins)
    return _cache[k]


def c1_case(oracle, zeros_first=False):
    return case(oracle, "c1", er.margin_table()[:, None], 9, zeros_first)


def mc_case(oracle, Cn, zeros_first=False):
    return case(oracle, f"mc{Cn}", er.softmax_rows(Cn)[0], 10 if Cn == 3 else 6, zeros_first)


def multiclass_handle(ta, nodes, T, depth, num_classes, **kw):
    """A dense handle through tahoe_forest_create_multiclass whatever num_classes is (ta.Forest takes the single-output entry
    point for num_classes == 1)."""
    f = ta.Forest.__new__(ta.Forest)
    nodes = np.ascontiguousarray(nodes, dtype=ta.capi.NODE_DTYPE)
    f.params = ta.ForestParams(0, depth, T, er.LOOKUP_COLS, 0, kw.get("output", 0), kw.get("threshold", 0.0),
                               kw.get("global_bias", 0.0), 0, er.MISSING)
    f._h = C.c_void_p()
    ta.capi._check(ta.capi.lib.tahoe_forest_create_multiclass(C.byref(f._h), nodes.ctypes.data, C.byref(f.params), num_classes, 0),
                   "tahoe_forest_create_multiclass")
    f.num_trees, f.depth, f.num_cols = T, depth, er.LOOKUP_COLS
    f.num_classes = ta.capi.lib.tahoe_forest_num_classes(f._h)
    return f


def staged(f, x, rounds):
    f.set_stages(rounds)
    out = host(f.predict_staged(x))
    f.check()
    return out


def csr_of(ta, torch, data):
    indptr, indices, values = ta.dense_to_csr(data, er.MISSING)
    assert values.size == data.size  # nothing is missing: the same rows
    return torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(), torch.from_numpy(values).cuda()


# ------------------------------------------------------------------------------------------------------ single output
@pytest.mark.parametrize("bias", BIASES)
@pytest.mark.parametrize("output", C1_OUTPUTS)
def test_single_output_every_entry_point(env, output, bias):
    ta, torch, oracle = env
    nodes, T, data, margins = c1_case(oracle)
    margins = margins[:, 0]
    thr = THR_SIGMOID if output & SIG else THR_LINEAR
    want = er.epilogue(margins, output, thr, bias, T)
    assert want.ambiguous[er.RANDOM_PART].mean() <= 0.01 and want.ambiguous.mean() <= 0.01  # on the CPU, before any GPU call
    kw = dict(missing=er.MISSING, output=output, threshold=thr, global_bias=bias)
    x = torch.from_numpy(data).cuda()

    f = ta.Forest(nodes, T, 9, er.LOOKUP_COLS, **kw)
    f.set_strategy(ta.STRATEGY_DIRECT)
    first = host(f.predict(x))
    f.check()
    report(f"output {output:#x} bias {bias}", *er.check(first, want, "predict DIRECT"))
    got = {}
    f.set_strategy(ta.STRATEGY_AUTO)
    got["predict AUTO"] = host(f.predict(x))
    raw = f.predict_raw(x)
    assert er.same_bits(host(raw), margins)
    got["predict_raw + transform_preds"] = host(ta.capi.transform_preds(raw.clone(), output, T, thr, bias))
    other = host(ta.capi.transform_preds(raw.clone(), output, OTHER_TOTAL, thr, bias))
    er.check(other, er.epilogue(margins, output, thr, bias, OTHER_TOTAL), "transform_preds with another total")
    got["predict_csr"] = host(f.predict_csr(*csr_of(ta, torch, data)))
    got["predict_host"] = f.predict_host(data)
    got["predict_staged [T]"] = staged(f, x, [T])[:, 0]
    both = staged(f, x, [1, T])
    got["predict_staged [1, T] stage 1"] = both[:, 1]
    er.check(both[:, 0], er.epilogue(margins, output, thr, bias, 1), "stage 0 of [1, T]: the lookup tree alone, averaged by 1")
    f.close()

    g = multiclass_handle(ta, nodes, T, 9, 1, **kw)
    got["multi-class handle with one class"] = host(g.predict(x))
    got["multi-class handle with one class, staged"] = staged(g, x, [T])[:, 0]
    g.close()

    zn, zT, zdata, zmargins = c1_case(oracle, zeros_first=True)
    z = ta.Forest(zn, zT, 9, er.LOOKUP_COLS, **kw)
    both = staged(z, x, [1, T])
    got["zero trees first, stage 1"] = both[:, 1]
    er.check(both[:, 0], er.epilogue(np.zeros_like(margins), output, thr, bias, 1), "zero trees first, stage 0: +0.0 averaged by 1")
    z.close()

    sn, tr = ta.capi.dense_to_sparse(nodes, T, 9)
    s = ta.capi.SparseForest(sn, tr, er.LOOKUP_COLS, **kw)
    got["sparse predict"] = host(s.predict(x))
    got["sparse predict_staged"] = staged(s, x, [1, T])[:, 1]
    s.close()
    for name, g in got.items():
        assert er.same_bits(g, first), (name, output, bias, np.flatnonzero(g.view(np.uint32) != first.view(np.uint32))[:4])


@pytest.mark.parametrize("output", C1_OUTPUTS)
def test_transform_preds_on_the_whole_table(env, output):
    """tahoe_transform_preds takes any buffer: the table itself, -0.0 included, at every bias and at two totals."""
    ta, torch, _ = env
    table = er.margin_table()
    thr = THR_SIGMOID if output & SIG else THR_LINEAR
    worst = (0.0, 0.0)
    for bias in BIASES:
        for total in (1, 3, OTHER_TOTAL):
            want = er.epilogue(table, output, thr, bias, total)
            assert want.ambiguous.mean() <= 0.01
            got = host(ta.capi.transform_preds(torch.from_numpy(table.copy()).cuda(), output, total, thr, bias))
            worst = tuple(max(a, b) for a, b in zip(worst, er.check(got, want, (output, bias, total))))
    report(f"tahoe_transform_preds output {output:#x}", *worst)
    if output == 0:  # RAW without a bias: nothing runs, -0.0 stays
        got = host(ta.capi.transform_preds(torch.from_numpy(table.copy()).cuda(), 0, 3, 0.0, 0.0))
        assert got.view(np.uint32)[1] == 0x80000000


def test_threshold_is_strict(env):
    ta, torch, oracle = env
    inf = F32(np.inf)

    def run(values, output, thr):
        """The values as margins through tahoe_transform_preds and, where a sum from 0.0f keeps them, through a forest's predict
        and predict_staged (dense and sparse)."""
        v = F32(values)
        outs = [host(ta.capi.transform_preds(torch.from_numpy(v.copy()).cuda(), output, 1, thr, 0.0))]
        with np.errstate(invalid="ignore"):
            kept = er.same_bits(F32(0.0) + v, v)
        if kept:
            nodes, T, data, margins = er.lookup_forest(v[:, None], 3, zero_trees=0)
            assert er.same_bits(er.oracle_margins(oracle, nodes, T, 3, data, 1)[:, 0], v)
            x = torch.from_numpy(data).cuda()
            sn, tr = ta.capi.dense_to_sparse(nodes, T, 3)
            for f in (ta.Forest(nodes, T, 3, er.LOOKUP_COLS, missing=er.MISSING, output=output, threshold=thr),
                      ta.capi.SparseForest(sn, tr, er.LOOKUP_COLS, missing=er.MISSING, output=output, threshold=thr)):
                outs.append(host(f.predict(x)))
                outs.append(staged(f, x, [1])[:, 0])
                f.close()
        for o in outs[1:]:
            assert er.same_bits(o, outs[0])
        return outs[0].tolist()

    for t in (1.0, 0.3, -2.5, 0.0, float(F32(2.0 ** -149)), float(er.FLT_MAX) / 2):
        tf = F32(t)
        assert run([tf, np.nextafter(tf, inf), np.nextafter(tf, -inf), np.nan, np.inf, -np.inf], THR, t) == [0, 1, 0, 0, 1, 0], t
    assert run([-0.0, 0.0, 2.0 ** -149], THR, 0.0) == [0, 0, 1]          # -0.0 > +0.0 is false
    assert run([0.0, -0.0, 2.0 ** -149], THR, -0.0) == [0, 0, 1]
    assert run([0.0], SIG | THR, 0.5) == [0]                              # sigmoid(0) is exactly 0.5
    assert run([0.0], SIG | THR, float(np.nextafter(F32(0.5), F32(0)))) == [1]
    assert run([np.nan, np.inf, -np.inf], SIG | THR, 0.5) == [0, 1, 0]
    assert run([np.inf], THR, float("inf")) == [0]                        # inf > inf is false


# -------------------------------------------------------------------------------------------------------- multi-class
@pytest.mark.parametrize("bias", BIASES)
@pytest.mark.parametrize("output", MC_OUTPUTS)
@pytest.mark.parametrize("Cn", [3, 10])
def test_classes_every_entry_point(env, Cn, output, bias):
    ta, torch, oracle = env
    nodes, T, data, margins = mc_case(oracle, Cn)
    depth, Tc = (10 if Cn == 3 else 6), 1 + ZERO_TREES
    assert T == Cn * Tc
    want = er.epilogue(margins, output, 0.0, bias, Tc)  # by the trees of a class, not by all
    kw = dict(missing=er.MISSING, output=output, global_bias=bias, num_classes=Cn)
    x = torch.from_numpy(data).cuda()

    f = ta.Forest(nodes, T, depth, er.LOOKUP_COLS, **kw)
    f.set_strategy(ta.STRATEGY_DIRECT)
    first = host(f.predict(x))
    f.check()
    report(f"C {Cn} output {output:#x} bias {bias}", *er.check(first, want, "predict DIRECT"))
    if output & SMX:
        er.softmax_invariants(first, er.linear(margins, output, bias, Tc), want, er.softmax_rows(Cn)[1])
    got = {}
    f.set_strategy(ta.STRATEGY_AUTO)
    got["predict AUTO"] = host(f.predict(x))
    raw = f.predict_raw(x)
    assert er.same_bits(host(raw), margins)
    if not output & SMX:  # transform_mc_kernel against transform_kernel: per element the same statements
        got["predict_raw + transform_preds"] = host(ta.capi.transform_preds(raw.clone(), output, Tc, 0.0, bias))
    got["predict_csr"] = host(f.predict_csr(*csr_of(ta, torch, data)))
    got["predict_staged [Tc]"] = staged(f, x, [Tc])[:, 0]
    both = staged(f, x, [1, Tc])
    got["predict_staged [1, Tc] stage 1"] = both[:, 1]
    er.check(both[:, 0], er.epilogue(margins, output, 0.0, bias, 1), "stage 0 of [1, Tc]: the lookup trees alone, averaged by 1")
    f.close()

    zn, zT, zdata, zmargins = mc_case(oracle, Cn, zeros_first=True)
    z = ta.Forest(zn, zT, depth, er.LOOKUP_COLS, **kw)
    both = staged(z, x, [1, Tc])
    got["zero trees first, stage 1"] = both[:, 1]
    er.check(both[:, 0], er.epilogue(np.zeros_like(margins), output, 0.0, bias, 1), "zero trees first, stage 0: +0.0 averaged by 1")
    z.close()

    sn, tr = ta.capi.dense_to_sparse(nodes, T, depth)
    s = ta.capi.SparseForest(sn, tr, er.LOOKUP_COLS, **kw)
    got["sparse predict"] = host(s.predict(x))
    got["sparse predict_staged"] = staged(s, x, [1, Tc])[:, 1]
    s.close()
    for name, g in got.items():
        assert er.same_bits(g, first), (name, Cn, output, bias, np.argwhere(g.view(np.uint32) != first.view(np.uint32))[:4].tolist())


# ----------------------------------------------------------------------------------------------------- partial blocks
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 513])
def test_rows_around_the_block_size(env, rows):
    """The epilogue kernels run kBlock = 256 threads per block, one per row (transform_kernel, transform_mc_kernel) or one per
    (row, stage) (transform_staged_kernel): a last partial block that is dropped leaves raw sums behind."""
    ta, torch, oracle = env
    table = np.resize(er.margin_table(), 513)
    nodes, T, data, margins = case(oracle, "c1x513", table[:, None], 10)
    x = torch.from_numpy(data[:rows].copy()).cuda()
    output, bias = AVG | SIG, 0.25
    want = er.epilogue(margins[:rows, 0], output, 0.0, bias, T)
    f = ta.Forest(nodes, T, 10, er.LOOKUP_COLS, missing=er.MISSING, output=output, global_bias=bias)
    worst = (0.0, 0.0)
    for strategy in (ta.STRATEGY_DIRECT, ta.STRATEGY_AUTO):
        f.set_strategy(strategy)
        got = host(f.predict(x))
        f.check()
        worst = tuple(max(a, b) for a, b in zip(worst, er.check(got, want, ("predict", strategy, rows))))
    both = staged(f, x, [1, T])
    assert both.shape == (rows, 2) and er.same_bits(both[:, 1], got)
    er.check(both[:, 0], er.epilogue(margins[:rows, 0], output, 0.0, bias, 1), ("stage 0", rows))
    f.close()

    rows3 = np.resize(er.softmax_rows(3)[0][31 * 31:], (513, 3))  # the rows after the pairs, repeated
    nodes, T, data, margins = case(oracle, "mc3x513", rows3, 10)
    output = AVG | SMX
    want = er.epilogue(margins[:rows], output, 0.0, bias, 3)
    f = ta.Forest(nodes, T, 10, er.LOOKUP_COLS, missing=er.MISSING, output=output, global_bias=bias, num_classes=3)
    for strategy in (ta.STRATEGY_DIRECT, ta.STRATEGY_AUTO):
        f.set_strategy(strategy)
        got = host(f.predict(x))
        f.check()
        worst = tuple(max(a, b) for a, b in zip(worst, er.check(got, want, ("classes", strategy, rows))))
    both = staged(f, x, [1, 3])
    assert both.shape == (rows, 2, 3) and er.same_bits(both[:, 1], got)
    er.check(both[:, 0], er.epilogue(margins[:rows], output, 0.0, bias, 1), ("classes, stage 0", rows))
    f.close()
    report(f"{rows} rows", *worst)
