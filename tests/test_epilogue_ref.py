"""tests/epilogue_ref.py without a GPU: the reference, its bars and the margin table against the CPU oracle (glibc expf), the
known answers for NaN and +-inf, the cap on the cases SIGMOID | THRESHOLD leaves undecided, and the lookup forests whose raw
margins are the table.  The softmax, which the oracle does not have, is checked against the kernel's statements in float32
with a correctly rounded exp; the same model with a statement changed (the max not subtracted, `>=` for `>`, another divisor)
must fail, which shows that the checks have teeth."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epilogue_ref as er  # noqa: E402

F32, F64 = np.float32, np.float64
AVG, SIG, THR, SMX = er.OUT_AVG, er.OUT_SIGMOID, er.OUT_THRESHOLD, er.OUT_SOFTMAX
C1_OUTPUTS = (0, AVG, SIG, AVG | SIG, THR, SIG | THR, AVG | THR)
BIASES = (0.0, 0.25, -88.0, 1e30)
THR_LINEAR, THR_SIGMOID = 1.0, 0.3
DEPTH = 9


@pytest.fixture(scope="module")
def env(built):
    import tahoe_amd as ta
    from oracle import oracle

    return ta, oracle


@pytest.fixture(scope="module")
def c1(env):
    """The table as a 3-tree lookup forest (the lookup tree and two root leaves of +0.0) and the oracle's raw sums."""
    ta, oracle = env
    nodes, T, data, margins = er.lookup_forest(er.margin_table()[:, None], DEPTH, zero_trees=2)
    raw = oracle.predict(nodes, T, DEPTH, data, er.MISSING)[0]
    return nodes, T, data, margins[:, 0], raw


def test_output_bits_are_the_librarys(env):
    ta, _ = env
    assert (er.OUT_RAW, AVG, SIG, THR, SMX) == (ta.OUT_RAW, ta.OUT_AVG, ta.OUT_SIGMOID, ta.OUT_THRESHOLD, ta.OUT_SOFTMAX)


def test_the_table_holds_what_it_should():
    t = er.margin_table()
    assert t.dtype == F32 and t.size == 331 and np.isnan(t[30]) and np.isnan(t).sum() == 1
    bits = t.view(np.uint32)
    for want in (0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000,
                 0xFF800000):
        assert want in bits, hex(want)
    # 16.635532 is where the float64 sigmoid rounds to 1 - u; 88.72284 is the first float32 whose exp overflows float32;
    # 103.27893 is ln 2^-149 rounded up
    assert F32(1.0 / (1.0 + np.exp(-F64(F32(16.635532))))) == F32(1.0) - F32(2.0 ** -24)
    assert np.exp(F64(F32(88.72283))) < F64(er.FLT_MAX) < np.exp(F64(F32(88.72284)))
    assert np.exp(-F64(F32(103.27893))) < 2.0 ** -149 < np.exp(-F64(np.nextafter(F32(103.27893), F32(0))))
    r = t[er.RANDOM_PART]
    assert np.abs(r[:200]).max() <= 20 and np.abs(r[200:]).min() >= 2.0 ** -141 and np.abs(r[200:]).max() <= 2.0 ** 100
    rows3, first3 = er.softmax_rows(3)
    assert rows3.shape[1] == 3 and first3 == 31 * 31 + 8 + 1 and rows3.shape[0] <= 1024
    assert np.nanmax(rows3[first3 - 1]) - np.nanmin(rows3[first3 - 1]) == 200
    rows10, _ = er.softmax_rows(10)
    assert rows10.shape[1] == 10 and rows10.shape[0] <= 512


def test_lookup_forest_gives_the_table(env, c1):
    """The fixture, not the library: the oracle's raw sums are 0.0f + table[i], and so per class, zero trees first or last."""
    ta, oracle = env
    nodes, T, data, margins, raw = c1
    assert T == 3 and er.same_bits(raw, margins) and er.same_bits(margins, F32(0.0) + er.margin_table())
    assert margins.view(np.uint32)[1] == 0  # -0.0 left the table as +0.0
    for C in (3, 10):
        rows, _ = er.softmax_rows(C)
        depth = 10 if C == 3 else 6
        for zeros_first in (False, True):
            nodes, T, data, m = er.lookup_forest(rows, depth, zero_trees=2, zeros_first=zeros_first)
            assert T == 3 * C
            assert er.same_bits(er.oracle_margins(oracle, nodes, T, depth, data, C), m), (C, zeros_first)
    # stage 0 of the zeros-first forest: +0.0 everywhere
    nodes, T, data, _ = er.lookup_forest(er.margin_table()[:, None], DEPTH, zero_trees=2, zeros_first=True)
    per = nodes.size // T
    assert not oracle.predict(nodes[:per], 1, DEPTH, data, er.MISSING)[0].view(np.uint32).any()


@pytest.mark.parametrize("bias", BIASES)
@pytest.mark.parametrize("output", C1_OUTPUTS)
def test_reference_against_the_oracle(env, c1, output, bias):
    """glibc expf under the same bars as the device's; the linear statements bit for bit.

    Measured maximum of the sigmoid: 1.61 u (glibc).  Before the sigmoid kept its negative tail (oracle_sigmoid), the cases
    with a margin in [-103.97, -88.72] failed here: 0 for 2.94e-39 at r = -88.72284, 1.4e6 x the bar."""
    ta, oracle = env
    nodes, T, data, margins, _ = c1
    thr = THR_SIGMOID if output & SIG else THR_LINEAR
    want = er.epilogue(margins, output, thr, bias, T)
    assert want.ambiguous.mean() <= 0.01
    got = oracle.predict(nodes, T, DEPTH, data, er.MISSING, output=output, threshold=thr, global_bias=bias)[0]
    in_u, in_tiny = er.check(got, want, (output, bias))
    print(f"output {output:#x} bias {bias}: max error {in_u:.3f} u, {in_tiny:.3f} x 2^-149 in the subnormal tail")
    if not output & SIG:
        assert not want.bar.any() and in_u == 0 and in_tiny == 0


def test_known_answers():
    inf, nan = np.inf, np.nan
    m = F32([nan, inf, -inf, 0.0, -0.0])
    s = er.epilogue(m, SIG)
    assert np.isnan(s.ref[0]) and s.ref[1] == 1 and s.ref[2] == 0 and s.ref[3] == 0.5 and s.ref[4] == 0.5
    t = er.epilogue(m, THR, threshold=0.0)
    assert t.ref.tolist() == [0, 1, 0, 0, 0] and not t.bar.any() and not t.ambiguous.any()  # NaN > t, 0 > 0, -0 > +0: all 0
    one = np.nextafter(F32(1.0), F32(np.inf))
    assert er.epilogue(F32([1.0, one]), THR, threshold=1.0).ref.tolist() == [0, 1]
    assert er.epilogue(F32([0.0]), SIG | THR, threshold=0.5).ref.tolist() == [0]  # sigmoid(0) is exactly 0.5
    assert er.epilogue(F32([0.0]), SIG | THR, threshold=float(np.nextafter(F32(0.5), F32(0)))).ref.tolist() == [1]
    rows = F32([[nan, 1, 2], [1, inf, 2], [-inf, -inf, -inf], [-inf, 0, 0], [1, 2, -inf], [nan, nan, nan], [inf, inf, -inf]])
    p = er.epilogue(rows, SMX).ref
    for r in (0, 1, 2, 5, 6):
        assert np.isnan(p[r]).all(), r
    assert p[3].tolist() == [0.0, 0.5, 0.5]
    assert p[4, 2] == 0 and abs(p[4, 0] - 1 / (1 + np.e)) < 1e-15 and abs(p[4].sum() - 1) < 1e-15
    # AVG divides, bias after: 5 / 3 in float32, not 5 * fl(1 / 3)
    assert er.linear(F32([5.0]), AVG, 0.0, 3).view(np.uint32)[0] == 0x3FD55555
    assert er.linear(F32([-0.0]), 0, 0.0, 3).view(np.uint32)[0] == 0x80000000      # no transform runs
    assert er.linear(F32([-0.0]), AVG, 0.0, 3).view(np.uint32)[0] == 0x00000000    # -0 / 3 + 0


def test_undecided_threshold_cases_stay_under_the_cap():
    t = er.margin_table()
    for bias in BIASES:
        for divisor in (1, 3, 7):
            for output in (SIG | THR, AVG | SIG | THR):
                assert er.ambiguous_share(t, THR_SIGMOID, bias, divisor, output) <= 0.01
            assert er.ambiguous_share(t[er.RANDOM_PART], THR_SIGMOID, bias, divisor) <= 0.01
    # the cap is there for a reason: a threshold that a table entry's sigmoid hits is seen as undecided
    assert er.epilogue(F32([0.0]), SIG | THR, threshold=0.5).ambiguous.all()


# ---- the softmax and the mutations, on a float32 model of the kernels' statements ----
def exp32(x):
    with np.errstate(all="ignore"):
        return np.exp(x.astype(F64)).astype(F32)  # correctly rounded


def sigmoid32(r):
    """The sigmoid in float32 with its negative tail kept: where expf(-r) overflows (r < -88.72), 1 + e^-r is e^-r and the
    value is expf(r) (sigmoid_value in forest.hip, oracle_sigmoid)."""
    with np.errstate(all="ignore"):
        e = exp32(-r)
        return np.where(e == np.inf, exp32(r), F32(1.0) / (F32(1.0) + e)).astype(F32)


def model_classes(margins, output, bias, divisor, subtract_max=True):
    """transform_mc_kernel's statements in float32 (the sigmoid as sigmoid32)."""
    r = er.linear(margins, output, bias, divisor)
    with np.errstate(all="ignore"):
        if output & SIG:
            r = sigmoid32(r)
        if not output & SMX:
            return r
        m = np.full(r.shape[0], -np.inf, dtype=F32)
        for c in range(r.shape[1]):
            m = np.fmax(m, r[:, c])
        e = exp32(r - m[:, None]) if subtract_max else exp32(r)
        s = np.zeros(r.shape[0], dtype=F32)
        for c in range(r.shape[1]):
            s = s + e[:, c]
        return e / s[:, None]


@pytest.mark.parametrize("C", [3, 10])
@pytest.mark.parametrize("bias", BIASES)
@pytest.mark.parametrize("output", [0, AVG, AVG | SIG, SMX, AVG | SMX])
def test_reference_against_the_float32_model(C, output, bias):
    rows, first = er.softmax_rows(C)
    margins = F32(0.0) + rows
    want = er.epilogue(margins, output, 0.0, bias, 3)
    got = model_classes(margins, output, bias, 3)
    in_u, in_tiny = er.check(got, want, (C, output, bias))
    print(f"C {C} output {output:#x} bias {bias}: max error {in_u:.3f} u, {in_tiny:.3f} x 2^-149")
    if output & SMX:
        checked = er.softmax_invariants(got, er.linear(margins, output, bias, 3), want, first)
        assert checked == 16 or output & AVG  # (a shift of 64 does not survive a division by 3 exactly)


def test_mutations_are_caught(env, c1):
    """Each of these is a way the epilogue could be wrong; the reference must reject every one."""
    rows, _ = er.softmax_rows(3)
    margins = F32(0.0) + rows
    with pytest.raises(AssertionError):  # the max not subtracted: expf overflows, NaN where the reference is 0 or 1
        er.check(model_classes(margins, SMX, 0.0, 3, subtract_max=False), er.epilogue(margins, SMX, 0.0, 0.0, 3))
    t = F32(0.0) + er.margin_table()
    with pytest.raises(AssertionError):  # >= for >
        with np.errstate(invalid="ignore"):
            er.check((t >= F32(THR_LINEAR)).astype(F32), er.epilogue(t, THR, THR_LINEAR))
    with pytest.raises(AssertionError):  # another divisor: all the trees for the trees of a class, the handle's for a stage's
        er.check(er.linear(t, AVG, 0.25, 9), er.epilogue(t, AVG, 0.0, 0.25, 3))
    with pytest.raises(AssertionError):  # the subnormal tail of the sigmoid flushed to zero
        with np.errstate(all="ignore"):
            er.check(F32(1.0) / (F32(1.0) + exp32(-t)), er.epilogue(t, SIG))
    with pytest.raises(AssertionError):  # NaN > t answered 1
        er.check(np.where(np.isnan(t), F32(1.0), (t > F32(1.0)).astype(F32)), er.epilogue(t, THR, 1.0))
