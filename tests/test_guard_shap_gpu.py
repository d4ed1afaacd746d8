"""Guard bands around the explanation calls that had none: predict_contribs, predict_interactions and
predict_contribs_interventional on dense, three-class dense, sparse, categorical sparse and vector-leaf handles (approx, every
oblivious explanation and vector approx carry theirs in their own files).  Needs an MI355X.

Neither a reference nor a bar is restated here.  For the length of a test the three calls of ta.Forest (and set_background) are
replaced by wrappers that run the real call into tests/guarded.py buffers -- output [rows, (C | K,) F + 1 (, F + 1)] and data,
384 rows of guard on either side -- check the bands and the input by bits, and hand the interior back; then the accuracy check
of the feature's own GPU test runs (its float64 reference, its bar) and judges what came out of the guarded call.  The wrapper
also runs the same call at the smaller row counts around the kernels' row tiles (63 / 64 / 65 for the 64-row tiles; R - 1, R,
R + 1, 2R + 1 for the interventional kernel's tile of R rows, 8 at few columns and 4 at 300), largest first,
each into fresh guarded buffers, and holds every smaller batch to the bits of the first rows of the largest: a row's values do
not depend on its batch (what every one of these features' own tests asserts), so equal bits put them under the same bar.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cat_shap_cases  # noqa: E402
import test_cat_shap_gpu as t_cat  # noqa: E402
import test_contribs_gpu as t_phi  # noqa: E402
import test_interactions_gpu as t_inter  # noqa: E402
import test_interventional_gpu as t_iv  # noqa: E402
import test_sparse_shap_gpu as t_sparse  # noqa: E402
import test_vector_inter_gpu as t_vinter  # noqa: E402
import test_vector_iv_gpu as t_viv  # noqa: E402
import test_vector_shap_gpu as t_vphi  # noqa: E402
from guarded import Guarded, guarded_input  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
TILE_ROWS = (65, 64, 63)                    # the 64-row tiles
IV_ROWS = (17, 9, 8, 7, 5, 4, 3)            # R - 1, R, R + 1, 2R + 1 for R = 8 and R = 4
CALLS = {"predict_contribs": 1, "predict_interactions": 2, "predict_contribs_interventional": 1}


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, torch


def same_bits(a, b):
    """Equal bits, any NaN equal to any NaN (a payload says nothing about the row)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture
def guarded_calls(env, monkeypatch):
    """Replaces the three calls and set_background on ta.Forest (every handle kind inherits them); -> the log of (call, kind of
    handle, classes, columns, rows) the wrappers ran."""
    ta, torch = env
    log = []
    keep = []  # guarded backgrounds stay allocated while their handles live

    def wrap(name, k):
        real = getattr(ta.Forest, name)

        def call(self, data, out=None, stream=None):
            assert out is None
            host = data.cpu().numpy()
            rows = host.shape[0]
            counts = [rows] + [r for r in TILE_ROWS + IV_ROWS + (1,) if r < rows]
            big = None
            for R in counts:  # largest first
                x = guarded_input(torch, host[:R], torch.float32, device="cuda")
                shape = (R,) + ((self.num_classes,) if self.num_classes > 1 else ()) + (self.num_cols + 1,) * k
                g = Guarded(torch, shape, torch.float32, device="cuda")
                real(self, x.view, out=g.view, stream=stream)
                self.check()
                tag = f"{name} on {type(self).__name__}, {self.num_classes} class(es), {self.num_cols} columns, rows {R}"
                got = g.check(tag)
                x.check_unchanged("data: " + tag)
                log.append((name, type(self).__name__, self.num_classes, self.num_cols, R))
                if big is None:
                    big = got
                else:
                    assert same_bits(got, big[:R]), f"{tag}: not the bits of the same rows in a batch of {rows}"
            return torch.from_numpy(big).cuda()

        monkeypatch.setattr(ta.Forest, name, call)

    for name, k in CALLS.items():
        wrap(name, k)
    real_bg = ta.Forest.set_background

    def set_background(self, bg, stream=None):
        if bg is None:
            return real_bg(self, None, stream)
        g = guarded_input(torch, bg.cpu().numpy(), torch.float32, device="cuda")
        real_bg(self, g.view, stream)  # synchronous: the handle has taken what it needs when it returns
        g.check_unchanged(f"background of {type(self).__name__}, {tuple(bg.shape)}")
        keep.append(g)
        log.append(("set_background", type(self).__name__, self.num_classes, self.num_cols, int(bg.shape[0])))

    monkeypatch.setattr(ta.Forest, "set_background", set_background)
    return log


def ran(log, name, kind, rows, classes=None, cols=None):
    """Asserts that the wrappers ran `name` on a handle of that kind at every row count of `rows`."""
    seen = {e[4] for e in log if e[0] == name and e[1] == kind and (classes is None or e[2] == classes) and (cols is None or e[3] == cols)}
    assert set(rows) <= seen, (name, kind, sorted(set(rows) - seen))


# ------------------------------------------------------------------------------------------------------------------- dense
def brute_forest(ta, seed, rng_seed, lo):
    """The forests of test_small_shapes_brute_force (test_contribs_gpu.py / test_interactions_gpu.py): random covers, a few NaN
    thresholds."""
    rng = np.random.default_rng(rng_seed)
    T, D, F = int(rng.integers(2, lo[0])), int(rng.integers(lo[1], 6)), int(rng.integers(lo[2], 9))
    nodes = ta.synth_forest(T, D, F, seed=seed, leaf_prob=0.15)
    nodes["weight"] = rng.uniform(0.05, 1.0, nodes.size).astype(np.float32)
    internal = (nodes["bits"].view(np.uint32) >> 31) == 0
    nodes["val"][internal & (rng.random(nodes.size) < 0.05)] = np.nan
    return nodes, T, D, F


def test_dense_contribs(env, guarded_calls):
    ta, _ = env
    nodes, T, D, F = brute_forest(ta, 0, 100, (21, 1, 2))
    x = ta.synth_data(131, F, seed=7, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    f, _, _ = t_phi.check(env, nodes, T, D, F, x, label=f"T={T} D={D} F={F}", brute=True)
    f.close()
    ran(guarded_calls, "predict_contribs", "Forest", (131, 65, 64, 63, 1))


def test_dense_interactions(env, guarded_calls):
    ta, _ = env
    nodes, T, D, F = brute_forest(ta, 0, 300, (13, 2, 3))
    x = ta.synth_data(71, F, seed=7, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    f, _ = t_inter.check(env, nodes, T, D, F, x, label=f"T={T} D={D} F={F}", brute=True)
    f.close()
    ran(guarded_calls, "predict_interactions", "Forest", (71, 65, 64, 63, 1))
    ran(guarded_calls, "predict_contribs", "Forest", (71, 65, 64, 63, 1))  # (the diagonal's check asks for them)


@pytest.mark.parametrize("F", ["few", 300])
def test_dense_interventional(env, guarded_calls, F):
    """Few columns: tiles of R = 8 rows (test_small_shapes_brute_force's forest); 300 columns: R = 4 (test_wide_rows' forest at
    300 columns).  DESIGN section 14."""
    ta, _ = env
    if F == "few":
        rng = np.random.default_rng(200)
        T, D, F = int(rng.integers(2, 16)), int(rng.integers(1, 6)), int(rng.integers(2, 8))
        nodes = ta.synth_forest(T, D, F, seed=0, leaf_prob=0.15)
        internal = (nodes["bits"].view(np.uint32) >> 31) == 0
        nodes["val"][internal & (rng.random(nodes.size) < 0.05)] = np.nan
        x = ta.synth_data(37, F, seed=7, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
        bg = ta.synth_data(6, F, seed=8, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
        f, _, _ = t_iv.check(env, nodes, T, D, F, x, bg, label=f"T={T} D={D} F={F}", brute=True)
        rows = (37, 17, 9, 8, 7, 1)
    else:
        nodes = ta.synth_forest(10, 7, F, seed=F, leaf_prob=0.05)
        x = ta.synth_data(11, F, seed=F + 1, missing_prob=0.02, missing=MISSING, nan_prob=0.01)
        bg = ta.synth_data(9, F, seed=F + 2, missing_prob=0.02, missing=MISSING, nan_prob=0.01)
        f, _, _ = t_iv.check(env, nodes, 10, 7, F, x, bg, label=f"wide F={F}")
        rows = (11, 9, 5, 4, 3, 1)
    f.close()
    ran(guarded_calls, "predict_contribs_interventional", "Forest", rows)
    ran(guarded_calls, "set_background", "Forest", (bg.shape[0],))


@pytest.mark.parametrize("call", ["contribs", "interactions", "interventional"])
def test_three_class_dense(env, guarded_calls, call):
    """test_multiclass' forest (C = 3: 12 trees of depth 6 on 16 columns, AVG | SOFTMAX with a bias) at 70 rows."""
    ta, _ = env
    C = 3
    T, D, F = 4 * C, 6, 16
    nodes = ta.synth_forest_hist(T, D, F, seed=C, feature_seed=C + 1)
    x = ta.synth_data_hist(70, F, seed=C + 2, feature_seed=C + 1, missing_prob=0.03, missing=MISSING)
    kw = dict(num_classes=C, output=ta.OUT_AVG | ta.OUT_SOFTMAX, bias=0.375, label=f"C={C}")
    if call == "contribs":
        f = t_phi.check(env, nodes, T, D, F, x, **kw)[0]
        ran(guarded_calls, "predict_contribs", "Forest", (70, 65, 64, 63, 1), classes=C)
    elif call == "interactions":
        f = t_inter.check(env, nodes, T, D, F, x, **kw)[0]
        ran(guarded_calls, "predict_interactions", "Forest", (70, 65, 64, 63, 1), classes=C)
    else:
        bg = ta.synth_data_hist(20, F, seed=C + 3, feature_seed=C + 1, missing_prob=0.03, missing=MISSING)
        f = t_iv.check(env, nodes, T, D, F, x, bg, **kw)[0]
        ran(guarded_calls, "predict_contribs_interventional", "Forest", (70, 65, 64, 63, 17, 9, 8, 7, 1), classes=C)
    f.close()


# ----------------------------------------------------------------------------------------------------- sparse, categorical
def test_sparse_handle(env, guarded_calls):
    """test_irregular_deep_forest_against_brute_force's forest (seed 0) at 65 rows: all three calls."""
    ta, _ = env
    F = 8
    sn, tr = ta.capi.synth_sparse_forest(6, F, 4, 24, 0.5, 300, 600)
    x = ta.synth_data(65, F, seed=0, missing_prob=0.1, missing=MISSING, nan_prob=0.05)
    bg = ta.synth_data(6, F, seed=50, missing_prob=0.1, missing=MISSING)
    f, *_ = t_sparse._check_against_brute(env, sn, tr, F, 1, x, bg, 0, 0.125, "irregular, 65 rows")
    f.close()
    for name in ("predict_contribs", "predict_interactions"):
        ran(guarded_calls, name, "SparseForest", (65, 64, 63, 1))
    ran(guarded_calls, "predict_contribs_interventional", "SparseForest", (65, 64, 63, 17, 9, 8, 7, 1))


def test_categorical_sparse_handle(env, guarded_calls, monkeypatch):
    """test_mixed_forest_against_brute_force (cat_shap_cases.mixed, F = 5) with 65 rows where it draws 9."""
    real = cat_shap_cases.mixed_rows
    monkeypatch.setattr(cat_shap_cases, "mixed_rows", lambda rows, F, seed: real(65 if rows == 9 else rows, F, seed))
    t_cat.test_mixed_forest_against_brute_force(env, 5, 3)
    for name in ("predict_contribs", "predict_interactions"):
        ran(guarded_calls, name, "SparseForest", (65, 64, 63, 1), cols=5)
    ran(guarded_calls, "predict_contribs_interventional", "SparseForest", (65, 64, 63, 17, 9, 8, 7, 1), cols=5)


# ------------------------------------------------------------------------------------------------------------- vector leaves
@pytest.mark.parametrize("name", ["nine_k1", "five_k9"])
@pytest.mark.parametrize("call", ["contribs", "interactions", "interventional"])
def test_vector_forest(env, guarded_calls, monkeypatch, call, name):
    """K = 1 and K = 9, the accuracy tests of test_vector_shap_gpu.py / test_vector_inter_gpu.py / test_vector_iv_gpu.py."""
    for k in t_vphi.KNOBS:
        monkeypatch.delenv(k, raising=False)
    K = 1 if name.endswith("k1") else 9
    if call == "contribs":
        t_vphi.test_contribs_against_the_float64_brute_force(env, name)  # 65 rows
        ran(guarded_calls, "predict_contribs", "VectorForest", (65, 64, 63, 1), classes=K)
    elif call == "interactions":
        t_vinter.test_interactions_against_the_float64_reference(env, name)  # 33 rows
        ran(guarded_calls, "predict_interactions", "VectorForest", (33, 17, 9, 8, 7, 1), classes=K)
    else:
        t_viv.test_against_the_float64_closed_form(env, name)  # 17 rows, 7 background rows
        ran(guarded_calls, "predict_contribs_interventional", "VectorForest", (17, 9, 8, 7, 1), classes=K)
        ran(guarded_calls, "set_background", "VectorForest", (7,), classes=K)
