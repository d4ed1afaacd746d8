"""NaN as a missing value (TAHOE_CREATE_NAN_MISSING): what the flag costs and what it saves, timed side by side.

Shapes: K3 and KR3 of BASELINE.json at 1 M rows (QRING: the rule is a second compare in the quantise pass) and K5's sparse forest
at 200 k rows.  Data: uniform in [-1, 1) built on the device (KR3's from its histogram-style generator, 100 k host rows repeated
ten times), with 0 %, 1 % and 10 % of the entries set to NaN.  Per shape and NaN share, three things, each the median of ITERS
single calls bracketed by events on the stream after WARMUP calls, measured twice (the spread between the two medians is kept):
  (a) the handle created with the flag, on the batch with its NaNs;
  (b) a handle without the flag, on the batch whose NaNs were replaced by the sentinel beforehand (not timed);
  (c) torch.where(torch.isnan(x), S, x) followed by (b): what a caller does today.
Nothing says (a) should differ from (b); the ratios a/b and a/c are recorded, not judged.  The bits of (a) are compared with
(b)'s: they are the same predictions.  Where the strategy is QRING the quantise pass alone is read from the handle's own events.
    python tools/nan_missing_time.py [out_dir] [iterations]      -> <out_dir>/nan_missing_time.json (default profiles/nan_missing)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nan_missing")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 3
MISSING = -999.0
SHARES = (0.0, 0.01, 0.10)


def uniform_rows(rows, cols, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((rows, cols), generator=g, device="cuda") * 2.0 - 1.0).contiguous()


def timed(call):
    """Two medians (ms) of ITERS event-timed calls each"""
    meds = []
    for _ in range(2):
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        t = []
        for _ in range(ITERS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
        meds.append(float(np.median(t)))
    return meds


def prepass(f, call):
    """Median (ms) of the handle's own pre-pass times over ITERS calls"""
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    f.set_profiling(ITERS)
    for _ in range(ITERS):
        call()
    torch.cuda.synchronize()
    t = f.prepass_times_ms()
    f.set_profiling(0)
    return float(np.median(t))


def shapes():
    T, D, C, R, fs, _, lp, _ = bench.BASELINE_SHAPES["K3"]
    k3 = ta.synth_forest(T, D, C, seed=fs, leaf_prob=lp)
    yield ("K3 (1000 x depth 12, 256 features)", lambda flag: ta.Forest(k3, T, D, C, missing=MISSING, nan_missing=flag),
           lambda: uniform_rows(R, C, 3))
    kr3 = ta.synth_forest_hist(1000, 12, 256, seed=42, feature_seed=7, max_bins=254, zipf_s=1.0, leaf_prob=0.02, scale_decades=3.0)
    yield ("KR3 (K3's shape, <= 254 thresholds per feature)", lambda flag: ta.Forest(kr3, 1000, 12, 256, missing=MISSING, nan_missing=flag),
           lambda: torch.from_numpy(ta.synth_data_hist(100_000, 256, seed=43, feature_seed=7, scale_decades=3.0)).cuda().repeat(10, 1).contiguous())
    k = bench.K5_SHAPE
    sn, tr = ta.capi.synth_sparse_forest(k["trees"], 256, k["min_depth"], k["max_depth"], k["leaf_prob"], k["max_tree_nodes"], k["forest_seed"])
    yield ("K5 (2000 sparse trees, 256 features)", lambda flag: ta.capi.SparseForest(sn, tr, 256, missing=MISSING, nan_missing=flag),
           lambda: uniform_rows(200_000, 256, 5))


def main():
    res = {"iterations": ITERS, "warmup": WARMUP, "cells": [], "spread_max": 0.0}
    for name, make, data in shapes():
        flagged, plain = make(True), make(False)
        base = data()
        rows, cols = base.shape
        flagged.reserve(rows)
        plain.reserve(rows)
        out = torch.empty(flagged._out_shape(rows), dtype=torch.float32, device="cuda")
        for share in SHARES:
            g = torch.Generator(device="cuda").manual_seed(int(share * 1000) + 1)
            x = torch.where(torch.rand(base.shape, generator=g, device="cuda") < share, torch.full_like(base, float("nan")), base)
            xs = torch.where(torch.isnan(x), MISSING, x)  # what (b) predicts on
            cell = {"shape": name, "rows": rows, "num_cols": cols, "nan_share": share, "nans": int(torch.isnan(x).sum()),
                    "flagged_form": flagged.kernel_form(rows), "plain_form": plain.kernel_form(rows)}
            cell["b_plain_on_replaced_ms"] = timed(lambda: plain.predict(xs, out))
            want = out.clone()
            out.zero_()
            cell["a_flagged_ms"] = timed(lambda: flagged.predict(x, out))
            cell["same_bits"] = bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
            out.zero_()
            cell["c_where_then_plain_ms"] = timed(lambda: plain.predict(torch.where(torch.isnan(x), MISSING, x), out))
            cell["same_bits"] = cell["same_bits"] and bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
            if cell["flagged_form"].startswith("qring"):
                cell["quantise_flagged_ms"] = prepass(flagged, lambda: flagged.predict(x, out))
                cell["quantise_plain_ms"] = prepass(plain, lambda: plain.predict(xs, out))
            a, b, c = (min(cell[key]) for key in ("a_flagged_ms", "b_plain_on_replaced_ms", "c_where_then_plain_ms"))
            cell["a_over_b"], cell["a_over_c"] = round(a / b, 3), round(a / c, 3)
            for key in ("a_flagged_ms", "b_plain_on_replaced_ms", "c_where_then_plain_ms"):
                res["spread_max"] = max(res["spread_max"], abs(cell[key][0] - cell[key][1]) / min(cell[key]))
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
            del x, xs, want
        flagged.check()
        plain.check()
        flagged.close()
        plain.close()
        del base, out
        torch.cuda.empty_cache()
    res["src_hash"] = bench.kernel_source_hash()
    res["same_bits_everywhere"] = all(c["same_bits"] for c in res["cells"])
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "nan_missing_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not res["same_bits_everywhere"]:
        sys.exit("the flagged handle and the handle on the replaced batch differ")


if __name__ == "__main__":
    main()
