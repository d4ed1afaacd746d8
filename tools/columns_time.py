"""Column-major batches (tahoe_forest_predict_columns): what reading the columns in place is worth, timed side by side.

Shapes: K1, K3, KR3 and K5 of BASELINE.json, the dense 500 x depth 8 forest on 500 features and K5's sparse forest widened to 480
features (tools/csr_time.py's two), and K2 (3072 features: no kernel reads its columns, chunks only).  1 M rows, or 200 k where
DESIGN.md section 19 used that (K2, K5 and the two of csr_time.py).  Data: uniform in [-1, 1) built on the device; KR3's comes
from its histogram-style generator (100 k host rows repeated ten times).
Per shape, four things, each the median of ITERS single calls bracketed by events on the stream after WARMUP calls, measured
twice (the spread between the two medians is reported):
  (a) predict_columns as AUTO plans it;
  (b) the same on a handle created with TAHOE_COLUMNS_FUSED=0 (transposed chunks into AUTO's kernel);
  (c) predict on a row-major matrix that already exists;
  (d) x.t().contiguous() followed by predict: what a caller who holds columns has today.
`pick` is AUTO's plan for (a).  same_path: AUTO itself plans chunks, so (a) and (b) launch the same kernels and there is no pick to
judge.  pick_ok: same_path, or (a) was the faster of (a) and (b), with no tolerance.  The bits of (a), (b) and (d) are compared
with (c).  On K3 and KR3 the quantise pass alone, from columns and from rows, is read from the handle's own events
(tahoe_forest_prepass_times).
    python tools/columns_time.py [out_dir] [iterations]      -> <out_dir>/columns_time.json (default profiles/columns)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "columns")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 3
MISSING = -999.0


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
    def dense(cfg, rows=None, cols=None):
        T, D, C, R, fs, _, lp, _ = bench.BASELINE_SHAPES[cfg]
        C = cols or C
        return (lambda: ta.Forest(ta.synth_forest(T, D, C, seed=fs, leaf_prob=lp), T, D, C, missing=MISSING)), C, rows or R

    make, C, R = dense("K1", rows=1_000_000)
    yield "K1 (500 x depth 8, 18 features)", make, lambda: uniform_rows(R, C, 1), False
    make3, C3, R3 = dense("K3")
    yield "K3 (1000 x depth 12, 256 features)", make3, lambda: uniform_rows(R3, C3, 3), True

    def kr3():
        nodes = ta.synth_forest_hist(1000, 12, 256, seed=42, feature_seed=7, max_bins=254, zipf_s=1.0, leaf_prob=0.02, scale_decades=3.0)
        return ta.Forest(nodes, 1000, 12, 256, missing=MISSING)

    yield ("KR3 (K3's shape, <= 254 thresholds per feature)", kr3,
           lambda: torch.from_numpy(ta.synth_data_hist(100_000, 256, seed=43, feature_seed=7, scale_decades=3.0)).cuda().repeat(10, 1).contiguous(),
           True)
    k = bench.K5_SHAPE

    def sparse(cols):
        sn, tr = ta.capi.synth_sparse_forest(k["trees"], cols, k["min_depth"], k["max_depth"], k["leaf_prob"], k["max_tree_nodes"], k["forest_seed"])
        return ta.capi.SparseForest(sn, tr, cols, missing=MISSING)

    yield "K5 (2000 sparse trees, 256 features)", lambda: sparse(256), lambda: uniform_rows(200_000, 256, 5), False
    make5, _, _ = dense("K2", cols=500)
    yield "dense 500 x depth 8, 500 features", make5, lambda: uniform_rows(200_000, 500, 6), False
    yield "K5 sparse forest widened to 480 features", lambda: sparse(480), lambda: uniform_rows(200_000, 480, 7), False
    make2, C2, _ = dense("K2")
    yield "K2 (500 x depth 8, 3072 features)", make2, lambda: uniform_rows(200_000, C2, 2), False


def main():
    res = {"iterations": ITERS, "warmup": WARMUP, "cells": [], "spread_max": 0.0}
    for name, make, data, with_prepass in shapes():
        os.environ["TAHOE_COLUMNS_FUSED"] = "0"
        chunked = make()
        del os.environ["TAHOE_COLUMNS_FUSED"]
        f = make()
        x = data()
        rows, cols = x.shape
        xc = x.t().contiguous().t()  # the same values, column-major: stride (1, rows)
        assert xc.stride() == (1, rows)
        out = torch.empty(f._out_shape(rows), dtype=torch.float32, device="cuda")
        f.reserve_columns(rows)
        chunked.reserve_columns(rows)
        f.reserve(rows)
        cell = {"shape": name, "rows": rows, "num_cols": cols, "row_major_form": f.kernel_form(rows)}
        cell["pick"], cell["pick_chunk_rows"] = f.columns_plan(rows)
        cell["chunked_form"], cell["chunk_rows"] = chunked.columns_plan(rows)
        cell["c_row_major_ms"] = timed(lambda: f.predict(x, out))
        want = out.clone()
        cell["a_columns_auto_ms"] = timed(lambda: f.predict_columns(xc, out))
        same = bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
        out.zero_()
        cell["b_columns_chunked_ms"] = timed(lambda: chunked.predict_columns(xc, out))
        same = same and bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
        out.zero_()
        cell["d_transpose_then_predict_ms"] = timed(lambda: f.predict(xc.contiguous(), out))
        same = same and bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
        cell["same_bits"] = same
        if with_prepass:
            cell["quantise_from_columns_ms"] = prepass(f, lambda: f.predict_columns(xc, out))
            cell["quantise_from_rows_ms"] = prepass(f, lambda: f.predict(x, out))
        a, b, c, d = (min(cell[key]) for key in ("a_columns_auto_ms", "b_columns_chunked_ms", "c_row_major_ms", "d_transpose_then_predict_ms"))
        cell["pick_is_fused"] = cell["pick_chunk_rows"] == 0
        cell["faster"] = "a" if a < b else "b"
        cell["same_path"] = (cell["pick"], cell["pick_chunk_rows"]) == (cell["chunked_form"], cell["chunk_rows"])
        cell["pick_ok"] = bool(cell["same_path"] or a < b)
        cell["a_over_b"], cell["a_over_c"], cell["a_over_d"] = round(a / b, 3), round(a / c, 3), round(a / d, 3)
        for key in ("a_columns_auto_ms", "b_columns_chunked_ms", "c_row_major_ms", "d_transpose_then_predict_ms"):
            res["spread_max"] = max(res["spread_max"], abs(cell[key][0] - cell[key][1]) / min(cell[key]))
        res["cells"].append(cell)
        print(json.dumps(cell), flush=True)
        f.check()
        chunked.check()
        f.close()
        chunked.close()
        del x, xc, out, want
        torch.cuda.empty_cache()
    res["src_hash"] = bench.kernel_source_hash()
    res["pick_ok_everywhere"] = all(c["pick_ok"] for c in res["cells"])
    res["same_bits_everywhere"] = all(c["same_bits"] for c in res["cells"])
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "columns_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not res["same_bits_everywhere"]:
        sys.exit("predictions from columns and from rows differ")


if __name__ == "__main__":
    main()
