"""Typed, nullable tables (tahoe_forest_predict_table): what converting and null-testing inside the load is worth, timed side by side.

Shapes: K3 and KR3 of BASELINE.json at 1 M rows, K5 at 200 k rows, and one chunked shape, K5's sparse forest widened to 480
features (200 k rows; AUTO's form there has no typed loader).  Per shape a table of float32 / float64 / int32 / int8 columns in equal
shares (column c has type c % 4; the integer columns hold rint(8 x)), with 0 % and with 10 % nulls in every column.
Per cell four things, each the median of ITERS single calls bracketed by events on the stream after WARMUP calls, measured twice:
  (a) predict_table as AUTO plans it;
  (b) the same on a handle created with TAHOE_TABLE_FUSED=0 (converted chunks into AUTO's kernel);
  (c) what a caller does today: per column .to(float32) and torch.where(valid, x, S) into float32 columns, then predict_columns;
  (d) predict_columns on float32 columns that already exist and hold no nulls (the table's values, materialised beforehand).
`pick` is AUTO's plan for (a).  same_path: AUTO itself plans chunks, so (a) and (b) launch the same kernels and there is no pick to
judge.  pick_ok: same_path, or (a) was the faster of (a) and (b), with no tolerance.  a / b, a / c and a / d are recorded; only
a against b is judged.  The bits of (a), (b) and (c) are compared with (d)'s.
    python tools/table_time.py [out_dir] [iterations]      -> <out_dir>/table_time.json (default profiles/table)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "table")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 3
MISSING = -999.0
TYPES = (torch.float32, torch.float64, torch.int32, torch.int8)


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


def shapes():
    T, D, C, R, fs, _, lp, _ = bench.BASELINE_SHAPES["K3"]
    yield ("K3 (1000 x depth 12, 256 features)", lambda: ta.Forest(ta.synth_forest(T, D, C, seed=fs, leaf_prob=lp), T, D, C, missing=MISSING),
           lambda: uniform_rows(R, C, 3))

    def kr3():
        nodes = ta.synth_forest_hist(1000, 12, 256, seed=42, feature_seed=7, max_bins=254, zipf_s=1.0, leaf_prob=0.02, scale_decades=3.0)
        return ta.Forest(nodes, 1000, 12, 256, missing=MISSING)

    yield ("KR3 (K3's shape, <= 254 thresholds per feature)", kr3,
           lambda: torch.from_numpy(ta.synth_data_hist(100_000, 256, seed=43, feature_seed=7, scale_decades=3.0)).cuda().repeat(10, 1).contiguous())
    k = bench.K5_SHAPE

    def sparse(cols):
        sn, tr = ta.capi.synth_sparse_forest(k["trees"], cols, k["min_depth"], k["max_depth"], k["leaf_prob"], k["max_tree_nodes"], k["forest_seed"])
        return ta.capi.SparseForest(sn, tr, cols, missing=MISSING)

    yield "K5 (2000 sparse trees, 256 features)", lambda: sparse(256), lambda: uniform_rows(200_000, 256, 5)
    yield "K5 sparse forest widened to 480 features (chunks)", lambda: sparse(480), lambda: uniform_rows(200_000, 480, 7)


def typed_columns(x, null_frac, seed):
    """(columns, validity bitmaps or None per column, boolean masks or None) for the float32 matrix x"""
    rows, cols = x.shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    columns, bitmaps, masks = [], [], []
    weights = (2 ** torch.arange(8, device="cuda", dtype=torch.int32))
    for c in range(cols):
        t = TYPES[c % 4]
        v = x[:, c]
        columns.append((v.to(t) if t.is_floating_point else torch.round(v * 8.0).to(t)).contiguous())
        if null_frac > 0:
            valid = torch.rand(rows, generator=g, device="cuda") >= null_frac
            pad = (-rows) % 8
            bits = torch.cat([valid, torch.zeros(pad, dtype=torch.bool, device="cuda")]).view(-1, 8).to(torch.int32)
            bitmaps.append((bits * weights).sum(dim=1).to(torch.uint8).contiguous())  # LSB first
            masks.append(valid)
        else:
            bitmaps.append(None)
            masks.append(None)
    return columns, bitmaps, masks


def main():
    res = {"iterations": ITERS, "warmup": WARMUP, "cells": [], "spread_max": 0.0}
    for name, make, data in shapes():
        os.environ["TAHOE_TABLE_FUSED"] = "0"
        chunked = make()
        del os.environ["TAHOE_TABLE_FUSED"]
        f = make()
        x = data()
        rows, cols = x.shape
        out = torch.empty(f._out_shape(rows), dtype=torch.float32, device="cuda")
        for h in (f, chunked):
            h.reserve_table(rows)
            h.reserve_columns(rows)
        sentinel = torch.tensor(MISSING, device="cuda")
        for null_frac in (0.0, 0.1):
            columns, bitmaps, masks = typed_columns(x, null_frac, seed=cols)
            table = ta.Table(columns, validity=bitmaps)

            def today():  # the caller's own pass: a float32 copy of every column, the nulls filled with the sentinel
                conv = [c.to(torch.float32) if m is None else torch.where(m, c.to(torch.float32), sentinel) for c, m in zip(columns, masks)]
                return f.predict_columns(conv, out)

            ready = [c.to(torch.float32) if m is None else torch.where(m, c.to(torch.float32), sentinel) for c, m in zip(columns, masks)]
            cell = {"shape": name, "rows": rows, "num_cols": cols, "nulls": null_frac, "row_major_form": f.kernel_form(rows)}
            cell["pick"], cell["pick_chunk_rows"] = f.table_plan(rows)
            cell["chunked_form"], cell["chunk_rows"] = chunked.table_plan(rows)
            cell["d_float32_columns_ms"] = timed(lambda: f.predict_columns(ready, out))
            want = out.clone()
            cell["a_table_auto_ms"] = timed(lambda: f.predict_table(table, out))
            same = bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
            out.zero_()
            cell["b_table_chunked_ms"] = timed(lambda: chunked.predict_table(table, out))
            same = same and bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
            out.zero_()
            cell["c_convert_then_columns_ms"] = timed(today)
            same = same and bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
            cell["same_bits"] = same
            a, b, c, d = (min(cell[key]) for key in ("a_table_auto_ms", "b_table_chunked_ms", "c_convert_then_columns_ms", "d_float32_columns_ms"))
            cell["pick_is_fused"] = cell["pick_chunk_rows"] == 0
            cell["faster"] = "a" if a < b else "b"
            cell["same_path"] = (cell["pick"], cell["pick_chunk_rows"]) == (cell["chunked_form"], cell["chunk_rows"])
            cell["pick_ok"] = bool(cell["same_path"] or a < b)
            cell["a_over_b"], cell["a_over_c"], cell["a_over_d"] = round(a / b, 3), round(a / c, 3), round(a / d, 3)
            for key in ("a_table_auto_ms", "b_table_chunked_ms", "c_convert_then_columns_ms", "d_float32_columns_ms"):
                res["spread_max"] = max(res["spread_max"], abs(cell[key][0] - cell[key][1]) / min(cell[key]))
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
            table.close()
            del columns, bitmaps, masks, ready, want
        f.check()
        chunked.check()
        f.close()
        chunked.close()
        del x, out
        torch.cuda.empty_cache()
    res["src_hash"] = bench.kernel_source_hash()
    res["pick_ok_everywhere"] = all(c["pick_ok"] for c in res["cells"])
    res["same_bits_everywhere"] = all(c["same_bits"] for c in res["cells"])
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "table_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not res["same_bits_everywhere"]:
        sys.exit("predictions from the table and from float32 columns differ")


if __name__ == "__main__":
    main()
