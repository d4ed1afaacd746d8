"""CSR rows (tahoe_forest_predict_csr): the fused tile kernels, the chunked fallback and today's dense call, timed side by side.

Forests: K2's (500 trees of depth 8 on 3072 features: no 64-row tile fits LDS, fallback only), a dense forest of the same trees
on 500 features (ROWTILE's tile fits: the fused form exists), K3's and K5's own forests (256 features, where AUTO takes QRING:
the shapes the rule must leave to the fallback), and K5's sparse forest (2000 irregular trees of depth 4..24)
widened to 480 features -- the widest round figure whose 64-row tile and tree tops fit LDS together -- under TILEBLOCK.
Data: 200 k rows with 1 %, 5 %, 25 % and 100 % of the entries stored (uniform in [-1, 1)), built on the device.
Per cell: (a) the fused form (the tile strategy forced), (b) the fallback into AUTO (a handle created with TAHOE_CSR_FUSED=0),
(c) what a caller has today: tahoe_forest_predict on the already dense matrix under AUTO and under the same tile strategy -- the
caller's own densify is not counted.  Times are the handles' own event times (pre-pass + kernels of one call), median of
ITERS launches after WARMUP, each cell measured twice (the spread between the two medians is reported); the bits of (a) and (b)
are compared with (c).  `rule` is what AUTO picks on a handle created without the knob; rule_ok: it picked the faster of (a) and
(b), or one within 3 % of it.
    python tools/csr_time.py [out_dir] [iterations]      -> <out_dir>/csr_time.json (default profiles/csr)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "csr")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 3
MISSING = -999.0
ROWS = 200_000
DENSITIES = (0.01, 0.05, 0.25, 1.0)


def make_rows(cols, density, seed):
    """(dense x, indptr, indices, values) on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((ROWS, cols), generator=g, device="cuda") * 2.0 - 1.0
    if density < 1.0:
        x = torch.where(torch.rand((ROWS, cols), generator=g, device="cuda") < density, x, torch.full_like(x, MISSING))
    keep = x != MISSING
    indptr = torch.zeros(ROWS + 1, dtype=torch.int64, device="cuda")
    indptr[1:] = torch.cumsum(keep.sum(dim=1), dim=0)
    indices = keep.nonzero()[:, 1].to(torch.int32)
    return x.contiguous(), indptr, indices, x[keep].contiguous()


def timed(f, call):
    """Two medians (ms) of ITERS launches each of call(), by the handle's events: pre-pass + kernels."""
    meds = []
    for _ in range(2):
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        f.set_profiling(ITERS)
        for _ in range(ITERS):
            call()
        torch.cuda.synchronize()
        t = f.kernel_times_ms() + f.prepass_times_ms()
        f.set_profiling(0)
        f.check()
        meds.append(float(np.median(t)))
    return meds


def forests():
    T, D, C, _, fs, _, _, _ = bench.BASELINE_SHAPES["K2"]
    yield "K2 (500 x depth 8, 3072 features)", C, None, lambda: ta.Forest(ta.synth_forest(T, D, C, seed=fs), T, D, C, missing=MISSING)
    yield ("dense 500 x depth 8, 500 features", 500, "ROWTILE",
           lambda: ta.Forest(ta.synth_forest(T, D, 500, seed=fs), T, D, 500, missing=MISSING))
    T3, D3, C3, _, fs3, _, _, _ = bench.BASELINE_SHAPES["K3"]
    yield ("K3 (1000 x depth 12, 256 features)", C3, "ROWTILE",
           lambda: ta.Forest(ta.synth_forest(T3, D3, C3, seed=fs3), T3, D3, C3, missing=MISSING))
    k = bench.K5_SHAPE
    s5, t5 = ta.capi.synth_sparse_forest(k["trees"], k["cols"], k["min_depth"], k["max_depth"], k["leaf_prob"], k["max_tree_nodes"],
                                         k["forest_seed"])
    yield "K5 (2000 sparse trees, 256 features)", k["cols"], "TILEBLOCK", lambda: ta.capi.SparseForest(s5, t5, k["cols"], missing=MISSING)
    sn, tr = ta.capi.synth_sparse_forest(k["trees"], 480, k["min_depth"], k["max_depth"], k["leaf_prob"], k["max_tree_nodes"],
                                         k["forest_seed"])
    yield "K5 sparse forest widened to 480 features", 480, "TILEBLOCK", lambda: ta.capi.SparseForest(sn, tr, 480, missing=MISSING)


def main():
    res = {"rows": ROWS, "iterations": ITERS, "warmup": WARMUP, "cells": [], "spread_max": 0.0}
    for name, cols, tile, make in forests():
        os.environ["TAHOE_CSR_FUSED"] = "0"
        f = make()  # AUTO on CSR rows = the fallback; a forced tile strategy still takes the fused kernel
        del os.environ["TAHOE_CSR_FUSED"]
        rule = make()  # the rule, asked only
        for density in DENSITIES:
            x, ip, ix, vals = make_rows(cols, density, seed=int(density * 1000) + cols)
            nnz = int(vals.numel())
            out = torch.empty(ROWS, dtype=torch.float32, device="cuda")
            cell = {"forest": name, "num_cols": cols, "density": density, "nnz_per_row": nnz / ROWS}
            f.set_strategy(ta.STRATEGY_AUTO)
            cell["dense_auto_form"] = f.kernel_form(ROWS)
            cell["dense_auto_ms"] = timed(f, lambda: f.predict_raw(x, out))
            want = out.clone()
            cell["fallback_form"], cell["fallback_chunk_rows"] = f.csr_plan(ROWS, nnz)
            cell["fallback_ms"] = timed(f, lambda: f.predict_csr(ip, ix, vals, out))
            same = bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
            if tile:
                f.set_strategy(getattr(ta, "STRATEGY_" + tile))
                cell["dense_tile_form"] = f.kernel_form(ROWS)
                cell["dense_tile_ms"] = timed(f, lambda: f.predict_raw(x, out))
                same = same and bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
                cell["fused_form"], chunk = f.csr_plan(ROWS, nnz)
                assert chunk == 0, cell
                cell["fused_ms"] = timed(f, lambda: f.predict_csr(ip, ix, vals, out))
                same = same and bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
            cell["same_bits"] = same
            cell["rule"] = "fused" if rule.csr_plan(ROWS, nnz)[1] == 0 else "fallback"
            a = min(cell["fused_ms"]) if tile else float("inf")
            b = min(cell["fallback_ms"])
            cell["faster"] = "fused" if a < b else "fallback"
            cell["rule_ok"] = bool((a if cell["rule"] == "fused" else b) <= 1.03 * min(a, b))
            for key in ("dense_auto_ms", "fallback_ms", "dense_tile_ms", "fused_ms"):
                if key in cell:
                    res["spread_max"] = max(res["spread_max"], abs(cell[key][0] - cell[key][1]) / min(cell[key]))
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
            del x, ip, ix, vals, out, want
        f.close()
        rule.close()
    res["src_hash"] = bench.kernel_source_hash()
    res["rule_ok_everywhere"] = all(c["rule_ok"] for c in res["cells"])
    res["same_bits_everywhere"] = all(c["same_bits"] for c in res["cells"])
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "csr_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not res["same_bits_everywhere"]:
        sys.exit("CSR and dense predictions differ")


if __name__ == "__main__":
    main()
