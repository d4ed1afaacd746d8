"""CSR rows on oblivious and vector-leaf handles (TAHOE_CREATE_CSR): the fused one-wave tile kernels, the
chunked fallback and today's dense call, timed side by side with the methodology of tools/csr_time.py.

Shapes, 64 features unless said: tools/oblivious_time.py's catboost_default_depth6 (1000 oblivious trees of depth 6, K = 1) and
vector_leaves_k8 (100 such trees, K = 8), tools/vector_time.py's random_forest_k8 (100 irregular trees of depth <= 16, K = 8) and
the same trees with K = 10 (two class blocks: the tile is staged twice), and one wide forest per kind on 512 features (a tile of
128 KiB: one workgroup per CU).
Data: ROWS rows with 1 %, 5 %, 25 % and 100 % of the entries stored (uniform in [-1, 1)), built on the device.
Per cell: (a) predict_csr with ROWTILE forced: the fused form; (b) predict_csr on a handle created with TAHOE_CSR_FUSED=0: densify + the
handle's own tile kernel, chunk by chunk; (c) what a caller has today: predict on the already dense matrix under AUTO -- the
caller's own densify is not counted.  Every time is the median of ITERS event-timed calls after WARMUP, each cell measured twice;
`spread` is the relative distance between the two medians.  The bits of (a) and (b) are compared with (c).  auto_pick is
what AUTO takes on a handle created without the knob; auto_loses: that pick is slower than the other CSR path by more than the
larger of the two spreads of that cell.
    python tools/native_csr_time.py [out_dir] [iterations] [rows]  -> <out_dir>/native_csr_time.json (default profiles/native_csr)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402

ARGS = sys.argv[1:]
OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "native_csr")
ITERS = int(ARGS[1]) if len(ARGS) > 1 else 20
ROWS = int(ARGS[2]) if len(ARGS) > 2 else 200_000
WARMUP = 3
MISSING = -999.0
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


def timed(call):
    """Two medians (ms) of ITERS event-timed launches each of call()."""
    meds = []
    for _ in range(2):
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
        for a, b in ev:
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        meds.append(float(np.median([a.elapsed_time(b) for a, b in ev])))
    return meds


def spread(pair):
    return abs(pair[0] - pair[1]) / min(pair)


def oblivious(name, T, D, cols, K):
    """tools/oblivious_time.py's forest of that name -> make(): a handle with TAHOE_CREATE_CSR"""
    rng = np.random.default_rng(len(name))
    fids = rng.integers(0, cols, T * D)
    thr = rng.uniform(-1.0, 1.0, T * D).astype(np.float32)
    def_left = rng.integers(0, 2, T * D).astype(bool)
    leaves = rng.standard_normal(T * (1 << D) * K).astype(np.float32)
    return lambda: ta.ObliviousForest(np.full(T, D, np.int32), fids, thr, def_left, leaves, cols, leaf_dim=K, missing=MISSING, csr=True)


def vector(T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K):
    """tools/vector_time.py's forest -> make()"""
    nodes, trees = ta.capi.synth_sparse_forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed)
    rng = np.random.default_rng(seed + 1)
    is_leaf = nodes["bits"] < 0
    L = int(is_leaf.sum())
    nodes["left_idx"][is_leaf] = rng.permutation(L).astype(np.int32)
    nodes["val"][is_leaf] = 0.0
    leaves = rng.standard_normal((L, K)).astype(np.float32)
    return lambda: ta.VectorForest(nodes, trees, leaves, cols, missing=MISSING, csr=True)


def shapes():
    yield "oblivious, 1000 x depth 6, 64 features, K = 1", 64, 1, oblivious("catboost_default_depth6", 1000, 6, 64, 1)
    yield "oblivious, 100 x depth 6, 64 features, K = 8", 64, 8, oblivious("vector_leaves_k8", 100, 6, 64, 8)
    yield "vector-leaf, 100 x depth <= 16, 64 features, K = 8", 64, 8, vector(100, 64, 4, 16, 0.32, 65535, 77, 8)
    yield "vector-leaf, 100 x depth <= 16, 64 features, K = 10", 64, 10, vector(100, 64, 4, 16, 0.32, 65535, 77, 10)
    yield "oblivious, 100 x depth 6, 512 features, K = 8", 512, 8, oblivious("vector_leaves_k8", 100, 6, 512, 8)
    yield "vector-leaf, 100 x depth <= 16, 512 features, K = 8", 512, 8, vector(100, 512, 4, 16, 0.32, 65535, 77, 8)


def main():
    res = {"rows": ROWS, "iterations": ITERS, "warmup": WARMUP, "cells": [], "spread_max": 0.0}
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "native_csr_time.json")
    for name, cols, K, make in shapes():
        f = make()  # AUTO: the rule, asked only; (a) and (c) run with ROWTILE forced, which is AUTO's strategy on dense rows here
        os.environ["TAHOE_CSR_FUSED"] = "0"
        g = make()  # AUTO on CSR rows = the chunked fallback
        del os.environ["TAHOE_CSR_FUSED"]
        for density in DENSITIES:
            x, ip, ix, vals = make_rows(cols, density, seed=int(density * 1000) + cols)
            nnz = int(vals.numel())
            out = torch.empty((ROWS, K) if K > 1 else (ROWS,), dtype=torch.float32, device="cuda")
            cell = {"shape": name, "num_cols": cols, "leaf_dim": K, "density": density, "nnz_per_row": nnz / ROWS}
            f.set_strategy(ta.STRATEGY_AUTO)
            cell["dense_form"] = f.kernel_form(ROWS)
            cell["dense_ms"] = timed(lambda: f.predict(x, out))
            want = out.clone()
            cell["auto_form"], chunk = f.csr_plan(ROWS, nnz)
            cell["auto_pick"] = "fused" if chunk == 0 else "fallback"
            f.set_strategy(ta.STRATEGY_ROWTILE)
            cell["fused_form"], chunk = f.csr_plan(ROWS, nnz)
            assert chunk == 0, cell
            cell["fused_ms"] = timed(lambda: f.predict_csr(ip, ix, vals, out))
            same = bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
            cell["fallback_form"], cell["fallback_chunk_rows"] = g.csr_plan(ROWS, nnz)
            assert cell["fallback_chunk_rows"] > 0, cell
            cell["fallback_ms"] = timed(lambda: g.predict_csr(ip, ix, vals, out))
            same = same and bool(torch.equal(out.view(torch.int32), want.view(torch.int32)))
            f.check()
            g.check()
            cell["same_bits"] = same
            a, b, c = min(cell["fused_ms"]), min(cell["fallback_ms"]), min(cell["dense_ms"])
            cell["spread"] = {k: spread(cell[k + "_ms"]) for k in ("fused", "fallback", "dense")}
            cell["fused_over_fallback"], cell["fused_over_dense"] = a / b, a / c
            noise = max(cell["spread"]["fused"], cell["spread"]["fallback"])
            picked, other = (a, b) if cell["auto_pick"] == "fused" else (b, a)
            cell["auto_loses"] = bool(picked > other * (1.0 + noise))
            cell["csr_slower_than_dense"] = bool(picked > c * (1.0 + max(noise, cell["spread"]["dense"])))
            res["spread_max"] = max(res["spread_max"], *cell["spread"].values())
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
            del x, ip, ix, vals, out, want
        f.close()
        g.close()
        res["src_hash"] = bench.kernel_source_hash()
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
    by = {(c["shape"], c["density"]): c for c in res["cells"]}
    k8, k10 = "vector-leaf, 100 x depth <= 16, 64 features, K = 8", "vector-leaf, 100 x depth <= 16, 64 features, K = 10"
    res["k10_over_k8"] = {str(d): {"fused": min(by[k10, d]["fused_ms"]) / min(by[k8, d]["fused_ms"]),
                                   "dense": min(by[k10, d]["dense_ms"]) / min(by[k8, d]["dense_ms"])} for d in DENSITIES}
    res["auto_loses_anywhere"] = any(c["auto_loses"] for c in res["cells"])
    res["same_bits_everywhere"] = all(c["same_bits"] for c in res["cells"])
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    if not res["same_bits_everywhere"]:
        sys.exit("CSR and dense predictions differ")


if __name__ == "__main__":
    main()
