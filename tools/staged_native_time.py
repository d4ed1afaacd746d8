"""Staged prediction on oblivious and vector-leaf handles (TAHOE_CREATE_STAGED) against what a caller does
without it, timed side by side.

Shapes, ROWS rows uniform in [-1, 1) with 2 % missing: tools/oblivious_time.py's catboost_default_depth6 (1000 oblivious trees of
depth 6 on 64 features, K = 1) and vector_leaves_k8 (100 such trees, K = 8), and tools/vector_time.py's random_forest_k8 (100
irregular trees of depth <= 16 on 64 features, K = 8).  Per shape:
  (a) predict_staged with 1, 10 and 100 evenly spaced stages (capped at the number of trees; the last one the whole forest), AUTO;
  (b) plain predict on the same handle with the strategy (a) ran forced: the same walk without the stage stores;
  (c) what a caller does today: one native handle per stage, created from the forest cut to that stage, predicted one after
      another -- the sum of the handles' times; their create time (host wall clock) is reported separately.
Every time is the median of ITERS event-timed calls after WARMUP, each cell measured twice; `spread` is the relative distance
between the two medians.  The bits of every stage of (a) are compared with (c)'s handle of that stage.  pass: (a) with one stage
is not slower than (b) by more than the spread the tool finds for (b).
    python tools/staged_native_time.py [out_dir] [iterations] [rows]  -> <out_dir>/staged_native_time.json (default
    profiles/staged_native)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402

ARGS = sys.argv[1:]
OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "staged_native")
ITERS = int(ARGS[1]) if len(ARGS) > 1 else 20
ROWS = int(ARGS[2]) if len(ARGS) > 2 else 1_000_000
WARMUP = 3
MISSING = -999.0
STAGE_COUNTS = (1, 10, 100)


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
    """tools/oblivious_time.py's forest of that name -> make(n, staged): the handle of its first n trees"""
    rng = np.random.default_rng(len(name))
    fids = rng.integers(0, cols, T * D)
    thr = rng.uniform(-1.0, 1.0, T * D).astype(np.float32)
    def_left = rng.integers(0, 2, T * D).astype(bool)
    leaves = rng.standard_normal(T * (1 << D) * K).astype(np.float32)
    return lambda n, staged=False: ta.ObliviousForest(np.full(n, D, np.int32), fids[: n * D], thr[: n * D], def_left[: n * D],
                                                      leaves[: n * (1 << D) * K], cols, leaf_dim=K, missing=MISSING, staged=staged)


def vector(T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K):
    """tools/vector_time.py's forest -> make(n, staged)"""
    nodes, trees = ta.capi.synth_sparse_forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed)
    rng = np.random.default_rng(seed + 1)
    is_leaf = nodes["bits"] < 0
    L = int(is_leaf.sum())
    nodes["left_idx"][is_leaf] = rng.permutation(L).astype(np.int32)
    nodes["val"][is_leaf] = 0.0
    leaves = rng.standard_normal((L, K)).astype(np.float32)
    ends = np.append(trees, nodes.size)
    return lambda n, staged=False: ta.VectorForest(nodes[: ends[n]], trees[:n], leaves, cols, missing=MISSING, staged=staged)


def shapes():
    yield "oblivious, 1000 x depth 6, 64 features, K = 1", 64, 1000, 1, oblivious("catboost_default_depth6", 1000, 6, 64, 1)
    yield "oblivious, 100 x depth 6, 64 features, K = 8", 64, 100, 8, oblivious("vector_leaves_k8", 100, 6, 64, 8)
    yield "vector-leaf, 100 x depth <= 16, 64 features, K = 8", 64, 100, 8, vector(100, 64, 4, 16, 0.32, 65535, 77, 8)


def main():
    res = {"rows": ROWS, "iterations": ITERS, "warmup": WARMUP, "shapes": []}
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "staged_native_time.json")
    for name, cols, T, K, make in shapes():
        torch.manual_seed(1234)
        x = torch.rand((ROWS, cols), device="cuda") * 2.0 - 1.0
        x[torch.rand((ROWS, cols), device="cuda") < 0.02] = MISSING
        f = make(T, staged=True)
        out1 = torch.empty((ROWS, K) if K > 1 else (ROWS,), dtype=torch.float32, device="cuda")
        entry = {"shape": name, "num_trees": T, "leaf_dim": K, "auto_form": f.kernel_form(ROWS), "staged": [], "same_bits": True}
        grids = {s: [T * (i + 1) // min(s, T) for i in range(min(s, T))] for s in STAGE_COUNTS}
        # (c), per stage of the finest grid: the coarser grids are subsets of it
        today = {}
        for n in sorted({n for g in grids.values() for n in g}):
            t0 = time.perf_counter()
            cut = make(n)
            create_s = time.perf_counter() - t0
            today[n] = {"ms": timed(lambda: cut.predict(x, out1)), "create_s": create_s,
                        "bits": out1.clone() if n in grids[10] else None}
            cut.close()
        for s in STAGE_COUNTS:
            stages = grids[s]
            f.set_strategy(ta.STRATEGY_AUTO)
            f.set_stages(stages)
            strat = f.staged_strategy(ROWS)
            out = torch.empty((ROWS, len(stages)) + ((K,) if K > 1 else ()), dtype=torch.float32, device="cuda")
            a = timed(lambda: f.predict_staged(x, out))
            f.check()
            for i, n in enumerate(stages):  # (every tenth of the forest keeps its bits)
                if today[n]["bits"] is not None:
                    entry["same_bits"] &= bool(torch.equal(out[:, i].contiguous().view(torch.int32), today[n]["bits"].view(torch.int32)))
            f.set_strategy(strat)
            b = timed(lambda: f.predict(x, out1))
            c = [sum(today[n]["ms"][k] for n in stages) for k in range(2)]
            cell = {"stages": len(stages), "strategy": ta.STRATEGY_NAMES[strat], "staged_ms": a, "plain_same_strategy_ms": b,
                    "handle_per_stage_ms": c, "handle_per_stage_create_s": sum(today[n]["create_s"] for n in stages),
                    "spread": {"staged": spread(a), "plain": spread(b), "handle_per_stage": spread(c)},
                    "staged_over_plain": min(a) / min(b), "staged_over_handle_per_stage": min(a) / min(c)}
            entry["staged"].append(cell)
            print(json.dumps({"shape": name, **cell}), flush=True)
            del out
        one = entry["staged"][0]
        entry["pass"] = bool(min(one["staged_ms"]) <= min(one["plain_same_strategy_ms"]) * (1.0 + one["spread"]["plain"]))
        f.close()
        res["shapes"].append(entry)
        res["src_hash"] = bench.kernel_source_hash()
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
        del x, today
    res["pass"] = all(e["pass"] for e in res["shapes"])
    res["same_bits_everywhere"] = all(e["same_bits"] for e in res["shapes"])
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    if not res["same_bits_everywhere"]:
        sys.exit("staged and per-handle predictions differ")


if __name__ == "__main__":
    main()
