"""Staged prediction (tahoe_forest_predict_staged) against what a caller does without it, timed side by side.

Forests: K3's (1000 trees of depth 12 on 256 features) and K5's sparse forest (2000 irregular trees of depth 4..24), 200 k rows
uniform in [-1, 1), built on the device.  Per forest:
  (a) predict_staged with 1, 10 and 100 evenly spaced stages (the last one the whole forest), under AUTO;
  (b) plain predict on the same handle with the strategy (a) ran forced: the same walk without the stage stores;
  (c) what a caller does today: one handle per stage, created from the forest cut to that stage, predicted one after another
      under AUTO -- the sum of the handles' times; their create time (host wall clock) is reported separately.
Every time is the median of ITERS event-timed calls after WARMUP, each cell measured twice; `spread` is the relative distance
between the two medians.  The bits of every stage of (a) are compared with (c)'s handle of that stage.  pass: (a) with one
stage is not slower than (b) by more than the spread the tool finds for (b).
    python tools/staged_time.py [out_dir] [iterations]      -> <out_dir>/staged_time.json (default profiles/staged)"""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "staged")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 3
MISSING = -999.0
ROWS = 200_000
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


def forests():
    T, D, C, _, fs, _, _, _ = bench.BASELINE_SHAPES["K3"]
    nodes = ta.synth_forest(T, D, C, seed=fs)
    per = ta.capi.tree_num_nodes(D)
    yield "K3 (1000 x depth 12, 256 features)", C, T, lambda n: ta.Forest(nodes[: n * per], n, D, C, missing=MISSING)
    k = bench.K5_SHAPE
    sn, tr = ta.capi.synth_sparse_forest(k["trees"], k["cols"], k["min_depth"], k["max_depth"], k["leaf_prob"], k["max_tree_nodes"],
                                         k["forest_seed"])
    ends = np.append(tr, sn.size)
    yield ("K5 (2000 sparse trees, 256 features)", k["cols"], k["trees"],
           lambda n: ta.capi.SparseForest(sn[: ends[n]], tr[:n], k["cols"], missing=MISSING))


def main():
    res = {"rows": ROWS, "iterations": ITERS, "warmup": WARMUP, "forests": []}
    os.makedirs(OUT, exist_ok=True)
    for name, cols, T, make in forests():
        g = torch.Generator(device="cuda").manual_seed(cols + T)
        x = (torch.rand((ROWS, cols), generator=g, device="cuda") * 2.0 - 1.0).contiguous()
        f = make(T)
        out1 = torch.empty(ROWS, dtype=torch.float32, device="cuda")
        entry = {"forest": name, "num_trees": T, "auto_form": f.kernel_form(ROWS), "staged": [], "same_bits": True}
        # (c), per stage of the finest grid: the coarser grids are subsets of it
        today = {}
        for n in sorted({T * (i + 1) // s for s in STAGE_COUNTS for i in range(s)}):
            t0 = time.perf_counter()
            cut = make(n)
            create_s = time.perf_counter() - t0
            today[n] = {"ms": timed(lambda: cut.predict(x, out1)), "create_s": create_s, "form": cut.kernel_form(ROWS),
                        "bits": out1.clone() if n % (T // 10) == 0 else None}
            cut.close()
        for s in STAGE_COUNTS:
            stages = [T * (i + 1) // s for i in range(s)]
            f.set_strategy(ta.STRATEGY_AUTO)
            f.set_stages(stages)
            strat = f.staged_strategy(ROWS)
            out = torch.empty((ROWS, s), dtype=torch.float32, device="cuda")
            a = timed(lambda: f.predict_staged(x, out))
            f.check()
            for i, n in enumerate(stages):  # (every tenth of the forest keeps its bits)
                if today[n]["bits"] is not None:
                    entry["same_bits"] &= bool(torch.equal(out[:, i].contiguous().view(torch.int32), today[n]["bits"].view(torch.int32)))
            f.set_strategy(strat)
            b = timed(lambda: f.predict(x, out1))
            c = [sum(today[n]["ms"][k] for n in stages) for k in range(2)]
            cell = {"stages": s, "strategy": ta.STRATEGY_NAMES[strat], "staged_ms": a, "plain_same_strategy_ms": b,
                    "handle_per_stage_auto_ms": c, "handle_per_stage_create_s": sum(today[n]["create_s"] for n in stages),
                    "spread": {"staged": spread(a), "plain": spread(b), "handle_per_stage": spread(c)},
                    "staged_over_plain": min(a) / min(b), "handle_per_stage_over_staged": min(c) / min(a)}
            entry["staged"].append(cell)
            print(json.dumps({"forest": name, **cell}), flush=True)
            del out
        one = entry["staged"][0]
        entry["pass"] = bool(min(one["staged_ms"]) <= min(one["plain_same_strategy_ms"]) * (1.0 + one["spread"]["plain"]))
        entry["handle_per_stage_forms"] = sorted({v["form"] for v in today.values()})
        f.close()
        res["forests"].append(entry)
        res["src_hash"] = bench.kernel_source_hash()
        with open(os.path.join(OUT, "staged_time.json"), "w") as fh:
            json.dump(res, fh, indent=1)
        del x, today
    res["pass"] = all(e["pass"] for e in res["forests"])
    res["same_bits_everywhere"] = all(e["same_bits"] for e in res["forests"])
    with open(os.path.join(OUT, "staged_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not res["same_bits_everywhere"]:
        sys.exit("staged and per-handle predictions differ")


if __name__ == "__main__":
    main()
