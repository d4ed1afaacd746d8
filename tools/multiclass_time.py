"""Multi-class forests on 1 M rows: the multi-class handle (one quantise pass, one walk, a per-class flush in the consumer)
against (i) an ordinary handle on the same trees -- the same walk with a single sum -- and (ii) one handle per class run back
to back.  Median of hipEvent-timed predicts (raw margins) after warm-up; the three are timed in turn inside every iteration.
Forest (a): K3's shape (1000 trees of depth 12, 256 features) read as 10 classes x 100 rounds; (b): a histogram-style
7-class x 150-round forest of depth 8 on 54 features.   python tools/multiclass_time.py [rows] [iterations] [out.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tahoe_amd as ta  # noqa: E402

MISSING = -999.0
R = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
OUT = sys.argv[3] if len(sys.argv) > 3 else None
WARMUP = 5


def forests():
    T, D, C = 1000, 12, 256
    yield "a_k3_10x100", 10, T, D, C, ta.synth_forest(T, D, C, seed=42), ta.synth_data(R, C, seed=43)
    T, D, C = 7 * 150, 8, 54
    yield ("b_hist_7x150", 7, T, D, C, ta.synth_forest_hist(T, D, C, seed=42, feature_seed=7, max_bins=254, scale_decades=3.0),
           ta.synth_data_hist(R, C, seed=43, feature_seed=7, scale_decades=3.0))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


results = {"rows": R, "iterations": ITERS, "warmup": WARMUP, "unit": "ms per predict (median of hipEvent pairs)", "forests": {}}
for name, K, T, D, C, nodes, data in forests():
    x = torch.from_numpy(data).cuda()
    mc = ta.Forest(nodes, T, D, C, missing=MISSING, num_classes=K)
    single = ta.Forest(nodes, T, D, C, missing=MISSING)
    by_tree = nodes.reshape(T, -1)
    per = [ta.Forest(np.ascontiguousarray(by_tree[c::K]).reshape(-1), T // K, D, C, missing=MISSING) for c in range(K)]
    out_mc = torch.empty((R, K), dtype=torch.float32, device="cuda")
    out_1 = torch.empty(R, dtype=torch.float32, device="cuda")
    out_c = [torch.empty(R, dtype=torch.float32, device="cuda") for _ in range(K)]
    for f in [mc, single] + per:
        f.reserve(R)
    runs = {"multiclass": lambda: mc.predict_raw(x, out_mc), "single_sum": lambda: single.predict_raw(x, out_1),
            "per_class_handles": lambda: [p.predict_raw(x, o) for p, o in zip(per, out_c)]}
    ev = {k: [] for k in runs}
    for i in range(WARMUP + ITERS):
        for k, fn in runs.items():
            pair = timed(fn)
            if i >= WARMUP:
                ev[k].append(pair)
    torch.cuda.synchronize()
    for f in [mc, single] + per:
        f.check()
    # the margins are the per-class handles' sums, bit for bit
    got = out_mc.cpu().numpy()
    same = all(np.array_equal(got[:, c].view(np.uint32), out_c[c].cpu().numpy().view(np.uint32)) for c in range(K))
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    results["forests"][name] = {
        "classes": K, "trees": T, "depth": D, "cols": C,
        "forms": {"multiclass": mc.kernel_form(R), "single_sum": single.kernel_form(R), "per_class_handle": per[0].kernel_form(R)},
        "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in ms.items()}, "max_ms": {k: float(np.max(v)) for k, v in ms.items()},
        "multiclass_over_single_sum": med["multiclass"] / med["single_sum"],
        "multiclass_over_per_class_handles": med["multiclass"] / med["per_class_handles"],
        "margins_equal_per_class_handles": bool(same),
    }
    print(name, json.dumps(results["forests"][name]), flush=True)
    for f in [mc, single] + per:
        f.close()
    del x
    torch.cuda.empty_cache()
if OUT:
    with open(OUT, "w") as fh:
        json.dump(results, fh, indent=1)
