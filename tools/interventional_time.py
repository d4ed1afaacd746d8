"""Interventional TreeSHAP (tahoe_forest_predict_contribs_interventional): kernel time against tahoe_forest_predict_contribs on
the same rows, the time of tahoe_forest_set_background, and the op-model rate in evaluations of (row, background row, bin lane).
    python tools/interventional_time.py [out.json] [iterations]
Forests: K1 at 10 k rows, KR3 at 32 rows and synth 30 x 12 on 256 columns at 256 rows, each against B = 100 background rows."""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "interventional", "interventional_time.json")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
B = 100


def forests():
    _, (nodes, T, D, C), data = bench.baseline_workload(ta, "K1")
    yield "K1", nodes, T, D, C, np.ascontiguousarray(np.resize(data, (10_000, C))), np.ascontiguousarray(data[-B:])
    _, (nodes, T, D, C), data = bench.baseline_workload(ta, "KR3")
    yield "KR3", nodes, T, D, C, np.ascontiguousarray(data[:32]), np.ascontiguousarray(data[-B:])
    nodes = ta.synth_forest(30, 12, 256, seed=9, leaf_prob=0.05)
    data = ta.synth_data(256 + B, 256, seed=10, missing_prob=0.02, missing=bench.MISSING)
    yield "synth_30x12_on_256", nodes, 30, 12, 256, np.ascontiguousarray(data[:256]), np.ascontiguousarray(data[256:])


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def main():
    torch.cuda.set_device(0)
    res = {"unit": "ms per call (median of hipEvent pairs after 1 warm-up)", "iterations": ITERS, "background_rows": B,
           "src_hash": bench.kernel_source_hash(),
           "op_model": "evaluations = rows x background rows x 64 x bins (every lane of every bin, padding included); "
                       "~17 VALU + 1 LDS read per evaluation and wave (ISA of interventional_kernel<true>)",
           "forests": {}}
    for name, nodes, T, D, F, x, bg in forests():
        t0 = time.perf_counter()
        f = ta.Forest(nodes, T, D, F, missing=bench.MISSING, contribs=True)
        create_s = time.perf_counter() - t0
        xd, bgd = torch.from_numpy(x).cuda(), torch.from_numpy(bg).cuda()
        base = f.info().device_bytes
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f.set_background(bgd)
        set_ms = (time.perf_counter() - t0) * 1e3
        bins = (f.info().device_bytes - base - (1024 + 1) * 4) // (8 * B)
        rows = x.shape[0]
        phi = f.predict_contribs(xd)
        iphi = f.predict_contribs_interventional(xd)
        c_ms, c_all = timed(lambda: f.predict_contribs(xd, out=phi), ITERS)
        i_ms, i_all = timed(lambda: f.predict_contribs_interventional(xd, out=iphi), ITERS)
        evals = rows * B * 64 * bins
        ent = {"rows": rows, "trees": T, "depth": D, "cols": F, "bins": int(bins),
               "interventional_ms_median": round(i_ms, 3), "interventional_ms_all": [round(v, 3) for v in i_all],
               "contribs_ms_median": round(c_ms, 3), "contribs_ms_all": [round(v, 3) for v in c_all],
               "ratio_interventional_to_contribs": round(i_ms / c_ms, 2),
               "set_background_ms": round(set_ms, 3), "background_mask_bytes": int(bins * 8 * B),
               "evaluations": int(evals), "evaluations_per_s": float(f"{evals / (i_ms * 1e-3):.4g}"),
               "create_s": round(create_s, 3)}
        res["forests"][name] = ent
        print(name, json.dumps(ent), flush=True)
        f.close()
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as fh:  # after every forest: a time limit on a later one keeps the earlier results
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
