"""SHAP interaction values (tahoe_forest_predict_interactions): kernel time against tahoe_forest_predict_contribs on the same
rows, with the ratio, the kernel form (LDS slabs or in place), the longest path and the op-model ratio (~ the longest path).
    python tools/interactions_time.py [out.json] [iterations]
Forests: K1 at 10 k rows (LDS form, F = 18), synth 30 x 12 on 256 columns and KR3 on a few dozen rows (in-place form)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import contribs_ref  # noqa: E402
import tahoe_amd as ta  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "interactions", "interactions_time.json")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def forests():
    _, (nodes, T, D, C), data = bench.baseline_workload(ta, "K1")
    yield "K1", nodes, T, D, C, np.ascontiguousarray(np.resize(data, (10_000, C)))
    nodes = ta.synth_forest(30, 12, 256, seed=9, leaf_prob=0.05)
    yield "synth_30x12_on_256", nodes, 30, 12, 256, ta.synth_data(256, 256, seed=10, missing_prob=0.02, missing=bench.MISSING)
    _, (nodes, T, D, C), data = bench.baseline_workload(ta, "KR3")
    yield "KR3", nodes, T, D, C, np.ascontiguousarray(data[:32])


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
    res = {"unit": "ms per call (median of hipEvent pairs after 1 warm-up)", "iterations": ITERS,
           "src_hash": bench.kernel_source_hash(), "forests": {}}
    for name, nodes, T, D, F, x in forests():
        t0 = time.perf_counter()
        f = ta.Forest(nodes, T, D, F, missing=bench.MISSING, contribs=True)
        create_s = time.perf_counter() - t0
        per = nodes.size // T
        longest = n_paths = n_elems = 0
        for t in range(T):
            for leaf, elems in contribs_ref._paths(nodes.reshape(T, per)[t]):
                n_paths += 1
                n_elems += len(elems) + 1
                longest = max(longest, len(elems) + 1)
        xd = torch.from_numpy(x).cuda()
        rows = x.shape[0]
        phi = f.predict_contribs(xd)
        inter = f.predict_interactions(xd)
        c_ms, c_all = timed(lambda: f.predict_contribs(xd, out=phi), ITERS)
        i_ms, i_all = timed(lambda: f.predict_interactions(xd, out=inter), ITERS)
        F1 = F + 1
        ent = {"rows": rows, "trees": T, "depth": D, "cols": F, "form": "lds_slabs" if 4 * F * F + F <= 20 * 1024 else "in_place",
               "paths": n_paths, "path_elements": n_elems, "longest_path_elements": longest,
               "interactions_ms_median": round(i_ms, 3), "interactions_ms_all": [round(v, 3) for v in i_all],
               "contribs_ms_median": round(c_ms, 3), "contribs_ms_all": [round(v, 3) for v in c_all],
               "ratio_interactions_to_contribs": round(i_ms / c_ms, 2),
               "op_model_ratio": "~ longest path (L^3 vs L^2 per path and row)",
               "output_bytes": rows * F1 * F1 * 4, "create_s": round(create_s, 3)}
        res["forests"][name] = ent
        print(name, json.dumps(ent), flush=True)
        f.close()
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as fh:  # after every forest: a time limit on a later one keeps the earlier results
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
