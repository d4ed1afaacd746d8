"""Per-feature contributions (tahoe_forest_predict_contribs): kernel time on BASELINE forests, with the path-element evaluations
per second, an op-count share of the FP32 vector peak, create time, table bytes, a max-error sample against the float64 reference
(tests/contribs_ref.py) and that reference's single-thread CPU time on the same sample.
    python tools/contribs_time.py [out.json] [iterations]
Rows per forest are set below (K3-sized forests are timed on fewer rows: one row evaluates ~0.8 M bins there)."""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "contribs", "contribs_time.json")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
PEAK_FP32 = 157.3e12  # MI355X FP32 vector peak, FLOP/s


def forests():
    _, (nodes, T, D, C), data = bench.baseline_workload(ta, "K1")
    yield "K1", nodes, T, D, C, 1, np.ascontiguousarray(np.resize(data, (100_000, C))), 16
    _, (nodes, T, D, C), data = bench.baseline_workload(ta, "K3")
    nodes = ta.capi.set_probability_weights(nodes, T, D)
    yield "K3_probability_weights", nodes, T, D, C, 1, np.ascontiguousarray(data[:2048]), 0
    _, (nodes, T, D, C), data = bench.baseline_workload(ta, "KR3")
    yield "KR3", nodes, T, D, C, 1, np.ascontiguousarray(data[:2048]), 0
    _, (nodes, T, D, C), data = bench.baseline_workload(ta, "K3")
    nodes = ta.capi.set_probability_weights(nodes, T, D)
    yield "K3_as_10_classes", nodes, T, D, C, 10, np.ascontiguousarray(data[:2048]), 0


def main():
    torch.cuda.set_device(0)
    res = {"unit": "ms per predict_contribs (median of hipEvent pairs after 1 warm-up)", "iterations": ITERS,
           "src_hash": bench.kernel_source_hash(), "forests": {}}
    for name, nodes, T, D, F, K, x, sample in forests():
        cover_note = "as generated"
        try:
            t0 = time.perf_counter()
            f = ta.Forest(nodes, T, D, F, missing=bench.MISSING, num_classes=K, contribs=True)
        except ta.TahoeError as e:  # a reachable node no row of the generator's distribution reaches: both children weigh 0
            nodes = nodes.copy()
            nodes["weight"] += np.float32(1e-6)
            cover_note = "weights + 1e-6 (create refused the generated covers: %s)" % e
            t0 = time.perf_counter()
            f = ta.Forest(nodes, T, D, F, missing=bench.MISSING, num_classes=K, contribs=True)
        create_s = time.perf_counter() - t0
        plain = ta.Forest(nodes, T, D, F, missing=bench.MISSING, num_classes=K)
        table_bytes = f.info().device_bytes - plain.info().device_bytes
        plain.close()
        # paths and their elements, from the reference's path list (host)
        per = nodes.size // T
        n_paths = n_elems = 0
        for t in range(T):
            for leaf, elems in contribs_ref._paths(nodes.reshape(T, per)[t]):
                n_paths += 1
                n_elems += len(elems) + 1
        xd = torch.from_numpy(x).cuda()
        out = f.predict_contribs(xd)
        torch.cuda.synchronize()
        ms = []
        for _ in range(ITERS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f.predict_contribs(xd, out=out)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        med = float(np.median(ms))
        rows = x.shape[0]
        L = n_elems / max(n_paths, 1)
        flop_model = 2.0 * L * L * n_paths * rows  # ~2 L^2 FP32 operations per (row, path): extend + unwind over L lanes
        ent = {"rows": rows, "trees": T, "depth": D, "cols": F, "classes": K, "ms_median": round(med, 3), "ms_all": [round(v, 3) for v in ms],
               "rows_per_s": rows / (med * 1e-3), "paths": n_paths, "path_elements": n_elems, "mean_path_elements": round(L, 2),
               "path_element_row_evals_per_s": n_elems * rows / (med * 1e-3),
               "op_model": "2 L^2 FP32 ops per (row, path), L = mean elements per path incl. root",
               "share_of_fp32_vector_peak_by_op_model": flop_model / (med * 1e-3) / PEAK_FP32,
               "covers": cover_note, "create_s": round(create_s, 3), "table_bytes": int(table_bytes)}
        if sample:
            xs = x[:sample]
            got = out[:sample].cpu().numpy().astype(np.float64).reshape(sample, K, F + 1)
            t0 = time.perf_counter()
            want, A, N = contribs_ref.poly(nodes, T, D, F, xs, bench.MISSING, num_classes=K)
            ent["cpu_reference_s_single_thread_numpy_float64"] = round(time.perf_counter() - t0, 3)
            ent["cpu_reference_rows"] = sample
            ent["max_err_rel_to_sum_abs_phi64"] = float(np.max(np.abs(got - want).max(-1) / (np.abs(want).sum(-1) + 1e-30)))
        res["forests"][name] = ent
        print(name, json.dumps(ent), flush=True)
        f.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
