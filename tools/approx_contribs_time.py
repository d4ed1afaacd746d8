"""Saabas contributions (tahoe_forest_predict_contribs_approx): kernel time on the BASELINE forests, beside the same handle's
predict_raw time and the exact TreeSHAP rows/s of profiles/contribs/contribs_time.json.
    python tools/approx_contribs_time.py [out.json] [iterations]
Times are medians of `iterations` hipEvent pairs after one warm-up call.  Lane = row: a batch smaller than the GPU's lanes leaves
most of it idle, so K3 is also timed on 1, 64 and 4096 rows (latency-bound).  Dense covers: set_probability_weights (the
probability of reaching each node under synth_data's distribution; + 1e-6 where create refuses them); KR3 keeps the generator's;
K5 (sparse, no covers of its own) takes uniform covers 1.0."""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "approx_contribs", "approx_contribs_time.json")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(v, 3) for v in ms]


def dense_forest(cfg, K=1, form=None):
    _, (nodes, T, D, F), data = bench.baseline_workload(ta, cfg)
    if cfg != "KR3":
        nodes = ta.capi.set_probability_weights(nodes, T, D)
    note = "probability weights" if cfg != "KR3" else "as generated"
    if form is not None:
        os.environ["TAHOE_APPROX_FORM"] = str(form)
    try:
        try:
            t0 = time.perf_counter()
            f = ta.Forest(nodes, T, D, F, missing=bench.MISSING, num_classes=K, approx_contribs=True)
        except ta.TahoeError as e:
            nodes = nodes.copy()
            nodes["weight"] += np.float32(1e-6)
            note += " + 1e-6 (create refused them: %s)" % e
            t0 = time.perf_counter()
            f = ta.Forest(nodes, T, D, F, missing=bench.MISSING, num_classes=K, approx_contribs=True)
    finally:
        os.environ.pop("TAHOE_APPROX_FORM", None)
    create_s = time.perf_counter() - t0
    plain = ta.Forest(nodes, T, D, F, missing=bench.MISSING, num_classes=K)
    table = f.info().device_bytes - plain.info().device_bytes
    plain.close()
    return f, data, dict(trees=T, depth=D, cols=F, classes=K, covers=note, create_s=round(create_s, 3), table_bytes=table)


def sparse_forest():
    _, (sn, tr, F), data = bench.baseline_workload(ta, "K5")
    t0 = time.perf_counter()
    f = ta.capi.SparseForest(sn, tr, F, missing=bench.MISSING, covers=np.ones(sn.size, np.float32), approx_contribs=True)
    create_s = time.perf_counter() - t0
    plain = ta.capi.SparseForest(sn, tr, F, missing=bench.MISSING)
    table = f.info().device_bytes - plain.info().device_bytes
    plain.close()
    return f, data, dict(trees=int(tr.size), nodes=int(sn.size), cols=F, classes=1, covers="uniform 1.0",
                         create_s=round(create_s, 3), table_bytes=table)


def measure(f, x, meta):
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rows, K, F = x.shape[0], f.num_classes, f.num_cols
    out = torch.empty((rows, K, F + 1) if K > 1 else (rows, F + 1), dtype=torch.float32, device="cuda")
    sums = torch.empty((rows, K) if K > 1 else (rows,), dtype=torch.float32, device="cuda")
    ms, ms_all = timed(lambda: f.predict_contribs_approx(xd, out=out))
    raw_ms, _ = timed(lambda: f.predict_raw(xd, sums=sums))
    out_bytes = rows * K * (F + 1) * 4
    ent = dict(meta, rows=rows, ms_median=round(ms, 4), ms_all=ms_all, rows_per_s=rows / (ms * 1e-3),
               predict_raw_ms_median=round(raw_ms, 4), ratio_to_predict_raw=round(ms / raw_ms, 2),
               output_bytes=out_bytes, output_write_GBps=round(out_bytes / (ms * 1e-3) / 1e9, 1))
    del xd, out, sums
    torch.cuda.empty_cache()
    return ent


def main():
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, "profiles", "contribs", "contribs_time.json")) as fh:
        exact = {k: v["rows_per_s"] for k, v in json.load(fh)["forests"].items()}
    res = {"unit": "ms per predict_contribs_approx (median of %d hipEvent pairs after 1 warm-up)" % ITERS, "iterations": ITERS,
           "src_hash": bench.kernel_source_hash(), "tool": "python tools/approx_contribs_time.py <out.json> %d" % ITERS,
           "exact_treeshap_rows_per_s": exact, "forests": {}}

    def save():
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as fh:
            json.dump(res, fh, indent=1)

    f, data, meta = dense_forest("K1")
    res["forests"]["K1"] = measure(f, data, meta)
    f.close()
    save()
    f, data, meta = dense_forest("K2")
    res["forests"]["K2"] = measure(f, data, meta)
    f.close()
    save()
    f, data, meta = dense_forest("K3")
    for r in (1, 64, 4096):
        res["forests"]["K3_rows_%d" % r] = measure(f, data[:r], meta)
    res["forests"]["K3"] = measure(f, data, meta)
    res["forests"]["K3"]["speedup_vs_exact_rows_per_s"] = round(res["forests"]["K3"]["rows_per_s"] / exact["K3_probability_weights"], 1)
    f.close()
    save()
    f, data, meta = dense_forest("K3", form=1)  # experiment: one wave's LDS slab (66 KB) instead of the in-place form
    res["forests"]["K3_lds_slab_form"] = measure(f, data, meta)
    f.close()
    save()
    f, data, meta = dense_forest("KR3")
    res["forests"]["KR3"] = measure(f, data, meta)
    res["forests"]["KR3"]["speedup_vs_exact_rows_per_s"] = round(res["forests"]["KR3"]["rows_per_s"] / exact["KR3"], 1)
    f.close()
    save()
    f, data, meta = sparse_forest()
    res["forests"]["K5"] = measure(f, data, meta)
    f.close()
    save()
    f, data, meta = dense_forest("K3", K=10)
    res["forests"]["K3_as_10_classes"] = measure(f, data, meta)
    f.close()
    save()
    for k, v in res["forests"].items():
        print(f"{k:18s} rows {v['rows']:>8d}  {v['ms_median']:>10.3f} ms  raw {v['predict_raw_ms_median']:>9.3f} ms  "
              f"x{v['ratio_to_predict_raw']}", flush=True)


if __name__ == "__main__":
    main()
