"""Multi-class and TreeSHAP sparse handles on an MI355X.
(a) K5's forest (2000 irregular trees of depth 4..24 on 256 features, 200 k rows) read as 10 classes x 200 trees, AUTO: the
    multi-class sparse handle against (i) the single-sum sparse handle on the same trees and (ii) ten per-class sparse handles
    run back to back; the three are timed in turn inside every iteration, median of hipEvent pairs after warm-up.  The margins
    are checked bit for bit against the per-class handles.
(b) TreeSHAP on one irregular forest (500 trees of depth 4..16 on 32 features, random positive covers, 10 k rows):
    predict_contribs and, against B = 100 background rows, set_background and predict_contribs_interventional; path-table and
    background sizes from tahoe_forest_get_info().device_bytes.
    python tools/sparse_classes_time.py [out_dir] [iterations]"""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_classes")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def sub_forest(sn, tr, c, C):
    ends = np.append(tr[1:], sn.size)
    idx = range(c, tr.size, C)
    nodes = np.concatenate([sn[tr[t]:ends[t]] for t in idx])
    roots = np.cumsum([0] + [int(ends[t] - tr[t]) for t in idx][:-1]).astype(np.int32)
    return nodes, roots


def classes_leg():
    K = 10
    _, (sn, tr, cols), data = bench.baseline_workload(ta, "K5")
    R = data.shape[0]
    x = torch.from_numpy(data).cuda()
    mc = ta.capi.SparseForest(sn, tr, cols, num_classes=K)
    single = ta.capi.SparseForest(sn, tr, cols)
    per = [ta.capi.SparseForest(*sub_forest(sn, tr, c, K), cols) for c in range(K)]
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
    got = out_mc.cpu().numpy()
    same = all(np.array_equal(got[:, c].view(np.uint32), out_c[c].cpu().numpy().view(np.uint32)) for c in range(K))
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = {"workload": f"K5 forest ({tr.size} trees, {sn.size} nodes, depth 4-24, {cols} features) as {K} classes x {tr.size // K}, "
                       f"{R} rows, AUTO",
           "forms": {"multiclass": mc.kernel_form(R), "single_sum": single.kernel_form(R), "per_class_handle": per[0].kernel_form(R)},
           "median_ms": med, "min_ms": {k: float(np.min(v)) for k, v in ms.items()},
           "max_ms": {k: float(np.max(v)) for k, v in ms.items()},
           "multiclass_over_single_sum": med["multiclass"] / med["single_sum"],
           "multiclass_over_per_class_handles": med["multiclass"] / med["per_class_handles"],
           "margins_equal_per_class_handles": bool(same)}
    for f in [mc, single] + per:
        f.close()
    return res


def shap_leg():
    T, F, R, B = 500, 32, 10_000, 100
    sn, tr = ta.capi.synth_sparse_forest(T, F, 4, 16, 0.32, 65535, 77)
    covers = np.random.default_rng(78).uniform(0.05, 1.0, sn.size).astype(np.float32)
    data = ta.synth_data(R + B, F, seed=79, missing_prob=0.02, missing=bench.MISSING)
    plain = ta.capi.SparseForest(sn, tr, F, missing=bench.MISSING)
    t0 = time.perf_counter()
    f = ta.capi.SparseForest(sn, tr, F, missing=bench.MISSING, covers=covers, contribs=True)
    create_s = time.perf_counter() - t0
    x, bg = torch.from_numpy(np.ascontiguousarray(data[:R])).cuda(), torch.from_numpy(np.ascontiguousarray(data[R:])).cuda()
    base = plain.info().device_bytes
    with_tables = f.info().device_bytes
    phi = torch.empty((R, F + 1), dtype=torch.float32, device="cuda")
    ms_c = []
    for i in range(2 + max(ITERS // 4, 3)):  # calls of a second or so: fewer of them
        pair = timed(lambda: f.predict_contribs(x, phi))
        if i >= 2:
            ms_c.append(pair)
    torch.cuda.synchronize()  # the queued contribs calls are not part of set_background
    t0 = time.perf_counter()
    f.set_background(bg)
    torch.cuda.synchronize()
    bg_s = time.perf_counter() - t0
    with_bg = f.info().device_bytes
    iv = torch.empty((R, F + 1), dtype=torch.float32, device="cuda")
    ms_i = []
    for i in range(2 + max(ITERS // 4, 3)):
        pair = timed(lambda: f.predict_contribs_interventional(x, iv))
        if i >= 2:
            ms_i.append(pair)
    torch.cuda.synchronize()
    f.check()
    ms_c = [a.elapsed_time(b) for a, b in ms_c]
    ms_i = [a.elapsed_time(b) for a, b in ms_i]
    res = {"workload": f"synthetic sparse forest {T} trees depth 4-16 on {F} features ({sn.size} nodes), random covers, {R} rows, "
                       f"B = {B} background rows",
           "create_with_tables_s": create_s, "set_background_s": bg_s,
           "contribs_median_ms": float(np.median(ms_c)), "contribs_min_ms": float(np.min(ms_c)),
           "interventional_median_ms": float(np.median(ms_i)), "interventional_min_ms": float(np.min(ms_i)),
           "device_bytes": {"forest": base, "with_path_tables": with_tables, "with_background": with_bg,
                            "path_tables": with_tables - base, "background": with_bg - with_tables},
           "finite": bool(torch.isfinite(phi).all().item() and torch.isfinite(iv).all().item())}
    f.close()
    plain.close()
    return res


def main():
    torch.cuda.set_device(0)
    os.makedirs(OUT, exist_ok=True)
    res = {"unit": "ms per call (median of hipEvent pairs after warm-up; SHAP calls: max(iterations / 4, 3) after 2)",
           "iterations": ITERS, "warmup": WARMUP,
           "src_hash": bench.kernel_source_hash(), "device": torch.cuda.get_device_name(0)}
    res["classes"] = classes_leg()
    print("classes", json.dumps(res["classes"]), flush=True)
    torch.cuda.empty_cache()
    res["shap"] = shap_leg()
    print("shap", json.dumps(res["shap"]), flush=True)
    with open(os.path.join(OUT, "sparse_classes_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
