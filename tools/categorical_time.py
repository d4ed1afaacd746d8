"""Categorical splits on K5's shape: what the extra dependent bitset read per categorical step costs.

K5's forest (2000 irregular trees of depth 4..24 on 256 features, 200 k rows).  A quarter of the features (64, every fourth)
become categorical with K_f categories each (64..256); the batch holds integers in [0, K_f) there.  Every node on such a feature
gets an integer threshold k in [0, K_f] in the numeric forest and the set {k, ..., K_f - 1} (members right) in the categorical
one, so both walk the same paths and differ only in how the branch is decided.  Per strategy (TILEBLOCK, ROWTILE, DIRECT) the
two handles are timed in turn by the handles' own kernel-time profiling (hipEvent pair per launch), median over the
iterations after warm-up; the sums and leaf indices of the two are compared bit for bit.
    python tools/categorical_time.py [out_dir] [iterations]      -> <out_dir>/categorical_time.json (default profiles/categorical)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "categorical")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 3
MISSING = -999.0


def workload():
    _, (sn, tr, cols), data = bench.baseline_workload(ta, "K5")
    rng = np.random.default_rng(2024)
    feats = np.arange(0, cols, 4)
    kf = dict(zip(feats.tolist(), rng.integers(64, 257, feats.size).tolist()))
    b = sn["bits"].view(np.uint32)
    inner = np.flatnonzero((b >> 31) == 0)
    fid = b[inner] & ((1 << 30) - 1)
    chosen = inner[np.isin(fid, feats)]
    kmax = np.array([kf[int(f)] for f in fid[np.isin(fid, feats)]])
    k = (rng.random(chosen.size) * (kmax + 1)).astype(np.int64)
    num = sn.copy()
    num["val"][chosen] = k.astype(np.float32)
    cats = {int(i): range(int(kk), int(km)) for i, kk, km in zip(chosen, k, kmax)}
    data = np.array(data, dtype=np.float32, copy=True)
    for f, K in kf.items():
        data[:, f] = rng.integers(0, K, data.shape[0]).astype(np.float32)
    return num, sn, tr, cols, cats, kf, data


def main():
    num, sn, tr, cols, cats, kf, data = workload()
    R = data.shape[0]
    x = torch.from_numpy(data).cuda()
    plain = ta.capi.SparseForest(num, tr, cols, missing=MISSING)
    cat = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, categories=cats)
    dev_bytes = cat.info().device_bytes
    out_p = torch.empty(R, dtype=torch.float32, device="cuda")
    out_c = torch.empty(R, dtype=torch.float32, device="cuda")
    res = {"workload": f"K5 forest ({tr.size} trees, {sn.size} nodes, depth 4-24, {cols} features), {R} rows; "
                       f"{len(kf)} categorical features with 64-256 categories, {len(cats)} categorical splits "
                       f"(the numeric forest: the same nodes as integer thresholds, the same paths)",
           "iterations": ITERS, "device_bytes_categorical": int(dev_bytes), "forms": {}}
    for name in ("TILEBLOCK", "ROWTILE", "DIRECT"):
        s = getattr(ta, "STRATEGY_" + name)
        plain.set_strategy(s)
        cat.set_strategy(s)
        for _ in range(WARMUP):
            plain.predict_raw(x, out_p)
            cat.predict_raw(x, out_c)
        torch.cuda.synchronize()
        plain.set_profiling(ITERS)
        cat.set_profiling(ITERS)
        for _ in range(ITERS):  # in turn: drift on the machine hits both
            plain.predict_raw(x, out_p)
            cat.predict_raw(x, out_c)
        torch.cuda.synchronize()
        tp, tc = plain.kernel_times_ms(), cat.kernel_times_ms()
        plain.set_profiling(0)
        cat.set_profiling(0)
        plain.check()
        cat.check()
        lp, sp_ = plain.predict_leaf_idx(x)
        lc, sc = cat.predict_leaf_idx(x)
        same = bool(torch.equal(sp_.view(torch.int32), sc.view(torch.int32)) and torch.equal(lp, lc)
                    and torch.equal(out_p.view(torch.int32), out_c.view(torch.int32)))
        r = {"kernel_form_numeric": plain.kernel_form(R), "kernel_form_categorical": cat.kernel_form(R),
             "numeric_ms_median": float(np.median(tp)), "categorical_ms_median": float(np.median(tc)),
             "numeric_ms_min": float(np.min(tp)), "categorical_ms_min": float(np.min(tc)),
             "numeric_ms_max": float(np.max(tp)), "categorical_ms_max": float(np.max(tc)),
             "ratio_median": float(np.median(tc) / np.median(tp)), "same_bits": same}
        res["forms"][name] = r
        print(name, json.dumps(r), flush=True)
    cat.set_strategy(ta.STRATEGY_AUTO)
    res["auto_form_categorical"] = cat.kernel_form(R)
    res["src_hash"] = bench.kernel_source_hash()
    plain.close()
    cat.close()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "categorical_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not all(r["same_bits"] for r in res["forms"].values()):
        sys.exit("categorical and numeric handles differ")


if __name__ == "__main__":
    main()
