"""The four explanation calls on a categorical handle against its integer-threshold twin: what the set test costs.

The forest is tools/categorical_time.py's (K5's irregular trees of depth 4..24 on 256 features, every fourth feature categorical),
cut down to its first TREES trees so that the path tables stay small; K5's paths hold at most 24 distinct features.  Every node on a
categorical feature tests an integer k: `x >= k` in the numeric twin, the set {k, ..., K_f - 1} (members right) in the categorical
handle, so both hold the same path bins and node deltas and differ only in how a one-fraction / a branch is decided.  The twin runs
the kernels without sets, which are the parent's instruction for instruction (tools/isa_diff.py): it is the baseline.
Two workloads:
  wide    K_f in 64..256: sets of 2..8 words, the lanes gather the word trunc(x) selects;
  narrow  K_f = 32: sets of one word, which the lane holds (no gather) -- and the same sets padded to two words by a category no row
          carries (`narrow_gather`), which takes the gather on the same work: the difference is what the one-word path saves.
Per call the handles are timed in turn, one hipEvent pair per launch, median of ITERS launches after warm-up; the outputs of the
handles of one workload are compared bit for bit.
    python tools/cat_shap_time.py [out_dir] [iterations]      -> <out_dir>/cat_shap_time.json (default profiles/cat_shap)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cat_shap")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 2
MISSING = -999.0
TREES = 48
ROWS = {"contribs": 2048, "interactions": 64, "interventional": 512, "approx": 65536}
BG_ROWS = 32


def workload(narrow):
    _, (sn, tr, cols), data = bench.baseline_workload(ta, "K5")
    sn, tr = sn[:int(tr[TREES])].copy(), tr[:TREES].copy()
    rng = np.random.default_rng(2024)
    feats = np.arange(0, cols, 4)
    kf = {int(f): 32 if narrow else int(k) for f, k in zip(feats, rng.integers(64, 257, feats.size))}
    b = sn["bits"].view(np.uint32)
    inner = np.flatnonzero((b >> 31) == 0)
    fid = b[inner] & ((1 << 30) - 1)
    chosen = inner[np.isin(fid, feats)]
    kmax = np.array([kf[int(f)] for f in fid[np.isin(fid, feats)]])
    k = (rng.random(chosen.size) * (kmax + 1)).astype(np.int64)
    num = sn.copy()
    num["val"][chosen] = k.astype(np.float32)
    cats = {int(i): range(int(kk), int(km)) for i, kk, km in zip(chosen, k, kmax)}
    data = np.array(data[:max(ROWS.values()) + BG_ROWS], dtype=np.float32, copy=True)
    for f, K in kf.items():
        data[:, f] = rng.integers(0, K, data.shape[0]).astype(np.float32)
    covers = rng.uniform(0.05, 1.0, sn.size).astype(np.float32)
    return num, sn, tr, cols, cats, covers, data


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run(name, narrow):
    num, sn, tr, cols, cats, covers, data = workload(narrow)
    kw = dict(missing=MISSING, covers=covers, contribs=True, approx_contribs=True)
    handles = {"numeric": ta.capi.SparseForest(num, tr, cols, **kw), "categorical": ta.capi.SparseForest(sn, tr, cols, categories=cats, **kw)}
    if narrow:  # the same sets with a second word that no row reaches
        handles["categorical_gather"] = ta.capi.SparseForest(sn, tr, cols, categories={i: list(c) + [40] for i, c in cats.items()}, **kw)
    bg = torch.from_numpy(data[-BG_ROWS:]).cuda()
    for h in handles.values():
        h.set_background(bg)
    res = {"trees": int(tr.size), "nodes": int(sn.size), "categorical_splits": len(cats),
           "device_bytes": {k: int(h.info().device_bytes) for k, h in handles.items()}, "calls": {}}
    calls = {"contribs": "predict_contribs", "interactions": "predict_interactions",
             "interventional": "predict_contribs_interventional", "approx": "predict_contribs_approx"}
    for call, method in calls.items():
        x = torch.from_numpy(data[:ROWS[call]]).cuda()
        outs = {k: getattr(h, method)(x) for k, h in handles.items()}
        for _ in range(WARMUP):
            for k, h in handles.items():
                getattr(h, method)(x, outs[k])
        torch.cuda.synchronize()
        ms = {k: [] for k in handles}
        for _ in range(ITERS):  # in turn: drift on the machine hits all
            for k, h in handles.items():
                ms[k].append(timed(lambda: getattr(h, method)(x, outs[k])))
        r = {"rows": ROWS[call], "same_bits": all(torch.equal(outs["numeric"].view(torch.int32), o.view(torch.int32)) for o in outs.values())}
        for k in handles:
            r[k + "_ms_median"], r[k + "_ms_min"], r[k + "_ms_max"] = float(np.median(ms[k])), float(np.min(ms[k])), float(np.max(ms[k]))
            if k != "numeric":
                r[k + "_ratio_median"] = r[k + "_ms_median"] / r["numeric_ms_median"]
        res["calls"][call] = r
        print(name, call, json.dumps(r), flush=True)
    for h in handles.values():
        h.check()
        h.close()
    return res


def main():
    res = {"workload": "K5's first %d trees (depth 4-24, 256 features), every fourth feature categorical; the numeric twin holds the same "
                       "nodes as integer thresholds (the same path bins and node deltas)" % TREES,
           "timing": "one hipEvent pair per launch, handles in turn, median of %d after %d warm-up launches" % (ITERS, WARMUP),
           "background_rows": BG_ROWS, "device": torch.cuda.get_device_name(0),
           "wide": run("wide", False), "narrow": run("narrow", True), "src_hash": bench.kernel_source_hash()}
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "cat_shap_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not all(c["same_bits"] for w in ("wide", "narrow") for c in res[w]["calls"].values()):
        sys.exit("categorical and numeric handles differ")


if __name__ == "__main__":
    main()
