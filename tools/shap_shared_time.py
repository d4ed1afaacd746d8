"""The TreeSHAP lane kernels of two builds side by side: one run times every kernel that calls treeshap_lanes.h on the workloads
of the per-kernel timing tools (contribs_time, interactions_time, interventional_time, vector_shap_time, vector_inter_time,
vector_iv_time, cat_shap_time: their forests, rows and calls, imported from them), native handles only and a few calls each, so
that five runs of each build fit one visit to the device.  Left out for time: K3, KR3 and the K-fold expansions (seconds per
call; the expansions run contribs_kernel / interactions_kernel / interventional_kernel, which K1 and the synthetic forest
cover), the forced class blocks, and cat_shap_time's numeric twin and narrow workload.  The verdicts cover the listed lines
only: an instantiation that only a forced class block or another shape selects is not timed here.
    python tools/shap_shared_time.py <out.json> [iterations]                  one run of the library in this tree
    python tools/shap_shared_time.py --compare <out.json> <parent runs dir> <branch runs dir>
The comparison holds, per kernel line, both builds' medians of every run, the parent's spread (max - min of its medians) and the
verdict: the branch's median of medians is not above the parent's plus that spread."""
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compare(out, parent_dir, branch_dir):
    runs = [[json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, "*.json")))] for d in (parent_dir, branch_dir)]
    lines = {}
    for key in runs[0][0]["ms_median"]:
        p, b = ([r["ms_median"][key] for r in rs] for rs in runs)
        spread = max(p) - min(p)
        lines[key] = {"parent_ms": p, "branch_ms": b, "parent_spread_ms": spread, "parent_median_ms": float(np.median(p)),
                      "branch_median_ms": float(np.median(b)), "passes": bool(np.median(b) <= np.median(p) + spread)}
    res = {"rule": "branch median <= parent median + (max - min of the parent's run medians)", "runs_per_build": [len(r) for r in runs],
           "iterations_per_run": runs[0][0]["iterations"], "device": runs[0][0]["device"], "all_pass": all(v["passes"] for v in lines.values()),
           "lines": lines}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    for k, v in lines.items():
        print("%-58s %10.3f %10.3f  spread %7.3f  %s" % (k, v["parent_median_ms"], v["branch_median_ms"], v["parent_spread_ms"],
                                                          "ok" if v["passes"] else "SLOWER"))


def main(out, iters):
    import torch

    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import bench
    import cat_shap_time as cst
    import interactions_time as it
    import tahoe_amd as ta
    import vector_inter_ref
    import vector_inter_time as vnt
    import vector_iv_time as vit
    import vector_shap_time as vst

    torch.cuda.set_device(0)
    ms = {}

    def timed(key, call):
        out, t = None, []
        for i in range(1 + iters):  # the first call allocates the output and is the warm-up; after one of more than 3 s, one timed call
            if i == 2 and t[0] > 3000.0:
                break
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = call(out)
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
        ms[key] = float(np.median(t[1:]))
        print(key, ms[key], flush=True)

    def uniform(rows, cols):
        torch.manual_seed(1234)
        x = torch.rand((rows, cols), device="cuda") * 2.0 - 1.0
        x[torch.rand((rows, cols), device="cuda") < 0.02] = vst.MISSING
        return x

    # contribs_time / interactions_time / interventional_time: K1 (LDS slabs) and the 256-column forest (in place)
    for name, nodes, T, D, F, x in it.forests():
        if name == "KR3":
            continue
        f = ta.Forest(nodes, T, D, F, missing=bench.MISSING, contribs=True)
        if name == "K1":
            big = torch.from_numpy(np.ascontiguousarray(np.resize(x, (100_000, F)))).cuda()
            timed("contribs_time/K1_100k_rows/contribs_kernel", lambda o: f.predict_contribs(big, out=o))
        xd = torch.from_numpy(x).cuda()
        timed(f"interactions_time/{name}/contribs_spare+interactions_kernel", lambda o: f.predict_interactions(xd, out=o))
        f.set_background(xd[:100])
        timed(f"interventional_time/{name}/interventional_kernel", lambda o: f.predict_contribs_interventional(xd, out=o))
        f.close()
    # vector_shap_time / vector_inter_time / vector_iv_time: the native handles
    for name, T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K in vit.SHAPES + vnt.SHAPES[-2:-1]:
        fo, covers = vst.forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K)
        if (name, T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K) in vst.SHAPES:
            h, x = vst.native_handle(fo, covers), uniform(4096, cols)
            timed(f"vector_shap_time/{name}/vector_contribs_kernel", lambda o: h.predict_contribs(x, out=o))
            h.close()
        h, x = vnt.native_handle(fo, covers), uniform(512 if vector_inter_ref.shape(cols, K)[0] else 256, cols)
        timed(f"vector_inter_time/{name}/vector_contribs_spare+interactions_kernel", lambda o: h.predict_interactions(x, out=o))
        h.close()
        h, x = vit.native_handle(fo), uniform(4096, cols)
        h.set_background(uniform(100, cols))
        timed(f"vector_iv_time/{name}/vector_interventional_kernel", lambda o: h.predict_contribs_interventional(x, out=o))
        h.close()
    # cat_shap_time, wide, the categorical handle: the SETS instantiations
    _, sn, tr, cols, cats, covers, data = cst.workload(False)
    h = ta.capi.SparseForest(sn, tr, cols, categories=cats, missing=cst.MISSING, covers=covers, contribs=True)
    h.set_background(torch.from_numpy(data[-cst.BG_ROWS:]).cuda())
    for call, method in (("contribs", "predict_contribs"), ("interactions", "predict_interactions"),
                         ("interventional", "predict_contribs_interventional")):
        x = torch.from_numpy(data[:cst.ROWS[call]]).cuda()
        timed(f"cat_shap_time/wide_categorical/{call}", lambda o: getattr(h, method)(x, out=o))
    h.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump({"iterations": iters, "device": torch.cuda.get_device_name(0), "unit": "ms per call, median of hipEvent pairs after 1 warm-up (one pair where the warm-up takes more than 3 s)",
               "ms_median": ms}, open(out, "w"), indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(*sys.argv[2:5])
    else:
        main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 5)
