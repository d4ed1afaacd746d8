"""SHAP interaction values of an oblivious forest: the native handle (tahoe_oblivious_forest_create_ex with
TAHOE_CREATE_INTERACTIONS) against the heap expansion on a dense handle, the only way to get them before.

Per shape (those of tools/oblivious_shap_time.py) one oblivious forest is served twice in one process: natively with
TAHOE_CREATE_CONTRIBS | TAHOE_CREATE_INTERACTIONS, and as its expansion into complete heap trees whose weights are the subtree
covers (tests/oblivious_shap_ref.py, expand_with_covers) on tahoe_forest_create -- with K outputs per leaf
tahoe_forest_create_multiclass on T x K trees -- with TAHOE_CREATE_CONTRIBS.  predict_interactions of both run in turn, each call
between two hipEvents; then the native predict_interactions and predict_contribs at the same rows.  Medians after warm-up, with
min and max.  The outputs are compared by their largest difference relative to the largest |Phi|, the bias corner bit for bit.
    python tools/oblivious_inter_time.py [out_dir] [iterations]   -> <out_dir>/oblivious_inter_time.json (default
                                                                      profiles/oblivious_inter)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import oblivious_shap_ref as osr  # noqa: E402
import tahoe_amd as ta  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "oblivious_inter")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
WARMUP = 2
MISSING = -999.0
# (name, trees, depth, num_cols, K, rows)
SHAPES = [("catboost_default_depth6", 1000, 6, 64, 1, 4096), ("vector_leaves_k8", 100, 6, 64, 8, 4096), ("depth10", 50, 10, 64, 1, 4096)]


def forest(T, D, cols, K, seed):
    rng = np.random.default_rng(seed)
    fo = dict(depths=np.full(T, D, np.int32), fids=rng.integers(0, cols, T * D), k=K, cols=cols,
              thr=rng.uniform(-1.0, 1.0, T * D).astype(np.float32), def_left=rng.integers(0, 2, T * D).astype(bool),
              leaves=rng.standard_normal(T * (1 << D) * K).astype(np.float32))
    return fo, rng.integers(1, 1025, T * (1 << D)).astype(np.float32)


def timed(calls):
    """calls: functions that each launch one call -> median / min / max ms of each, run in turn"""
    for _ in range(WARMUP):
        for c in calls:
            c()
    torch.cuda.synchronize()
    ms = [[] for _ in calls]
    for _ in range(ITERS):
        for i, c in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            c()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [dict(median=float(np.median(m)), min=float(np.min(m)), max=float(np.max(m))) for m in ms]


def main():
    res = {"iterations": ITERS, "warmup": WARMUP, "shapes": {}}
    for name, T, D, cols, K, rows in SHAPES:
        fo, covers = forest(T, D, cols, K, seed=len(name))
        ob = ta.ObliviousForest(fo["depths"], fo["fids"], fo["thr"], fo["def_left"], fo["leaves"], cols, leaf_dim=K,
                                leaf_covers=covers, missing=MISSING, contribs=True, interactions=True)
        nodes = np.stack([osr.expand_with_covers(fo, covers, c)[0].reshape(T, -1) for c in range(K)], axis=1).reshape(-1)
        de = ta.Forest(nodes, T * K, D, cols, num_classes=K, missing=MISSING, contribs=True)
        torch.manual_seed(1234)
        x = torch.rand((rows, cols), device="cuda") * 2.0 - 1.0
        x[torch.rand(x.shape, device="cuda") < 0.02] = MISSING
        kdim = (K,) if K > 1 else ()
        outs = [torch.empty((rows,) + kdim + (cols + 1, cols + 1), device="cuda") for _ in range(2)]
        phi = torch.empty((rows,) + kdim + (cols + 1,), device="cuda")
        t_ob, t_de = timed([lambda: ob.predict_interactions(x, out=outs[0]), lambda: de.predict_interactions(x, out=outs[1])])
        t_in, t_phi = timed([lambda: ob.predict_interactions(x, out=outs[0]), lambda: ob.predict_contribs(x, out=phi)])
        distinct = float(np.mean([np.unique(fo["fids"][t * D:(t + 1) * D]).size for t in range(T)]))
        r = {"trees": T, "depth": D, "num_cols": cols, "leaf_dim": K, "rows": rows, "mean_distinct_features_per_tree": distinct,
             "oblivious_device_bytes": int(ob.info().device_bytes), "expansion_device_bytes": int(de.info().device_bytes),
             "oblivious_ms": t_ob, "expansion_ms": t_de, "oblivious_rows_per_s": rows / (t_ob["median"] * 1e-3),
             "expansion_rows_per_s": rows / (t_de["median"] * 1e-3),
             "ratio_median_expansion_over_oblivious": t_de["median"] / t_ob["median"],
             "native_interactions_ms": t_in, "native_contribs_ms": t_phi,
             "ratio_median_interactions_over_contribs": t_in["median"] / t_phi["median"],
             "max_abs_diff_over_max_abs": float((outs[0] - outs[1]).abs().max() / outs[1].abs().max()),
             "bias_corner_same_bits": bool(torch.equal(outs[0][..., cols, cols].view(torch.int32),
                                                       outs[1][..., cols, cols].view(torch.int32)))}
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        ob.close()
        de.close()
        del x, outs, phi
    res["src_hash"] = bench.kernel_source_hash()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "oblivious_inter_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not all(r["bias_corner_same_bits"] and r["max_abs_diff_over_max_abs"] < 1e-4 for r in res["shapes"].values()):
        sys.exit("the interaction values of the oblivious handle and of the expansion differ")


if __name__ == "__main__":
    main()
