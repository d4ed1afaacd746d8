"""Interventional TreeSHAP of an oblivious forest: the native handle (tahoe_oblivious_forest_create_ex with
TAHOE_CREATE_OBLIVIOUS_INTERVENTIONAL) against the heap expansion on a dense handle, the only way to get it before.

Per shape one oblivious forest (random features, thresholds uniform over the data's range, random leaves) is served twice in one
process: natively with the flag alone, and as its expansion into complete heap trees of unit leaf covers
(tests/oblivious_shap_ref.py, expand_with_covers) on tahoe_forest_create -- with K outputs per leaf tahoe_forest_create_multiclass
on T x K trees -- with TAHOE_CREATE_CONTRIBS.  Per background size both handles take the same background (set_background timed
once by the host clock around the synchronous call), then predict_contribs_interventional of both runs in turn, each call between
two hipEvents; the medians after warm-up are compared.  The outputs are compared by their largest difference relative to the
largest |phi|, the bias columns bit for bit.
    python tools/oblivious_iv_time.py [out_dir] [iterations]   -> <out_dir>/oblivious_iv_time.json (default profiles/oblivious_iv)"""
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
import oblivious_shap_ref as osr  # noqa: E402
import tahoe_amd as ta  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "oblivious_iv")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
WARMUP = 2
MISSING = -999.0
ROWS = 4096
BACKGROUNDS = [100, 1000]
# (name, trees, depth, num_cols, K)
SHAPES = [("catboost_default_depth6", 1000, 6, 64, 1), ("vector_leaves_k8", 100, 6, 64, 8), ("depth10", 50, 10, 64, 1)]


def forest(T, D, cols, K, seed):
    rng = np.random.default_rng(seed)
    return dict(depths=np.full(T, D, np.int32), fids=rng.integers(0, cols, T * D), k=K, cols=cols,
                thr=rng.uniform(-1.0, 1.0, T * D).astype(np.float32), def_left=rng.integers(0, 2, T * D).astype(bool),
                leaves=rng.standard_normal(T * (1 << D) * K).astype(np.float32))


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


def set_background_ms(f, bg):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f.set_background(bg)
    return (time.perf_counter() - t0) * 1e3


def main():
    res = {"iterations": ITERS, "warmup": WARMUP, "rows": ROWS, "shapes": {}}
    for name, T, D, cols, K in SHAPES:
        fo = forest(T, D, cols, K, seed=len(name))
        ob = ta.ObliviousForest(fo["depths"], fo["fids"], fo["thr"], fo["def_left"], fo["leaves"], cols, leaf_dim=K, missing=MISSING,
                                interventional=True)
        ones = np.ones(T * (1 << D), np.float32)
        nodes = np.stack([osr.expand_with_covers(fo, ones, c)[0].reshape(T, -1) for c in range(K)], axis=1).reshape(-1)
        de = ta.Forest(nodes, T * K, D, cols, num_classes=K, missing=MISSING, contribs=True)
        torch.manual_seed(1234)
        x = torch.rand((ROWS + max(BACKGROUNDS), cols), device="cuda") * 2.0 - 1.0
        x[torch.rand(x.shape, device="cuda") < 0.02] = MISSING
        xr = x[:ROWS].contiguous()
        r = {"trees": T, "depth": D, "num_cols": cols, "leaf_dim": K, "oblivious_device_bytes_no_background": int(ob.info().device_bytes),
             "expansion_device_bytes_no_background": int(de.info().device_bytes), "backgrounds": {}}
        shape = (ROWS,) + ((K,) if K > 1 else ()) + (cols + 1,)
        for B in BACKGROUNDS:
            bg = x[ROWS:ROWS + B].contiguous()
            set_ob, set_de = set_background_ms(ob, bg), set_background_ms(de, bg)
            outs = [torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")]
            t_ob, t_de = timed([lambda: ob.predict_contribs_interventional(xr, out=outs[0]),
                                lambda: de.predict_contribs_interventional(xr, out=outs[1])])
            r["backgrounds"][str(B)] = {
                "oblivious_set_background_ms": set_ob, "expansion_set_background_ms": set_de,
                "oblivious_device_bytes": int(ob.info().device_bytes), "expansion_device_bytes": int(de.info().device_bytes),
                "oblivious_ms": t_ob, "expansion_ms": t_de, "ratio_median_expansion_over_oblivious": t_de["median"] / t_ob["median"],
                "max_abs_diff_over_max_abs_phi": float((outs[0][..., :cols] - outs[1][..., :cols]).abs().max()
                                                       / outs[1][..., :cols].abs().max()),
                "bias_same_bits": bool(torch.equal(outs[0][..., cols].contiguous().view(torch.int32),
                                                   outs[1][..., cols].contiguous().view(torch.int32)))}
            print(name, B, json.dumps(r["backgrounds"][str(B)]), flush=True)
            del outs
        res["shapes"][name] = r
        ob.close()
        de.close()
        del x
    res["src_hash"] = bench.kernel_source_hash()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "oblivious_iv_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
