"""Oblivious forests: the native handle against the only way to serve the same model without it, the heap expansion.

Per shape, one oblivious forest (random features, thresholds uniform over the data's range, random leaves) is served twice in one
process: by tahoe_oblivious_forest_create under AUTO, and by its expansion into complete heap trees (tests/oblivious_ref.py,
expand_to_dense) on tahoe_forest_create -- or, with K outputs per leaf, tahoe_forest_create_multiclass on T x K trees -- under
AUTO.  Both are timed in turn by the handles' own kernel-time profiling (one hipEvent pair per launch; a quantise pre-pass is
added to its walk), median over the iterations after warm-up; afterwards the two outputs are compared bit for bit.
    python tools/oblivious_time.py [out_dir] [iterations] [rows]   -> <out_dir>/oblivious_time.json (default profiles/oblivious)
    python tools/oblivious_time.py --walk <shape> <oblivious|expansion> [predicts]
        only that handle's predicts of one shape and nothing else on the GPU: the target of a rocprofv3 --pmc run"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import tahoe_amd as ta  # noqa: E402

WALK = sys.argv[2:] if len(sys.argv) > 1 and sys.argv[1] == "--walk" else None
ARGS = [] if WALK else sys.argv[1:]
OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "oblivious")
ITERS = int(ARGS[1]) if len(ARGS) > 1 else 20
ROWS = int(ARGS[2]) if len(ARGS) > 2 else 1_000_000
WARMUP = 3
MISSING = -999.0
# (name, trees, depth, num_cols, K)
SHAPES = [("catboost_default_depth6", 1000, 6, 64, 1), ("vector_leaves_k8", 100, 6, 64, 8), ("depth10_cols256", 1000, 10, 256, 1)]


def forest(T, D, cols, K, seed):
    rng = np.random.default_rng(seed)
    depths = np.full(T, D, np.int32)
    fids = rng.integers(0, cols, T * D)
    thr = rng.uniform(-1.0, 1.0, T * D).astype(np.float32)
    def_left = rng.integers(0, 2, T * D).astype(bool)
    leaves = rng.standard_normal(T * (1 << D) * K).astype(np.float32)
    return dict(depths=depths, fids=fids, thr=thr, def_left=def_left, leaves=leaves, k=K, cols=cols)


def timed(handles, x, outs):
    for _ in range(WARMUP):
        for h, o in zip(handles, outs):
            h.predict_raw(x, o)
    torch.cuda.synchronize()
    for h in handles:
        h.set_profiling(ITERS)
    for _ in range(ITERS):  # in turn: drift on the machine hits both
        for h, o in zip(handles, outs):
            h.predict_raw(x, o)
    torch.cuda.synchronize()
    ms = [h.kernel_times_ms() + h.prepass_times_ms() for h in handles]
    for h in handles:
        h.set_profiling(0)
        h.check()
    return ms


def handles(name, T, D, cols, K, which=("oblivious", "expansion")):
    fo = forest(T, D, cols, K, seed=len(name))
    ob = dense = None
    if "oblivious" in which:
        ob = ta.ObliviousForest(fo["depths"], fo["fids"], fo["thr"], fo["def_left"], fo["leaves"], cols, leaf_dim=K, missing=MISSING)
    if "expansion" in which:
        per_class = [obr.dense_of(fo, c)[0].reshape(T, -1) for c in range(K)]
        nodes = np.stack(per_class, axis=1).reshape(-1)
        dense = ta.Forest(nodes, T * K, D, cols, missing=MISSING, num_classes=K)
    torch.manual_seed(1234)
    x = torch.rand((ROWS, cols), device="cuda") * 2.0 - 1.0
    x[torch.rand((ROWS, cols), device="cuda") < 0.02] = MISSING
    return ob, dense, x


def walk(name, which, predicts=4):
    _, T, D, cols, K = next(s for s in SHAPES if s[0] == name)
    ob, dense, x = handles(name, T, D, cols, K, which=(which,))
    h = ob or dense
    out = torch.empty((ROWS, K) if K > 1 else (ROWS,), device="cuda")
    for _ in range(int(predicts)):
        h.predict_raw(x, out)
    torch.cuda.synchronize()
    h.check()
    print(name, which, h.kernel_form(ROWS), predicts, "predicts")


def main():
    res = {"rows": ROWS, "iterations": ITERS, "warmup": WARMUP, "shapes": {}}
    for name, T, D, cols, K in SHAPES:
        ob, dense, x = handles(name, T, D, cols, K)
        shape = (ROWS, K) if K > 1 else (ROWS,)
        outs = [torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")]
        t_ob, t_de = timed([ob, dense], x, outs)
        same = bool(torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)))
        r = {"trees": T, "depth": D, "num_cols": cols, "leaf_dim": K,
             "oblivious_form": ob.kernel_form(ROWS), "expansion_form": dense.kernel_form(ROWS),
             "oblivious_ms_median": float(np.median(t_ob)), "expansion_ms_median": float(np.median(t_de)),
             "oblivious_ms_min": float(np.min(t_ob)), "expansion_ms_min": float(np.min(t_de)),
             "oblivious_ms_max": float(np.max(t_ob)), "expansion_ms_max": float(np.max(t_de)),
             "ratio_median_oblivious_over_expansion": float(np.median(t_ob) / np.median(t_de)),
             "oblivious_device_bytes": int(ob.info().device_bytes), "expansion_device_bytes": int(dense.info().device_bytes),
             "split_records": T * D, "heap_node_records": T * K * ((1 << D) - 1),
             "node_record_ratio": float(K * ((1 << D) - 1) / D), "same_bits": same}
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        ob.close()
        dense.close()
        del x, outs
    res["src_hash"] = bench.kernel_source_hash()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "oblivious_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not all(r["same_bits"] for r in res["shapes"].values()):
        sys.exit("the oblivious handle and the expansion differ")


if __name__ == "__main__":
    walk(*WALK) if WALK else main()
