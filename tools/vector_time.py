"""Vector-leaf forests: the native handle against the only way to serve the same model without it, the K-fold expansion.

Per shape, one irregular forest (tahoe_synth_sparse_forest) gets a table of random leaf vectors, one per leaf in shuffled order,
and is served twice in one process: by tahoe_vector_forest_create under AUTO, and by its expansion into T x K trees with scalar
leaves (tests/vector_ref.py, expand) on tahoe_sparse_forest_create_ex(num_classes = K) -- tahoe_sparse_forest_create for K == 1 --
under AUTO.  Both are timed in turn by the handles' own kernel-time profiling (one hipEvent pair per launch; a pre-pass, where a
handle has one, is added to its walk), median over the iterations after warm-up; afterwards the two outputs are compared bit for
bit.  The native handle is then timed alone under forced DIRECT and forced ROWTILE.
    python tools/vector_time.py [out_dir] [iterations] [rows]   -> <out_dir>/vector_time.json (default profiles/vector)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402
import vector_ref as vr  # noqa: E402

ARGS = sys.argv[1:]
OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "vector")
ITERS = int(ARGS[1]) if len(ARGS) > 1 else 20
ROWS = int(ARGS[2]) if len(ARGS) > 2 else 1_000_000
WARMUP = 3
MISSING = -999.0
K5 = bench.K5_SHAPE
# (name, trees, num_cols, min_depth, max_depth, leaf_prob, max_tree_nodes, seed, K)
SHAPES = [("random_forest_k1", 100, 64, 4, 16, 0.32, 65535, 77, 1),
          ("random_forest_k8", 100, 64, 4, 16, 0.32, 65535, 77, 8),
          ("random_forest_k10", 100, 64, 4, 16, 0.32, 65535, 77, 10),
          ("k5_forest_k8", K5["trees"], K5["cols"], K5["min_depth"], K5["max_depth"], K5["leaf_prob"], K5["max_tree_nodes"],
           K5["forest_seed"], 8)]


def forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K):
    nodes, trees = ta.capi.synth_sparse_forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed)
    rng = np.random.default_rng(seed + 1)
    is_leaf = nodes["bits"] < 0
    L = int(is_leaf.sum())
    nodes["left_idx"][is_leaf] = rng.permutation(L).astype(np.int32)
    nodes["val"][is_leaf] = 0.0
    return dict(nodes=nodes, trees=trees, leaves=rng.standard_normal((L, K)).astype(np.float32), k=K, cols=cols)


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


def stats(prefix, ms):
    return {prefix + "_ms_median": float(np.median(ms)), prefix + "_ms_min": float(np.min(ms)), prefix + "_ms_max": float(np.max(ms))}


def main():
    res = {"rows": ROWS, "iterations": ITERS, "warmup": WARMUP, "shapes": {}}
    for name, T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K in SHAPES:
        fo = forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K)
        native = ta.VectorForest(fo["nodes"], fo["trees"], fo["leaves"], cols, missing=MISSING)
        exp_nodes, exp_trees = vr.expand(fo)
        expansion = ta.capi.SparseForest(exp_nodes, exp_trees, cols, missing=MISSING, num_classes=K)
        torch.manual_seed(1234)
        x = torch.rand((ROWS, cols), device="cuda") * 2.0 - 1.0
        x[torch.rand((ROWS, cols), device="cuda") < 0.02] = MISSING
        shape = (ROWS, K) if K > 1 else (ROWS,)
        outs = [torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")]
        t_na, t_ex = timed([native, expansion], x, outs)
        same = bool(torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)))
        r = {"trees": T, "num_cols": cols, "min_depth": dmin, "max_depth": dmax, "leaf_dim": K, "nodes": int(fo["nodes"].size),
             "leaf_vectors": int(fo["leaves"].shape[0]), "native_form": native.kernel_form(ROWS),
             "expansion_form": expansion.kernel_form(ROWS), **stats("native", t_na), **stats("expansion", t_ex),
             "ratio_median_native_over_expansion": float(np.median(t_na) / np.median(t_ex)),
             "native_device_bytes": int(native.info().device_bytes), "expansion_device_bytes": int(expansion.info().device_bytes),
             "same_bits": same}
        expansion.close()
        del exp_nodes
        for strat in ("DIRECT", "ROWTILE"):  # the native handle's two forms, alone
            native.set_strategy(getattr(ta, "STRATEGY_" + strat))
            (t_f,) = timed([native], x, outs[:1])
            r.update(stats("native_" + strat.lower(), t_f))
            r["same_bits"] = r["same_bits"] and bool(torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)))
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        native.close()
        del x, outs
    res["src_hash"] = bench.kernel_source_hash()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "vector_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not all(r["same_bits"] for r in res["shapes"].values()):
        sys.exit("the vector-leaf handle and the expansion differ")


if __name__ == "__main__":
    main()
