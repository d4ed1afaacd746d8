"""SHAP interaction values on a vector-leaf forest: the native handle (tahoe_vector_forest_create_ex with TAHOE_CREATE_CONTRIBS |
TAHOE_CREATE_VECTOR_INTERACTIONS) against the only way to get the same values without it, the K-fold expansion on
tahoe_sparse_forest_create_ex(num_classes = K).

The forests are those of tools/vector_shap_time.py (100 irregular trees of depth <= 16 on 64 columns: the LDS-triangle form) and
the 200-column variant of tools/vector_iv_time.py (the in-place form), with random leaf vectors and covers from reach
probabilities.  Each is served twice in one process, natively and as its expansion into T x K trees whose copies of a tree carry
that tree's covers; the two outputs are compared bit for bit first.  Then predict_interactions of both runs in turn, each call
-- two kernel launches -- between two hipEvents on the stream; median, min and max after warm-up.  predict_contribs of the native
handle is timed the same way over fewer calls.  The native handle is then created again under each class block
(TAHOE_VECTOR_SHAP_KB), with the class blocks in a workgroup's loop and over gridDim.y (TAHOE_VECTOR_SHAP_GRID = 0 / 1), and timed
alone over fewer iterations.  The row count is per form: in place a wave owns a row, so rows are the only parallelism and a few
hundred of them already take what a thousand take.
    python tools/vector_inter_time.py [out_dir] [iterations] [slab_rows] [in_place_rows]
        -> <out_dir>/vector_inter_time.json (default profiles/vector_inter)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402
import vector_inter_ref as vir  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402
import vector_shap_time as vst  # noqa: E402

ARGS = sys.argv[1:]
OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "vector_inter")
ITERS = int(ARGS[1]) if len(ARGS) > 1 else 20
SLAB_ROWS = int(ARGS[2]) if len(ARGS) > 2 else 512
INPLACE_ROWS = int(ARGS[3]) if len(ARGS) > 3 else 256
WARMUP = 3
VARIANT_ITERS = 3   # the forced class blocks, timed alone after one warm-up call (the slow ones take seconds per call)
CONTRIBS_ITERS = 5
MISSING = vst.MISSING
# (name, trees, num_cols, min_depth, max_depth, leaf_prob, max_tree_nodes, seed, K)
SHAPES = vst.SHAPES + [("random_forest_k1_200_cols", 100, 200, 4, 16, 0.32, 65535, 78, 1),
                       ("random_forest_k8_200_cols", 100, 200, 4, 16, 0.32, 65535, 78, 8)]


def timed(calls, iters, warmup):
    """Each call of `calls` in turn (drift on the machine hits all) -> ms per call, iters each"""
    for _ in range(warmup):
        for c in calls:
            c()
    torch.cuda.synchronize()
    ms = [[] for _ in calls]
    for _ in range(iters):
        for i, c in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            c()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [np.array(m) for m in ms]


def native_handle(fo, covers, kb=None, grid=None):
    for name, v in (("TAHOE_VECTOR_SHAP_KB", kb), ("TAHOE_VECTOR_SHAP_GRID", grid)):  # read once, at create
        os.environ.pop(name, None)
        if v is not None:
            os.environ[name] = str(v)
    h = ta.VectorForest(fo["nodes"], fo["trees"], fo["leaves"], fo["cols"], missing=MISSING, covers=covers, interactions=True)
    for name in ("TAHOE_VECTOR_SHAP_KB", "TAHOE_VECTOR_SHAP_GRID"):
        os.environ.pop(name, None)
    return h


def main():
    res = {"iterations": ITERS, "warmup": WARMUP, "variant_iterations": VARIANT_ITERS,
           "timing": "hipEvent pair around each predict_interactions call (two kernel launches)", "shapes": {}}
    for name, T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K in SHAPES:
        fo, covers = vst.forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K)
        slabs, kb, R, lds = vir.shape(cols, K)
        rows = SLAB_ROWS if slabs else INPLACE_ROWS
        native = native_handle(fo, covers)
        exp_nodes, exp_trees = vr.expand(fo)
        expansion = ta.capi.SparseForest(exp_nodes, exp_trees, cols, missing=MISSING, num_classes=K,
                                         covers=vsr.tile_covers(fo, covers), contribs=True)
        torch.manual_seed(1234)
        x = torch.rand((rows, cols), device="cuda") * 2.0 - 1.0
        x[torch.rand((rows, cols), device="cuda") < 0.02] = MISSING
        shape = (rows,) + ((K,) if K > 1 else ()) + (cols + 1, cols + 1)
        outs = [torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")]
        native.predict_interactions(x, out=outs[0])
        expansion.predict_interactions(x, out=outs[1])
        torch.cuda.synchronize()
        want = outs[1].clone()
        same = bool(torch.equal(outs[0].view(torch.int32), want.view(torch.int32)))
        t_na, t_ex = timed([lambda: native.predict_interactions(x, out=outs[0]),
                            lambda: expansion.predict_interactions(x, out=outs[1])], ITERS, WARMUP)
        phi = torch.empty(shape[:-1], device="cuda")
        (t_phi,) = timed([lambda: native.predict_contribs(x, out=phi)], CONTRIBS_ITERS, 1)
        native.check()
        expansion.check()
        print(name, "native", float(np.median(t_na)), "expansion", float(np.median(t_ex)), "ms", flush=True)
        r = {"trees": T, "num_cols": cols, "min_depth": dmin, "max_depth": dmax, "leaf_dim": K, "nodes": int(fo["nodes"].size),
             "rows": rows, "form": "lds_triangles" if slabs else "in_place", "class_block": kb, "rows_per_tile": R, "lds_bytes": lds,
             **vst.stats("native", t_na), **vst.stats("expansion", t_ex), **vst.stats("native_contribs", t_phi),
             "ratio_median_native_over_expansion": float(np.median(t_na) / np.median(t_ex)),
             "ratio_interactions_to_contribs_native": float(np.median(t_na) / np.median(t_phi)),
             "native_device_bytes": int(native.info().device_bytes), "expansion_device_bytes": int(expansion.info().device_bytes),
             "same_bits": same, "variants": {}}
        native.close()
        expansion.close()
        del exp_nodes, phi
        for vkb in (1, 2, 4, 8):  # the native handle under each class block, blocks looped and over gridDim.y, alone
            if vkb > 1 and vkb >= 2 * K:
                continue
            got = vir.shape(cols, K, vkb)
            if got[1] != vkb:
                continue  # the forced block leaves no row: the handle falls back to 1, timed already
            for grid in (0, 1):
                if grid and vkb >= K:
                    continue  # one block: the two are the same launch
                h = native_handle(fo, covers, vkb, grid)
                (t_v,) = timed([lambda: h.predict_interactions(x, out=outs[0])], VARIANT_ITERS, 1)
                h.check()
                ok = bool(torch.equal(outs[0].view(torch.int32), want.view(torch.int32)))
                r["variants"][f"kb{vkb}_{'grid' if grid else 'loop'}"] = {"class_block": vkb, "rows_per_tile": got[2], "lds_bytes": got[3],
                                                                         "same_bits": ok, **vst.stats("native", t_v)}
                r["same_bits"] = r["same_bits"] and ok
                h.close()
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        del x, outs, want
    res["src_hash"] = bench.kernel_source_hash()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "vector_inter_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not all(r["same_bits"] for r in res["shapes"].values()):
        sys.exit("the vector-leaf handle and the expansion differ")


if __name__ == "__main__":
    main()
