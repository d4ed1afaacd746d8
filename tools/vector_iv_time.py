"""Interventional TreeSHAP on a vector-leaf forest: the native handle (tahoe_vector_forest_create_ex with
TAHOE_CREATE_INTERVENTIONAL, no covers) against the only way to get the same values without it, the K-fold expansion on
tahoe_sparse_forest_create_ex(num_classes = K, TAHOE_CREATE_CONTRIBS).

The forests are those of tools/vector_shap_time.py (100 trees from tahoe_synth_sparse_forest, depth <= 16, 64 features, K in
{1, 8, 10}) and one of the same shape on 200 features with K = 8, each served twice in one process.  Both handles get the same
background of B rows (set_background is timed once per handle, host clock: the call is synchronous); the two outputs are compared
bit for bit first.  Then predict_contribs_interventional of both runs in turn, each call -- one kernel launch -- between two hipEvents on the stream;
median, min and max after warm-up.  The native handle is then created again under each class block (TAHOE_VECTOR_SHAP_KB), with the
class blocks in a workgroup's loop and over gridDim.y (TAHOE_VECTOR_SHAP_GRID = 0 / 1), and timed alone over fewer iterations:
the alternatives to the rule of vector_iv_shape.
    python tools/vector_iv_time.py [out_dir] [iterations] [rows] [background rows]
        -> <out_dir>/vector_iv_time.json (default profiles/vector_iv)"""
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
import tahoe_amd as ta  # noqa: E402
import vector_iv_ref as vir  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402
import vector_shap_time as vst  # noqa: E402  (the forests; its command line has the same first three arguments)

ARGS = sys.argv[1:]
OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "vector_iv")
ITERS = int(ARGS[1]) if len(ARGS) > 1 else 20
ROWS = int(ARGS[2]) if len(ARGS) > 2 else 4096
BG_ROWS = int(ARGS[3]) if len(ARGS) > 3 else 100
WARMUP = 3
VARIANT_ITERS = 5  # the forced class blocks, timed alone after one warm-up call
MISSING = vst.MISSING
KNOBS = ("TAHOE_VECTOR_SHAP_KB", "TAHOE_VECTOR_SHAP_GRID")
# tools/vector_shap_time.py's shapes, and the same forest shape on 200 features with K = 8: there the rule's widest block leaves a
# tile of 2 rows (KB, R) = (8, 2), and the forced KB = 4 gives (4, 4) -- what a rule that wants R >= 4 first would choose
SHAPES = vst.SHAPES + [("random_forest_k8_200_cols", 100, 200, 4, 16, 0.32, 65535, 78, 8)]


def timed(handles, x, outs, iters, warmup):
    """predict_contribs_interventional of each handle in turn (drift on the machine hits all) -> ms per handle"""
    for _ in range(warmup):
        for h, o in zip(handles, outs):
            h.predict_contribs_interventional(x, out=o)
    torch.cuda.synchronize()
    ms = [[] for _ in handles]
    for _ in range(iters):
        for i, (h, o) in enumerate(zip(handles, outs)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            h.predict_contribs_interventional(x, out=o)
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    for h in handles:
        h.check()
    return [np.array(m) for m in ms]


def native_handle(fo, kb=None, grid=None):
    for name, v in zip(KNOBS, (kb, grid)):  # read once, at create
        os.environ.pop(name, None)
        if v is not None:
            os.environ[name] = str(v)
    h = ta.VectorForest(fo["nodes"], fo["trees"], fo["leaves"], fo["cols"], missing=MISSING, interventional=True)
    for name in KNOBS:
        os.environ.pop(name, None)
    return h


def with_background(h, bg):
    """-> (seconds of set_background, device bytes it added)"""
    base = int(h.info().device_bytes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h.set_background(bg)
    return time.perf_counter() - t0, int(h.info().device_bytes) - base


def main():
    res = {"rows": ROWS, "background_rows": BG_ROWS, "iterations": ITERS, "warmup": WARMUP,
           "timing": "hipEvent pair around each predict_contribs_interventional call", "shapes": {}}
    for name, T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K in SHAPES:
        fo, covers = vst.forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K)
        native = native_handle(fo)
        exp_nodes, exp_trees = vr.expand(fo)
        expansion = ta.capi.SparseForest(exp_nodes, exp_trees, cols, missing=MISSING, num_classes=K,
                                         covers=vsr.tile_covers(fo, covers), contribs=True)
        torch.manual_seed(1234)
        x = torch.rand((ROWS, cols), device="cuda") * 2.0 - 1.0
        x[torch.rand((ROWS, cols), device="cuda") < 0.02] = MISSING
        bg = torch.rand((BG_ROWS, cols), device="cuda") * 2.0 - 1.0
        bg[torch.rand((BG_ROWS, cols), device="cuda") < 0.02] = MISSING
        base_na, base_ex = int(native.info().device_bytes), int(expansion.info().device_bytes)
        s_na, add_na = with_background(native, bg)
        s_ex, add_ex = with_background(expansion, bg)
        shape = (ROWS,) + ((K,) if K > 1 else ()) + (cols + 1,)
        outs = [torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")]
        native.predict_contribs_interventional(x, out=outs[0])
        expansion.predict_contribs_interventional(x, out=outs[1])
        torch.cuda.synchronize()
        want = outs[1].clone()
        same = bool(torch.equal(outs[0].view(torch.int32), want.view(torch.int32)))
        t_na, t_ex = timed([native, expansion], x, outs, ITERS, WARMUP)
        kb, R, wlds, lds = vir.iv_shape(cols, K)
        consts = (1024 + K) * 4
        r = {"trees": T, "num_cols": cols, "min_depth": dmin, "max_depth": dmax, "leaf_dim": K, "nodes": int(fo["nodes"].size),
             "class_block": kb, "rows_per_tile": R, "weights_in_lds": wlds, "lds_bytes": lds,
             **vst.stats("native", t_na), **vst.stats("expansion", t_ex),
             "native_rows_per_s": ROWS / (float(np.median(t_na)) * 1e-3), "expansion_rows_per_s": ROWS / (float(np.median(t_ex)) * 1e-3),
             "ratio_median_native_over_expansion": float(np.median(t_na) / np.median(t_ex)),
             "native_set_background_ms": s_na * 1e3, "expansion_set_background_ms": s_ex * 1e3,
             "native_mask_bytes": add_na - consts, "expansion_mask_bytes": add_ex - consts,
             "native_device_bytes": base_na, "expansion_device_bytes": base_ex,
             "native_device_bytes_with_background": base_na + add_na, "expansion_device_bytes_with_background": base_ex + add_ex,
             "same_bits": same, "variants": {}}
        native.close()
        expansion.close()
        del exp_nodes
        for vkb in (1, 2, 4, 8):  # the native handle under each class block, blocks looped and over gridDim.y, alone
            if vkb > 1 and vkb >= 2 * K:
                continue
            for grid in (0, 1):
                if grid and vkb >= K:
                    continue  # one block: the two are the same launch
                h = native_handle(fo, vkb, grid)
                h.set_background(bg)
                (t_v,) = timed([h], x, outs[:1], VARIANT_ITERS, 1)
                vk, vrows = vir.iv_shape(cols, K, vkb)[:2]
                ok = bool(torch.equal(outs[0].view(torch.int32), want.view(torch.int32)))
                r["variants"][f"kb{vkb}_{'grid' if grid else 'loop'}"] = {"class_block": vk, "rows_per_tile": vrows, "same_bits": ok,
                                                                         **vst.stats("native", t_v)}
                r["same_bits"] = r["same_bits"] and ok
                h.close()
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        del x, bg, outs
    res["src_hash"] = bench.kernel_source_hash()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "vector_iv_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not all(r["same_bits"] for r in res["shapes"].values()):
        sys.exit("the vector-leaf handle and the expansion differ")


if __name__ == "__main__":
    main()
