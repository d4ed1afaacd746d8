"""Saabas contributions on a vector-leaf forest: the native handle (tahoe_vector_forest_create_ex with TAHOE_CREATE_VECTOR_APPROX)
against the only way to get the same values without it, the K-fold expansion on tahoe_sparse_forest_create_ex(num_classes = K,
TAHOE_CREATE_APPROX_CONTRIBS).

Per shape one irregular forest (tools/vector_shap_time.py's: random leaf vectors in shuffled order, covers from reach
probabilities) is served twice in one process: natively, and as its expansion into T x K trees with scalar leaves whose copies of a
tree carry that tree's covers.  The two outputs are compared bit for bit first.  Then predict_contribs_approx of both runs in turn,
each call -- one kernel launch -- between two hipEvents on the stream; median, min and max after warm-up.  Where a shape asks for
it the native handle is created again under every class block (TAHOE_VECTOR_SHAP_KB) and both accumulation forms
(TAHOE_APPROX_FORM), with the class blocks over gridDim.y and in a workgroup's loop (TAHOE_VECTOR_SHAP_GRID), timed alone and
compared bit for bit: the table the form rule of vector_approx.hip is chosen from.
    python tools/vector_approx_time.py [out_dir] [iterations]   -> <out_dir>/vector_approx_time.json (default
                                                                    profiles/vector_approx)"""
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
import vector_approx_ref as var  # noqa: E402
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402
from vector_shap_time import forest, stats  # noqa: E402

ARGS = sys.argv[1:]
OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "vector_approx")
ITERS = int(ARGS[1]) if len(ARGS) > 1 else 11
WARMUP = 2
VARIANT_ITERS = 5
MISSING = -999.0
KNOBS = ("TAHOE_VECTOR_SHAP_KB", "TAHOE_APPROX_FORM", "TAHOE_VECTOR_SHAP_GRID")
# (name, trees, num_cols, min_depth, max_depth, leaf_prob, max_tree_nodes, seed, K, batches, variants?): the random-forest shape of
# tools/vector_time.py at three K, and a wide one whose expansion's output (rows x 8 x 201 floats) stays at 211 MB
SHAPES = [("random_forest_k1", 100, 64, 4, 16, 0.32, 65535, 77, 1, (262144, 4096), False),
          ("random_forest_k8", 100, 64, 4, 16, 0.32, 65535, 77, 8, (262144, 4096), True),
          ("random_forest_k10", 100, 64, 4, 16, 0.32, 65535, 77, 10, (262144, 4096), False),
          ("wide_k8", 100, 200, 4, 16, 0.32, 65535, 78, 8, (32768,), True)]


def timed(handles, x, outs, iters, warmup):
    """predict_contribs_approx of each handle in turn (drift on the machine hits all) -> ms per handle"""
    for _ in range(warmup):
        for h, o in zip(handles, outs):
            h.predict_contribs_approx(x, out=o)
    torch.cuda.synchronize()
    ms = [[] for _ in handles]
    for _ in range(iters):
        for i, (h, o) in enumerate(zip(handles, outs)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            h.predict_contribs_approx(x, out=o)
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    for h in handles:
        h.check()
    return [np.array(m) for m in ms]


def native_handle(fo, covers, kb=None, form=None, grid=None):
    for name, v in zip(KNOBS, (kb, form, grid)):  # read once, at create
        os.environ.pop(name, None)
        if v is not None:
            os.environ[name] = str(v)
    h = ta.VectorForest(fo["nodes"], fo["trees"], fo["leaves"], fo["cols"], missing=MISSING, covers=covers, approx_contribs=True)
    for name in KNOBS:
        os.environ.pop(name, None)
    return h


def main():
    res = {"iterations": ITERS, "warmup": WARMUP, "variant_iterations": VARIANT_ITERS,
           "timing": "hipEvent pair around each predict_contribs_approx call", "shapes": {}}
    for name, T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K, batches, variants in SHAPES:
        fo, covers = forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K)
        native = native_handle(fo, covers)
        exp_nodes, exp_trees = vr.expand(fo)
        expansion = ta.capi.SparseForest(exp_nodes, exp_trees, cols, missing=MISSING, num_classes=K,
                                         covers=vsr.tile_covers(fo, covers), approx_contribs=True)
        kb, slab, waves = var.form_rule(cols, K)
        r = {"trees": T, "num_cols": cols, "min_depth": dmin, "max_depth": dmax, "leaf_dim": K, "nodes": int(fo["nodes"].size),
             "class_block": kb, "form": "slab" if slab else "in place", "waves_per_workgroup": waves,
             "native_device_bytes": int(native.info().device_bytes), "expansion_device_bytes": int(expansion.info().device_bytes),
             "same_bits": True, "batches": {}}
        for rows in batches:
            torch.manual_seed(1234)
            x = torch.rand((rows, cols), device="cuda") * 2.0 - 1.0
            x[torch.rand((rows, cols), device="cuda") < 0.02] = MISSING
            shape = (rows,) + ((K,) if K > 1 else ()) + (cols + 1,)
            outs = [torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")]
            native.predict_contribs_approx(x, out=outs[0])
            expansion.predict_contribs_approx(x, out=outs[1])
            torch.cuda.synchronize()
            want = outs[1].clone()
            same = bool(torch.equal(outs[0].view(torch.int32), want.view(torch.int32)))
            t_na, t_ex = timed([native, expansion], x, outs, ITERS, WARMUP)
            ratio = float(np.median(t_na) / np.median(t_ex))
            b = {**stats("native", t_na), **stats("expansion", t_ex), "native_rows_per_s": rows / (float(np.median(t_na)) * 1e-3),
                 "expansion_rows_per_s": rows / (float(np.median(t_ex)) * 1e-3), "ratio_median_native_over_expansion": ratio,
                 "winner": "native" if ratio < 1.0 else "expansion", "same_bits": same}
            if variants and rows == batches[0]:  # every class block and form, blocks over gridDim.y and looped, alone
                b["variants"] = {}
                for vkb in (1, 2, 4, 8):
                    for form in (1, 2):
                        for grid in (1, 0):
                            if not grid and vkb >= K:
                                continue  # one block: the two are the same launch
                            h = native_handle(fo, covers, vkb, form, grid)
                            (t_v,) = timed([h], x, outs[:1], VARIANT_ITERS, 1)
                            ok = bool(torch.equal(outs[0].view(torch.int32), want.view(torch.int32)))
                            fk, fs, fw = var.form_rule(cols, K, vkb, form)
                            b["variants"][f"kb{vkb}_{'slab' if fs else 'inplace'}_{'grid' if grid else 'loop'}"] = {
                                "class_block": fk, "slab": fs, "waves_per_workgroup": fw,
                                "wave_slab_bytes": var.wave_slab_bytes(cols, fk) if fs else 0, "same_bits": ok, **stats("native", t_v)}
                            same = same and ok
                            h.close()
            r["batches"][str(rows)] = b
            r["same_bits"] = r["same_bits"] and same
            print(name, rows, json.dumps(b), flush=True)
            del x, outs, want
        native.close()
        expansion.close()
        del exp_nodes
        res["shapes"][name] = r
    res["src_hash"] = bench.kernel_source_hash()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "vector_approx_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not all(r["same_bits"] for r in res["shapes"].values()):
        sys.exit("the vector-leaf handle and the expansion differ")


if __name__ == "__main__":
    main()
