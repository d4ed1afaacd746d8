"""TreeSHAP on a vector-leaf forest: the native handle (tahoe_vector_forest_create_ex with TAHOE_CREATE_CONTRIBS) against the only
way to get the same values without it, the K-fold expansion on tahoe_sparse_forest_create_ex(num_classes = K).

Per shape one irregular forest (tahoe_synth_sparse_forest) gets a table of random leaf vectors, one per leaf in shuffled order, and
covers from reach probabilities (the root 1, a child its parent's cover times a random share), and is served twice in one process:
natively, and as its expansion into T x K trees with scalar leaves (tests/vector_ref.py, expand) whose copies of a tree carry that
tree's covers.  The two outputs are compared bit for bit first.  Then predict_contribs of both runs in turn, each call -- one
kernel launch -- between two hipEvents on the stream (the explanation calls are not covered by the handles' kernel-time
profiling); median, min and max after warm-up.  The native handle is then created again under each class block
(TAHOE_VECTOR_SHAP_KB), with the class blocks in a workgroup's loop and over gridDim.y (TAHOE_VECTOR_SHAP_GRID = 0 / 1), and timed
alone over fewer iterations; where the handle has more than one class block the two are timed once more on 32768 rows.
    python tools/vector_shap_time.py [out_dir] [iterations] [rows]   -> <out_dir>/vector_shap_time.json (default
                                                                         profiles/vector_shap)"""
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
import vector_shap_ref as vsr  # noqa: E402

ARGS = sys.argv[1:]
OUT = ARGS[0] if len(ARGS) > 0 else os.path.join(ROOT, "profiles", "vector_shap")
ITERS = int(ARGS[1]) if len(ARGS) > 1 else 20
ROWS = int(ARGS[2]) if len(ARGS) > 2 else 4096
WARMUP = 3
VARIANT_ITERS = 5   # the forced class blocks, timed alone after one warm-up call (the slow ones take seconds per call)
LARGE_ROWS = 32768  # ... and the two ways of running the class blocks once more where the row tiles alone fill the device
MISSING = -999.0
# (name, trees, num_cols, min_depth, max_depth, leaf_prob, max_tree_nodes, seed, K): the random-forest shape of tools/vector_time.py
SHAPES = [("random_forest_k1", 100, 64, 4, 16, 0.32, 65535, 77, 1),
          ("random_forest_k8", 100, 64, 4, 16, 0.32, 65535, 77, 8),
          ("random_forest_k10", 100, 64, 4, 16, 0.32, 65535, 77, 10)]


def forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K):
    nodes, trees = ta.capi.synth_sparse_forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed)
    rng = np.random.default_rng(seed + 1)
    is_leaf = nodes["bits"] < 0
    L = int(is_leaf.sum())
    nodes["left_idx"][is_leaf] = rng.permutation(L).astype(np.int32)
    nodes["val"][is_leaf] = 0.0
    fo = dict(nodes=nodes, trees=trees, leaves=rng.standard_normal((L, K)).astype(np.float32), k=K, cols=cols)
    # reach probabilities: children come after their parent, so one forward pass per tree
    covers = np.ones(nodes.size)
    share = rng.uniform(0.1, 0.9, nodes.size)
    bounds = list(trees) + [nodes.size]
    for t in range(trees.size):
        lo, hi = int(bounds[t]), int(bounds[t + 1])
        for i in np.nonzero(~is_leaf[lo:hi])[0]:
            li = lo + int(nodes["left_idx"][lo + i])
            covers[li], covers[li + 1] = covers[lo + i] * share[lo + i], covers[lo + i] * (1.0 - share[lo + i])
    return fo, np.maximum(covers, 1e-30).astype(np.float32)


def timed(handles, x, outs, iters=None, warmup=None):
    """predict_contribs of each handle in turn (drift on the machine hits all) -> ms per handle, ITERS each"""
    iters, warmup = iters or ITERS, warmup or WARMUP
    for _ in range(warmup):
        for h, o in zip(handles, outs):
            h.predict_contribs(x, out=o)
    torch.cuda.synchronize()
    ms = [[] for _ in handles]
    for _ in range(iters):
        for i, (h, o) in enumerate(zip(handles, outs)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            h.predict_contribs(x, out=o)
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    for h in handles:
        h.check()
    return [np.array(m) for m in ms]


def stats(prefix, ms):
    return {prefix + "_ms_median": float(np.median(ms)), prefix + "_ms_min": float(np.min(ms)), prefix + "_ms_max": float(np.max(ms))}


def native_handle(fo, covers, kb=None, grid=None):
    for name, v in (("TAHOE_VECTOR_SHAP_KB", kb), ("TAHOE_VECTOR_SHAP_GRID", grid)):  # read once, at create
        os.environ.pop(name, None)
        if v is not None:
            os.environ[name] = str(v)
    h = ta.VectorForest(fo["nodes"], fo["trees"], fo["leaves"], fo["cols"], missing=MISSING, covers=covers, contribs=True)
    for name in ("TAHOE_VECTOR_SHAP_KB", "TAHOE_VECTOR_SHAP_GRID"):
        os.environ.pop(name, None)
    return h


def tile_shape(cols, K, kb=None):
    """(KB, R) of the handle: the rule of vector_shap_build, restated for the record"""
    def rows(kb, floor):
        per_row, r = (1 + 4 * kb) * cols * 4, 64
        while r > 1 and r * per_row > 80 * 1024:
            r //= 2
        return r if kb == 1 or (r * per_row <= 80 * 1024 and r >= floor) else 0
    if kb is None:
        kb = next((c for c in (8, 4, 2) if c < 2 * K and rows(c, 4)), 1)
    elif not rows(kb, 1):
        kb = 1
    return kb, rows(kb, 1)


def main():
    res = {"rows": ROWS, "iterations": ITERS, "warmup": WARMUP, "timing": "hipEvent pair around each predict_contribs call",
           "shapes": {}}
    for name, T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K in SHAPES:
        fo, covers = forest(T, cols, dmin, dmax, leaf_prob, max_nodes, seed, K)
        native = native_handle(fo, covers)
        exp_nodes, exp_trees = vr.expand(fo)
        expansion = ta.capi.SparseForest(exp_nodes, exp_trees, cols, missing=MISSING, num_classes=K,
                                         covers=vsr.tile_covers(fo, covers), contribs=True)
        torch.manual_seed(1234)
        x = torch.rand((ROWS, cols), device="cuda") * 2.0 - 1.0
        x[torch.rand((ROWS, cols), device="cuda") < 0.02] = MISSING
        shape = (ROWS,) + ((K,) if K > 1 else ()) + (cols + 1,)
        outs = [torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")]
        native.predict_contribs(x, out=outs[0])
        expansion.predict_contribs(x, out=outs[1])
        torch.cuda.synchronize()
        want = outs[1].clone()
        same = bool(torch.equal(outs[0].view(torch.int32), want.view(torch.int32)))
        t_na, t_ex = timed([native, expansion], x, outs)
        kb, R = tile_shape(cols, K)
        r = {"trees": T, "num_cols": cols, "min_depth": dmin, "max_depth": dmax, "leaf_dim": K, "nodes": int(fo["nodes"].size),
             "class_block": kb, "rows_per_tile": R, **stats("native", t_na), **stats("expansion", t_ex),
             "native_rows_per_s": ROWS / (float(np.median(t_na)) * 1e-3), "expansion_rows_per_s": ROWS / (float(np.median(t_ex)) * 1e-3),
             "ratio_median_native_over_expansion": float(np.median(t_na) / np.median(t_ex)),
             "native_device_bytes": int(native.info().device_bytes), "expansion_device_bytes": int(expansion.info().device_bytes),
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
                h = native_handle(fo, covers, vkb, grid)
                (t_v,) = timed([h], x, outs[:1], VARIANT_ITERS, 1)
                vk, vr_ = tile_shape(cols, K, vkb)
                ok = bool(torch.equal(outs[0].view(torch.int32), want.view(torch.int32)))
                r["variants"][f"kb{vkb}_{'grid' if grid else 'loop'}"] = {"class_block": vk, "rows_per_tile": vr_, "same_bits": ok,
                                                                         **stats("native", t_v)}
                r["same_bits"] = r["same_bits"] and ok
                h.close()
        if (K + kb - 1) // kb > 1:  # more than one class block: loop against gridDim.y on a batch whose tiles fill the device
            xl = torch.rand((LARGE_ROWS, cols), device="cuda") * 2.0 - 1.0
            ol = [torch.empty((LARGE_ROWS,) + shape[1:], device="cuda")]
            r["large_batch"] = {"rows": LARGE_ROWS}
            for grid in (0, 1):
                h = native_handle(fo, covers, kb, grid)
                (t_v,) = timed([h], xl, ol, VARIANT_ITERS, 1)
                r["large_batch"][f"kb{kb}_{'grid' if grid else 'loop'}"] = stats("native", t_v)
                h.close()
            del xl, ol
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        del x, outs
    res["src_hash"] = bench.kernel_source_hash()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "vector_shap_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    if not all(r["same_bits"] for r in res["shapes"].values()):
        sys.exit("the vector-leaf handle and the expansion differ")


if __name__ == "__main__":
    main()
