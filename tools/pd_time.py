"""Partial dependence (tahoe_forest_predict_partial_dependence): time per call and per visited node.

Two forests: 1000 complete trees of depth 6 on 64 features (through dense_to_sparse), and K5's irregular forest (2000 trees of
depth 4..24 on 256 features; no leaf deeper than 32 edges, so nothing is cut).  Neither generator gives covers: a leaf gets a
random cover in [1, 100), an internal node the sum of its children's.  One and two targets, grids of 100 and 10 000 points drawn
from the standard normal (the generators' thresholds lie in the same range).  Per shape: the GPU time of a call (hipEvent pair
around its launches, median / min / max over the iterations after warm-up) and its wall time with a synchronise, the nodes a grid
point visits under the restatement's rule (counted on the host for a sample of 64 grid points: a target split passes a point to one
child, any other split to every child of positive cover), and from the two the time per visited node.
For scale only, the time of predict_raw on G x 1000 rows: what replicating a background of 1000 rows per grid point would cost.
That is a DIFFERENT quantity (an average over a data set, not over the node covers); it is here to size the work, not to compare.
No threshold on any time.
    python tools/pd_time.py [out_dir] [iterations]      -> <out_dir>/pd_time.json (default profiles/pd)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import tahoe_amd as ta  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pd")
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
WARMUP = 3
MISSING = -999.0
SAMPLE = 64


def synth_covers(sn, tr):
    rng = np.random.default_rng(7)
    cv = rng.uniform(1.0, 100.0, sn.size)
    root_of = np.repeat(tr, np.diff(np.append(tr, sn.size)))
    inner = np.flatnonzero(sn["bits"] >= 0)
    left = root_of[inner] + sn["left_idx"][inner]
    for i, l in zip(inner[::-1], left[::-1]):  # children lie after their parent
        cv[i] = cv[l] + cv[l + 1]
    return cv.astype(np.float32), root_of


def max_depth(sn, tr, root_of):
    depth = np.zeros(sn.size, np.int32)
    inner = np.flatnonzero(sn["bits"] >= 0)
    left = root_of[inner] + sn["left_idx"][inner]
    for i, l in zip(inner, left):
        depth[l] = depth[l + 1] = depth[i] + 1
    return int(depth.max())


def visited_nodes(sn, tr, root_of, cv, feats, pts):
    """Nodes each of the points visits, summed over the trees: level by level over all trees at once."""
    bits = sn["bits"].view(np.uint32)
    col = {f: j for j, f in enumerate(feats)}
    nodes = tr.astype(np.int64)
    mask = np.ones((nodes.size, pts.shape[0]), bool)
    total = np.zeros(pts.shape[0], np.int64)
    while nodes.size:
        total += mask.sum(0)
        keep = (bits[nodes] >> 31) == 0
        nodes, mask = nodes[keep], mask[keep]
        fid = (bits[nodes] & ((1 << 30) - 1)).astype(np.int64)
        left = root_of[nodes] + sn["left_idx"][nodes]
        ml = mask & (cv[left] > 0)[:, None]
        mr = mask & (cv[left + 1] > 0)[:, None]
        for f, j in col.items():
            at = np.flatnonzero(fid == f)
            right = pts[None, :, j] >= sn["val"][nodes[at]][:, None]  # (no missing values or NaN in these grids)
            ml[at] = mask[at] & ~right
            mr[at] = mask[at] & right
        nodes = np.concatenate([left, left + 1])
        mask = np.concatenate([ml, mr])
        live = mask.any(1)
        nodes, mask = nodes[live], mask[live]
    return total


def time_calls(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    slow = time.perf_counter() - t0 > 0.25  # a call of a quarter second: 5 timed calls after that one say enough
    for _ in range(0 if slow else WARMUP - 1):
        fn()
    torch.cuda.synchronize()
    gpu, wall = [], []
    for _ in range(5 if slow else ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        gpu.append(a.elapsed_time(b))
    return {"gpu_ms_median": float(np.median(gpu)), "gpu_ms_min": float(np.min(gpu)), "gpu_ms_max": float(np.max(gpu)),
            "wall_ms_median": float(np.median(wall)), "timed_calls": len(gpu)}


def run(name, sn, tr, cols, res):
    cv, root_of = synth_covers(sn, tr)
    depth = max_depth(sn, tr, root_of)
    assert depth <= 32, depth
    f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, covers=cv, partial_dependence=True)
    inner = sn[sn["bits"] >= 0]
    used = np.bincount(inner["bits"] & ((1 << 30) - 1), minlength=cols)
    top = np.argsort(-used)[:2].tolist()  # the two most used features: the targets that divide the most
    entry = {"trees": int(tr.size), "nodes": int(sn.size), "features": cols, "max_depth": depth,
             "device_bytes": int(f.info().device_bytes), "targets": top, "shapes": {}}
    rng = np.random.default_rng(5)
    for nt in (1, 2):
        feats = top[:nt]
        for G in (100, 10_000):
            pts = rng.normal(size=(G, nt)).astype(np.float32)
            grid = torch.from_numpy(pts).cuda()
            out = torch.empty(G, dtype=torch.float32, device="cuda")
            t = time_calls(lambda: f.partial_dependence(feats, grid, out))
            f.check()
            visited = visited_nodes(sn, tr, root_of, cv, feats, pts[:SAMPLE])
            per_point = float(visited.mean())
            t.update({"visited_nodes_per_grid_point": per_point, "visited_sample": int(min(SAMPLE, G)),
                      "ns_per_visited_node": t["gpu_ms_median"] * 1e6 / (per_point * G)})
            entry["shapes"][f"targets{nt}_G{G}"] = t
            print(name, nt, G, json.dumps(t), flush=True)
    for G in (100, 10_000):  # for scale: predict on G x 1000 rows (a different quantity)
        x = torch.randn((G * 1000, cols), dtype=torch.float32, device="cuda")
        o = torch.empty(G * 1000, dtype=torch.float32, device="cuda")
        t = time_calls(lambda: f.predict_raw(x, o))
        t["rows"], t["kernel_form"] = G * 1000, f.kernel_form(G * 1000)
        entry["shapes"][f"predict_raw_replicated_G{G}"] = t
        print(name, "predict_raw", G, json.dumps(t), flush=True)
        del x, o
    f.close()
    res["forests"][name] = entry


def main():
    res = {"what": "tahoe_forest_predict_partial_dependence; predict_raw_replicated_* is predict on G x 1000 random rows, a "
                   "different quantity, for scale only", "iterations": ITERS, "forests": {}}
    T, D, cols = 1000, 6, 64
    sn, tr = ta.capi.dense_to_sparse(ta.synth_forest(T, D, cols, seed=42), T, D)
    run("depth6_1000trees_64features", sn, tr, cols, res)
    # the chunk (TAHOE_PD_CHUNK_ROWS, read at create): 100 000 grid points, one target, through workspaces of 4 MiB .. 512 MiB
    cv, _ = synth_covers(sn, tr)
    grid = torch.randn((100_000, 1), dtype=torch.float32, device="cuda")
    out = torch.empty(100_000, dtype=torch.float32, device="cuda")
    sweep = {}
    for chunk in (1024, 4096, 0, 32768, 131072):  # 0: the default
        if chunk:
            os.environ["TAHOE_PD_CHUNK_ROWS"] = str(chunk)
        f = ta.capi.SparseForest(sn, tr, cols, missing=MISSING, covers=cv, partial_dependence=True)
        os.environ.pop("TAHOE_PD_CHUNK_ROWS", None)
        t = time_calls(lambda: f.partial_dependence([0], grid, out))
        t["device_bytes"] = int(f.info().device_bytes)
        sweep["default" if not chunk else str(chunk)] = t
        print("chunk", chunk, json.dumps(t), flush=True)
        f.close()
    res["chunk_sweep_depth6_G100000"] = sweep
    _, (sn, tr, cols), _ = bench.baseline_workload(ta, "K5")
    run("K5", sn, tr, cols, res)
    res["src_hash"] = bench.kernel_source_hash()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "pd_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
