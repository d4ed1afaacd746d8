"""Category-set splits on oblivious forests (tahoe_oblivious_forest_create_cat): two measurements.

(b) Sets against the only other way to serve such a model, the expansion into complete trees on a categorical SparseForest:
    python tools/oblivious_cat_time.py [out_dir] [iterations] [rows]   -> <out_dir>/oblivious_cat_time.json (default
    profiles/oblivious_cat).  One forest of 1000 trees of depth 6 on 64 features, a third of them categorical (every level on such
    a feature is a set), once with one-hot sets on 32 categories (a set rides in its split record) and once with sets of about
    half of 100 categories (four words in the pool).  Both handles run under AUTO, in turn, timed by their own kernel-time
    profiling; the outputs are compared bit for bit and the device bytes recorded.

(a) Numeric handles must not pay for the sets.  Two builds of the library in two checkouts -- the parent commit and this tree --
    run the same numeric shapes alternately in one session, each run a process of its own, and the parent also against itself:
    python tools/oblivious_cat_time.py --compare <parent_checkout> <branch_checkout> [out_dir] [rounds]
    merges "numeric_parent_vs_branch" into the same JSON: per measurement the medians of every run, the branch / parent ratio of
    the medians over the rounds, and the parent / parent spread it has to lie in.  The shapes are those of tools/oblivious_time.py
    (predict_raw, 1 M rows) and, for the four explanation kernels, those of tools/oblivious_shap_time.py, oblivious_inter_time.py
    and oblivious_iv_time.py.
    python tools/oblivious_cat_time.py --numeric <checkout>    one such run: a JSON line of medians (what --compare starts)"""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1].startswith("--") else None
LIB_ROOT = sys.argv[2] if MODE == "--numeric" else ROOT
sys.path.insert(0, LIB_ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MISSING = -999.0
WARMUP = 3
# (name, trees, depth, num_cols, K) of tools/oblivious_time.py
WALK_SHAPES = [("catboost_default_depth6", 1000, 6, 64, 1), ("vector_leaves_k8", 100, 6, 64, 8), ("depth10_cols256", 1000, 10, 256, 1)]
# (name, trees, depth, num_cols, K, rows of Saabas, rows of the interaction and interventional values)
SHAP_SHAPES = [("catboost_default_depth6", 1000, 6, 64, 1, 262144, 4096), ("vector_leaves_k8", 100, 6, 64, 8, 262144, 4096)]


def numeric_forest(T, D, cols, K, seed):
    rng = np.random.default_rng(seed)
    return dict(depths=np.full(T, D, np.int32), fids=rng.integers(0, cols, T * D), thr=rng.uniform(-1.0, 1.0, T * D).astype(np.float32),
                def_left=rng.integers(0, 2, T * D).astype(bool), leaves=rng.standard_normal(T * (1 << D) * K).astype(np.float32),
                k=K, cols=cols)


def numeric_rows(torch, rows, cols):
    torch.manual_seed(1234)
    x = torch.rand((rows, cols), device="cuda") * 2.0 - 1.0
    x[torch.rand((rows, cols), device="cuda") < 0.02] = MISSING
    return x


def event_ms(torch, call, iters):
    """Medians need every sample: one hipEvent pair per call, after warm-up"""
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def numeric(iters=15):
    """The numeric shapes on the library of LIB_ROOT -> {measurement: median ms}"""
    import torch

    import tahoe_amd as ta

    res = {}
    for name, T, D, cols, K in WALK_SHAPES:
        fo = numeric_forest(T, D, cols, K, seed=len(name))
        f = ta.ObliviousForest(fo["depths"], fo["fids"], fo["thr"], fo["def_left"], fo["leaves"], cols, leaf_dim=K, missing=MISSING)
        x = numeric_rows(torch, 1_000_000, cols)
        out = torch.empty((x.shape[0], K) if K > 1 else (x.shape[0],), device="cuda")
        res["predict_raw " + name] = event_ms(torch, lambda: f.predict_raw(x, out), iters)
        f.check()
        f.close()
        del x, out
    for name, T, D, cols, K, rows_approx, rows_pairs in SHAP_SHAPES:
        fo = numeric_forest(T, D, cols, K, seed=len(name))
        covers = np.random.default_rng(7).integers(1, 1025, T << D).astype(np.float32)
        f = ta.ObliviousForest(fo["depths"], fo["fids"], fo["thr"], fo["def_left"], fo["leaves"], cols, leaf_dim=K, missing=MISSING,
                               leaf_covers=covers, contribs=True, approx_contribs=True, interactions=True, interventional=True)
        x = numeric_rows(torch, rows_approx, cols)
        shape = lambda rows, dims: (rows,) + ((K,) if K > 1 else ()) + (cols + 1,) * dims  # noqa: E731
        out = torch.empty(shape(rows_approx, 1), device="cuda")
        res["contribs_approx " + name] = event_ms(torch, lambda: f.predict_contribs_approx(x, out=out), iters)
        xs = x[:rows_pairs].contiguous()
        out = torch.empty(shape(rows_pairs, 1), device="cuda")
        res["contribs " + name] = event_ms(torch, lambda: f.predict_contribs(xs, out=out), max(iters // 3, 3))
        f.set_background(x[rows_pairs:rows_pairs + 100].contiguous())
        res["interventional_b100 " + name] = event_ms(torch, lambda: f.predict_contribs_interventional(xs, out=out), max(iters // 3, 3))
        out = torch.empty(shape(rows_pairs, 2), device="cuda")
        res["interactions " + name] = event_ms(torch, lambda: f.predict_interactions(xs, out=out), max(iters // 3, 3))
        f.check()
        f.close()
        del x, xs, out
    print(json.dumps(res), flush=True)


def compare(parent, branch, out_dir, rounds):
    """parent, branch, parent, parent, ... in turn; every run is a process of its own"""
    def run(root):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--numeric", root], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.exit(f"--numeric {root} failed ({out.returncode}): {out.stderr[-1500:]}")
        return json.loads(out.stdout.strip().splitlines()[-1])

    runs = {"parent_a": [], "branch": [], "parent_b": []}
    for _ in range(rounds):
        runs["parent_a"].append(run(parent))
        runs["branch"].append(run(branch))
        runs["parent_b"].append(run(parent))
    res = {"rounds": rounds, "order": "parent, branch, parent per round; each run its own process; hipEvent medians per run", "measurements": {}}
    for key in runs["branch"][0]:
        med = {who: [r[key] for r in rs] for who, rs in runs.items()}
        parent_all = med["parent_a"] + med["parent_b"]
        pp = [a / b for a, b in zip(med["parent_a"], med["parent_b"])] + [b / a for a, b in zip(med["parent_a"], med["parent_b"])]
        ratio = float(np.median(med["branch"]) / np.median(parent_all))
        res["measurements"][key] = {"ms_median_per_run": med, "branch_over_parent": ratio,
                                    "parent_over_parent_min": float(min(pp)), "parent_over_parent_max": float(max(pp)),
                                    "inside_parent_spread": bool(min(pp) <= ratio <= max(pp))}
        print(key, json.dumps(res["measurements"][key]), flush=True)
    merge(out_dir, "numeric_parent_vs_branch", res)


def merge(out_dir, key, value):
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "oblivious_cat_time.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[key] = value
    text = re.sub(r"\[\s+([^\[\]{}]*?)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", json.dumps(doc, indent=1))
    with open(path, "w") as fh:  # (a run's medians on one line)
        fh.write(text + "\n")


# ---- (b) sets against the categorical sparse expansion ----
def cat_forest(T, D, cols, ncat_cols, ncat, one_hot, seed):
    """-> (forest of tests/oblivious_cat_ref.py's kind, categorical columns): every level on one of the first ncat_cols features is
    a set over ncat categories -- one category (one-hot) or each category with probability 1/2"""
    import oblivious_cat_ref as ocr

    fo = numeric_forest(T, D, cols, 1, seed)
    rng = np.random.default_rng(seed + 1)
    sets = {}
    for s in np.flatnonzero(fo["fids"] < ncat_cols):
        sets[int(s)] = [int(rng.integers(0, ncat))] if one_hot else np.flatnonzero(rng.random(ncat) < 0.5).tolist()
    return ocr.with_sets(fo, sets)


def sets_against_the_expansion(out_dir, iters, rows):
    import torch

    import bench
    import oblivious_cat_ref as ocr
    import tahoe_amd as ta

    T, D, cols, ncat_cols = 1000, 6, 64, 21
    res = {"rows": rows, "iterations": iters, "warmup": WARMUP, "trees": T, "depth": D, "num_cols": cols,
           "categorical_cols": ncat_cols, "shapes": {}}
    for name, ncat, one_hot in (("one_hot_32_inline", 32, True), ("sets_of_100_pooled", 100, False)):
        fo = cat_forest(T, D, cols, ncat_cols, ncat, one_hot, seed=len(name))
        ob = ta.ObliviousForest(fo["depths"], fo["fids"], fo["thr"], fo["def_left"], fo["leaves"], cols, missing=MISSING,
                                **ocr.handle_args(fo))
        nodes, trees, categories, members_left, _ = ocr.expand_to_sparse(fo)
        sp = ta.capi.SparseForest(nodes, trees, cols, missing=MISSING, categories=categories, members_left=members_left)
        torch.manual_seed(1234)
        x = torch.rand((rows, cols), device="cuda") * 2.0 - 1.0
        x[:, :ncat_cols] = torch.randint(0, ncat + 4, (rows, ncat_cols), device="cuda").float()  # (a few ids no set holds)
        x[torch.rand((rows, cols), device="cuda") < 0.02] = MISSING
        outs = [torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")]
        hs = [ob, sp]
        for _ in range(WARMUP):
            for h, o in zip(hs, outs):
                h.predict_raw(x, o)
        torch.cuda.synchronize()
        for h in hs:
            h.set_profiling(iters)
        for _ in range(iters):  # in turn: drift on the machine hits both
            for h, o in zip(hs, outs):
                h.predict_raw(x, o)
        torch.cuda.synchronize()
        t_ob, t_sp = [h.kernel_times_ms() + h.prepass_times_ms() for h in hs]
        for h in hs:
            h.set_profiling(0)
            h.check()
        nsets = len(fo["cats"])
        r = {"categories": ncat, "levels_with_sets": nsets, "levels": T * D, "pool_bytes": ocr.pool_bytes(fo),
             "oblivious_form": ob.kernel_form(rows), "expansion_form": sp.kernel_form(rows),
             "oblivious_ms_median": float(np.median(t_ob)), "expansion_ms_median": float(np.median(t_sp)),
             "oblivious_ms_min": float(np.min(t_ob)), "expansion_ms_min": float(np.min(t_sp)),
             "ratio_median_oblivious_over_expansion": float(np.median(t_ob) / np.median(t_sp)),
             "oblivious_device_bytes": int(ob.info().device_bytes), "expansion_device_bytes": int(sp.info().device_bytes),
             "same_bits": bool(torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)))}
        res["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        ob.close()
        sp.close()
        del x, outs
    res["src_hash"] = bench.kernel_source_hash()
    merge(out_dir, "sets_against_the_sparse_expansion", res)
    if not all(r["same_bits"] for r in res["shapes"].values()):
        sys.exit("the oblivious handle and the expansion differ")


if __name__ == "__main__":
    default_out = os.path.join(ROOT, "profiles", "oblivious_cat")
    if MODE == "--numeric":
        numeric()
    elif MODE == "--compare":
        compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else default_out, int(sys.argv[5]) if len(sys.argv) > 5 else 3)
    else:
        args = sys.argv[1:]
        sets_against_the_expansion(args[0] if args else default_out, int(args[1]) if len(args) > 1 else 20,
                                   int(args[2]) if len(args) > 2 else 1_000_000)
