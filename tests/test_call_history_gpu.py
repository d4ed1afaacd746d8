"""One long-lived handle per kind, every option it can carry switched on at create, serving a fixed, written-out sequence of every
entry point the kind has -- twice over -- with the strategy cycling through those set_strategy accepts and the row count
alternating large / 65 / 1.  Needs an MI355X.

The property under test is independence from call history: predict_csr may free and reallocate the chunk buffer, predict_staged
and the stages live beside the plain walk, set_background predicts as DIRECT and then restores the strategy, predict_host owns
three streams, check clears two flag words, QRING's workspace grows and stays.  So
  - every output is the interior of a tests/guarded.py buffer and the handle is check()ed after each call;
  - prediction calls are held to the oracle (the numpy restatements for the categorical and the native handles), bit for bit;
  - explanation calls are held to the bits the same call gives on a FRESH handle that has made no other call -- bitwise
    reproducibility is what the header promises; the values themselves are pinned by the per-feature tests -- and a smaller batch
    to the bits of the same rows in the large one;
  - get_strategy after set_background is the strategy set before it.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import categorical_ref  # noqa: E402
import oblivious_ref as obr  # noqa: E402
import pd_cases  # noqa: E402
import pd_ref  # noqa: E402
import test_staged_native_gpu as sng  # noqa: E402  (running_sums, the per-tree leaf vectors)
import vector_ref as vr  # noqa: E402
import vector_shap_ref as vsr  # noqa: E402
from guarded import Guarded, guarded_input  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING = -999.0
LARGE = "large"

# The sequence: (entry point, rows or an argument).  A kind skips what it does not serve (SERVES below); everything else runs in
# this order, and the whole list runs twice on the same handle.
SEQUENCE = [
    ("predict_raw", LARGE),
    ("predict_contribs", 65),
    ("predict_csr_chunked", 1),      # DIRECT: the densified fallback, its chunk buffer sized for one row ...
    ("predict_staged", LARGE),
    ("set_background", "b"),
    ("predict_contribs_interventional", 65),
    ("predict_leaf_idx", 1),
    ("predict_host", LARGE),
    ("predict_interactions", 65),
    ("check", None),
    ("predict_contribs_approx", 1),
    ("set_background", "a"),
    ("predict_contribs_interventional", LARGE),
    ("set_stages", "b"),
    ("predict_staged", 65),
    ("set_stages", "a"),
    ("predict_csr_chunked", 65),     # ... which this call frees and reallocates (the first lap; checked in device_bytes)
    ("predict_accumulate", 1),
    ("reserve_csr", None),
    ("predict_csr", LARGE),
    ("partial_dependence", 65),
    ("predict", 1),
    ("predict_contribs", LARGE),
    ("predict_staged", 1),
    ("predict_leaf_idx", LARGE),
    ("predict_csr", 65),
    ("predict_interactions", 1),
    ("predict_host", 65),
    ("predict_contribs_approx", LARGE),
    ("predict_raw", 65),
    ("predict_accumulate", LARGE),
    ("partial_dependence", LARGE),
    ("predict_host", 1),
    ("predict_contribs_interventional", 1),
    ("predict", LARGE),
    ("check", None),
]
EXPLAIN = {"predict_contribs": 1, "predict_interactions": 2, "predict_contribs_interventional": 1, "predict_contribs_approx": 1}
COMMON = {"predict", "predict_raw", "predict_leaf_idx", "predict_staged", "set_stages", "set_background", "check"} | set(EXPLAIN)
CSR = {"predict_csr", "predict_csr_chunked", "reserve_csr"}
SERVES = {
    "dense": COMMON | CSR | {"predict_accumulate", "predict_host"},
    "dense3": COMMON | CSR,
    "sparse": COMMON | CSR | {"predict_accumulate", "predict_host", "partial_dependence"},
    "categorical": COMMON | CSR | {"predict_accumulate", "predict_host", "partial_dependence"},
    "oblivious": COMMON | {"predict_accumulate"},
    "vector9": COMMON,
}


@pytest.fixture(scope="module")
def env(built):
    import torch

    import tahoe_amd as ta
    from oracle import oracle

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    return ta, oracle, torch


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


class Kind:
    """make() -> a handle with every option on; data [large, cols]; raw [large] / [large, C]; leaf [large, T] uint32;
    cont(start) -> continued sums; stages / staged: {"a" / "b": rounds / the raw stage sums [large, S(, C)]}; bg: {"a" / "b": rows};
    pd: (targets, grid [large, nt], want [large, C]) or None."""


def staged_of(run, rounds, C):
    w = run[:, np.asarray(rounds) - 1]
    return np.ascontiguousarray(w[:, :, 0] if C == 1 else w)


def build(kind, env):
    ta, oracle, torch = env
    k = Kind()
    k.name, k.pd, k.cont = kind, None, None
    if kind in ("dense", "dense3"):
        C = 1 if kind == "dense" else 3
        T, D, cols, R = 36, 6, 16, 1000
        nodes = ta.synth_forest(T, D, cols, seed=31 + C, leaf_prob=0.1)
        nodes["weight"] = np.random.default_rng(5).uniform(0.05, 1.0, nodes.size).astype(np.float32)  # covers
        per = ta.capi.tree_num_nodes(D)
        k.data = ta.synth_data(R, cols, seed=33, missing_prob=0.05, missing=MISSING, nan_prob=0.01)
        k.make = lambda: ta.Forest(nodes, T, D, cols, missing=MISSING, num_classes=C, contribs=True, approx_contribs=True)
        by_tree = nodes.reshape(T, per)
        sub = lambda c, n: np.ascontiguousarray(by_tree[c::C][:n]).reshape(-1)  # noqa: E731
        k.raw = np.stack([oracle.predict(sub(c, T // C), T // C, D, k.data, MISSING, threads=8)[0] for c in range(C)], axis=1)
        k.leaf = oracle.predict(nodes, T, D, k.data, MISSING, want_leaf=True, threads=8)[1]
        if C == 1:
            k.cont = lambda start: oracle.predict_continue(nodes, T, D, k.data, MISSING, start.copy(), threads=8)
        k.stages = {"a": [1, 5, T // C], "b": [2, T // C]}
        k.staged = {key: np.stack([np.stack([oracle.predict(sub(c, n), n, D, k.data, MISSING, threads=8)[0] for c in range(C)], axis=1)
                                   for n in rounds], axis=1) for key, rounds in k.stages.items()}
        k.missing = MISSING
    elif kind in ("sparse", "categorical"):
        cat = kind == "categorical"
        fo = pd_cases.random_forest(seed=13 if cat else 11, num_trees=8 if cat else 12, num_cols=8, max_depth=7 if cat else 9,
                                    leaf_prob=0.2 if cat else 0.25, cat_features=(1, 6) if cat else ())
        C, cols, R = 1, fo["num_cols"], 300
        T = fo["trees"].size
        k.missing = fo["missing"]
        k.data = np.ascontiguousarray(pd_cases.random_grid(fo, list(range(cols)), R, seed=41))
        k.make = lambda: ta.capi.SparseForest(fo["nodes"], fo["trees"], cols, missing=fo["missing"], covers=fo["covers"],
                                              contribs=True, approx_contribs=True, categories=fo["categories"],
                                              members_left=fo["members_left"], partial_dependence=True)
        cats = fo["cats"] if cat else ()
        ref = lambda trees, init=None: categorical_ref.predict(fo["nodes"], trees, k.data, fo["missing"], *cats, init=init)  # noqa: E731
        k.raw, k.leaf = ref(fo["trees"])
        if not cat:  # the restatement is held to the oracle where the oracle has the rule
            want, leaf = oracle.sparse_predict(fo["nodes"], fo["trees"], k.data, fo["missing"], want_leaf=True)
            assert np.array_equal(bits(k.raw), bits(want)) and np.array_equal(k.leaf, leaf)
        k.raw = k.raw[:, None]
        k.cont = lambda start: ref(fo["trees"], init=start)[0]
        k.stages = {"a": [1, 4, T], "b": [3, T]}
        k.staged = {key: np.stack([ref(fo["trees"][:n])[0] for n in rounds], axis=1) for key, rounds in k.stages.items()}
        feats = [0, 5]
        grid = np.ascontiguousarray(k.data[:, feats])
        k.pd = (feats, grid, pd_ref.pd_f32(fo["nodes"], fo["trees"], fo["covers"], feats, grid, fo["missing"], 1, fo["cats"]))
    elif kind == "oblivious":
        depths, cols, C = [6, 2, 1, 0, 1, 6, 2, 1, 0], 8, 1
        forest = obr.make_forest(depths, cols, C, seed=51)
        covers = np.random.default_rng(52).uniform(0.5, 50.0, int((1 << np.asarray(depths)).sum())).astype(np.float32)
        k.missing = obr.MISSING
        k.data = obr.make_data(200, cols, seed=53)
        k.make = lambda: ta.ObliviousForest(forest["depths"], forest["fids"], forest["thr"], forest["def_left"], forest["leaves"], cols,
                                            leaf_dim=C, missing=obr.MISSING, leaf_covers=covers, contribs=True, approx_contribs=True,
                                            interactions=True, interventional=True, staged=True)
        k.raw, k.leaf = obr.ref_of(forest, k.data)
        k.cont = lambda start: obr.ref_of(forest, k.data, init=start)[0][:, 0]
        run = sng.running_sums(sng.oblivious_leaf_vectors(forest, k.leaf))
        k.stages = {"a": [1, 4, 9], "b": [5, 9]}
        k.staged = {key: staged_of(run, rounds, C) for key, rounds in k.stages.items()}
    else:
        forest, data, covers = vsr.case("five_k9")
        C, cols = forest["k"], forest["cols"]
        k.missing = vr.MISSING
        k.data = np.ascontiguousarray(data)
        k.make = lambda: ta.VectorForest(forest["nodes"], forest["trees"], forest["leaves"], cols, missing=vr.MISSING,
                                         covers=covers["consistent"], contribs=True, interventional=True, interactions=True,
                                         approx_contribs=True, staged=True)
        k.raw, k.leaf, _ = vr.vector_ref(forest, k.data)
        run = sng.running_sums(sng.vector_leaf_vectors(forest, k.leaf))
        k.stages = {"a": [1, 3, 5], "b": [2, 5]}
        k.staged = {key: staged_of(run, rounds, C) for key, rounds in k.stages.items()}
    k.data = np.array(k.data, dtype=np.float32, order="C")
    k.staged = {key: np.ascontiguousarray(w[:, :, 0] if C == 1 and w.ndim == 3 else w) for key, w in k.staged.items()}
    k.C, k.cols, k.large = C, cols, k.data.shape[0]
    k.leaf = np.ascontiguousarray(k.leaf).view(np.uint32)
    k.raw = np.ascontiguousarray(k.raw[:, 0] if C == 1 else k.raw, dtype=np.float32)
    rng = np.random.default_rng(61)
    k.bg = {"a": np.ascontiguousarray(k.data[rng.choice(k.large, 9, replace=False)]),
            "b": np.ascontiguousarray(k.data[rng.choice(k.large, 20, replace=False)])}
    k.start = rng.uniform(-2.0, 2.0, k.large).astype(np.float32)
    return k


def accepted(ta, f):
    ok = []
    for name in ("DIRECT", "ROWTILE", "TILEBLOCK", "TILERING", "QRING", "AUTO"):
        try:
            f.set_strategy(getattr(ta, "STRATEGY_" + name))
            ok.append(name)
        except ta.TahoeError as e:
            assert e.status == 7, str(e)
    return ok


def fresh_bits(env, k, cache, name, bg):
    """What `name` gives, at the large row count, on a fresh handle that has made no other call (but set_background, where the
    call needs one)."""
    ta, oracle, torch = env
    key = (name, bg)
    if key not in cache:
        f = k.make()
        if name == "predict_contribs_interventional":
            f.set_background(torch.from_numpy(k.bg[bg]).cuda())
        out = getattr(f, name)(torch.from_numpy(k.data).cuda())
        f.check()
        cache[key] = out.cpu().numpy()
        f.close()
    return cache[key]


@pytest.mark.parametrize("kind", list(SERVES))
def test_call_history(env, kind):
    ta, oracle, torch = env
    k = build(kind, env)
    f = k.make()
    C, T = k.C, f.num_trees
    assert f.num_classes == C
    strategies = accepted(ta, f)
    assert "DIRECT" in strategies and len(strategies) >= 3, strategies
    f.set_stages(k.stages["a"])  # once ...
    staged_strategies = []  # the strategies that have a staged form on this handle (QRING and TILERING have none)
    for s in strategies:
        f.set_strategy(getattr(ta, "STRATEGY_" + s))
        if s != "AUTO" and f.staged_strategy(k.large) == getattr(ta, "STRATEGY_" + s):
            staged_strategies.append(s)
    assert "DIRECT" in staged_strategies and "ROWTILE" in staged_strategies, staged_strategies
    f.set_background(torch.from_numpy(k.bg["a"]).cuda())  # ... and once
    state = {"bg": "a", "stages": "a"}
    cache, step, done = {}, 0, []
    keep = []
    shape = lambda R, *tail: (R,) + ((C,) if C > 1 else ()) + tail  # noqa: E731
    for lap in (1, 2):
        for op, arg in SEQUENCE:
            if op not in SERVES[kind]:
                continue
            step += 1
            pool = staged_strategies if op == "predict_staged" else strategies
            sname = pool[step % len(pool)]
            strategy = getattr(ta, "STRATEGY_" + sname)
            R = k.large if arg == LARGE else arg
            tag = f"{kind}, lap {lap}, step {step}: {op}({arg}) under {sname}"
            done.append(op)
            if op == "check":
                f.check()
                continue
            if op == "set_stages":
                f.set_stages(k.stages[arg])
                state["stages"] = arg
                continue
            if op == "reserve_csr":
                f.reserve_csr(2 * k.large, 2 * k.large * k.cols)
                f.check()
                continue
            f.set_strategy(strategy)
            if op == "set_background":
                before = f.get_strategy(k.large)
                g = guarded_input(torch, k.bg[arg], torch.float32, device="cuda")
                f.set_background(g.view)
                g.check_unchanged("background: " + tag)
                keep.append(g)
                assert f.get_strategy(k.large) == before, tag  # predicted as DIRECT, strategy restored
                state["bg"] = arg
                continue
            if op == "predict_host":
                src = guarded_input(np, k.data[:R], np.float32)
                out = Guarded(np, (R,), np.float32)
                f.predict_host(src.view, preds=out.view, chunk_rows=128)
                f.check()
                assert np.array_equal(bits(out.check(tag)), bits(k.raw[:R])), tag
                src.check_unchanged("data: " + tag)
                continue
            if op == "partial_dependence":
                feats, grid, want = k.pd
                gg = guarded_input(torch, grid[:R], torch.float32, device="cuda")
                out = Guarded(torch, shape(R), torch.float32, device="cuda")
                f.partial_dependence(feats, gg.view, out=out.view)
                f.check()
                assert np.array_equal(bits(out.check(tag).reshape(R, -1)), bits(np.ascontiguousarray(want[:R], np.float32))), tag
                gg.check_unchanged("grid: " + tag)
                continue
            if op in ("predict_csr", "predict_csr_chunked"):
                indptr, indices, values = ta.dense_to_csr(k.data[:R], k.missing)
                if op == "predict_csr_chunked":
                    f.set_strategy(ta.STRATEGY_DIRECT)
                    assert f.csr_plan(R, values.size)[0] == ("direct" if "dense" in kind else "sparse_direct"), tag
                    assert f.csr_plan(R, values.size)[1] > 0, tag  # rows per densified chunk: not a fused form
                    bytes_before = f.info().device_bytes
                ip = guarded_input(torch, indptr, torch.int64, device="cuda")
                ix = guarded_input(torch, indices, torch.int32, device="cuda")
                vals = guarded_input(torch, values, torch.float32, device="cuda")
                out = Guarded(torch, shape(R), torch.float32, device="cuda")
                f.predict_csr(ip.view, ix.view, vals.view, out=out.view)
                f.check()
                assert np.array_equal(bits(out.check(tag)), bits(k.raw[:R])), tag
                for gd, what in ((ip, "indptr"), (ix, "indices"), (vals, "values")):
                    gd.check_unchanged(f"{what}: {tag}")
                if op == "predict_csr_chunked" and lap == 1 and R == 65:
                    assert f.info().device_bytes >= bytes_before + 64 * k.cols * 4, tag  # the chunk buffer: 1 row -> 65 rows
                continue
            x = guarded_input(torch, k.data[:R], torch.float32, device="cuda")
            if op in ("predict", "predict_raw"):
                out = Guarded(torch, shape(R), torch.float32, device="cuda")
                getattr(f, op)(x.view, out.view)
                f.check()
                assert np.array_equal(bits(out.check(tag)), bits(k.raw[:R])), tag  # (the handle has no epilogue: predict is raw)
            elif op == "predict_leaf_idx":
                leaf = Guarded(torch, (R, T), torch.int32, device="cuda")
                sums = Guarded(torch, shape(R), torch.float32, device="cuda")
                f.predict_leaf_idx(x.view, leaf=leaf.view, sums=sums.view)
                f.check()
                assert np.array_equal(bits(leaf.check(tag)), k.leaf[:R]), tag
                assert np.array_equal(bits(sums.check(tag)), bits(k.raw[:R])), tag
            elif op == "predict_accumulate":
                acc = Guarded(torch, (R,), torch.float32, device="cuda").load(k.start[:R])
                f.predict_accumulate(x.view, acc.view)
                f.check()
                cont = cache.setdefault("cont", None)
                if cont is None:
                    cont = cache["cont"] = k.cont(k.start)
                assert np.array_equal(bits(acc.check(tag)), bits(cont[:R])), tag
            elif op == "predict_staged":
                assert f.staged_strategy(R) == strategy, tag
                want = k.staged[state["stages"]]
                out = Guarded(torch, (R,) + want.shape[1:], torch.float32, device="cuda")
                f.predict_staged(x.view, out=out.view)
                f.check()
                assert np.array_equal(bits(out.check(tag)), bits(want[:R])), tag
            else:
                want = fresh_bits(env, k, cache, op, state["bg"])
                out = Guarded(torch, shape(R, *((k.cols + 1,) * EXPLAIN[op])), torch.float32, device="cuda")
                getattr(f, op)(x.view, out=out.view)
                f.check()
                assert same_bits(out.check(tag), want[:R]), f"{tag}: not the bits of a fresh handle"
            x.check_unchanged("data: " + tag)
    f.close()
    assert set(done) == SERVES[kind], sorted(SERVES[kind] - set(done))  # the sequence reaches every entry point the kind serves
