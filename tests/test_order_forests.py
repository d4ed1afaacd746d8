"""The closed form of tests/order_forests.py against the CPU oracle, bit for bit, on every forest and row set that
tests/test_rank_exact_gpu.py judges a kernel by (at reduced row counts).  A case that disagrees here is a bug in the helper."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import order_forests as O  # noqa: E402
from oracle import oracle  # noqa: E402

CPU_ROWS = 3000


@pytest.fixture(scope="module")
def ta(built):
    import tahoe_amd

    return tahoe_amd


DENSE_CASES = (
    [(f"quantiser-{c}-{d}", O.quantiser_case, (c, d)) for c in (32, 8, 6, 7) for d in (7, 10)]
    + [(f"u8-limit-{e}", O.u8_limit_case, (e,)) for e in (0, 1)]
    + [(f"table-{n}", O.table_size_case, (n,)) for n in O.TABLE_SIZES]
    + [(f"large-{k}", O.large_case, (k,)) for k in ("pair", "together", "single", "groups")]
    + [(f"bucket-{k}", O.bucket_case, (k,)) for k in O.BUCKET_KINDS]
    + [(f"levels-{c}-{d}", O.levels_case, (c, d)) for c in (256, 64) for d in O.LEVEL_DEPTHS]
    + [("slices", O.slices_case, ())]
    + [(f"wide-{c}-{d}", O.wide_case, (c, d)) for c in (700, 1200, 3072, 5000) for d in (9, 13)]
    + [(f"stream-{k}", O.stream_case, (k,)) for k in O.STREAM_KINDS]
    + [("multiclass", O.multiclass_case, ())]
)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def reduced(data, n_triples):
    idx = O.take_rows(data.shape[0], n_triples, CPU_ROWS)
    return np.ascontiguousarray(data[idx])


@pytest.mark.parametrize("name,build,args", DENSE_CASES, ids=[c[0] for c in DENSE_CASES])
def test_dense_closed_form_equals_the_oracle(ta, name, build, args):
    of, data, n_triples, missing = build(*args)
    x = reduced(data, n_triples)
    want, want_leaf = oracle.predict(of.nodes, of.T, of.D, x, missing, want_leaf=True)
    leaf = O.expected_leaf(of, x, missing)
    assert np.array_equal(leaf, want_leaf), O.first_mismatch(of, x, leaf, want_leaf)
    assert np.array_equal(bits(O.expected_sums(of, leaf)), bits(want))
    assert np.unique(leaf).size > 1  # the rows do not all end in one leaf
    band = O.in_band(x[:, [t[1] for t in of.trees]], missing)
    assert band.any() and not band.all(axis=1).all()


def test_multiclass_sums_are_per_class_sums_in_tree_order(ta):
    of, data, n_triples, missing = O.multiclass_case()
    x = reduced(data, n_triples)
    leaf = O.expected_leaf(of, x, missing)
    got = O.expected_sums(of, leaf, num_classes=3)
    per = ta.capi.tree_num_nodes(of.D)
    for c in range(3):
        nodes_c = np.concatenate([of.nodes[t * per:(t + 1) * per] for t in range(c, of.T, 3)])
        want, _ = oracle.predict(nodes_c, len(range(c, of.T, 3)), of.D, x, missing)
        assert np.array_equal(bits(got[:, c]), bits(want)), c


SPARSE_DENSE = [("quantiser-6-10", O.quantiser_case, (6, 10)), ("quantiser-32-7", O.quantiser_case, (32, 7)),
                ("levels-64-12", O.levels_case, (64, 12)), ("table-257", O.table_size_case, (257,))]


@pytest.mark.parametrize("name,build,args", SPARSE_DENSE, ids=[c[0] for c in SPARSE_DENSE])
def test_converted_forests_closed_form_equals_the_sparse_oracle(ta, name, build, args):
    of, data, n_triples, missing = build(*args)
    x = reduced(data, n_triples)
    sn, tr = ta.capi.dense_to_sparse(of.nodes, of.T, of.D)
    sf = O.sparse_from_dense(of, sn, tr)
    assert sf.nodes.tobytes() == sn.tobytes() and np.array_equal(sf.roots, tr)
    want, want_leaf = oracle.sparse_predict(sn, tr, x, missing, want_leaf=True)
    leaf = O.sparse_expected_leaf(sf, x, missing)
    assert np.array_equal(leaf, want_leaf), O.sparse_first_mismatch(sf, x, leaf, want_leaf)
    assert np.array_equal(bits(O.sparse_expected_sums(sf, leaf)), bits(want))
    assert np.array_equal(bits(want), bits(O.expected_sums(of, O.expected_leaf(of, x, missing))))  # and the dense closed form


@pytest.mark.parametrize("cols", [6, 255])
def test_irregular_closed_form_equals_the_sparse_oracle(ta, cols):
    sf, data, n_triples, missing = O.irregular_case(cols)
    x = reduced(data, n_triples)
    depth = []
    for part in sf._parts:  # the builder's shapes: unbalanced trees and vines, no deeper than 24
        d = {0: 0}
        for i in np.flatnonzero(part["bits"] >= 0):
            d[int(part["left_idx"][i])] = d[int(part["left_idx"][i]) + 1] = d[int(i)] + 1
        depth.append(max(d.values()))
    assert max(depth) == 24 and min(depth) == 1 and all(p.size <= 65535 for p in sf._parts), depth
    want, want_leaf = oracle.sparse_predict(sf.nodes, sf.roots, x, missing, want_leaf=True)
    leaf = O.sparse_expected_leaf(sf, x, missing)
    assert np.array_equal(leaf, want_leaf), O.sparse_first_mismatch(sf, x, leaf, want_leaf)
    assert np.array_equal(bits(O.sparse_expected_sums(sf, leaf)), bits(want))


def test_builder_layout_and_row_sets():
    """What the closed form rests on: the in-order layout, the padding, the three rows per threshold and the specials."""
    assert O.inorder_to_heap(3).tolist() == [3, 1, 5, 0, 2, 4, 6]
    assert O.pad_sorted([1.0, 2.0], 2).tolist() == [1.0, 2.0, np.inf] and O.pad_sorted([1.0, 2.0], 2, "repeat").tolist() == [1.0, 2.0, 2.0]
    thr = np.float32([-1.5, 0.0, 3.0])
    rows = O.critical_rows(thr, 3, 1, O.M_IN, n_random=10)
    col = rows[:, 1]
    assert (rows[:, 0] == O.BENIGN).all() and (rows[:, 2] == O.BENIGN).all()
    for t in thr:
        for v in (t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))):
            assert (bits(col) == bits(np.float32([v]))[0]).any(), v
    m = np.float32(O.M_IN)
    for v in (0.0, -0.0, np.inf, -np.inf, O.FLT_MAX, -O.FLT_MAX, O.DENORM_MIN, O.FLT_MIN, m, m + np.float32(5e-7), m - np.float32(1e-6),
              m + np.float32(2e-6), np.nextafter(m + np.float32(1e-6), np.float32(np.inf))):
        assert (bits(col) == bits(np.float32([v]))[0]).any(), v
    assert np.isnan(col).any()
    idx = O.take_rows(1000, 900, 513)
    assert idx.size == 513 and (idx[:449] < 900).all() and (idx[449:] >= 900).all()
