"""tests/collect_ref.py held to values typed in by hand and, where pyarrow is importable, to pyarrow's hash_list /
hash_distinct and list_parent_indices / list_flatten on inputs without NULL and float-zero subtleties (pyarrow has its own
rules there; the header's are the hand-written cases)."""
import numpy as np
import pytest

import collect_ref as R

NAN = float("nan")


def lists_of(offsets, flat):
    return [list(flat[offsets[g]:offsets[g + 1]]) for g in range(len(offsets) - 1)]


def test_list_keeps_row_order_and_drops_nulls():
    k = np.array([2, 1, 2, 1, 2, 3], dtype=np.int32)
    v = np.array([10, 11, 12, 13, 14, 15], dtype=np.int64)
    ok = np.array([True, True, False, True, True, False])
    rows, offs, child, vals = R.collect_ref([(k,)], (v, ok), "list")
    assert rows.tolist() == [1, 0, 5]                     # groups 1, 2, 3 in key order: their first rows
    assert offs.tolist() == [0, 2, 4, 4]                  # key 3 has only a NULL value: an EMPTY list
    assert child.tolist() == [1, 3, 0, 4] and vals.tolist() == [11, 13, 10, 14]
    assert rows.dtype == np.uint32 and offs.dtype == np.int32 and child.dtype == np.uint32 and vals.dtype == np.int64


def test_set_sorts_values_and_points_at_the_smallest_row():
    k = np.array([1, 1, 1, 1, 0, 0], dtype=np.int64)
    v = np.array([5, 3, 5, 3, 9, 9], dtype=np.int16)
    rows, offs, child, vals = R.collect_ref([(k,)], (v,), "set")
    assert rows.tolist() == [4, 0] and offs.tolist() == [0, 1, 3]
    assert child.tolist() == [4, 1, 0] and vals.tolist() == [9, 3, 5]


def test_null_key_group_is_last_and_no_keys_is_one_group():
    k = np.array([7, 0, 7, 0], dtype=np.int64)
    kok = np.array([True, False, True, False])
    v = np.array([1.5, 2.5, 0.5, 2.5])
    rows, offs, child, vals = R.collect_ref([(k, kok)], (v,), "list")
    assert rows.tolist() == [0, 1] and offs.tolist() == [0, 2, 4] and child.tolist() == [0, 2, 1, 3]
    rows, offs, child, vals = R.collect_ref([], (v,), "set")
    assert rows.tolist() == [0] and offs.tolist() == [0, 3] and child.tolist() == [2, 0, 1] and vals.tolist() == [0.5, 1.5, 2.5]


def test_float_zeros_and_nans_are_one_value_each_and_come_out_canonical():
    other_nan = np.array([0x7FF0000000000001], dtype=np.uint64).view(np.float64)[0]
    v = np.array([NAN, -0.0, 1.0, 0.0, other_nan, np.inf, -np.inf])
    rows, offs, child, vals = R.collect_ref([], (v,), "set")
    assert offs.tolist() == [0, 5]
    assert child.tolist() == [6, 1, 2, 5, 0]              # -inf, zero (smallest row: the -0.0), 1, +inf, NaN (row 0) last
    assert vals.view(np.uint64).tolist() == [0xFFF0000000000000, 0, 0x3FF0000000000000, 0x7FF0000000000000, 0x7FF8000000000000]
    _, _, child, vals = R.collect_ref([], (v,), "list")   # list copies bits
    assert child.tolist() == list(range(7)) and vals.view(np.uint64).tolist() == v.view(np.uint64).tolist()
    f = np.array([-0.0, 0.0], dtype=np.float32)
    assert R.collect_ref([], (f,), "set")[3].view(np.uint32).tolist() == [0]


def test_utf8_values_compare_by_bytes_and_the_empty_string_is_a_value():
    k = np.array([0, 0, 0, 0, 0, 1], dtype=np.int8)
    v = [b"b", b"", None, b"a\0", b"a", None]
    rows, offs, child, vals = R.collect_ref([(k,)], (v,), "set")
    assert vals is None and rows.tolist() == [0, 5]
    assert offs.tolist() == [0, 4, 4] and child.tolist() == [1, 4, 3, 0]   # "" < "a" < "a\0" < "b"
    _, offs, child, _ = R.collect_ref([(k,)], (v,), "list")
    assert offs.tolist() == [0, 4, 4] and child.tolist() == [0, 1, 3, 4]


def test_zero_rows():
    rows, offs, child, vals = R.collect_ref([(np.zeros(0, dtype=np.int32),)], (np.zeros(0),), "set")
    assert len(rows) == len(offs) == len(child) == len(vals) == 0


def test_explode_by_hand():
    offs = [2, 4, 4, 7, 9]                                # rows: 2 elements, empty, 3 elements (NULL), 2 elements
    valid = np.array([True, True, False, True])
    p, c, pos, ev = R.explode_ref(offs, valid)
    assert p.tolist() == [0, 0, 3, 3] and c.tolist() == [2, 3, 7, 8] and pos.tolist() == [0, 1, 0, 1] and ev.all()
    p, c, pos, ev = R.explode_ref(offs, valid, outer=True)
    assert p.tolist() == [0, 0, 1, 2, 3, 3] and ev.tolist() == [True, True, False, False, True, True]
    assert c[ev].tolist() == [2, 3, 7, 8] and pos[ev].tolist() == [0, 1, 0, 1]
    assert len(R.explode_ref([0])[0]) == 0 and len(R.explode_ref([5, 5, 5])[0]) == 0
    assert R.explode_ref([5, 5, 5], outer=True)[0].tolist() == [0, 1]


def test_against_pyarrow():
    pa = pytest.importorskip("pyarrow")
    import pyarrow.compute as pc
    rng = np.random.default_rng(5)
    n = 500
    k = rng.integers(0, 17, n).astype(np.int32)
    v = rng.integers(-9, 9, n).astype(np.int64)
    t = pa.table({"k": k, "v": v})
    by_list = {r["k"]: r["v_list"] for r in t.group_by("k", use_threads=False).aggregate([("v", "list")]).to_pylist()}
    by_set = {r["k"]: sorted(r["v_distinct"]) for r in t.group_by("k").aggregate([("v", "distinct")]).to_pylist()}
    for kind, exp in (("list", by_list), ("set", by_set)):
        rows, offs, child, vals = R.collect_ref([(k,)], (v,), kind)
        assert [int(k[r]) for r in rows] == sorted(exp)
        assert lists_of(offs, vals.tolist()) == [exp[key] for key in sorted(exp)]
        assert np.array_equal(v[child], vals)
    lens = rng.integers(0, 5, 60)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    arr = pa.ListArray.from_arrays(pa.array(offs), pa.array(np.arange(offs[-1], dtype=np.int64) * 3))
    p, c, pos, ev = R.explode_ref(offs)
    assert pc.list_parent_indices(arr).to_pylist() == p.tolist()
    assert pc.list_flatten(arr).to_pylist() == (c.astype(np.int64) * 3).tolist()
