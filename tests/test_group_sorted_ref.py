"""tests/group_sorted_ref.py held to hand-written cases whose answers are typed in: what the GPU tests compare the library
with must itself say what the header says."""
import math

import numpy as np
import pytest

import group_sorted_ref as R

T, F = True, False
i64 = lambda *v: np.array(v, dtype=np.int64)      # noqa: E731
f64 = lambda *v: np.array(v, dtype=np.float64)    # noqa: E731
ALL = ["count_distinct", "sum_distinct", "first", "last", ("first", 1), ("last", 1)]


def check(got, group_rows, count, total, first, last, first_nn, last_nn):
    rows, outs = got
    assert rows.dtype == np.uint32 and rows.tolist() == group_rows
    assert outs[0].dtype == np.int64 and outs[0].tolist() == count
    assert [repr(x) for x in outs[1].tolist()] == [repr(x) for x in total]          # repr: NaN equals NaN, -0.0 is not 0.0
    for out, want in zip(outs[2:], (first, last, first_nn, last_nn)):
        idx, valid = out
        assert idx.dtype == np.uint32 and valid.dtype == bool
        assert [int(i) if v else None for i, v in zip(idx, valid)] == want


def test_groups_come_in_key_order_with_the_null_key_last():
    key = (i64(5, 0, 5, 3, 0, 9), np.array([T, F, T, T, F, T]))                     # rows 1 and 4: NULL key
    val = (i64(7, 1, 7, 2, 4, -1),)
    check(R.group_sorted_ref([key], val, ALL), [3, 0, 5, 1], [1, 1, 1, 2], [2, 7, -1, 5],
          [3, 0, 5, 1], [3, 2, 5, 4], [3, 0, 5, 1], [3, 2, 5, 4])


def test_no_keys_is_one_group_and_no_rows_no_group():
    check(R.group_sorted_ref([], (i64(4, 4, 2),), ALL), [0], [2], [6], [0], [2], [0], [2])
    rows, outs = R.group_sorted_ref([(i64(),)], (i64(),), ALL)
    assert rows.shape == (0,) and outs[0].shape == (0,) and outs[2][0].shape == (0,)


def test_signed_zeros_are_one_value_and_nans_are_one_value():
    key = (i64(1, 1, 1, 2, 2, 2, 2),)
    nan2 = np.frombuffer(np.uint64(0xFFF8000000000123).tobytes(), dtype=np.float64)[0]
    val = (f64(-0.0, 0.0, 1.5, math.nan, nan2, 2.0, 2.0),)
    rows, outs = R.group_sorted_ref([key], val, ["count_distinct", "sum_distinct"])
    assert outs[0].tolist() == [2, 2]
    assert repr(float(outs[1][0])) == "1.5" and math.isnan(outs[1][1])
    rows, outs = R.group_sorted_ref([], (f64(-0.0, -0.0),), ["count_distinct", "sum_distinct"])
    assert outs[0].tolist() == [1] and repr(float(outs[1][0])) == "0.0"             # -0.0 counts once, as +0.0


def test_float_keys_are_canonical_too():
    key = (f64(-0.0, math.nan, 0.0, -math.nan, math.inf, 1.0),)
    rows, outs = R.group_sorted_ref([key], (i64(1, 2, 3, 4, 5, 6),), ["sum_distinct"])
    assert rows.tolist() == [0, 5, 4, 1]                                            # 0, 1, inf, NaN
    assert outs[0].tolist() == [4, 6, 5, 6]


def test_infinities_follow_ieee():
    key = (i64(0, 0, 1, 1, 2, 2),)
    val = (f64(math.inf, 1.0, math.inf, -math.inf, -math.inf, -math.inf),)
    _, outs = R.group_sorted_ref([key], val, ["sum_distinct", "count_distinct"])
    assert outs[0][0] == math.inf and math.isnan(outs[0][1]) and outs[0][2] == -math.inf
    assert outs[1].tolist() == [2, 2, 1]


def test_an_all_null_group_counts_zero_sums_zero_and_has_no_first_non_null():
    key = (i64(1, 2, 2, 1),)
    val = (i64(9, 3, 3, 9), np.array([F, T, T, F]))
    check(R.group_sorted_ref([key], val, ALL), [0, 1], [0, 1], [0, 3], [0, 1], [3, 2], [None, 1], [None, 2])


def test_ignore_nulls_on_and_off():
    key = (i64(1, 1, 1, 1),)
    val = (f64(8.0, 2.0, 2.0, 5.0), np.array([F, T, T, F]))
    check(R.group_sorted_ref([key], val, ALL), [0], [1], [2.0], [0], [3], [1], [2])


def test_the_empty_string_is_a_value_and_null_is_not():
    key = ([b"k", b"k", b"k", b"", None, b"", None],)
    val = ([b"", None, b"", None, b"x", b"a", b"x\0"],)
    rows, outs = R.group_sorted_ref([key], val, ["count_distinct", "first", ("first", 1), ("last", 1)])
    assert rows.tolist() == [3, 0, 4]                                               # "" < "k" < NULL
    assert outs[0].tolist() == [1, 1, 2]
    assert outs[1][0].tolist() == [3, 0, 4] and outs[1][1].all()
    assert outs[2][0].tolist() == [5, 0, 4] and outs[3][0].tolist() == [5, 2, 6]
    with pytest.raises(ValueError):
        R.group_sorted_ref([key], val, ["sum_distinct"])


def test_unsigned_sums_wrap_mod_2_64():
    val = (np.array([2**64 - 1, 2, 2**64 - 1, 2**63], dtype=np.uint64),)
    _, outs = R.group_sorted_ref([], val, ["sum_distinct"])
    assert outs[0].dtype == np.int64 and outs[0].tolist() == [-(2**63) + 1]         # 2^64 - 1 + 2 + 2^63 mod 2^64 = 2^63 + 1
    _, outs = R.group_sorted_ref([], (np.array([-128, 127, -128], dtype=np.int8),), ["sum_distinct"])
    assert outs[0].tolist() == [-1]


def test_float_sums_are_exact_and_float32_is_widened():
    _, outs, terms = R.group_sorted_ref([], (f64(1e16, -1e16, 1.0, 1.0),), ["sum_distinct"], with_terms=True)
    assert outs[0].tolist() == [1.0] and terms["m"].tolist() == [3] and terms["sum_abs"].tolist() == [2e16 + 1.0]
    _, outs = R.group_sorted_ref([], (np.array([16777216.0, 1.0, 1.0, 2.0], dtype=np.float32),), ["sum_distinct"])
    assert outs[0].dtype == np.float64 and outs[0].tolist() == [16777219.0]         # not representable in Float32


def test_several_keys_and_mixed_types():
    k0 = (np.array([1, 1, 2, 2, 1], dtype=np.int32), np.array([T, T, T, F, T]))
    k1 = ([b"b", b"a", b"a", b"a", b"b"],)
    val = (i64(10, 20, 30, 40, 11),)
    check(R.group_sorted_ref([k0, k1], val, ALL), [1, 0, 2, 3], [1, 2, 1, 1], [20, 21, 30, 40],
          [1, 0, 2, 3], [1, 4, 2, 3], [1, 0, 2, 3], [1, 4, 2, 3])


def test_no_calls_returns_the_distinct_key_tuples():
    rows, outs = R.group_sorted_ref([(i64(3, 1, 3, 2, 1),)], None, [])
    assert rows.tolist() == [1, 3, 0] and outs == []
