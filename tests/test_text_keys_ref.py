"""The pure-Python reference of the text-key tests (tests/text_keys_ref.py), pinned by cases written out by hand."""
from collections import Counter

import text_keys_ref as R


def test_factorize_first_occurrence_order():
    codes, dic = R.factorize([["b", None, "a", "b", ""]])
    assert codes == [[0, None, 1, 0, 2]]
    assert dic == ["b", "a", ""]


def test_factorize_runs_over_the_concatenation_of_the_chunks():
    codes, dic = R.factorize([["x"], [], [None, "y", "x"], ["y", "z"]])
    assert codes == [[0], [], [None, 1, 0], [1, 2]]
    assert dic == ["x", "y", "z"]
    assert R.factorize([]) == ([], [])
    assert R.factorize([[None, None]]) == ([[None, None]], [])


def test_nul_bytes_and_prefixes_are_distinct_values():
    codes, dic = R.factorize([[b"a", b"a\0", b"a\0b", b"a\0", b"a"]])
    assert codes == [[0, 1, 2, 1, 0]]
    assert dic == [b"a", b"a\0", b"a\0b"]


def test_groupby_sql_semantics():
    keys = [["x", None, "y", "x", None, "y"]]
    vals = [1, 2, None, 4, None, None]
    assert R.groupby(keys, vals, "sum") == {("x",): (5, 2), (None,): (2, 1), ("y",): (0, 0)}
    assert R.groupby(keys, vals, "min") == {("x",): (1, 2), (None,): (2, 1), ("y",): (None, 0)}
    assert R.groupby(keys, vals, "max") == {("x",): (4, 2), (None,): (2, 1), ("y",): (None, 0)}
    assert R.groupby(keys, vals, "count") == {("x",): (2, 2), (None,): (2, 2), ("y",): (2, 2)}
    assert R.groupby(keys, None, "sum") == R.groupby(keys, vals, "count")
    two = R.groupby([["a", "a", "b"], [1, None, 1]], [10, 20, 30], "sum")
    assert two == {("a", 1): (10, 1), ("a", None): (20, 1), ("b", 1): (30, 1)}


def test_full_join_with_null_keys_on_both_sides():
    left = [["a", None, "b", "a"]]
    right = [[None, "a", "c"]]
    assert R.equijoin(left, right, "full") == Counter({(0, 1): 1, (3, 1): 1, (1, None): 1, (2, None): 1, (None, 0): 1, (None, 2): 1})
    assert R.equijoin(left, right, "inner") == Counter({(0, 1): 1, (3, 1): 1})
    assert R.equijoin(left, right, "left") == Counter({(0, 1): 1, (3, 1): 1, (1, None): 1, (2, None): 1})
    assert R.equijoin(left, right, "right") == Counter({(0, 1): 1, (3, 1): 1, (None, 0): 1, (None, 2): 1})
    assert R.ordered_pairs(left, right, "left") == [(0, 1), (1, None), (2, None), (3, 1)]


def test_join_duplicates_multiply_and_two_column_keys():
    left = [["k", "k"], [1, 2]]
    right = [["k", "k", "k"], [1, 1, None]]
    assert R.equijoin(left, right, "inner") == Counter({(0, 0): 1, (0, 1): 1})
    assert R.ordered_pairs(left, right, "inner") == [(0, 0), (0, 1)]
    assert R.equijoin(left, right, "full") == Counter({(0, 0): 1, (0, 1): 1, (1, None): 1, (None, 2): 1})


def test_ordered_pairs_right_and_full():
    left = [["a", None, "b", "a"]]
    right = [[None, "a", "c", "a"]]
    assert R.ordered_pairs(left, right, "inner") == [(0, 1), (0, 3), (3, 1), (3, 3)]
    # RIGHT probes with the right rows: right rows ascending, their left partners ascending
    assert R.ordered_pairs(left, right, "right") == [(None, 0), (0, 1), (3, 1), (None, 2), (0, 3), (3, 3)]
    full = R.ordered_pairs(left, right, "full")
    assert full == [(0, 1), (0, 3), (1, None), (2, None), (3, 1), (3, 3), (None, 0), (None, 2)]
    assert R.full_probe_rows(left, right) == 6
    for how in ("inner", "left", "right", "full"):
        assert Counter(R.ordered_pairs(left, right, how)) == R.equijoin(left, right, how)
    R.assert_ordered(full[:6] + [(None, 2), (None, 0)], left, right, "full")      # the tail is a set
