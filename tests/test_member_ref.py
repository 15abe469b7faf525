"""tests/member_ref.py, the model the GPU tests of rdf_member_mask / rdf_first_occurrence compare against, held to typed-in
SQL answers and — where pyarrow is installed — to pyarrow on the inputs where the two rules agree."""
import numpy as np
import pytest

import member_ref as R

NAN = float("nan")


def test_is_in_is_sql_three_valued():
    assert R.member_mask([1], [2, None], R.IS_IN) == [None]            # 1 IN (2, NULL) is NULL
    assert R.member_mask([2], [2, None], R.IS_IN) == [True]            # a match wins over the NULL
    assert R.member_mask([None], [], R.IS_IN) == [False]               # NULL IN () is FALSE
    assert R.member_mask([None, 1], [1], R.IS_IN) == [None, True]
    assert R.member_mask([3, 1], [1, 2], R.IS_IN) == [False, True]
    assert R.member_mask([None], [None], R.IS_IN) == [None]            # NULL never equals NULL
    assert R.true_rows([True, None, False, True]) == 2


def test_semi_and_anti():
    left = [1, None, 2, 2, 3]
    assert R.member_mask(left, [2, 2, None, 9], R.SEMI) == [False, False, True, True, False]
    assert R.member_mask(left, [2, 2, None, 9], R.ANTI) == [True, True, False, False, True]     # ANTI keeps NULL rows
    assert R.member_mask(left, [], R.SEMI) == [False] * 5 and R.member_mask(left, [], R.ANTI) == [True] * 5
    # tuples: a NULL in any component never matches, on either side
    l2 = [(1, b"a"), (1, None), (2, b"a"), (1, b"")]
    r2 = [(1, b"a"), (None, b"a"), (1, None), (1, b"")]
    assert R.member_mask(l2, r2, R.SEMI) == [True, False, False, True]
    assert R.member_mask(l2, r2, R.ANTI) == [False, True, True, False]


def test_float_keys_follow_spark():
    assert R.member_mask([-0.0, 0.0, NAN, 1.5], [0.0, -NAN], R.SEMI) == [True, True, True, False]
    assert R.first_occurrence([0.0, -0.0, NAN, -NAN, 1.0], R.FIRST) == [True, False, True, False, True]


def test_first_occurrence_keeps():
    assert R.first_occurrence([1, 1, 2], R.FIRST) == [True, False, True]
    assert R.first_occurrence([1, 1, 2], R.LAST) == [False, True, True]
    assert R.first_occurrence([1, 1, 2], R.NONE) == [False, False, True]           # pandas keep=False
    # NULL is a key value of its own, component-wise
    rows = [(None, None), (None, 1), (1, None), (None, None), (1, None)]
    assert R.first_occurrence(rows, R.FIRST) == [True, True, True, False, False]
    assert R.first_occurrence(rows, R.LAST) == [False, True, False, True, True]
    assert R.first_occurrence(rows, R.NONE) == [False, True, False, False, False]
    assert R.first_occurrence([b"", None, b"", None], R.FIRST) == [True, True, False, False]   # "" is a value, not NULL
    assert R.first_occurrence([], R.FIRST) == []


def test_model_agrees_with_pyarrow():
    pa = pytest.importorskip("pyarrow")
    pc = pytest.importorskip("pyarrow.compute")
    rng = np.random.default_rng(5)
    for _ in range(20):
        left = [None if rng.random() < 0.2 else int(v) for v in rng.integers(0, 12, size=40)]
        right = [int(v) for v in rng.integers(0, 12, size=int(rng.integers(0, 8)))]     # (no NULL on the right: there the rules differ)
        got = pc.is_in(pa.array(left, type=pa.int64()), value_set=pa.array(right, type=pa.int64())).to_pylist()
        assert got == R.member_mask(left, right, R.SEMI)                # arrow's is_in answers FALSE for a NULL row: SEMI
        lt = pa.table({"k": pa.array(left, type=pa.int64()), "i": pa.array(range(len(left)))})
        rt = pa.table({"k": pa.array(right, type=pa.int64())})
        semi = sorted(lt.join(rt, "k", join_type="left semi")["i"].to_pylist())
        anti = sorted(lt.join(rt, "k", join_type="left anti")["i"].to_pylist())
        assert semi == [i for i, b in enumerate(R.member_mask(left, right, R.SEMI)) if b]
        assert anti == [i for i, b in enumerate(R.member_mask(left, right, R.ANTI)) if b]
