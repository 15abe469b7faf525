"""tests/select_ref.py, the model of the conditional and NULL functions, held to pyarrow where the two agree and to Spark's
documented answers where they do not:

    pyarrow   pc.coalesce, pc.case_when (a NULL condition falls through to the next branch), pc.is_null; pc.is_nan on the
              rows that are not NULL (pyarrow gives NULL there, Spark false); pc.max_element_wise / pc.min_element_wise on
              inputs without NaN (pyarrow ignores NaN, Spark ranks it above every number)
    Spark     greatest(10, 9, 2, 4, 3) = 10, least(10, 9, 2, 4, 3) = 2, coalesce(NULL, 1, NULL) = 1, nanvl(NaN, 123) = 123.0
    by hand   ties return the leftmost part's bits, NaN is the greatest value, -0.0 == 0.0, the extremes of every dtype
              (Int64 min / max, UInt64 above 2^63: a signed comparison would fail there), +-inf, two NaNs of different payloads"""
import numpy as np
import pytest

import select_ref as R

try:                                      # the hand cases and Spark's answers below need no pyarrow: only the comparisons are skipped without it
    import pyarrow as pa
    import pyarrow.compute as pc
except ImportError:
    pa = pc = None
needs_pyarrow = pytest.mark.skipif(pa is None, reason="pyarrow is not installed")

N = 4000


def arrow(v, m):
    return pa.array(v, mask=~m)


def back(a, dtype):
    m = ~np.asarray(a.is_null())
    return np.where(m, a.fill_null(0).to_numpy(zero_copy_only=False), 0).astype(dtype), m


def same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(R.bits_of(got[0]), R.bits_of(want[0]))


def columns(name, k, rng, nan=True):
    out = []
    for _ in range(k):
        v = R.random_values(name, N, rng)
        if not nan and v.dtype.kind == "f":
            v = np.where(np.isnan(v), np.float64(7.5).astype(v.dtype), v)
        out.append((v, rng.uniform(size=N) > 0.4))
    return out


@needs_pyarrow
@pytest.mark.parametrize("name", list(R.DTYPES))
def test_coalesce_is_pyarrows(name):
    rng = np.random.default_rng(1)
    for k in (1, 2, 3, 8):
        parts = columns(name, k, rng, nan=False)       # (bits are compared, and pyarrow promises nothing about a NaN's payload: those are checked by hand below)
        same(R.coalesce(parts, R.DTYPES[name]), back(pc.coalesce(*[arrow(v, m) for v, m in parts]), R.DTYPES[name]))
    parts = columns(name, 2, rng, nan=False)
    lit = 3
    got = R.coalesce([parts[0], None, lit, parts[1]], R.DTYPES[name])
    want = pc.coalesce(arrow(*parts[0]), pa.scalar(None, type=pa.from_numpy_dtype(R.DTYPES[name])), pa.scalar(lit, type=pa.from_numpy_dtype(R.DTYPES[name])), arrow(*parts[1]))
    same(got, back(want, R.DTYPES[name]))
    assert got[1].all()


@needs_pyarrow
@pytest.mark.parametrize("name", list(R.DTYPES))
def test_case_when_is_pyarrows_and_a_null_condition_falls_through(name):
    rng = np.random.default_rng(2)
    dt = R.DTYPES[name]
    for nb in (1, 2, 3, 8):
        conds = [(rng.uniform(size=N) > 0.7, rng.uniform(size=N) > 0.3) for _ in range(nb)]
        parts = columns(name, nb + 1, rng, nan=False)
        struct = pa.StructArray.from_arrays([arrow(c, m) for c, m in conds], names=[f"c{i}" for i in range(nb)])
        same(R.case_when(conds, parts[:-1], parts[-1], dt), back(pc.case_when(struct, *[arrow(v, m) for v, m in parts]), dt))
        same(R.case_when(conds, parts[:-1], None, dt), back(pc.case_when(struct, *[arrow(v, m) for v, m in parts[:-1]]), dt))
    # one row: the first condition is NULL, the second true
    got = R.case_when([(np.array([True]), np.array([False])), (np.array([True]), None)], [np.array([1], dtype=dt).item(), np.array([2], dtype=dt).item()], 9, dt)
    assert got[0][0] == 2 and got[1][0]
    # overlapping true conditions: the first wins; all false takes otherwise; no otherwise is NULL
    t, f = (np.array([True]), None), (np.array([False]), None)
    assert R.case_when([t, t], [4, 5], 6, dt)[0][0] == 4
    assert R.case_when([f, f], [4, 5], 6, dt)[0][0] == 6
    assert not R.case_when([f, f], [4, 5], None, dt)[1][0]


@needs_pyarrow
@pytest.mark.parametrize("name", list(R.DTYPES))
def test_null_tests_are_pyarrows(name):
    rng = np.random.default_rng(3)
    (v, m), = columns(name, 1, rng)
    a = arrow(v, m)
    assert np.array_equal(R.null_test(R.IS_NULL, v, m), np.asarray(pc.is_null(a)))
    assert np.array_equal(R.null_test(R.IS_NOT_NULL, v, m), np.asarray(pc.is_valid(a)))
    assert np.array_equal(R.null_test(R.IS_NULL, v, None), np.zeros(N, dtype=bool))
    if name in R.FLOATS:
        got = R.null_test(R.IS_NAN, v, m)
        want = pc.is_nan(a)
        assert np.array_equal(got[m], np.asarray(want.filter(pa.array(m))))
        assert not got[~m].any() and want.null_count == int((~m).sum())           # isnan(NULL): Spark false, pyarrow NULL
        assert got.any()


@needs_pyarrow
@pytest.mark.parametrize("name", list(R.DTYPES))
def test_extremum_without_nan_is_pyarrows_element_wise(name):
    rng = np.random.default_rng(4)
    dt = R.DTYPES[name]
    for k in (2, 3, 8):
        parts = columns(name, k, rng, nan=False)
        cols = [arrow(v, m) for v, m in parts]
        for greatest, fn in ((True, pc.max_element_wise), (False, pc.min_element_wise)):
            got, want = R.extremum(greatest, parts, dt), back(fn(*cols, skip_nulls=True), dt)
            assert np.array_equal(got[1], want[1])
            assert np.array_equal(got[0], want[0])             # by value: of -0.0 and 0.0 pyarrow may return either


def test_sparks_documented_answers():
    col = lambda x, dt=np.int32: (np.array([x], dtype=dt), None)
    five = [col(10), col(9), col(2), col(4), col(3)]
    assert R.extremum(True, five, np.int32)[0][0] == 10
    assert R.extremum(False, five, np.int32)[0][0] == 2
    got = R.coalesce([(np.array([0], dtype=np.int32), np.array([False])), 1, None], np.int32)
    assert got[0][0] == 1 and got[1][0]
    got = R.nanvl((np.array([np.nan]), None), 123.0, np.float64)
    assert got[0][0] == 123.0 and got[1][0]


def f64(*bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


def test_ties_nan_and_signed_zero_by_hand():
    one = lambda v: (np.array([v]) if not isinstance(v, np.ndarray) else v, None)
    nan_a, nan_b = f64(0x7FF8000000000001), f64(0xFFF8000000000002)
    bits = lambda r: int(R.bits_of(r[0])[0])
    # greatest(NaN, 1) = NaN, least(NaN, 1) = 1; NaN above +inf
    assert bits(R.extremum(True, [one(nan_a), one(1.0)], np.float64)) == 0x7FF8000000000001
    assert R.extremum(False, [one(nan_a), one(1.0)], np.float64)[0][0] == 1.0
    assert bits(R.extremum(True, [one(np.inf), one(nan_a)], np.float64)) == 0x7FF8000000000001
    assert R.extremum(False, [one(nan_a), one(-np.inf)], np.float64)[0][0] == -np.inf
    # two NaNs are equal: the leftmost one's payload comes back, from greatest and from least
    for g in (True, False):
        assert bits(R.extremum(g, [one(nan_a), one(nan_b)], np.float64)) == 0x7FF8000000000001
        assert bits(R.extremum(g, [one(nan_b), one(nan_a)], np.float64)) == 0xFFF8000000000002
    # -0.0 == 0.0: the leftmost
    for g in (True, False):
        assert bits(R.extremum(g, [one(-0.0), one(0.0)], np.float64)) == 0x8000000000000000
        assert bits(R.extremum(g, [one(0.0), one(-0.0)], np.float64)) == 0
    # a NULL part is skipped wherever it stands; all NULL is NULL
    null = (np.array([5.0]), np.array([False]))
    assert R.extremum(True, [null, one(1.0), null], np.float64)[0][0] == 1.0
    assert not R.extremum(True, [null, None], np.float64)[1][0]
    # coalesce and nanvl keep bits
    assert bits(R.coalesce([null, one(nan_b)], np.float64)) == 0xFFF8000000000002
    assert bits(R.coalesce([one(-0.0), one(1.0)], np.float64)) == 0x8000000000000000
    assert bits(R.nanvl(one(nan_a), one(nan_b), np.float64)) == 0xFFF8000000000002
    assert bits(R.nanvl(one(-0.0), one(1.0), np.float64)) == 0x8000000000000000
    assert not R.nanvl(null, one(1.0), np.float64)[1][0]
    assert not R.nanvl(one(nan_a), null, np.float64)[1][0]
    assert R.nanvl(one(2.0), null, np.float64)[1][0]


def test_the_extremes_of_every_dtype():
    for name, dt in R.DTYPES.items():
        e = R.edge_values(name)
        if np.dtype(dt).kind == "f":
            continue
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
        parts = [(np.array([x], dtype=dt), None) for x in e]
        assert R.extremum(True, parts, dt)[0][0] == hi and R.extremum(False, parts, dt)[0][0] == lo
        assert R.extremum(True, parts[::-1], dt)[0][0] == hi and R.extremum(False, parts[::-1], dt)[0][0] == lo
    # UInt64 above 2^63 is greater than 1 (it is negative as Int64)
    big = (np.array([2**63 + 5], dtype=np.uint64), None)
    assert R.extremum(True, [(np.array([1], dtype=np.uint64), None), big], np.uint64)[0][0] == 2**63 + 5
    assert R.extremum(False, [big, (np.array([1], dtype=np.uint64), None)], np.uint64)[0][0] == 1
    assert R.extremum(True, [(np.array([np.iinfo(np.int64).min]), None), (np.array([np.iinfo(np.int64).max]), None)], np.int64)[0][0] == np.iinfo(np.int64).max
    for dt in (np.float32, np.float64):
        inf = [(np.array([np.inf], dtype=dt), None), (np.array([-np.inf], dtype=dt), None), (np.array([np.finfo(dt).max], dtype=dt), None)]
        assert R.extremum(True, inf, dt)[0][0] == np.inf and R.extremum(False, inf, dt)[0][0] == -np.inf


@needs_pyarrow
def test_the_utf8_model_is_pyarrows():
    rng = np.random.default_rng(5)
    words = [b"", b"a", b"x" * 15, b"y" * 16, b"z" * 17, "grüß".encode()]
    cols = [[None if rng.uniform() < 0.4 else words[rng.integers(len(words))] for _ in range(500)] for _ in range(3)]
    arr = [pa.array(c, type=pa.binary()) for c in cols]
    assert R.utf8_coalesce(cols) == pc.coalesce(*arr).to_pylist()
    assert R.utf8_coalesce([cols[0], b"unknown"]) == pc.coalesce(arr[0], pa.scalar(b"unknown", type=pa.binary())).to_pylist()
    assert R.utf8_coalesce([cols[0], None]) == cols[0]
    conds = [(rng.uniform(size=500) > 0.6, rng.uniform(size=500) > 0.3) for _ in range(2)]
    struct = pa.StructArray.from_arrays([arrow(c, m) for c, m in conds], names=["a", "b"])
    assert R.utf8_case_when(conds, cols[:2], cols[2]) == pc.case_when(struct, *arr).to_pylist()
    assert R.utf8_case_when(conds, [b"low", cols[1]], None) == pc.case_when(struct, pa.scalar(b"low", type=pa.binary()), arr[1]).to_pylist()
