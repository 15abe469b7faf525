"""tests/percentile_ref.py — the executable definition of rdf_groupby_percentile — held to answers that do not come from it:
hand-written cases, numpy.quantile(method="linear") for CONT, numpy's inverted_cdf and a walk over the sorted list for DISC.

The bound against numpy.quantile: both formulas are a convex combination of v_lo and v_hi whose weights are exact and sum to
1; the model rounds three times (two products, one sum), numpy's lerp at most three times, each rounding an error of at most
u * max(|v_lo|, |v_hi|) with u = 2^-53, and the two exact combinations agree up to the one rounding of pos = (m - 1) * p that
both share: 8 u max(|v_lo|, |v_hi|) covers it with room.  Finite inputs only.
"""
import math

import numpy as np
import pytest

import percentile_ref as R

U = 2.0 ** -53


def cont(values, p, valid=None):
    _, outs, counts = R.percentile_ref([], (np.asarray(values), valid), [("cont", p)])
    vals, ok = outs[0]
    return (R.from_bits(int(vals[0])) if ok[0] else None), int(counts[0])


def disc(values, p, valid=None):
    _, outs, _ = R.percentile_ref([], (values, valid), [("disc", p)])
    vals, ok = outs[0]
    return int(vals[0]) if ok[0] else None


def test_hand_written_cont():
    assert cont([1.0, 2.0, 3.0, 4.0], 0.5) == (2.5, 4)
    assert cont([4.0, 1.0, 3.0, 2.0], 0.5) == (2.5, 4)
    assert cont([1.0, 2.0, 3.0], 0.5) == (2.0, 3)
    assert cont([10.0], 0.3) == (10.0, 1)
    assert cont([1.0, 2.0], 0.0) == (1.0, 2)
    assert cont([1.0, 2.0], 1.0) == (2.0, 2)
    assert cont([1.0, 2.0], 0.25) == (1.25, 2)
    assert cont(np.array([1, 2, 3, 10], dtype=np.int32), 0.75) == (4.75, 4)      # pos 2.25: 0.75 * 3 + 0.25 * 10
    assert cont([5.0, 7.0, 1.0], 0.5, valid=np.array([True, False, True])) == (3.0, 2)
    assert cont([5.0, 7.0], 0.5, valid=np.array([False, False])) == (None, 0)


def test_hand_written_cont_specials():
    nan_bits = R.NAN_BITS
    r, _ = cont([1.0, np.nan], 1.0)
    assert R.bits_of(r) == nan_bits                                              # NaN is the maximum
    assert cont([1.0, np.nan], 0.0)[0] == 1.0
    r, _ = cont([-np.inf, np.inf], 0.5)
    assert R.bits_of(r) == nan_bits                                              # IEEE: 0.5 * -inf + 0.5 * inf
    assert cont([np.inf, np.inf, 1.0], 0.75)[0] == np.inf                        # peers: no inf - inf, no 0 * inf
    r, _ = cont(np.array([np.nan, -np.nan]), 0.5)
    assert R.bits_of(r) == nan_bits
    r, _ = cont([-0.0], 0.5)
    assert R.bits_of(r) == 0                                                     # -0.0 is read as +0.0
    r, _ = cont([-0.0, 0.0], 0.5)
    assert R.bits_of(r) == 0
    assert cont(np.array([2 ** 53 + 1], dtype=np.int64), 0.5)[0] == float(2 ** 53)          # ties to even
    assert cont(np.array([2 ** 53 + 3], dtype=np.int64), 0.5)[0] == float(2 ** 53 + 4)
    assert cont(np.array([2 ** 64 - 1], dtype=np.uint64), 0.5)[0] == 2.0 ** 64
    assert cont(np.array([1.1], dtype=np.float32), 0.5)[0] == float(np.float32(1.1))


def test_hand_written_disc():
    v = np.array([30, 10, 20, 10, 40], dtype=np.int64)
    assert disc(v, 0.0) == 1                      # the smallest row holding 10
    assert disc(v, 0.4) == 1                      # k = ceil(2.0) - 1 = 1: still 10
    assert disc(v, 0.41) == 2                     # k = 2: 20
    assert disc(v, 0.5) == 2
    assert disc(v, 0.8) == 0                      # k = 3: 30
    assert disc(v, 1.0) == 4
    assert disc(v, 0.5, valid=np.array([True, False, True, False, True])) == 0      # of 20, 30, 40: k = 1
    assert disc(v, 0.5, valid=np.zeros(5, dtype=bool)) is None
    assert disc([b"pear", b"apple", None, b"fig", b"apple"], 0.5) == 1               # apple apple fig pear: k = 1, the smaller row of the two apples
    assert disc([b"pear", b"apple", None, b"fig", b"apple"], 0.75) == 3
    f = np.array([np.nan, 1.0, -0.0, 0.0, np.inf])
    assert disc(f, 1.0) == 0                      # NaN after +inf
    assert disc(f, 0.0) == 2                      # -0.0 and +0.0 are peers: the smaller row
    assert disc(f, 0.4) == 2


def test_disc_text_is_by_unsigned_bytes():
    rows = [b"b", b"\xc3\xa9", b"a", b"B", b""]
    order = sorted(range(5), key=lambda i: rows[i])
    for k, p in enumerate((0.2, 0.4, 0.6, 0.8, 1.0)):
        assert disc(rows, p) == order[k]
    assert rows[disc(rows, 0.0)] == b"" and rows[disc(rows, 1.0)] == b"\xc3\xa9"


def test_groups_counts_and_order():
    key = (np.array([2, 1, 2, 1, 3, 2], dtype=np.int32), np.array([True, True, True, True, False, True]))
    val = (np.array([1.0, 5.0, 3.0, 7.0, 9.0, 2.0]), np.array([True, True, True, False, False, True]))
    rows, outs, counts = R.percentile_ref([key], val, ["median", ("disc", 1.0), ("cont", 1.0)])
    assert rows.tolist() == [1, 0, 4]                                  # keys 1, 2, NULL
    assert counts.tolist() == [1, 3, 0]
    med, ok = outs[0]
    assert ok.tolist() == [True, True, False]
    assert [R.from_bits(int(b)) for b in med[:2]] == [5.0, 2.0] and med[2] == 0
    assert outs[1][0].tolist() == [1, 2, 0] and outs[1][1].tolist() == [True, True, False]
    assert [R.from_bits(int(b)) for b in outs[2][0][:2]] == [5.0, 3.0]


def test_refusals_of_the_model():
    with pytest.raises(ValueError):
        R.percentile_ref([], (np.array([1.0]),), [("cont", 1.5)])
    with pytest.raises(ValueError):
        R.percentile_ref([], (np.array([1.0]),), [("cont", math.nan)])
    with pytest.raises(ValueError):
        R.percentile_ref([], ([b"a"],), [("cont", 0.5)])


@pytest.mark.parametrize("dtype", ["f64", "f32", "i64", "i32", "u8"])
def test_cont_against_numpy_linear(dtype):
    rng = np.random.default_rng(11)
    checked = 0
    for m in (1, 2, 3, 4, 5, 8, 17, 100, 1001):
        if dtype.startswith("f"):
            v = (rng.normal(size=m) * 10.0 ** rng.integers(-3, 6)).astype(R.NP[dtype])
        else:
            ii = np.iinfo(R.NP[dtype])
            v = rng.integers(max(ii.min, -(1 << 52)), min(ii.max, 1 << 52), size=m).astype(R.NP[dtype])      # exactly representable: numpy converts first
        s = np.sort(v.astype(np.float64))
        for p in [0.0, 1.0, 0.5, 0.25, 0.75, 0.99, 1e-300, float(np.nextafter(1.0, 0.0))] + list(rng.uniform(size=12)):
            got, cnt = cont(v, p)
            assert cnt == m
            lo, hi, _, _ = R.rank(m, p)
            want = float(np.quantile(s, p, method="linear"))
            bound = 8 * U * max(abs(s[lo]), abs(s[hi]))
            assert abs(got - want) <= bound, (dtype, m, p, got, want, bound)
            assert s[lo] <= got <= s[hi] or abs(got - s[lo]) <= bound
            checked += 1
    assert checked == 9 * 20


def test_disc_against_numpy_inverted_cdf_where_p_times_m_is_exact():
    rng = np.random.default_rng(12)
    for m in (8, 16, 64, 1000, 4096):
        v = rng.integers(-50, 50, size=m).astype(np.int64)
        for k8 in range(9):
            p = k8 / 8.0
            row = disc(v, p)
            assert v[row] == np.quantile(v, p, method="inverted_cdf"), (m, p)
            assert row == int(np.flatnonzero(v == v[row])[0])


def test_disc_against_a_walk_over_the_sorted_list():
    rng = np.random.default_rng(13)
    for m in (1, 2, 3, 7, 10, 33, 257):
        v = rng.integers(0, 12, size=m).astype(np.int16)
        valid = rng.uniform(size=m) > 0.2
        live = sorted(int(x) for x, ok in zip(v, valid) if ok)
        for p in [0.0, 1.0, 0.5, 1e-300, float(np.nextafter(1.0, 0.0)), 0.1, 0.3, 0.7] + list(rng.uniform(size=10)):
            row = disc(v, p, valid)
            if not live:
                assert row is None
                continue
            # the smallest value whose cumulative share reaches p: the first position j (1-based) with j >= p * len
            j = 1
            while j < p * float(len(live)):
                j += 1
            want = live[j - 1]
            assert valid[row] and int(v[row]) == want, (m, p)
            assert row == min(i for i in range(m) if valid[i] and int(v[i]) == want)


def test_the_result_depends_on_the_multiset_only():
    rng = np.random.default_rng(14)
    n = 500
    key = rng.integers(0, 7, size=n).astype(np.int32)
    val = rng.normal(size=n)
    val[rng.integers(0, n, size=40)] = 1.0
    valid = rng.uniform(size=n) > 0.1
    calls = ["median", ("cont", 0.9), ("disc", 0.3)]
    _, a, ca = R.percentile_ref([(key,)], (val, valid), calls)
    perm = rng.permutation(n)
    _, b, cb = R.percentile_ref([(key[perm],)], (val[perm], valid[perm]), calls)
    assert ca.tolist() == cb.tolist()
    for c in range(2):
        assert a[c][0].tolist() == b[c][0].tolist() and a[c][1].tolist() == b[c][1].tolist()
    assert val[a[2][0]].tolist() == val[perm][b[2][0]].tolist()
