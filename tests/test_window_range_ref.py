"""tests/window_range_ref.py — the model the GPU tests of rdf_window_range_agg are held to — against three independent references:
pandas' time-based rolling windows, window_frame_ref.frame_ref (the model of rdf_window_agg) where a value frame IS a ROWS or an
offset-free RANGE frame, and a table worked out by hand.  No GPU."""
import math

import numpy as np
import pandas as pd
import pytest

import window_frame_ref as F
import window_range_ref as R

UP, UF = R.UNBOUNDED_PRECEDING, R.UNBOUNDED_FOLLOWING


def same(got, want):
    gv, gok = got
    wv, wok = want
    assert np.array_equal(gok, wok), (gok, wok)
    if gv.dtype.kind == "f":
        assert np.array_equal(gv[gok].view(np.uint64), np.asarray(wv, dtype=np.float64)[wok].view(np.uint64)), (gv, wv)
    else:
        assert np.array_equal(gv[gok], np.asarray(wv)[wok]), (gv, wv)


# ---------------------------------------------------------------- pandas
# rolling("<s>s", closed="both") over a DatetimeIndex is [t - s, t]: `s PRECEDING .. CURRENT ROW`.  It agrees ONLY when the
# order keys are unique inside a partition: pandas' window of a row ends AT that row, so the later peers of a duplicated key
# are left out (keys 1, 1, 2, 2, 5 with s = 1 count 1, 2, 3, 4, 1 there; SQL's RANGE frame counts 2, 2, 4, 4, 1).  The keys of
# this leg are therefore drawn without repetition per partition.
def test_pandas_documents_why_the_keys_must_be_unique():
    s = pd.Series(1.0, index=pd.to_datetime([1, 1, 2, 2, 5], unit="s"))
    assert s.rolling("1s", closed="both").count().tolist() == [1, 2, 3, 4, 1]
    k = np.array([1, 1, 2, 2, 5], dtype=np.int64)
    got = R.range_ref([], (k, None, False), [], [("count", -1, (-1, 0))])[0][0]
    assert got.tolist() == [2, 2, 4, 4, 1]


@pytest.mark.parametrize("s", [0, 1, 3, 10, 1000])
def test_preceding_frames_agree_with_pandas_rolling(s):
    rng = np.random.default_rng(11 + s)
    n, nparts = 120, 5
    part = rng.integers(0, nparts, size=n).astype(np.int64)
    key = np.zeros(n, dtype=np.int64)
    for p in range(nparts):
        m = part == p
        key[m] = rng.choice(60, size=int(m.sum()), replace=False)          # unique inside the partition
    x = rng.integers(-50, 50, size=n).astype(np.float64)
    valid = rng.random(n) > 0.15
    df = pd.DataFrame({"p": part, "x": np.where(valid, x, np.nan)}, index=pd.to_datetime(key, unit="s"))
    calls = [(name, 0, (-s, 0)) for name in ("sum", "count", "min", "max", "avg")]
    got = R.range_ref([(part,)], (key, None, False), [(x, valid)], calls)
    srt = df.sort_index(kind="stable")
    for (name, _, _), (gv, gok) in zip(calls, got):
        for p in range(nparts):
            rows = np.flatnonzero(part == p)
            rows = rows[np.argsort(key[rows], kind="stable")]
            sub = srt[srt["p"] == p]["x"]
            if s > 0:
                r = sub.rolling(f"{s}s", closed="both", min_periods=1)
                cnt = sub.rolling(f"{s}s", closed="both").count().to_numpy()
                want = {"sum": r.sum, "count": lambda: sub.rolling(f"{s}s", closed="both").count(), "min": r.min, "max": r.max, "avg": r.mean}[name]().to_numpy()
            else:                                                           # (pandas has no zero-length window: the row alone)
                cnt = sub.notna().to_numpy().astype(float)
                want = cnt if name == "count" else sub.to_numpy()
            if name == "count":
                assert np.array_equal(gv[rows], want.astype(np.int64)) and gok[rows].all()
            else:
                assert np.array_equal(gok[rows], cnt > 0)
                assert np.array_equal(gv[rows][cnt > 0], want[cnt > 0])     # integer-valued data: exact in both


def test_whole_column_rolling_without_partitions_agrees_with_pandas():
    rng = np.random.default_rng(5)
    key = rng.choice(500, size=200, replace=False).astype(np.int64)
    x = rng.integers(-9, 9, size=200).astype(np.float64)
    s = pd.Series(x, index=pd.to_datetime(key, unit="s")).sort_index()
    got = R.range_ref([], (key, None, False), [(x, None)], [("sum", 0, (-7, 0)), ("count", 0, (-7, 0))])
    order = np.argsort(key, kind="stable")
    assert np.array_equal(got[0][0][order], s.rolling("7s", closed="both").sum().to_numpy())
    assert np.array_equal(got[1][0][order], s.rolling("7s", closed="both").count().to_numpy().astype(np.int64))


# ---------------------------------------------------------------- the model of rdf_window_agg
@pytest.mark.parametrize("desc", [False, True])
def test_offset_zero_is_the_offset_free_range_frame(desc):
    rng = np.random.default_rng(3)
    n = 90
    part = rng.integers(0, 4, size=n).astype(np.int64)
    key = rng.integers(0, 6, size=n).astype(np.float64)
    key[rng.random(n) < 0.1] = np.nan
    kvalid = rng.random(n) > 0.1
    x = rng.integers(-5, 5, size=n).astype(np.int64)
    xv = rng.random(n) > 0.2
    zero_p, zero_f = (R.PRECEDING, 0.0), (R.FOLLOWING, 0.0)
    for name in F.FNS:
        vi = 0
        want = F.frame_ref([(part,)], [(key, kvalid, desc)], [(x, xv)], [(name, vi, ("range", 0, 0))])[0]
        for frame in ((0, 0), (zero_p, zero_f), (zero_p, 0), (0, zero_f)):
            same(R.range_ref([(part,)], (key, kvalid, desc), [(x, xv)], [(name, vi, frame)])[0], want)
        want = F.frame_ref([(part,)], [(key, kvalid, desc)], [(x, xv)], [(name, vi, ("range", UP, 0))])[0]
        same(R.range_ref([(part,)], (key, kvalid, desc), [(x, xv)], [(name, vi, (UP, zero_f))])[0], want)
        want = F.frame_ref([(part,)], [(key, kvalid, desc)], [(x, xv)], [(name, vi, ("range", 0, UF))])[0]
        same(R.range_ref([(part,)], (key, kvalid, desc), [(x, xv)], [(name, vi, (zero_p, UF))])[0], want)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.float64])
def test_dense_unique_keys_make_value_frames_rows_frames(desc, dtype):
    rng = np.random.default_rng(9)
    sizes = [1, 2, 7, 30]
    part = np.concatenate([np.full(m, i, dtype=np.int64) for i, m in enumerate(sizes)])
    key = np.concatenate([rng.permutation(m) for m in sizes]).astype(dtype)
    perm = rng.permutation(len(part))
    part, key = part[perm], key[perm]
    x = rng.normal(size=len(part)) * 10.0 ** rng.integers(-3, 6, size=len(part))
    xv = rng.random(len(part)) > 0.2
    one = dtype(1)
    for start, end in ((-2, 1), (-3, -1), (1, 4), (0, 2), (-5, 0), (UP, 2), (-1, UF), (UP, UF), (-40, 40)):
        conv = lambda b: b if isinstance(b, str) else (b * one if dtype == np.float64 else int(b))
        for name in F.FNS:
            want = F.frame_ref([(part,)], [(key, None, desc)], [(x, xv)], [(name, 0, ("rows", start, end))])[0]
            same(R.range_ref([(part,)], (key, None, desc), [(x, xv)], [(name, 0, (conv(start), conv(end)))])[0], want)


def test_the_fast_model_is_the_model():
    rng = np.random.default_rng(21)
    n = 150
    part = rng.integers(0, 5, size=n).astype(np.int64)
    for dtype, desc in ((np.int64, False), (np.int64, True), (np.float64, True), (np.int32, False)):
        key = rng.integers(-8, 8, size=n).astype(dtype)
        kvalid = rng.random(n) > 0.1
        if dtype == np.float64:
            key[rng.random(n) < 0.1] = np.nan
        xi = rng.integers(-100, 100, size=n).astype(np.int64)
        xf = rng.integers(-100, 100, size=n).astype(np.float64)
        xv = rng.random(n) > 0.1
        conv = (lambda b: float(b)) if dtype == np.float64 else (lambda b: b)
        calls = []
        for start, end in ((-2, 1), (-3, -1), (1, 4), (0, 2), (UP, 2), (-1, UF), (UP, UF), ((R.PRECEDING, 0), 3)):
            fr = tuple(b if isinstance(b, (str, tuple)) else conv(b) for b in (start, end))
            one_sided = start == UP or end == UF
            for name in F.FNS:
                if name in ("min", "max") and not one_sided:
                    continue
                calls += [(name, 0, fr), (name, 1, fr)]
        slow = R.range_ref([(part,)], (key, kvalid, desc), [(xi, xv), (xf, None)], calls)
        fast = R.range_ref_fast([(part,)], (key, kvalid, desc), [(xi, xv), (xf, None)], calls)
        for g, w in zip(fast, slow):
            same(g, w)


# ---------------------------------------------------------------- by hand
#            row:   0    1    2    3    4     5     6    7    8    9     10   11
HAND_PART = ["A", "A", "A", "A", "A", "A", "B", "B", "B", "B", "B", "A"]
HAND_KEY = [1, 1, 2, 5, None, None, 3, 7, 7, 8, 20, 6]
HAND_X = [10, 20, 30, 40, 50, 60, 1, 2, 3, None, 5, 70]
# ascending, partition A in order: rows 0 1 2 3 11 4 5 (keys 1 1 2 5 6 NULL NULL); B: rows 6 7 8 9 10 (keys 3 7 7 8 20)
HAND = [
    # (call, descending, expected values by row, expected valid by row (None: all))
    (("count", -1, (-1, 0)), False, [2, 2, 3, 1, 2, 2, 1, 2, 2, 3, 1, 2], None),
    (("sum", 0, (-1, 0)), False, [30, 30, 60, 40, 110, 110, 1, 5, 5, 5, 5, 110], None),
    # 2 FOLLOWING .. 3 FOLLOWING: empty for most rows; the NULL rows keep their peer group
    (("count", -1, (2, 3)), False, [0, 0, 1, 0, 2, 2, 0, 0, 0, 0, 0, 0], None),
    (("first_value", -1, (2, 3)), False, [0, 0, 3, 0, 4, 4, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0]),
    (("sum", 0, (2, 3)), False, [0, 0, 40, 0, 110, 110, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0]),
    # 3 PRECEDING .. 2 PRECEDING: the first row of the first partition has the empty frame [0, -1]
    (("count", -1, (-3, -2)), False, [0, 0, 0, 1, 2, 2, 0, 0, 0, 0, 0, 0], None),
    (("last_value", -1, (-3, -2)), False, [0, 0, 0, 2, 5, 5, 0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0]),
    # UNBOUNDED PRECEDING .. 1 FOLLOWING; a NULL row's end is its last peer, the partition's last row
    (("sum", 0, (UP, 1)), False, [60, 60, 60, 170, 280, 280, 1, 6, 6, 6, 11, 170], None),
    (("max", 0, (UP, 1)), False, [30, 30, 30, 70, 70, 70, 1, 3, 3, 3, 5, 70], None),
    # 1 PRECEDING .. UNBOUNDED FOLLOWING reaches the NULL rows at the partition's end
    (("count", -1, (-1, UF)), False, [7, 7, 7, 4, 2, 2, 5, 4, 4, 4, 1, 4], None),
    (("min", 0, (-1, UF)), False, [10, 10, 10, 40, 50, 50, 1, 2, 2, 2, 5, 40], None),
    # descending: A in order rows 11 3 2 0 1 4 5 (keys 6 5 2 1 1 NULL NULL); 1 PRECEDING is key + 1
    (("count", -1, (-1, 0)), True, [3, 3, 1, 2, 2, 2, 1, 3, 3, 1, 1, 1], None),
    (("last_value", -1, (-1, 0)), True, [1, 1, 2, 3, 5, 5, 6, 8, 8, 9, 10, 11], None),
    (("first_value", -1, (-1, 0)), True, [2, 2, 2, 11, 4, 4, 6, 9, 9, 9, 10, 11], None),
    (("sum", 0, (0, 1)), True, [30, 30, 60, 40, 110, 110, 1, 5, 5, 5, 5, 110], None),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_the_hand_written_table(case):
    call, desc, want, wok = HAND[case]
    part = np.array([ord(c) for c in HAND_PART], dtype=np.int64)
    key = np.array([k if k is not None else 0 for k in HAND_KEY], dtype=np.int64)
    kvalid = np.array([k is not None for k in HAND_KEY])
    x = np.array([v if v is not None else -999 for v in HAND_X], dtype=np.int64)
    xv = np.array([v is not None for v in HAND_X])
    wok = np.ones(12, dtype=bool) if wok is None else np.array(wok, dtype=bool)
    for ref in (R.range_ref, R.range_ref_fast):
        gv, gok = ref([(part,)], (key, kvalid, desc), [(x, xv)], [call])[0]
        assert gok.tolist() == wok.tolist(), (call, gok)
        assert gv[wok].tolist() == np.array(want)[wok].tolist(), (call, gv)
    # Int32 and Float64 keys of the same values answer alike
    for kk, off in ((key.astype(np.int32), int), (key.astype(np.float64), float)):
        fr = tuple(b if isinstance(b, str) else off(b) for b in call[2])
        gv, gok = R.range_ref([(part,)], (kk, kvalid, desc), [(x, xv)], [(call[0], call[1], fr)])[0]
        assert gok.tolist() == wok.tolist() and gv[wok].tolist() == np.array(want)[wok].tolist()


def test_float_bounds_are_one_ieee_operation():
    key = np.array([0.1, 0.3, -0.0, 0.0, np.nan, np.inf, -np.inf])
    c = lambda fr, desc=False: R.range_ref([], (key, None, desc), [], [("count", -1, fr)])[0][0].tolist()
    assert 0.1 >= np.float64(0.3) - np.float64(0.2) and not (np.float64(0.1) + np.float64(0.2) <= 0.3)
    got = c((-0.2, 0.0))
    assert got[1] == 2                    # 0.1 >= fl(0.3 - 0.2) = 0.09999999999999998: 0.1 is in 0.3's frame
    assert c((0.0, 0.2))[0] == 2          # fl(0.1 + 0.2) = 0.30000000000000004 >= 0.3
    assert got[2] == got[3] == 2          # -0.0 == +0.0
    assert got[4] == 1                    # the NaN row: its own peer group
    assert got[5] == 1 and got[6] == 1    # inf - 0.2 = inf
    assert c((-1e300, 1e300))[:4] == [4, 4, 4, 4] and c((UP, 1e300))[0] == 5 and c((-1e300, UF))[0] == 6
    assert c((-0.2, 0.0), True)[0] == 2 and c((-0.2, 0.0), True)[4] == 1


def test_integer_bounds_do_not_wrap():
    mn, mx = R.I64_MIN, R.I64_MAX
    key = np.array([mn, mn + 1, -1, 0, 1, mx - 1, mx], dtype=np.int64)
    c = lambda fr, desc=False: R.range_ref([], (key, None, desc), [], [("count", -1, fr)])[0][0].tolist()
    assert c((-1, 0)) == [1, 2, 1, 2, 2, 1, 2]
    assert c((0, 1)) == [2, 1, 2, 2, 1, 2, 1]
    assert c((-mx, 0)) == [1, 2, 3, 3, 3, 4, 4]      # MIN's frame is [MIN - (2^63 - 1), MIN]: itself alone
    assert c((0, mx)) == [3, 3, 4, 4, 3, 2, 1]        # MIN + (2^63 - 1) = -1
    assert c((-mx, mx)) == [3, 4, 6, 6, 5, 5, 4]
    assert c((-mx, 0), True) == [3, 3, 4, 4, 3, 2, 1]


def test_sum_slack_is_the_bound_of_section_11():
    x = np.array([1e16, -1e16, 1.0, 1.0, 1.0])
    key = np.arange(5, dtype=np.int64)
    sl = R.sum_slack([], (key, None, False), (x, None), (-1, 1))
    assert sl[0] == 8.0 * 3 * 2.0 ** -106 * np.nextafter(2e16, math.inf) and sl[4] == 8.0 * 6 * 2.0 ** -106 * np.nextafter(2e16 + 3, math.inf)
    want = F.sum_slack([], [(key, None, False)], (x, None), ("rows", -1, 1))
    assert np.array_equal(sl, want)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("is_float", [False, True])
def test_the_host_table_s_positions_are_the_brute_force_bounds(desc, is_float):
    """window_range_ref._positions, which writes the expected column of the table tests/cpp/test_window_range_host.cpp reads,
    restates the search's predicate; range_bounds does not.  Over one partition they must agree: a start is a, an end b + 1."""
    rng = np.random.default_rng(31)
    sub = float(np.nextafter(0.0, 1.0))
    if is_float:
        pools = [[-math.inf, -1e300, -1.0, -sub, -0.0, 0.0, sub, 0.1, 0.2, 0.3, 0.30000000000000004, 1.0, 1e300, math.inf, math.inf],
                 (rng.integers(-30, 30, size=40) / 10.0).tolist()]
        offsets = [0.0, sub, 0.1, 0.2, 0.5, 1e300]
    else:
        pools = [[R.I64_MIN, R.I64_MIN + 1, -(1 << 31), -1, 0, 1, 1, 7, (1 << 31) - 1, R.I64_MAX - 1, R.I64_MAX, R.I64_MAX], rng.integers(-20, 20, size=40).tolist()]
        offsets = [0, 1, 7, 1 << 62, R.I64_MAX]
    for pool in pools:
        for nlow, nhigh in ((0, 0), (2 if (desc and is_float) else 0, 3)):
            ordinary = sorted(pool, reverse=desc)
            nan_high = 1 if (is_float and not desc and nhigh) else 0                # ascending Float64: one NaN among the HIGH rows
            nulls = nhigh - nan_high
            keys = [math.nan] * nlow + ordinary + [math.nan] * nan_high + [0] * nulls
            classes = [1] * nlow + [0] * len(ordinary) + [2] * nhigh
            kv = np.array(keys, dtype=np.float64 if is_float else np.int64)
            kvalid = np.array([True] * (len(keys) - nulls) + [False] * nulls)
            for s in offsets:
                for following in (0, 1):
                    b = (R.FOLLOWING if following else R.PRECEDING, s)
                    _o, _ps, a, _b = R.range_bounds([], (kv, kvalid, desc), (b, UF))
                    _o, _ps, _a, e = R.range_bounds([], (kv, kvalid, desc), (UP, b))
                    for j, c in enumerate(classes):
                        if c != 0:
                            continue
                        assert R._positions(keys, classes, keys[j], is_float, desc, 0, following, s) == a[j], (keys[j], s, following)
                        assert R._positions(keys, classes, keys[j], is_float, desc, 1, following, s) == e[j] + 1, (keys[j], s, following)
