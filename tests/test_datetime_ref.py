"""tests/datetime_ref.py — the exact reference the GPU results are compared with — held to independent calendars: Python's
datetime over every day of years 1..9999, numpy datetime64 over the whole Int32 day range, the 400-year period of the
Gregorian calendar (which carries the datetime check to the rest of the domain), pyarrow.compute where it does not overflow,
and Spark's documented examples as literals.  No GPU."""
import datetime as pydt

import numpy as np
import pytest

import datetime_ref as R

EPOCH = pydt.date(1970, 1, 1).toordinal()


def test_every_day_of_years_1_to_9999_against_datetime():
    lo, hi = pydt.date(1, 1, 1).toordinal() - EPOCH, pydt.date(9999, 12, 31).toordinal() - EPOCH
    days = np.arange(lo, hi + 1, dtype=np.int64)
    y, m, d = R.civil_from_days(days)
    wd, yd, wk = R.weekday(days), R.day_of_year(days), R.iso_week(days)
    dow = R.field(days, R.DAY, "day_of_week")
    assert np.array_equal(R.days_from_civil(y, m, d), days)
    start = 0
    for year in range(1, 10000):                     # one comparison per year, vectorised
        n = 366 if (year % 4 == 0 and year % 100 != 0) or year % 400 == 0 else 365
        dates = [pydt.date.fromordinal(int(o)) for o in range(lo + EPOCH + start, lo + EPOCH + start + n)]
        sl = slice(start, start + n)
        assert (y[sl] == year).all(), year
        assert np.array_equal(m[sl], [t.month for t in dates]) and np.array_equal(d[sl], [t.day for t in dates]), year
        assert np.array_equal(wd[sl], [t.weekday() for t in dates]), year
        assert np.array_equal(yd[sl], np.arange(1, n + 1)), year
        assert np.array_equal(wk[sl], [t.isocalendar()[1] for t in dates]), year
        assert np.array_equal(dow[sl], [t.isoweekday() % 7 + 1 for t in dates]), year
        start += n
    assert start == len(days)


def test_numpy_datetime64_over_the_whole_int32_day_range():
    rng = np.random.default_rng(5)
    days = np.concatenate([np.arange(R.I32_MIN, R.I32_MAX, 9973, dtype=np.int64), np.arange(R.I32_MIN, R.I32_MIN + 4096, dtype=np.int64),
                           np.arange(R.I32_MAX - 4095, R.I32_MAX + 1, dtype=np.int64), rng.integers(R.I32_MIN, R.I32_MAX, 200_000), R.edge_days()])
    d64 = days.astype("datetime64[D]")
    y, m, d = R.civil_from_days(days)
    ny = d64.astype("datetime64[Y]")
    nm = d64.astype("datetime64[M]")
    assert np.array_equal(y, ny.astype(np.int64) + 1970)
    assert np.array_equal(m, (nm - ny.astype("datetime64[M]")).astype(np.int64) + 1)
    assert np.array_equal(d, (d64 - nm.astype("datetime64[D]")).astype(np.int64) + 1)
    assert np.array_equal(R.day_of_year(days), (d64 - ny.astype("datetime64[D]")).astype(np.int64) + 1)
    assert np.array_equal(R.days_from_civil(y, m, d), days)
    # the extremes, by name
    assert [int(x[0]) for x in R.civil_from_days([R.I32_MIN])] == [-5877641, 6, 23]
    assert [int(x[0]) for x in R.civil_from_days([R.I32_MAX])] == [5881580, 7, 11]


def test_the_400_year_period_reaches_both_ends_of_int32():
    """146 097 days are 400 years and exactly 20 871 weeks: every field of day + 146097 k is that of day, the year moved by
    400 k.  With k reaching both ends of Int32 this carries the datetime check of one whole period to the whole domain."""
    assert R.ERA_DAYS == 20871 * 7
    base = np.arange(R.d(2000, 3, 1), R.d(2400, 2, 29) + 1, dtype=np.int64)
    assert len(base) == R.ERA_DAYS
    ref = {f: R.field(base, R.DAY, f).astype(np.int64) for f in R.FIELDS[:7]}
    kmin, kmax = -((base[0] - R.I32_MIN) // R.ERA_DAYS) - 1, (R.I32_MAX - base[-1]) // R.ERA_DAYS + 1
    for k in (int(kmin), int(kmin) + 1, -5000, -14, -1, 1, 9, 5000, int(kmax) - 1, int(kmax)):
        days = base + R.ERA_DAYS * k
        keep = (days >= R.I32_MIN) & (days <= R.I32_MAX)
        assert keep.any() and (k not in (kmin, kmax) or not keep.all())     # the outermost periods are cut by the ends of Int32
        for f in R.FIELDS[:7]:
            got = R.field(days[keep], R.DAY, f).astype(np.int64)
            assert np.array_equal(got, ref[f][keep] + (400 * k if f == "year" else 0)), (k, f)


def test_time_of_day_and_day_number_against_python_ints():
    rng = np.random.default_rng(6)
    for unit in (R.S, R.MS, R.US, R.NS):
        v = np.concatenate([rng.integers(R.I64_MIN, R.I64_MAX, 3000, endpoint=True), [R.I64_MIN, R.I64_MAX, -1, 0, 1]]).astype(np.int64)
        ups, upd = R.UNITS_PER_SECOND[unit], R.UNITS_PER_DAY[unit]
        secs = [int(x) // ups % 86400 for x in v]
        assert R.field(v, unit, "hour").tolist() == [s // 3600 for s in secs]
        assert R.field(v, unit, "minute").tolist() == [s // 60 % 60 for s in secs]
        assert R.field(v, unit, "second").tolist() == [s % 60 for s in secs]
        assert R.field(v, unit, "date").tolist() == [((int(x) // upd + 2 ** 31) % 2 ** 32) - 2 ** 31 for x in v]
        for level, step in (("day", upd), ("hour", 3600 * ups), ("minute", 60 * ups), ("second", ups)):
            assert R.trunc(v, unit, level).tolist() == [((int(x) - int(x) % step + 2 ** 63) % 2 ** 64) - 2 ** 63 for x in v]
    m1 = np.array([-1], dtype=np.int64)
    for unit in (R.S, R.MS, R.US, R.NS):                                 # -1 in every unit is 1969-12-31 23:59:59
        assert [int(R.field(m1, unit, f)[0]) for f in ("year", "month", "day_of_month", "hour", "minute", "second")] == [1969, 12, 31, 23, 59, 59]


def test_pyarrow_compute_inside_its_range():
    """pyarrow overflows outside timestamps 1678..2262 and dates of years 1..9999 (its `year` of day -2^31 + 1 is 20599), so it is
    asked only inside."""
    pa = pytest.importorskip("pyarrow")
    pc = pytest.importorskip("pyarrow.compute")
    rng = np.random.default_rng(8)
    lo, hi = R.d(1678, 1, 1), R.d(2262, 1, 1)
    names = {"year": pc.year, "quarter": pc.quarter, "month": pc.month, "day_of_month": pc.day, "day_of_year": pc.day_of_year,
             "week_of_year": pc.iso_week, "minute": pc.minute, "second": pc.second, "hour": pc.hour}
    for unit, code in ((R.S, "s"), (R.MS, "ms"), (R.US, "us"), (R.NS, "ns")):
        upd = R.UNITS_PER_DAY[unit]
        v = np.concatenate([rng.integers(lo * upd, hi * upd, 20000), R.scaled(R.common_days(), unit, rng)]).astype(np.int64)
        ts = pa.array(v, type=pa.timestamp(code))
        for f, fn in names.items():
            assert np.array_equal(R.field(v, unit, f), fn(ts).to_numpy().astype(np.int32)), (code, f)
        assert np.array_equal(R.field(v, unit, "day_of_week"), pc.day_of_week(ts, count_from_zero=False, week_start=7).to_numpy().astype(np.int32))
        for level, u in (("year", "year"), ("quarter", "quarter"), ("month", "month"), ("week", "week"), ("day", "day"), ("hour", "hour"),
                         ("minute", "minute"), ("second", "second")):
            assert np.array_equal(R.trunc(v, unit, level), pc.floor_temporal(ts, unit=u).cast(pa.int64()).to_numpy()), (code, level)
        w = rng.permutation(v)
        assert np.array_equal(R.diff(v, unit, w, unit), pc.days_between(pa.array(w, type=pa.timestamp(code)), ts).to_numpy().astype(np.int32))
    days = np.concatenate([rng.integers(R.d(1, 1, 1), R.d(9999, 12, 31), 20000), R.common_days()]).astype(np.int32)
    dates = pa.array(days, type=pa.date32())
    for f, fn in names.items():
        if f not in ("hour", "minute", "second"):
            assert np.array_equal(R.field(days, R.DAY, f), fn(dates).to_numpy().astype(np.int32)), f
    assert np.array_equal(R.field(days, R.DAY, "day_of_week"), pc.day_of_week(dates, count_from_zero=False, week_start=7).to_numpy().astype(np.int32))
    for level in ("year", "quarter", "month", "week", "day"):
        assert np.array_equal(R.trunc(days, R.DAY, level, 32), pc.floor_temporal(dates, unit=level).cast(pa.int32()).to_numpy()), level


def test_add_months_last_day_next_day_against_datetime():
    rng = np.random.default_rng(9)
    days = np.concatenate([rng.integers(R.d(1000, 1, 1), R.d(3000, 1, 1), 3000), R.common_days()]).astype(np.int64)
    months = rng.integers(-2000, 2000, len(days))
    wds = rng.integers(1, 7, len(days), endpoint=True)
    got_m, _ = R.shift(days, R.DAY, "months", months)
    got_l, _ = R.shift(days, R.DAY, "last_day", 0)
    got_n, ok = R.shift(days, R.DAY, "next_day", wds)
    assert ok.all()
    for i, o in enumerate(days):
        t = pydt.date.fromordinal(int(o) + EPOCH)
        total = t.year * 12 + t.month - 1 + int(months[i])
        ny, nm = total // 12, total % 12 + 1
        last = (pydt.date(ny + (nm == 12), nm % 12 + 1, 1) - pydt.timedelta(days=1)).day
        assert int(got_m[i]) == pydt.date(ny, nm, min(t.day, last)).toordinal() - EPOCH
        assert int(got_l[i]) == (pydt.date(t.year + (t.month == 12), t.month % 12 + 1, 1) - pydt.timedelta(days=1)).toordinal() - EPOCH
        nxt = t + pydt.timedelta(days=1)
        while nxt.isoweekday() % 7 + 1 != int(wds[i]):
            nxt += pydt.timedelta(days=1)
        assert int(got_n[i]) == nxt.toordinal() - EPOCH
    _, ok = R.shift(days[:6], R.DAY, "next_day", [0, 1, 7, 8, -1, 2 ** 31 - 1])
    assert ok.tolist() == [False, True, True, False, False, False]
    assert R.shift([R.I32_MAX], R.DAY, "days", 1)[0].tolist() == [R.I32_MIN]                       # integers wrap
    assert R.diff([R.I32_MIN], R.DAY, [1], R.DAY).tolist() == [R.I32_MAX]


def test_spark_documented_examples():
    D = R.d
    one = lambda x: np.array([x], dtype=np.int64)
    assert R.field(one(D(2009, 7, 30)), R.DAY, "day_of_week")[0] == 5
    assert R.field(one(D(2008, 2, 20)), R.DAY, "week_of_year")[0] == 8
    assert R.field(one(D(2016, 4, 9)), R.DAY, "day_of_year")[0] == 100
    assert R.field(one(D(2016, 8, 31)), R.DAY, "quarter")[0] == 3
    assert R.shift(one(D(2009, 1, 12)), R.DAY, "last_day", 0)[0][0] == D(2009, 1, 31)
    assert R.shift(one(D(2015, 1, 14)), R.DAY, "next_day", 3)[0][0] == D(2015, 1, 20)            # Tuesday = 3
    assert R.shift(one(D(2016, 8, 31)), R.DAY, "months", 1)[0][0] == D(2016, 9, 30)
    assert R.shift(one(D(2019, 2, 28)), R.DAY, "months", 1)[0][0] == D(2019, 3, 28)
    ts = (D(2015, 3, 5) * 86400 + 9 * 3600 + 32 * 60 + 5) * 1000 + 359
    assert R.trunc(one(ts), R.MS, "week")[0] == D(2015, 3, 2) * 86400 * 1000
    assert R.trunc(one(D(2019, 8, 4)), R.DAY, "week", 32)[0] == D(2019, 7, 29)
    assert R.trunc(one(D(2019, 8, 4)), R.DAY, "quarter", 32)[0] == D(2019, 7, 1)
    assert R.diff(one(D(2009, 7, 31)), R.DAY, one(D(2009, 7, 30)), R.DAY)[0] == 1
    assert (D(1970, 1, 1), D(2009, 7, 30)) == (0, 14455)


def test_the_golden_table_is_what_the_generator_writes():
    got = np.load(R.GOLDEN)["cases"]
    assert got.dtype == np.int64 and got.shape[1] == 28 and len(got) >= 3000 and np.array_equal(got, R.golden_table())
