"""The model of rdf_utf8_parse / rdf_utf8_format (tests/textconv_ref.py) held to independent references where they agree:
int() and str() for integers, datetime's fromisoformat / strptime / strftime for the years 1..9999, the known answers of the
issue, the pattern compile errors with their positions, and the round trip parse(format(x)) == x."""
import datetime as dt

import numpy as np
import pytest

import datetime_ref as D
import textconv_ref as R

EPOCH = dt.date(1970, 1, 1)


def test_plain_integers_agree_with_int_and_str():
    rng = np.random.default_rng(1)
    for dtype in R.INT_DTYPES:
        lo, hi = R.int_limits(dtype)
        vals = R.edge_values(R.INT, dtype=dtype) + [int(x) for x in rng.integers(max(lo, -2 ** 62), min(hi, 2 ** 62), size=2000, endpoint=True)]
        for v in vals:
            t = str(v).encode()
            assert R.format(R.INT, v) == t
            assert R.parse_int(t, dtype) == int(t) == v
            assert R.parse_int(b" \t" + t + b"\n", dtype) == v
        for v in (lo - 1, hi + 1):
            assert R.parse_int(str(v).encode(), dtype) is None
    for t in (b"12", b"+12", b"-12", b"0012", b"-0"):
        assert R.parse_int(t) == int(t)


def test_the_known_answers():
    for kind, text, unit, dtype, pat, exp in R.KNOWN_PARSE:
        toks = R.compile_pattern(pat, True) if pat is not None else None
        assert R.parse(kind, text, unit, dtype, toks) == exp, (kind, text, pat)
    for kind, v, unit, pat, exp in R.KNOWN_FORMAT:
        toks = R.compile_pattern(pat, False) if pat is not None else None
        assert R.format(kind, v, unit, toks) == exp, (kind, v, pat)
    for t in (b"t", b"TRUE", b"y", b"Yes", b"1"):
        assert R.parse_bool(t) is True
    for t in (b"f", b"False", b"N", b"no", b"0"):
        assert R.parse_bool(t) is False


def test_trimming_takes_the_ten_bytes_and_no_other():
    for c in range(256):
        got = R.parse_int(bytes([c]) + b"42" + bytes([c]))
        assert (got == 42) == (c in R.WS), c
    assert sorted(R.WS) == [9, 10, 11, 12, 13, 28, 29, 30, 31, 32]
    assert R.parse_int(" 42".encode()) is None and R.parse_date("　2020".encode()) is None


def test_dates_agree_with_datetime_for_the_years_1_to_9999():
    rng = np.random.default_rng(2)
    days = [int(x) for x in D.common_days()] + [int(x) for x in rng.integers((dt.date(1, 1, 1) - EPOCH).days, (dt.date(9999, 12, 31) - EPOCH).days, size=3000)]
    for day in days:
        date = EPOCH + dt.timedelta(days=day)
        if not 1 <= date.year <= 9999:
            continue
        iso = date.isoformat().encode()
        assert R.format(R.DATE, day, D.DAY) == iso
        assert R.parse_date(iso) == (dt.date.fromisoformat(iso.decode()) - EPOCH).days == day
    for bad in ("2019-02-29", "2020-04-31", "2020-13-01", "2020-00-01"):
        with pytest.raises(ValueError):
            dt.date.fromisoformat(bad)
        assert R.parse_date(bad.encode()) is None


def test_patterns_agree_with_strptime_and_strftime():
    pairs = [("yyyy-MM-dd HH:mm:ss", "%Y-%m-%d %H:%M:%S"), ("yyyy DDD", "%Y %j"), ("dd MMM yyyy", "%d %b %Y"), ("yyyy-MM-dd hh:mm:ss a", "%Y-%m-%d %I:%M:%S %p"),
             ("EEE, dd MMM yyyy", "%a, %d %b %Y")]
    rng = np.random.default_rng(3)
    secs = [int(x) for x in rng.integers(-62135596800 + 86400 * 366 * 1000, 253402300799, size=1500)] + [0, -1, 86399, 951782400, 1582979696]
    for pat, fmt in pairs:
        for s in secs:
            t = dt.datetime(1970, 1, 1) + dt.timedelta(seconds=s)
            if t.year < 1000:      # (strftime's %Y does not pad on every platform)
                continue
            text = t.strftime(fmt).encode()
            assert R.format(R.TIMESTAMP, s, R.S, R.compile_pattern(pat, False)) == text, (pat, s)
            if "EEE" in pat:
                continue
            back = dt.datetime.strptime(text.decode(), fmt)
            assert R.parse(R.TIMESTAMP, text, R.S, R.I64, R.compile_pattern(pat, True)) == int((back - dt.datetime(1970, 1, 1)).total_seconds()), (pat, text)


def test_every_compile_error_names_its_position():
    for pat, for_parse, what, pos in R.PATTERN_ERRORS:
        with pytest.raises(R.PatternError) as e:
            R.compile_pattern(pat, for_parse)
        assert (e.value.what, e.value.pos) == (what, pos), pat
    for pat in R.PATTERNS_PARSE:
        R.compile_pattern(pat, True)
    for pat in R.PATTERNS_FORMAT:
        R.compile_pattern(pat, False)
    assert len(R.format(R.TIMESTAMP, D.I64_MIN, R.S, R.compile_pattern(R.CAP_PATTERN, False))) == R.MAX_ROW_BYTES


def test_the_round_trip_over_the_edge_values():
    for dtype in R.INT_DTYPES:
        for v in R.edge_values(R.INT, dtype=dtype):
            assert R.parse_int(R.format(R.INT, v), dtype) == v
    for day in R.edge_values(R.DATE):
        assert R.parse_date(R.format(R.DATE, day, D.DAY)) == day
    lo, hi = int(D.days_from_civil(-999999, 1, 1)), int(D.days_from_civil(9999999, 12, 31))
    for unit in (R.S, R.MS, R.US, R.NS):
        for v in R.edge_values(R.TIMESTAMP, unit):
            if lo <= v // (86400 * R.PER_SECOND[unit]) <= hi:
                assert R.parse_timestamp(R.format(R.TIMESTAMP, v, unit), unit) == v, (unit, v)
    for v in (0, 1):
        assert R.parse_bool(R.format(R.BOOL, v)) == bool(v)


def test_the_generators_cover_both_outcomes():
    for kind in range(4):
        got = [R.parse(kind, t) for t in R.branch_cases(kind) + R.long_rows(kind) + R.random_cases(kind, 500, 9)]
        assert any(g is None for g in got) and sum(g is not None for g in got) >= 50, kind
    assert {len(t) for t in R.long_rows(R.INT)} >= {R.SHORT_ROW - 1, R.SHORT_ROW, R.SHORT_ROW + 1, 10000}
