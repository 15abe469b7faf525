"""The executable model of rdf_utf8_parse / rdf_utf8_format: pure Python over bytes, written from the rules of the header's
"text to values and back" section and DESIGN.md, not from the kernels.  The calendar is tests/datetime_ref.py's.

Rules (each place they knowingly differ from Spark 3 is listed in DESIGN.md):

  trimming    the CAST grammars trim the bytes 0x09-0x0D, 0x1C-0x1F and 0x20 from both ends and nothing else; a pattern trims
              nothing and has to consume the whole row
  INT         [+-]? digit+ ( '.' digit* )?   the fraction is checked and dropped; a value outside the dtype is NULL; unsigned:
              '-0' is 0, any other negative NULL; no digit before the '.' is NULL (Spark gives 0 for some such forms)
  BOOL        t true y yes 1 / f false n no 0, ASCII case-insensitive
  DATE        [+-]? y{4,7} ( - m{1,2} ( - d{1,2} ( [ T] anything )? )? )?   missing month / day = 1; an impossible date, or a
              day number outside Int32, is NULL
  TIMESTAMP   the date part; optionally, after a full date, [ T] h{1,2} : m{1,2} ( : s{1,2} ( . digit* )? )?; optionally a zone
              Z | UTC | [+-] h{1,2} ( : m{1,2} )? of at most 18:00, subtracted; digits beyond the unit dropped; a value outside
              Int64 is NULL; a time without a date is NULL
  patterns    see compile_pattern / parse_pattern / format_pattern
  year rule   0..9999 four digits; above '+' and the digits; below 0 '-' and at least four digits
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import datetime_ref as D  # noqa: E402

BOOL, INT, DATE, TIMESTAMP = range(4)
KINDS = ("bool", "int", "date", "timestamp")
S, MS, US, NS, DAY = D.S, D.MS, D.US, D.NS, D.DAY
# rdf_dtype codes of the eight integer types, and their (bits, signed)
I8, I16, I32, I64, U8, U16, U32, U64 = range(8)
INT_DTYPES = (I8, I16, I32, I64, U8, U16, U32, U64)
NP_DTYPES = {I8: np.int8, I16: np.int16, I32: np.int32, I64: np.int64, U8: np.uint8, U16: np.uint16, U32: np.uint32, U64: np.uint64}
WS = frozenset(list(range(0x09, 0x0E)) + list(range(0x1C, 0x21)))
MONTHS = ("Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec")
WEEKDAYS = ("Mon", "Tue", "Wed", "Thu", "Fri", "Sat", "Sun")
MAX_TOKENS, MAX_LITERAL, MAX_ROW_BYTES = 32, 64, 256
SHORT_ROW = 256         # kUtf8ShortRow: a longer row of a CAST grammar is taken by its wave
LDS_BYTES = 8192        # kTcLdsBytes: a tile whose byte span is at most this is staged in LDS
PER_SECOND = {S: 1, MS: 10 ** 3, US: 10 ** 6, NS: 10 ** 9}


def int_limits(dtype):
    bits = 8 << (dtype & 3)
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if dtype < U8 else (0, (1 << bits) - 1)


@functools.lru_cache(maxsize=1 << 16)
def _days(y, m, d):
    return int(D.days_from_civil(y, m, d))


@functools.lru_cache(maxsize=1 << 16)
def _civil(day):
    y, m, d = D.civil_from_days(day)
    return int(y), int(m), int(d)


def _month_len(y, m):
    return int(D.last_day_of_month(y, m))


def _is_digit(c):
    return 0x30 <= c <= 0x39


def trim(b):
    i, j = 0, len(b)
    while i < j and b[i] in WS:
        i += 1
    while j > i and b[j - 1] in WS:
        j -= 1
    return b[i:j]


# ------------------------------------------------------------------------------------------------------------------ parse
def parse_int(b, dtype=I64):
    b = trim(bytes(b))
    if not b:
        return None
    neg, i = False, 0
    if b[0] in b"+-":
        neg, i = b[0] == 0x2D, 1
    j = i
    while j < len(b) and _is_digit(b[j]):
        j += 1
    if j == i:
        return None
    digits = b[i:j].lstrip(b"0")
    mag = int(digits or b"0") if len(digits) <= 20 else 10 ** 21   # (beyond every dtype; int() refuses thousands of digits)
    if j < len(b):
        if b[j] != 0x2E or not all(_is_digit(c) for c in b[j + 1:]):
            return None
    lo, hi = int_limits(dtype)
    v = -mag if neg else mag
    return v if lo <= v <= hi else None


def parse_bool(b):
    t = trim(bytes(b)).lower()   # (bytes.lower() changes ASCII letters only)
    if t in (b"t", b"true", b"y", b"yes", b"1"):
        return True
    if t in (b"f", b"false", b"n", b"no", b"0"):
        return False
    return None


def _take_digits(b, i, least, most):
    j = i
    while j < len(b) and j - i < most and _is_digit(b[j]):
        j += 1
    return (int(b[i:j]), j) if j - i >= least else None


def _date_part(b):
    """-> (year, month, day, stage, next index) or None; the date is checked."""
    i, neg = 0, False
    if b[:1] in (b"+", b"-"):
        neg, i = b[:1] == b"-", 1
    t = _take_digits(b, i, 4, 8)
    if t is None or t[1] - i > 7:
        return None
    y, i = (-t[0] if neg else t[0]), t[1]
    m = d = stage = 1
    if b[i:i + 1] == b"-":
        t = _take_digits(b, i + 1, 1, 2)
        if t is None:
            return None
        (m, i), stage = t, 2
        if b[i:i + 1] == b"-":
            t = _take_digits(b, i + 1, 1, 2)
            if t is None:
                return None
            (d, i), stage = t, 3
    if not 1 <= m <= 12 or not 1 <= d <= _month_len(y, m):
        return None
    return y, m, d, stage, i


def parse_date(b):
    b = trim(bytes(b))
    p = _date_part(b)
    if p is None:
        return None
    y, m, d, stage, i = p
    if i < len(b) and not (stage == 3 and b[i] in b" T"):
        return None
    day = _days(y, m, d)
    return day if D.I32_MIN <= day <= D.I32_MAX else None


def _compose(secs, nanos, unit):
    v = secs * PER_SECOND[unit] + nanos // (10 ** 9 // PER_SECOND[unit])
    return v if D.I64_MIN <= v <= D.I64_MAX else None


def parse_timestamp(b, unit=S):
    b = trim(bytes(b))
    p = _date_part(b)
    if p is None:
        return None
    y, mo, d, stage, i = p
    hh = mi = ss = nanos = zone = 0
    if i < len(b) and b[i] in b" T":
        if stage != 3:
            return None
        t = _take_digits(b, i + 1, 1, 2)
        if t is None or b[t[1]:t[1] + 1] != b":":
            return None
        hh, i = t
        t = _take_digits(b, i + 1, 1, 2)
        if t is None:
            return None
        mi, i = t
        if b[i:i + 1] == b":":
            t = _take_digits(b, i + 1, 1, 2)
            if t is None:
                return None
            ss, i = t
            if b[i:i + 1] == b".":
                j = i + 1
                while j < len(b) and _is_digit(b[j]):
                    j += 1
                nanos = int((b[i + 1:j][:9] + b"000000000")[:9])
                i = j
        if hh > 23 or mi > 59 or ss > 59:
            return None
    if i < len(b):
        if b[i:i + 1] == b"Z":
            i += 1
        elif b[i:i + 3] == b"UTC":
            i += 3
        elif b[i] in b"+-":
            west = b[i] == 0x2D
            t = _take_digits(b, i + 1, 1, 2)
            if t is None:
                return None
            zh, i = t
            zm = 0
            if b[i:i + 1] == b":":
                t = _take_digits(b, i + 1, 1, 2)
                if t is None:
                    return None
                zm, i = t
            if zm > 59 or zh * 60 + zm > 18 * 60:
                return None
            zone = (zh * 3600 + zm * 60) * (-1 if west else 1)
        else:
            return None
        if i != len(b):
            return None
    return _compose(_days(y, mo, d) * 86400 + hh * 3600 + mi * 60 + ss - zone, nanos, unit)


# ---------------------------------------------------------------------------------------------------------------- patterns
class PatternError(ValueError):
    def __init__(self, what, pos):
        super().__init__(f"{what} at position {pos}")
        self.what, self.pos = what, pos


E_LETTER, E_RUN, E_QUOTE, E_TOKENS, E_LITERAL, E_EEE, E_AMPM, E_LONG, E_EMPTY = (
    "a letter that is no pattern letter", "a run length the letter does not take", "a quote that is not closed", "more than 32 tokens",
    "more than 64 literal bytes", "EEE is taken by format only", "a clock hour (h) needs 'a'", "a row could pass 256 bytes", "an empty pattern")
_RUNS = {"y": {4: 13, 2: 2}, "M": {1: 2, 2: 2, 3: 3}, "d": {1: 2, 2: 2}, "D": {1: 3, 3: 3}, "H": {1: 2, 2: 2}, "h": {1: 2, 2: 2}, "a": {1: 2},
         "m": {1: 2, 2: 2}, "s": {1: 2, 2: 2}, "S": {k: k for k in range(1, 10)}, "E": {3: 3}}


def compile_pattern(p, for_parse):
    """-> [(letter, run) | ("lit", bytes)]; raises PatternError(what, position)."""
    p = p.encode() if isinstance(p, str) else bytes(p)
    if not p:
        raise PatternError(E_EMPTY, 0)
    toks, nlit, width, first_h, has_a = [], 0, 0, -1, False

    def lit(c, at):
        nonlocal nlit, width
        if nlit >= MAX_LITERAL:
            raise PatternError(E_LITERAL, at)
        if not toks or toks[-1][0] != "lit":
            if len(toks) >= MAX_TOKENS:
                raise PatternError(E_TOKENS, at)
            toks.append(("lit", b""))
        toks[-1] = ("lit", toks[-1][1] + bytes([c]))
        nlit += 1
        width += 1

    i, n = 0, len(p)
    while i < n:
        c = p[i]
        if c == 0x27:
            if p[i + 1:i + 2] == b"'":
                lit(0x27, i)
                i += 2
                continue
            start, i, closed = i, i + 1, False
            while i < n:
                if p[i] == 0x27:
                    if p[i + 1:i + 2] == b"'":
                        lit(0x27, i)
                        i += 2
                        continue
                    closed, i = True, i + 1
                    break
                lit(p[i], i)
                i += 1
            if not closed:
                raise PatternError(E_QUOTE, start)
            continue
        ch = chr(c)
        if not (ch.isascii() and ch.isalpha()):
            lit(c, i)
            i += 1
            continue
        j = i
        while j < n and p[j] == c:
            j += 1
        if ch not in _RUNS:
            raise PatternError(E_LETTER, i)
        if j - i not in _RUNS[ch]:
            raise PatternError(E_RUN, i)
        if ch == "E" and for_parse:
            raise PatternError(E_EEE, i)
        if len(toks) >= MAX_TOKENS:
            raise PatternError(E_TOKENS, i)
        toks.append((ch, j - i))
        width += _RUNS[ch][j - i]
        if ch == "h" and first_h < 0:
            first_h = i
        has_a |= ch == "a"
        i = j
    if first_h >= 0 and not has_a:
        raise PatternError(E_AMPM, first_h)
    if not for_parse and width > MAX_ROW_BYTES:
        raise PatternError(E_LONG, n - 1)
    return toks


def parse_pattern(toks, b):
    """-> (day number, second of the day, nanoseconds) or None."""
    b = bytes(b)
    f = {}

    def put(name, v):
        if name in f and f[name] != v:
            return False
        f[name] = v
        return True

    i = 0
    for t, run in toks:
        if t == "lit":
            if b[i:i + len(run)] != run:
                return None
            i += len(run)
            continue
        if t == "y" and run == 4:
            neg = sign = False
            if b[i:i + 1] in (b"+", b"-"):
                neg, sign, i = b[i:i + 1] == b"-", True, i + 1
            r = _take_digits(b, i, 4, 8 if sign else 4)
            if r is None or r[1] - i > 7:
                return None
            ok, i = put("year", -r[0] if neg else r[0]), r[1]
        elif t == "y":
            r = _take_digits(b, i, 2, 2)
            if r is None:
                return None
            ok, i = put("year", 2000 + r[0]), r[1]
        elif t == "M" and run == 3:
            name = b[i:i + 3].decode("latin-1")
            if name not in MONTHS:
                return None
            ok, i = put("month", MONTHS.index(name) + 1), i + 3
        elif t == "a":
            if b[i:i + 2] not in (b"AM", b"PM"):
                return None
            ok, i = put("pm", int(b[i:i + 2] == b"PM")), i + 2
        elif t == "S":
            r = _take_digits(b, i, run, run)
            if r is None:
                return None
            ok, i = put("nanos", r[0] * 10 ** (9 - run)), r[1]
        else:
            name = {"M": "month", "d": "day", "D": "doy", "H": "hour", "h": "hour12", "m": "minute", "s": "second"}[t]
            most = 3 if t == "D" else 2
            r = _take_digits(b, i, (most if run > 1 else 1), most)
            if r is None:
                return None
            ok, i = put(name, r[0]), r[1]
        if not ok:
            return None
    if i != len(b):
        return None
    y = f.get("year", 1970)
    if "doy" in f:
        leap = _month_len(y, 2) == 29
        if not 1 <= f["doy"] <= (366 if leap else 365):
            return None
        day = _days(y, 1, 1) + f["doy"] - 1
        if "month" in f or "day" in f:
            if not D.I32_MIN <= day <= D.I32_MAX:
                return None
            _, cm, cd = _civil(day)
            if ("month" in f and cm != f["month"]) or ("day" in f and cd != f["day"]):
                return None
    else:
        m, d = f.get("month", 1), f.get("day", 1)
        if not 1 <= m <= 12 or not 1 <= d <= _month_len(y, m):
            return None
        day = _days(y, m, d)
    hour = f.get("hour", 0)
    if "hour12" in f:
        if not 1 <= f["hour12"] <= 12:
            return None
        h = f["hour12"] % 12 + 12 * f.get("pm", 0)
        if "hour" in f and f["hour"] != h:
            return None
        hour = h
    elif "pm" in f and "hour" in f and (hour >= 12) != bool(f["pm"]):
        return None
    minute, second = f.get("minute", 0), f.get("second", 0)
    if hour > 23 or minute > 59 or second > 59:
        return None
    return day, hour * 3600 + minute * 60 + second, f.get("nanos", 0)


def parse(kind, b, unit=S, dtype=I64, pattern=None):
    """One row of rdf_utf8_parse: the value (bool / int) or None.  pattern: compiled tokens."""
    if pattern is not None:
        r = parse_pattern(pattern, b)
        if r is None:
            return None
        day, sod, nanos = r
        if kind == DATE:
            return day if D.I32_MIN <= day <= D.I32_MAX else None
        return _compose(day * 86400 + sod, nanos, unit)
    return (parse_bool(b) if kind == BOOL else parse_int(b, dtype) if kind == INT else parse_date(b) if kind == DATE else parse_timestamp(b, unit))


# ------------------------------------------------------------------------------------------------------------------ format
def format_year(y):
    return b"-%04d" % -y if y < 0 else (b"+%d" % y if y > 9999 else b"%04d" % y)


def _split(v, unit):
    """-> (year, month, day, day number, second of day, nanoseconds).  The day number is NOT wrapped to Int32 (rdf_datetime_fields
    wraps it): text has to round-trip, so every Int64 value prints its true date, with years of up to twelve digits."""
    v = int(v)
    day = v if unit == DAY else v // (86400 * PER_SECOND[unit])
    sod = 0 if unit == DAY else v // PER_SECOND[unit] % 86400
    nanos = 0 if unit in (DAY, S) else (int(v) % PER_SECOND[unit]) * (10 ** 9 // PER_SECOND[unit])
    return _civil(day) + (day, sod, nanos)


def format_temporal(v, unit, kind):
    y, m, d, _, sod, nanos = _split(v, unit)
    out = format_year(y) + b"-%02d-%02d" % (m, d)
    if kind == TIMESTAMP:
        out += b" %02d:%02d:%02d" % (sod // 3600, sod // 60 % 60, sod % 60)
        if nanos:
            out += b"." + (b"%09d" % nanos).rstrip(b"0")
    return out


def format_pattern(toks, v, unit):
    y, m, d, day, sod, nanos = _split(v, unit)
    h, mi, s = sod // 3600, sod // 60 % 60, sod % 60
    out = b""
    for t, run in toks:
        if t == "lit":
            out += run
        elif t == "y":
            out += format_year(y) if run == 4 else b"%02d" % (y % 100)
        elif t == "M":
            out += MONTHS[m - 1].encode() if run == 3 else b"%0*d" % (run, m)
        elif t == "d":
            out += b"%0*d" % (run, d)
        elif t == "D":
            out += b"%0*d" % (run, int(D.day_of_year(day)))
        elif t == "H":
            out += b"%0*d" % (run, h)
        elif t == "h":
            out += b"%0*d" % (run, h % 12 or 12)
        elif t == "a":
            out += b"PM" if h >= 12 else b"AM"
        elif t == "m":
            out += b"%0*d" % (run, mi)
        elif t == "s":
            out += b"%0*d" % (run, s)
        elif t == "S":
            out += (b"%09d" % nanos)[:run]
        else:
            out += WEEKDAYS[int(D.weekday(day))].encode()
    return out


def format(kind, v, unit=S, pattern=None):  # noqa: A001
    """One row of rdf_utf8_format (v is not NULL).  pattern: compiled tokens."""
    if kind == BOOL:
        return b"true" if v else b"false"
    if kind == INT:
        return b"%d" % int(v)
    return format_pattern(pattern, v, unit) if pattern is not None else format_temporal(v, unit, kind)


# ----------------------------------------------------------------------------------------------------------- known answers
# (kind, text, unit, dtype, pattern, expected)
KNOWN_PARSE = [
    (INT, b"12.7", S, I64, None, 12), (INT, b"-12.7", S, I64, None, -12), (INT, b"12.", S, I64, None, 12), (INT, b" 42", S, I64, None, 42),
    (INT, b"128", S, I8, None, None), (INT, b"-128", S, I8, None, -128), (INT, b"9223372036854775808", S, I64, None, None),
    (INT, b"-9223372036854775808", S, I64, None, -2 ** 63), (INT, b"-0", S, U8, None, 0), (INT, b"-1", S, U8, None, None),
    (INT, b"", S, I64, None, None), (INT, b"   ", S, I64, None, None), (INT, b"-", S, I64, None, None), (INT, b".5", S, I64, None, None),
    (INT, b"1e3", S, I64, None, None), (INT, b"0x1f", S, I64, None, None), (INT, b"1 2", S, I64, None, None),
    (INT, "１２".encode(), S, I64, None, None), (INT, b"00012", S, I64, None, 12),
    (DATE, b"2020-02-29", S, I32, None, 18321), (DATE, b"2020-2-9", S, I32, None, 18301), (DATE, b"2020", S, I32, None, 18262),
    (DATE, b"2020-03", S, I32, None, 18322), (DATE, b"2020-02-29 junk", S, I32, None, 18321), (DATE, b"20-02-29", S, I32, None, None),
    (DATE, b"+10000-01-01", S, I32, None, 2932897), (DATE, b"2019-02-29", S, I32, None, None),
    (TIMESTAMP, b"2020-02-29 12:34:56.789", MS, I64, None, 1582979696789), (TIMESTAMP, b"12:34:56", S, I64, None, None),
    (TIMESTAMP, b"2016-04-08", S, I64, "yyyy-MM-dd", 1460073600),
    (TIMESTAMP, b"2016-13-08", S, I64, "yyyy-MM-dd", None), (TIMESTAMP, b"2019 366", S, I64, "yyyy DDD", None),
    (TIMESTAMP, b"2020 366", S, I64, "yyyy DDD", 1609372800), (TIMESTAMP, b"24", S, I64, "HH", None),
]
# (kind, value, unit, pattern, expected)
KNOWN_FORMAT = [
    (DATE, 18321, DAY, "EEE, d MMM yyyy", b"Sat, 29 Feb 2020"), (TIMESTAMP, 0, S, "yyyy-MM-dd HH:mm:ss", b"1970-01-01 00:00:00"),
    (DATE, 18321, DAY, None, b"2020-02-29"), (TIMESTAMP, 1582979696789, MS, None, b"2020-02-29 12:34:56.789"),
    (TIMESTAMP, 1582979696000, MS, None, b"2020-02-29 12:34:56"), (DATE, 2932897, DAY, None, b"+10000-01-01"),
    (INT, -2 ** 63, S, None, b"-9223372036854775808"), (BOOL, 1, S, None, b"true"), (BOOL, 0, S, None, b"false"),
]


# ---------------------------------------------------------------------------------------------------------------- generators
def _around(text):
    """A text behind and before every trimmed byte and its untrimmed neighbours."""
    out = []
    for c in (0x08, 0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x0E, 0x1B, 0x1C, 0x1D, 0x1E, 0x1F, 0x20, 0x21, 0xA0):
        out += [bytes([c]) + text, text + bytes([c]), bytes([c]) + text + bytes([c])]
    out.append(b"\xc2\xa0" + text)
    out.append("　".encode() + text)
    return out


def branch_cases(kind, dtype=I64):
    """Every grammar branch of the kind's CAST and every way out of it."""
    if kind == BOOL:
        words = [b"t", b"true", b"y", b"yes", b"1", b"f", b"false", b"n", b"no", b"0"]
        out = list(words) + [w.upper() for w in words] + [w.title() for w in words] + [b"tru", b"truee", b"ye", b"2", b"", b" ", b"t rue", b"fals\xc3\xa9", b"on"]
        return out + _around(b"true") + _around(b"0")
    if kind == INT:
        out = [b"0", b"7", b"+7", b"-7", b"007", b"-007", b"+", b"-", b"+-1", b"--1", b"1.", b"1.0", b"1.999", b"-1.5", b".5", b"-.5", b"1.5.5", b"1.a", b"1e3",
               b"0x1f", b"1 2", b"1,000", "１２".encode(), b"", b" ", b"-0", b"+0", b"-0.9", b"0.9", b"1\x00", b"\x001"]
        for dt in INT_DTYPES:
            lo, hi = int_limits(dt)
            for v in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1):
                out += [b"%d" % v, b"%d.9" % v, b"000%d" % v if v >= 0 else b"-000%d" % -v]
        out += [b"18446744073709551615", b"18446744073709551616", b"99999999999999999999", b"100000000000000000000", b"-18446744073709551616"]
        return out + _around(b"42") + _around(b"-1.5")
    dates = [b"2020-02-29", b"2020-2-9", b"2020", b"2020-03", b"2020-02-29 junk", b"2020-02-29Tjunk", b"2020-02-29x", b"20-02-29", b"202-02-29", b"+10000-01-01",
             b"2019-02-29", b"2020-00-10", b"2020-13-10", b"2020-01-00", b"2020-01-32", b"2020-04-31", b"1900-02-29", b"2000-02-29", b"-0001-01-01", b"+2020-01-01",
             b"12345678-01-01", b"1234567-01-01", b"+1234567-12-31", b"5881580-07-11", b"5881580-07-12", b"-5877641-06-23", b"-5877641-06-22", b"2020-", b"2020-03-",
             b"2020-123", b"2020-03-123", b"2020 junk", b"2020-03 junk", b"2020T", b"", b" ", b"-", b"0000-01-01", b"9999-12-31", b"0001-1-1", b"2020/02/29", b"2020-02-29 ",
             b"+-2020", b"2020--02"]
    if kind == DATE:
        return dates + _around(b"2020-02-29") + _around(b"2020")
    times = [b" 12:34:56.789", b"T12:34:56.789", b" 1:2:3", b" 1:2", b" 12:34", b" 12:34:56", b" 12:34:56.", b" 12:34:56.1", b" 12:34:56.123456789", b" 12:34:56.1234567891234",
             b" 24:00:00", b" 23:60:00", b" 23:59:60", b" 23:59:59", b" 00:00:00", b" 12", b" 12:", b" 12:34:", b" 123:00", b" 12:345", b" 12:34:567", b" 12:34:56.x", b" 12:34:56 ",
             b" x", b"T", b" "]
    zones = [b"Z", b"UTC", b"+1", b"+01", b"-1", b"+01:30", b"+1:3", b"-08:00", b"+18:00", b"-18:00", b"+18:01", b"+19", b"+01:60", b"+", b"+:30", b"+01:", b"+001", b"+01:300",
             b"z", b"utc", b"GMT", b" UTC", b"Europe/Paris", b"ZZ", b"UTCx", b"+01x"]
    out = list(dates)
    for t in times:
        out.append(b"2020-02-29" + t)
    for z in zones:
        out += [b"2020-02-29 12:34:56" + z, b"2020-02-29 12:34:56.5" + z, b"2020-02-29 12:34" + z, b"2020-02-29" + z, b"2020" + z, b"2020-02" + z]
    out += [b"2020 12:34", b"2020-02 12:34", b"12:34:56", b"T12:34:56", b"-292277022657-01-27 08:29:52", b"+9999999-12-31 23:59:59.999999999",
            b"-9999999-01-01 00:00:00", b"2262-04-11 23:47:16.854775807", b"2262-04-11 23:47:16.854775808", b"1677-09-21 00:12:43.145224192", b"1677-09-21 00:12:43.145224191",
            b"1969-12-31 23:59:59.999", b"1969-12-31 23:59:59.9999999999"]
    return out + _around(b"2020-02-29 12:34:56") + _around(b"2020-02-29")


# 64 + 8 * (13 + 9) + 3 + 2 + 3 + 2 + 2 + 2 + 2 = 256 bytes for a year of twelve digits and a sign (Int64 seconds reach it): the row cap exactly
CAP_PATTERN = "'" + "=" * 64 + "'" + "yyyySSSSSSSSS" * 8 + "DDDddMMMHHmmssa"
PATTERNS_PARSE = ["yyyy-MM-dd", "yyyy-MM-dd HH:mm:ss", "yyyy-MM-dd'T'HH:mm:ss.SSS", "d/M/yy", "dd MMM yyyy", "yyyy DDD", "yyyy D", "hh:mm a", "h:m:s a", "yyyyMMdd",
                  "yyyy-MM-dd HH:mm:ss.SSSSSSSSS", "MM/dd/yyyy hh:mm:ss a", "yyyy-MM-dd DDD", "HH 'o''clock'", "yyyy-MM-dd HH hh a", "S", "yyyy yyyy", "H a"]
PATTERNS_FORMAT = PATTERNS_PARSE + ["EEE, d MMM yyyy", "EEE", "yy", "'" + "x" * 40 + "'yyyy-MM-dd HH:mm:ss.SSSSSSSSS EEE MMM DDD D yy a hh h", "''", "'a''b'", CAP_PATTERN]
# (pattern, for_parse, what, position)
PATTERN_ERRORS = [
    ("", True, E_EMPTY, 0), ("yyyy-MM-dd x", True, E_LETTER, 11), ("yyy", True, E_RUN, 0), ("yyyyy", True, E_RUN, 0), ("y", True, E_RUN, 0), ("MMMM", True, E_RUN, 0),
    ("ddd", True, E_RUN, 0), ("DD", True, E_RUN, 0), ("DDDD", True, E_RUN, 0), ("HHH", True, E_RUN, 0), ("aa", True, E_RUN, 0), ("mmm", True, E_RUN, 0),
    ("sss", True, E_RUN, 0), ("SSSSSSSSSS", True, E_RUN, 0), ("EE", False, E_RUN, 0), ("EEEE", False, E_RUN, 0), ("yyyy 'abc", True, E_QUOTE, 5), ("EEE", True, E_EEE, 0),
    ("yyyy EEE", True, E_EEE, 5), ("hh:mm", True, E_AMPM, 0), ("HH h", False, E_AMPM, 3), ("yyyy-MM-dd G", False, E_LETTER, 11), ("Q", True, E_LETTER, 0),
    ("-".join(["d"] * 17), True, E_TOKENS, 32), ("'" + "x" * 65 + "'", True, E_LITERAL, 65), ("." * 65, False, E_LITERAL, 64),
    (CAP_PATTERN + "H", False, E_LONG, len(CAP_PATTERN)),
]


def _rand_text(kind, rng, unit, dtype, pattern):
    """One valid text of the kind."""
    if kind == BOOL:
        w = [b"t", b"true", b"y", b"yes", b"1", b"f", b"false", b"n", b"no", b"0"][rng.integers(10)]
        return bytes(c - 32 if 97 <= c <= 122 and rng.integers(2) else c for c in w)
    if kind == INT:
        lo, hi = int_limits(dtype)
        span = int(rng.integers(1, hi.bit_length() + 2))
        v = int(rng.integers(0, 2 ** 62)) % (1 << span)
        v = max(lo, min(hi + 1, -v if rng.integers(2) else v))
        t = b"%d" % v
        r = rng.integers(8)
        return t + b".%d" % rng.integers(1000) if r == 0 else b"+" + t if r == 1 and v >= 0 else b" " + t if r == 2 else t
    day = int(rng.integers(-800000, 3000000)) if rng.integers(4) == 0 else int(rng.integers(-30000, 60000))
    if kind == TIMESTAMP:   # (the unit's Int64 holds fewer days than the calendar)
        lim = D.I64_MAX // (86400 * PER_SECOND[unit]) - 1
        day = max(-lim, min(lim, day))
    v = day if kind == DATE else day * 86400 * PER_SECOND[unit] + int(rng.integers(0, 86400 * PER_SECOND[unit]))
    u = DAY if kind == DATE else unit
    if pattern is not None:
        return format_pattern(pattern, v, u)
    t = format_temporal(v, u, kind)
    if kind == TIMESTAMP and rng.integers(4) == 0:
        t += [b"Z", b"UTC", b"+01:00", b"-8"][rng.integers(4)]
    return t


def random_cases(kind, n, seed, unit=S, dtype=I64, pattern=None):
    """n rows: valid text, valid text with one byte changed, and noise, about a third each."""
    rng = np.random.default_rng(seed)
    alphabet = b"0123456789-+:. TZ" + bytes(range(256))
    out = []
    for _ in range(n):
        r = rng.integers(3)
        if r == 2:
            out.append(bytes(alphabet[rng.integers(len(alphabet))] for _ in range(rng.integers(0, 24))))
            continue
        t = bytearray(_rand_text(kind, rng, unit, dtype, pattern))
        if r == 1 and t:
            t[rng.integers(len(t))] = alphabet[rng.integers(len(alphabet))]
        out.append(bytes(t))
    return out


def long_rows(kind):
    """Rows around and far beyond kUtf8ShortRow: padding of white space or zeros, a 10 000-digit fraction, noise."""
    core = {BOOL: b"true", INT: b"-12345", DATE: b"2020-02-29", TIMESTAMP: b"2020-02-29 12:34:56.789"}[kind]
    out = []
    for n in (SHORT_ROW - 1, SHORT_ROW, SHORT_ROW + 1, 10000):
        pad = n - len(core)
        out += [b" " * pad + core, core + b"\t" * pad, b" " * (pad // 2) + core + b" " * (pad - pad // 2), b" " * (pad - 1) + core + b"x", b"x" + b" " * (pad - 1) + core]
        if kind == INT:
            out += [b"-" + b"0" * (n - 6) + b"12345", b"0" * n, b"0" * (n - 1) + b"x", b"+" + b"0" * (n - 4) + b"128", b" " * 10 + b"0" * (n - 10 - 22) + b"18446744073709551616.5",
                    b"7." + b"9" * (n - 2), b"7." + b"9" * (n - 3) + b"x", b"7." + b"9" * (n // 2) + b" " + b"9" * (n - n // 2 - 3), b"1" * n]
        if kind in (DATE, TIMESTAMP):
            out += [b"2020-02-29 " + b"j" * (n - 11), b"2020-02-29T" + b"j" * (n - 11), b"2020-02-29x" + b"j" * (n - 11), b"2020-02 " + b" " * (n - 9) + b"x", b"2020-02" + b" " * (n - 8) + b"x",
                    b"2020-02-29 12:34:56." + b"7" * (n - 20), b"2020-02-29 12:34:56." + b"7" * (n - 21) + b"Z", b"2020-02-29 12:34:56." + b"7" * (n - 21) + b"x"]
    rng = np.random.default_rng(77 + kind)
    out.append(bytes(rng.integers(0, 256, size=10000, dtype=np.uint8)))
    out.append(bytes(rng.choice(np.frombuffer(b"0123456789 .-", dtype=np.uint8), size=10000)))
    return out


def edge_values(kind, unit=S, dtype=I64):
    """Values for format and the round trip: every dtype's limits, the edge days, and for timestamps the ends of the year range."""
    if kind == BOOL:
        return [0, 1]
    if kind == INT:
        lo, hi = int_limits(dtype)
        cand = {lo, lo + 1, -1, 0, 1, hi - 1, hi} | {v for k in range(1, 20) for v in (10 ** k - 1, 10 ** k, -(10 ** k) + 1, -(10 ** k))}
        return sorted(v for v in cand if lo <= v <= hi)
    days = [int(x) for x in D.edge_days()]
    if kind == DATE:
        return days
    upd = 86400 * PER_SECOND[unit]
    lo_day, hi_day = _days(-999999, 1, 1), _days(9999999, 12, 31)
    out = []
    for day in days + [lo_day, hi_day]:
        if not lo_day <= day <= hi_day:
            continue
        for t in (0, 1, upd - 1, 45296 * PER_SECOND[unit] + PER_SECOND[unit] // 8 * (unit != S), 12 * 3600 * PER_SECOND[unit] + 500 * (PER_SECOND[unit] // 1000)):
            v = day * upd + t
            if D.I64_MIN <= v <= D.I64_MAX:
                out.append(v)
    return out + [D.I64_MIN, D.I64_MAX, 0, -1]


# ------------------------------------------------------------------------------------------- the table of the host program
def _hex(b):
    return "x" + bytes(b).hex()


def write_case_table(path, rows_per_kind=100000):
    """The table tests/cpp/test_textconv_host.cpp reads, one case a line:
         P kind unit dtype pattern text ok value      (pattern and text as 'x' + hex; value as a signed decimal)
         F kind unit dtype pattern value text
       At least rows_per_kind rows per kind and direction.  -> {("P" | "F", kind): rows}"""
    counts = {}
    with open(path, "w") as f:
        def emit_parse(kind, unit, dtype, pat, texts):
            toks = compile_pattern(pat, True) if pat is not None else None
            for t in texts:
                v = parse(kind, t, unit, dtype, toks)
                f.write(f"P {kind} {unit} {dtype} {_hex((pat or '').encode())} {_hex(t)} {int(v is not None)} {int(v or 0)}\n")
            counts[("P", kind)] = counts.get(("P", kind), 0) + len(texts)

        def emit_format(kind, unit, dtype, pat, values):
            toks = compile_pattern(pat, False) if pat is not None else None
            for v in values:
                f.write(f"F {kind} {unit} {dtype} {_hex((pat or '').encode())} {int(v)} {_hex(format(kind, v, unit, toks))}\n")
            counts[("F", kind)] = counts.get(("F", kind), 0) + len(values)

        rng = np.random.default_rng(4242)
        for kind in (BOOL, INT, DATE, TIMESTAMP):
            per = rows_per_kind
            if kind == INT:
                for dt in INT_DTYPES:
                    emit_parse(kind, S, dt, None, branch_cases(kind) + long_rows(kind) + random_cases(kind, per // 8, 100 + dt, dtype=dt))
                    lo, hi = int_limits(dt)
                    vals = edge_values(kind, dtype=dt) + [int(x) for x in rng.integers(max(lo, -2 ** 62), min(hi, 2 ** 62), size=per // 8, endpoint=True)]
                    emit_format(kind, S, dt, None, vals)
            elif kind == BOOL:
                emit_parse(kind, S, 10, None, branch_cases(kind) + long_rows(kind) + random_cases(kind, per, 200))
                emit_format(kind, S, 10, None, [int(x) for x in rng.integers(0, 2, size=per)])
            else:
                units = (S,) if kind == DATE else (S, MS, US, NS)
                share = per // (len(units) * 2)
                for u in units:
                    emit_parse(kind, u, I32 if kind == DATE else I64, None, branch_cases(kind) + long_rows(kind) + random_cases(kind, share, 300 + 10 * kind + u, unit=u))
                    for k, pat in enumerate(PATTERNS_PARSE):
                        toks = compile_pattern(pat, True)
                        emit_parse(kind, u, I32 if kind == DATE else I64, pat, random_cases(kind, share // len(PATTERNS_PARSE) + 1, 400 + 20 * kind + u + 100 * k, unit=u, pattern=toks))
                funits = (DAY, S, MS, US, NS)
                share = per // (len(funits) * 2)
                for u in funits:
                    if u == DAY:
                        vals = edge_values(DATE) + [int(x) for x in rng.integers(D.I32_MIN, D.I32_MAX, size=share)]
                    else:
                        vals = edge_values(TIMESTAMP, u) + [int(x) for x in rng.integers(D.I64_MIN, D.I64_MAX, size=share // 2)] + \
                            [int(x) for x in rng.integers(-10 ** 9, 4 * 10 ** 9, size=share // 2) * PER_SECOND[u] + rng.integers(0, PER_SECOND[u], size=share // 2)]
                    dt = I32 if u == DAY else I64
                    emit_format(kind, u, dt, None, vals)
                    for k, pat in enumerate(PATTERNS_FORMAT):
                        emit_format(kind, u, dt, pat, vals[k::len(PATTERNS_FORMAT)] + vals[:8])
    return counts
