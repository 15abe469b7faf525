"""The exact reference of the date and time functions (rdf_datetime_fields / rdf_datetime_trunc / rdf_date_shift /
rdf_date_diff): vectorised numpy Int64 with its own floor division, civil conversion, ISO week and month clamp, written
independently of rust_dataframe_amd/csrc/rdf_datetime.h (the ISO week is "the year of this week's Thursday", month lengths
are differences of day numbers, floor division is numpy's).  tests/test_datetime_ref.py holds it to datetime, numpy
datetime64, pyarrow and Spark's documented examples.

Domain rule, as the ABI states it: the day number of a value is floor_div(value, units per day) in Int64, WRAPPED to Int32;
every result that can leave its type is wrapped explicitly (wrap32 / wrap_storage) the way the ABI says.

`python tests/datetime_ref.py` rewrites tests/golden/datetime_cases.npz, the table tests/cpp/test_datetime_host.cpp checks
the header against (kept as a compressed Int64 matrix; tests/test_datetime_host.py writes it out as the text the program
reads, one row per line)."""
import os

import numpy as np

S, MS, US, NS, DAY = range(5)
UNITS = (S, MS, US, NS, DAY)
UNITS_PER_DAY = {S: 86400, MS: 86400 * 10 ** 3, US: 86400 * 10 ** 6, NS: 86400 * 10 ** 9, DAY: 1}
UNITS_PER_SECOND = {S: 1, MS: 10 ** 3, US: 10 ** 6, NS: 10 ** 9}
FIELDS = ("year", "quarter", "month", "day_of_month", "day_of_week", "day_of_year", "week_of_year", "hour", "minute", "second", "date")
LEVELS = ("year", "quarter", "month", "week", "day", "hour", "minute", "second")
SHIFTS = ("days", "months", "last_day", "next_day")
ERA_DAYS = 146097
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def i64(x):
    return np.asarray(x, dtype=np.int64)


def wrap32(x):
    """Int64 -> the Int32 with the same low 32 bits (returned as Int64 values in Int32's range)."""
    return (i64(x).view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).astype(np.int64)


def day_number(v, unit):
    """floor_div(value, units per day) in Int64, wrapped to Int32."""
    v = i64(v)
    return wrap32(v if unit == DAY else np.floor_divide(v, UNITS_PER_DAY[unit]))


def second_of_day(v, unit):
    v = i64(v)
    if unit == DAY:
        return np.zeros(v.shape, dtype=np.int64)
    return np.mod(np.floor_divide(v, UNITS_PER_SECOND[unit]), 86400)


def civil_from_days(day):
    """Proleptic Gregorian (year, month, day), astronomical years, of day numbers counted from 1970-01-01."""
    z = i64(day) + 719468
    era = np.floor_divide(z, ERA_DAYS)
    doe = z - era * ERA_DAYS
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    d = doy - (153 * mp + 2) // 5 + 1
    m = np.where(mp < 10, mp + 3, mp - 9)
    y = yoe + era * 400 + (m <= 2)
    return y, m, d


def days_from_civil(y, m, d):
    y, m, d = i64(y), i64(m), i64(d)
    y = y - (m <= 2)
    era = np.floor_divide(y, 400)
    yoe = y - era * 400
    doy = (153 * np.where(m > 2, m - 3, m + 9) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * ERA_DAYS + doe - 719468


def weekday(day):
    """Monday = 0 .. Sunday = 6; 1970-01-01 is a Thursday."""
    return np.mod(i64(day) + 3, 7)


def day_of_year(day):
    y, _, _ = civil_from_days(day)
    return i64(day) - days_from_civil(y, 1, 1) + 1


def iso_week(day):
    """The ISO-8601 week: that of the year this week's Thursday lies in."""
    day = i64(day)
    thursday = day - weekday(day) + 3
    y, _, _ = civil_from_days(thursday)
    return (thursday - days_from_civil(y, 1, 1)) // 7 + 1


def last_day_of_month(y, m):
    y, m = i64(y), i64(m)
    ny, nm = np.where(m == 12, y + 1, y), np.where(m == 12, 1, m + 1)
    return days_from_civil(ny, nm, 1) - days_from_civil(y, m, 1)


def field(v, unit, name):
    """One field of rdf_datetime_fields as Int32."""
    day = day_number(v, unit)
    sod = second_of_day(v, unit)
    y, m, d = civil_from_days(day)
    r = {"year": y, "quarter": (m - 1) // 3 + 1, "month": m, "day_of_month": d, "day_of_week": np.mod(weekday(day) + 1, 7) + 1,
         "day_of_year": day_of_year(day), "week_of_year": iso_week(day), "hour": sod // 3600, "minute": sod // 60 % 60, "second": sod % 60,
         "date": day}[name]
    return r.astype(np.int32)


def wrap_storage(u, bits):
    """uint64 bit patterns -> the signed storage value (Int32 or Int64) with the same low bits."""
    u = np.asarray(u, dtype=np.uint64)
    return u.view(np.int64) if bits == 64 else (u & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def trunc_allowed(unit, level):
    return not (unit == DAY and level in ("hour", "minute", "second"))


def trunc(v, unit, level, bits=64):
    """rdf_datetime_trunc: same unit and storage out, wrapping modulo 2^bits."""
    v = i64(v)
    upd = UNITS_PER_DAY[unit]
    if level in ("year", "quarter", "month", "week"):
        day = day_number(v, unit)
        y, m, _ = civil_from_days(day)
        first = {"year": lambda: days_from_civil(y, 1, 1), "quarter": lambda: days_from_civil(y, (m - 1) // 3 * 3 + 1, 1),
                 "month": lambda: days_from_civil(y, m, 1), "week": lambda: day - weekday(day)}[level]()
        return wrap_storage(first.view(np.uint64) * np.uint64(upd), bits)
    if unit == DAY:
        assert level == "day"
        return wrap_storage(v.view(np.uint64), bits)
    step = {"day": upd, "hour": 3600 * UNITS_PER_SECOND[unit], "minute": 60 * UNITS_PER_SECOND[unit], "second": UNITS_PER_SECOND[unit]}[level]
    return wrap_storage(v.view(np.uint64) - np.mod(v, step).astype(np.uint64), bits)


def shift(v, unit, op, amount):
    """rdf_date_shift -> (Int32 day numbers, ok): ok is False where a next_day weekday is outside 1..7 (a NULL row)."""
    day = day_number(v, unit)
    amount = np.broadcast_to(i64(amount), day.shape)
    ok = np.ones(day.shape, dtype=bool)
    if op == "days":
        r = day + amount
    elif op == "last_day":
        y, m, d = civil_from_days(day)
        r = days_from_civil(y, m, last_day_of_month(y, m))
    elif op == "next_day":
        ok = (amount >= 1) & (amount <= 7)
        target = np.mod(amount + 5, 7)                           # 1 = Sunday -> Monday-based 6
        r = day + np.mod(target - weekday(day) + 6, 7) + 1       # strictly later: 1..7 days ahead
    else:
        y, m, d = civil_from_days(day)
        months = y * 12 + (m - 1) + amount
        ny, nm = np.floor_divide(months, 12), np.mod(months, 12) + 1
        r = days_from_civil(ny, nm, np.minimum(d, last_day_of_month(ny, nm)))
    return np.where(ok, wrap32(r), 0).astype(np.int32), ok


def diff(end, end_unit, start, start_unit):
    return wrap32(day_number(end, end_unit) - day_number(start, start_unit)).astype(np.int32)


# ---------------------------------------------------------------- interesting values
def d(y, m, dd):
    return int(days_from_civil(y, m, dd))


def edge_days():
    """Day numbers at which a calendar can go wrong: both Int32 extremes, 0 and -1, the century rules, every year shape's turn."""
    days = [I32_MIN, I32_MIN + 1, I32_MAX - 1, I32_MAX, 0, -1, 1]
    for y in (1600, 1900, 2000, 2100):
        days += [d(y, 2, 28), d(y, 2, 28) + 1, d(y, 3, 1)]
    for y in range(2004, 2033):                                   # all 14 calendar shapes, the 53-week years
        days += list(range(d(y, 12, 25), d(y + 1, 1, 7) + 1))
    return np.array(sorted(set(days)), dtype=np.int64)


def common_days():
    """edge_days() without the Int32 extremes: the ones datetime and pyarrow can take."""
    e = edge_days()
    return e[np.abs(e) < 10 ** 6]


def scaled(days, unit, rng=None):
    """Day numbers as values of `unit` that keep their day number (plus a time of day when rng is given); day numbers whose
    values do not fit Int64 are dropped."""
    days, upd = i64(days), UNITS_PER_DAY[unit]
    days = days[(days >= I64_MIN // upd + 1) & (days <= I64_MAX // upd - 1)]
    tod = 0 if rng is None or unit == DAY else rng.integers(0, upd, size=len(days), dtype=np.int64)
    return days * upd + tod


# ---------------------------------------------------------------- the table of tests/golden/datetime_cases.npz
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datetime_cases.npz")


def golden_values(unit):
    rng = np.random.default_rng(20260 + unit)
    days = edge_days()
    extra = rng.integers(I32_MIN, I32_MAX, size=60, dtype=np.int64)
    if unit == DAY:
        return np.concatenate([days, extra])
    vals = [scaled(days, unit), scaled(days[::3], unit, rng), rng.integers(I64_MIN, I64_MAX, size=150, dtype=np.int64, endpoint=True),
            scaled(extra, unit, rng), np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], dtype=np.int64)]
    return np.concatenate(vals)


def golden_table():
    """Int64 [rows, 28]: unit value | the 11 fields | the 8 truncations (0 where the level is refused) | days months weekday |
    the 4 shifts.  Storage is Int64 except for RDF_TIME_DAY (Int32)."""
    blocks = []
    for unit in UNITS:
        v = golden_values(unit)
        rng = np.random.default_rng(77 + unit)
        bits = 32 if unit == DAY else 64
        cols = [np.full(len(v), unit, dtype=np.int64), v]
        cols += [field(v, unit, f).astype(np.int64) for f in FIELDS]
        cols += [trunc(v, unit, lv, bits).astype(np.int64) if trunc_allowed(unit, lv) else np.zeros(len(v), dtype=np.int64) for lv in LEVELS]
        k_days = rng.integers(-40000, 40000, size=len(v), dtype=np.int64)
        k_days[::7] = rng.integers(I32_MIN, I32_MAX, size=len(k_days[::7]), dtype=np.int64, endpoint=True)
        k_months = rng.integers(-1300, 1300, size=len(v), dtype=np.int64)
        k_months[::5] = rng.integers(I32_MIN, I32_MAX, size=len(k_months[::5]), dtype=np.int64, endpoint=True)
        k_wd = rng.integers(1, 7, size=len(v), dtype=np.int64, endpoint=True)
        cols += [k_days, k_months, k_wd]
        cols += [shift(v, unit, op, k)[0].astype(np.int64) for op, k in zip(SHIFTS, (k_days, k_months, 0, k_wd))]
        blocks.append(np.stack(cols, axis=1))
    return np.concatenate(blocks)


def write_table_text(path, table=None):
    """The committed table (or `table`) as the text tests/cpp/test_datetime_host.cpp reads: 28 numbers per line."""
    table = np.load(GOLDEN)["cases"] if table is None else table
    with open(path, "w") as f:
        f.write("# unit value  11 fields  8 truncations  days months weekday  4 shifts\n")
        f.writelines(" ".join(str(int(x)) for x in row) + "\n" for row in table)


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, cases=golden_table())
    print(f"{GOLDEN}: {len(golden_table())} rows")
