"""rdf_datetime_fields / rdf_datetime_trunc / rdf_date_shift / rdf_date_diff on the MI355X: every result bit-exact against
tests/datetime_ref.py.  Every case runs over host and over device memory, twice each, and the four results are identical
bytes (values, bitmap, length, NULL count).  NULL rows hold 0 and the bits past `length` in a bitmap's last byte are 0, as
rdf_unary writes them.

Shapes are the smallest at which each part of the kernels can go wrong: lengths around one bitmap byte (8), one lane row
(64), one wave tile (512) and one block tile (2048), chunks behind odd element / bit offsets (which also decide between the
16-byte and the element loads), and 200 003 rows in seven unequal chunks, one of a single row and one empty, with 10 % NULLs.

Bounds worked out here, not taken from the code under test: none — integer results are compared for equality."""
import functools

import numpy as np
import pytest

import datetime_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WAVE_TILE, TILE = 512, 2048          # kDtWaveTile, kCsTile: rows of one wave's and one block's tile
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, WAVE_TILE - 1, WAVE_TILE, WAVE_TILE + 1, TILE - 1, TILE, TILE + 1]
OFFSETS = [0, 1, 3, 7, 9, 13, 64]
BIG = 200_003
CUTS = [1, 2049, 2049, 40_511, 100_000, 163_840]   # seven chunks: 1 row, 2048, EMPTY, 38 462, 59 489, 63 840, 36 163
FIELDS8 = ["year", "quarter", "month", "day_of_month", "day_of_week", "day_of_year", "week_of_year", "hour"]
REST = ["minute", "second", "date"]
STORAGES = [(unit, dt) for unit in (R.S, R.MS, R.US, R.NS) for dt in (A.I64, A.I32)] + [(R.DAY, A.I32)]
IDS = [f"{'s ms us ns day'.split()[u]}-{'i64' if dt == A.I64 else 'i32'}" for u, dt in STORAGES]
NP = {A.I32: np.int32, A.I64: np.int64}


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


# ---------------------------------------------------------------- plumbing
def to_device(x):
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def split(x, valid=None, cuts=(), offsets=None, dtype=None):
    bounds = [0] + [c for c in cuts if c <= len(x)] + [len(x)]
    return [A.HostArray.from_numpy(x[a:b], None if valid is None else valid[a:b], offset=offsets[i % len(offsets)] if offsets else 0, dtype=dtype)
            for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]


def chunks_of_lengths(x, valid, dtype):
    """x cut into chunks of LENGTHS (repeated while rows last), chunk i behind offset OFFSETS[i % 7]."""
    cuts, at = [], 0
    while at < len(x):
        for n in LENGTHS:
            at += n
            cuts.append(min(at, len(x)))
    return split(x, valid, cuts[:-1], OFFSETS, dtype)


def out_bytes(o):
    """(values bytes, bitmap bytes | None, length, NULL count) of one output chunk, wherever it lives."""
    n = o.length
    if isinstance(o, A.HostArray):
        vals, bits = o.values[:n], o.validity
    else:
        t, v = o.keep
        vals = t.cpu().numpy().view(A.NP_OF[o.dtype])[:n]
        bits = v.cpu().numpy() if v is not None else None
    return vals.tobytes(), None if bits is None else bits[:(n + 7) // 8].tobytes(), n, o.null_count


def four_ways(call, chunk_lists):
    """call(*lists) over host memory and over device memory, twice each: identical bytes; -> [(values, valid mask | None)] per chunk
    (a call with several outputs: a list of those)."""
    dev = [None if c is None else [to_device(a) for a in c] for c in chunk_lists]
    runs = [call(*chunk_lists), call(*dev), call(*chunk_lists), call(*dev)]
    nested = len(runs[0]) > 0 and isinstance(runs[0][0], list)
    flat = [[o for per in r for o in per] if nested else list(r) for r in runs]
    sig = [[out_bytes(o) for o in r] for r in flat]
    assert all(s == sig[0] for s in sig[1:]), "host / device / repeated runs differ"

    def view(o):
        vals, bits, n, nulls = out_bytes(o)
        v = np.frombuffer(vals, dtype=A.NP_OF[o.dtype])
        m = None if bits is None else A.unpack_bits(np.frombuffer(bits, dtype=np.uint8), 0, n)
        if bits is not None and n % 8:
            assert bits[-1] >> (n % 8) == 0, "bits past the length are 0"
        assert nulls == (0 if m is None else int(n - m.sum()))
        return v, m
    return [[view(o) for o in per] for per in runs[0]] if nested else [view(o) for o in runs[0]]


def expect(got, chunks, want, ok=None, also_valid=None, what=""):
    """got: [(values, mask)] per chunk; want: the reference over the concatenated rows; rows that are NULL hold 0."""
    at = 0
    assert len(got) == len(chunks)
    for i, ((v, m), ch) in enumerate(zip(got, chunks)):
        n = ch.length
        valid = ch.valid_mask()
        if also_valid is not None:
            valid = valid & also_valid[i].valid_mask()
        if ok is not None:
            valid = valid & ok[at:at + n]
        assert len(v) == n, what
        if m is None:
            assert valid.all(), what
        else:
            assert np.array_equal(m, valid), (what, i)
        w = np.where(valid, want[at:at + n], 0).astype(v.dtype)
        if not np.array_equal(v, w):
            bad = np.flatnonzero(v != w)[:5]
            raise AssertionError(f"{what} chunk {i}: rows {bad}: got {v[bad]}, expected {w[bad]}, inputs {ch.to_numpy()[bad]}")
        at += n


def logical(chunks):
    return np.concatenate([np.zeros(0, dtype=np.int64)] + [c.to_numpy().astype(np.int64) for c in chunks])


# ---------------------------------------------------------------- values
@functools.lru_cache(maxsize=None)
def era_days():
    """All 146 097 days of the era 2000-03-01 .. 2400-02-29, the same era moved to a negative and to a far-positive one, the Int32
    extremes, 0 and -1, the century rules and the turns of 2004..2032."""
    base = np.arange(R.d(2000, 3, 1), R.d(2400, 2, 29) + 1, dtype=np.int64)
    return np.concatenate([base, base - 9000 * R.ERA_DAYS, base + 14000 * R.ERA_DAYS, R.edge_days()])


@functools.lru_cache(maxsize=None)
def values_of(unit, dtype, n=9000):
    """A column of `unit` in `dtype` storage: the edge days scaled to the unit with a time of day, -1, 0, the type's extremes,
    and random values over the type's full range (Int64 seconds / milliseconds: the day number wraps)."""
    rng = np.random.default_rng(100 + 10 * unit + dtype)
    info = np.iinfo(NP[dtype])
    if unit == R.DAY:
        v = np.concatenate([R.edge_days(), rng.integers(info.min, info.max, 6000, endpoint=True)])
    else:
        v = np.concatenate([R.scaled(R.edge_days(), unit, rng), R.scaled(R.edge_days(), unit), [-1, 0, 1, info.min, info.max, info.min + 1, info.max - 1],
                            rng.integers(info.min, info.max, 6000, endpoint=True)])
        v = v[(v >= info.min) & (v <= info.max)]
    v = v.astype(np.int64)
    v = np.concatenate([v, rng.integers(info.min, info.max, max(0, n - len(v)), endpoint=True)])[:n]
    return rng.permutation(v)


# ---------------------------------------------------------------- fields
@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("unit,dtype", STORAGES, ids=IDS)
def test_fields_every_unit_storage_length_and_offset(api, unit, dtype, nulls):
    v = values_of(unit, dtype)
    valid = np.random.default_rng(3).uniform(size=len(v)) > 0.2 if nulls else None
    chunks = chunks_of_lengths(v, valid, dtype)
    assert {c.length for c in chunks} >= set(LENGTHS) and {c.offset for c in chunks} == set(OFFSETS)
    for names in (FIELDS8, REST):
        got = four_ways(lambda c: api.datetime_fields(c, unit, names), [chunks])
        for f, per in zip(names, got):
            expect(per, chunks, R.field(v, unit, f), what=f"{f} unit {unit}")


def test_fields_exhaustive_era_sweep_as_dates(api):
    v = era_days()
    chunks = split(v, None, [146_097, 2 * 146_097, 3 * 146_097 - 5], [0, 3, 1, 13], A.I32)
    for names in (FIELDS8, REST):
        got = four_ways(lambda c: api.datetime_fields(c, R.DAY, names), [chunks])
        for f, per in zip(names, got):
            expect(per, chunks, R.field(v, R.DAY, f), what=f"{f} of dates")


@pytest.mark.parametrize("unit", [R.S, R.MS, R.US, R.NS])
def test_fields_era_sweep_scaled_to_every_unit(api, unit):
    rng = np.random.default_rng(unit)
    v = np.concatenate([R.scaled(era_days(), unit, rng), [-1, R.I64_MIN, R.I64_MAX]]).astype(np.int64)
    chunks = split(v, None, [100_000, 300_001], [1, 0, 9], A.I64)
    got = four_ways(lambda c: api.datetime_fields(c, unit, FIELDS8), [chunks])
    for f, per in zip(FIELDS8, got):
        expect(per, chunks, R.field(v, unit, f), what=f"{f} unit {unit}")
    m1 = [A.HostArray.from_numpy(np.array([-1], dtype=np.int64))]                   # 1969-12-31 23:59:59 in every unit
    got = api.datetime_fields(m1, unit, ["year", "month", "day_of_month", "hour", "minute", "second"])
    assert [int(g[0].to_numpy()[0]) for g in got] == [1969, 12, 31, 23, 59, 59]


@functools.lru_cache(maxsize=None)
def big(unit):
    """200 003 random Int64 over the full range (the day number of seconds / milliseconds wraps), 10 % NULLs, seven unequal chunks."""
    rng = np.random.default_rng(40 + unit)
    v = rng.integers(R.I64_MIN, R.I64_MAX, BIG, endpoint=True)
    valid = rng.uniform(size=BIG) > 0.1
    return v, valid, split(v, valid, CUTS, OFFSETS, A.I64)


@pytest.mark.parametrize("unit", [R.S, R.MS, R.US, R.NS])
def test_the_big_column_eight_fields_equal_eight_calls_and_hour_equals_rdf_hour(api, unit):
    v, valid, chunks = big(unit)
    assert sorted(c.length for c in chunks)[:2] == [0, 1] and len(chunks) == 7
    got = four_ways(lambda c: api.datetime_fields(c, unit, FIELDS8), [chunks])
    dev = [to_device(c) for c in chunks]
    together = api.datetime_fields(dev, unit, FIELDS8)
    for f, per, per_dev in zip(FIELDS8, got, together):
        expect(per, chunks, R.field(v, unit, f), what=f"{f} unit {unit}")
        single = api.datetime_fields(dev, unit, [f])[0]
        assert [out_bytes(o) for o in single] == [out_bytes(o) for o in per_dev], f     # one read, eight outputs = eight calls
    hour = api.hour(chunks, unit)
    mine = api.datetime_fields(chunks, unit, ["hour"])[0]
    assert [out_bytes(o) for o in hour] == [out_bytes(o) for o in mine]


@pytest.mark.parametrize("unit,dtype", STORAGES, ids=IDS)
def test_hour_field_is_rdf_hour_byte_for_byte(api, unit, dtype):
    v = values_of(unit, dtype)
    for valid in (None, np.random.default_rng(4).uniform(size=len(v)) > 0.3):
        chunks = chunks_of_lengths(v, valid, dtype)
        assert [out_bytes(o) for o in api.hour(chunks, unit)] == [out_bytes(o) for o in api.datetime_fields(chunks, unit, ["hour"])[0]]


# ---------------------------------------------------------------- trunc
@pytest.mark.parametrize("unit,dtype", STORAGES, ids=IDS)
def test_trunc_every_level(api, unit, dtype):
    v = values_of(unit, dtype)
    valid = np.random.default_rng(5).uniform(size=len(v)) > 0.2
    chunks = chunks_of_lengths(v, valid, dtype)
    bits = 32 if dtype == A.I32 else 64
    for level in R.LEVELS:
        if not R.trunc_allowed(unit, level):
            with pytest.raises(A.RdfError) as ei:
                api.datetime_trunc(chunks, unit, level)
            assert ei.value.status == A.RDF_INVALID_ARGUMENT
            continue
        got = four_ways(lambda c: api.datetime_trunc(c, unit, level), [chunks])
        expect(got, chunks, R.trunc(v, unit, level, bits), what=f"trunc {level} unit {unit}")


def test_trunc_of_the_era_sweep_and_the_big_columns(api):
    v = era_days()
    chunks = split(v, None, [146_097, 2 * 146_097], [7, 0, 64], A.I32)
    for level in ("year", "quarter", "month", "week", "day"):
        expect(four_ways(lambda c: api.datetime_trunc(c, R.DAY, level), [chunks]), chunks, R.trunc(v, R.DAY, level, 32), what=f"trunc {level} of dates")
    for unit in (R.S, R.NS):
        w, valid, big_chunks = big(unit)
        for level in ("quarter", "week", "minute"):
            expect(four_ways(lambda c: api.datetime_trunc(c, unit, level), [big_chunks]), big_chunks, R.trunc(w, unit, level), what=f"trunc {level} unit {unit}")


@pytest.mark.parametrize("unit", [R.S, R.MS, R.US, R.NS])
def test_trunc_day_is_date_times_units_per_day(api, unit):
    """Wherever the day number fits Int32 (every microsecond / nanosecond value; seconds / milliseconds inside year +-5.8 million:
    beyond, DATE wraps by the domain rule while trunc(DAY) = v - floor_mod(v, units per day) does not)."""
    rng = np.random.default_rng(50 + unit)
    upd = R.UNITS_PER_DAY[unit]
    lo, hi = max(R.I64_MIN, R.I32_MIN * upd), min(R.I64_MAX, R.I32_MAX * upd)
    v = np.concatenate([rng.integers(lo, hi, 5000, endpoint=True), [lo, hi, -1, 0]]).astype(np.int64)
    chunks = split(v, None, [2048, 2049], [3, 0, 1], A.I64)
    date = logical(api.datetime_fields(chunks, unit, ["date"])[0])
    day = logical(api.datetime_trunc(chunks, unit, "day"))
    assert np.array_equal(day, date * upd)


# ---------------------------------------------------------------- shift and diff
@pytest.mark.parametrize("unit,dtype", STORAGES, ids=IDS)
def test_shift_every_operation_scalar_and_column_amounts(api, unit, dtype):
    v = values_of(unit, dtype)
    rng = np.random.default_rng(6)
    valid = rng.uniform(size=len(v)) > 0.2
    chunks = chunks_of_lengths(v, valid, dtype)
    for op, k in (("days", 45), ("days", -400_000), ("days", R.I32_MAX), ("months", 1), ("months", -25), ("months", 1_000_003), ("months", R.I32_MIN),
                  ("last_day", 0), ("next_day", 1), ("next_day", 3), ("next_day", 7)):
        want, _ = R.shift(v, unit, op, k)
        expect(four_ways(lambda c: api.date_shift(c, unit, op, k), [chunks]), chunks, want, what=f"{op} {k} unit {unit}")
    # per-row amounts with NULLs of their own; next_day: weekdays outside 1..7 are NULL rows
    for op, amounts in (("days", rng.integers(R.I32_MIN, R.I32_MAX, len(v), endpoint=True)), ("months", rng.integers(-30_000, 30_000, len(v))),
                        ("next_day", rng.integers(-1, 9, len(v), endpoint=True))):
        kvalid = rng.uniform(size=len(v)) > 0.15
        kchunks = [A.HostArray.from_numpy(amounts[a:a + c.length], kvalid[a:a + c.length], offset=OFFSETS[(i + 3) % 7], dtype=A.I32)
                   for i, (c, a) in enumerate(zip(chunks, np.cumsum([0] + [c.length for c in chunks[:-1]])))]
        want, ok = R.shift(v, unit, op, amounts)
        got = four_ways(lambda c, k: api.date_shift(c, unit, op, k), [chunks, kchunks])
        expect(got, chunks, want, ok=ok, also_valid=kchunks, what=f"{op} by column unit {unit}")
        if op == "next_day":
            assert not ok.all() and sum(int(m.sum()) for _, m in got) == int((valid & kvalid & ok).sum())
    with pytest.raises(A.RdfError):                                   # per-row weekdays can fail: the output needs a bitmap
        dense = [A.HostArray.from_numpy(np.arange(5, dtype=NP[dtype]))]
        api.date_shift(dense, unit, "next_day", [A.HostArray.from_numpy(np.arange(5, dtype=np.int32))], outs=[A.HostArray.empty_out(A.I32, 5, False)])


def test_shift_of_the_era_sweep_and_round_trips(api):
    v = era_days()
    chunks = split(v, None, [146_097, 2 * 146_097], [1, 0, 9], A.I32)
    for op, k in (("months", 1), ("months", -13), ("last_day", 0), ("next_day", 2), ("days", -1)):
        expect(four_ways(lambda c: api.date_shift(c, R.DAY, op, k), [chunks]), chunks, R.shift(v, R.DAY, op, k)[0], what=f"{op} {k} of dates")
    # date_add(k) then date_diff against the input gives k; add_months(+m) then (-m) returns wherever the day is <= 28
    for k in (1, -1, 365, -146_097, 1_000_000):
        moved = api.date_shift(chunks, R.DAY, "days", k)
        assert (logical(api.date_diff(moved, R.DAY, chunks, R.DAY)) == k).all()
    dom = R.field(v, R.DAY, "day_of_month")
    for m in (1, 7, 12, 4801):
        there = api.date_shift(chunks, R.DAY, "months", m)
        back = logical(api.date_shift(there, R.DAY, "months", -m))
        inside = (dom <= 28) & (np.abs(v) < R.I32_MAX - 200_000)      # (the outermost months of Int32 wrap)
        assert np.array_equal(back[inside], v[inside])


@pytest.mark.parametrize("ua,da", STORAGES, ids=IDS)
def test_diff_every_pair_of_units_and_storages(api, ua, da):
    a = values_of(ua, da)
    rng = np.random.default_rng(7)
    va = rng.uniform(size=len(a)) > 0.2
    ca = chunks_of_lengths(a, va, da)
    for ub, db in STORAGES:
        b = values_of(ub, db, len(a))
        vb = rng.uniform(size=len(a)) > 0.2
        cb = [A.HostArray.from_numpy(b[s:s + c.length], vb[s:s + c.length], offset=OFFSETS[(i + 2) % 7], dtype=db)
              for i, (c, s) in enumerate(zip(ca, np.cumsum([0] + [c.length for c in ca[:-1]])))]
        run = four_ways if ub in (ua, R.DAY) else (lambda call, lists: [(o.to_numpy(), o.valid_mask()) for o in call(*lists)])
        got = run(lambda x, y: api.date_diff(x, ua, y, ub), [ca, cb])
        expect(got, ca, R.diff(a, ua, b, ub), also_valid=cb, what=f"diff {ua}/{da} - {ub}/{db}")


def test_diff_of_the_big_columns(api):
    a, va, ca = big(R.NS)
    b, vb, cb = big(R.S)
    expect(four_ways(lambda x, y: api.date_diff(x, R.NS, y, R.S), [ca, cb]), ca, R.diff(a, R.NS, b, R.S), also_valid=cb, what="diff ns - s")


# ---------------------------------------------------------------- the results as keys
def test_year_of_the_big_column_as_group_by_key(api):
    v, valid, chunks = big(R.NS)
    years = api.datetime_fields([to_device(c) for c in chunks], R.NS, ["year"])[0]
    keys, _, counts = api.groupby_agg([years], None, "count", 4096,
                                      outs=([api._window_out(A.I32, 4098, True, True)], api._window_out(A.I64, 4098, True, False), api._window_out(A.I64, 4098, True, False)))
    k, kvalid = four_view(keys[0])
    c, _ = four_view(counts)
    want_k, want_c = np.unique(R.field(v, R.NS, "year")[valid], return_counts=True)
    got = dict(zip(k[kvalid].tolist(), c[kvalid].tolist()))
    assert got == dict(zip(want_k.tolist(), want_c.tolist()))
    assert c[~kvalid].sum() in (0, int((~valid).sum()))               # the NULL group, where the operator reports one


def four_view(o):
    vals, bits, n, _ = out_bytes(o)
    v = np.frombuffer(vals, dtype=A.NP_OF[o.dtype])
    return v, (np.ones(n, dtype=bool) if bits is None else A.unpack_bits(np.frombuffer(bits, dtype=np.uint8), 0, n))
