"""rdf_sort_to_indices on the MI355X at 65 536 to 200 000 rows, where its planner (os_column_passes, csrc/rdf_sort_plan.h,
csrc/rdf_sort_map.h) has a choice, held to the exact numpy model tests/sort_ref.py on every route.  Every case asserts two
things: the index array equals the model's, element for element, and the route note of rdf_last_kernel says what the case
was built for (include/rdf_mi355x.h has the vocabulary) — no case goes without a route expectation.

Inputs come from tests/sort_cases.py: integer keys (bucket << R) | low with the rows of every bucket counted out, Float64
columns whose specials sit on or off the rows the planner's sample reads.  The plan of every Float64 input was confirmed on
the CPU with os_plan_f64 / os_top_plan before its first run on a device.

Measured on an MI355X, seconds per test function summed over its cases, host arrays and the model included (the slowest
single case in brackets); the whole module, 44 cases, in 6.1 s with the library's start-up:

    test_bucket_size_ladder_every_lds_class_edge                    0.17
    test_each_launch_shape_of_the_lds_finish                        0.18  (0.03)
    test_late_fallback_after_two_top_passes                         0.06  (0.03)
    test_remaining_bits_edges                                       0.24  (0.03)
    test_route_edge_controls                                        0.12
    test_chunked_input_with_offsets                                 0.03
    test_every_dtype_between_65536_and_70000_rows                   0.52  (0.06)
    test_f64_value_buckets_then_lds_finish                          0.20  (0.02)
    test_f64_sentinel_met_by_the_sample_three_passes_then_bytes     1.62  (0.82: a 2^24-entry bounds table per sort)
    test_f64_plans_refused                                          0.26
    test_f64_linear_map_without_the_sample                          0.08  (0.04)
    test_all_null_and_single_value_columns                          0.05
"""
import re

import numpy as np
import pytest

import sort_cases as S
import sort_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


@pytest.fixture(autouse=True)
def _default_options():
    yield
    lib.set_option("sort_msd", 1)
    lib.set_option("sort_sample", 1)


# ---------------------------------------------------------------- the route note

def routes():
    """the entries of "(sort routes: a; b)" as dicts: {"kind": first word, key: value, ...}, in the order the columns were sorted"""
    name = lib.last_kernel()
    m = re.search(r" \(sort routes: (.*)\)$", name)
    assert m, name
    out = []
    for entry in m.group(1).split("; "):
        words = entry.split(" ")
        d = {"kind": words[0], "then": "then" in words}
        for w in words[1:]:
            if "=" in w:
                k, v = w.split("=")
                d[k] = v if k == "map" else int(v)
        out.append(d)
    assert name.startswith("os_scatter_kernel")
    assert ("os_local_kernel" in name) == any(d["kind"] == "top+lds" for d in out), name
    return out


def want(entry, kind, **fields):
    assert entry["kind"] == kind, (entry, kind, fields)
    for k, v in fields.items():
        assert entry.get(k) == v, (k, entry, fields)


def chunked(values, valid=None, dtype=None, cuts=(), offsets=None):
    bounds = [0] + list(cuts) + [len(values)]
    out = []
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        off = offsets[i] if offsets else 0
        out.append(A.HostArray.from_numpy(values[a:b], valid=None if valid is None else valid[a:b], offset=off, dtype=dtype))
    return out


def run(api, cols, desc):
    """-> the route entries, after holding the order to the model"""
    got = api.sort_to_indices(cols, desc).to_numpy()
    note = routes()
    exp = R.sort_to_indices(cols, desc)
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (lib.last_kernel(), desc, len(bad), bad[:5], got[bad[:5]], exp[bad[:5]])
    return note


def three_ways(api, main, check, tag, cuts=(), directions=(False, True)):
    """`main` sorted as the only column (identity order in, idx_in == nullptr), as column 0 in front of an Int16 column (it
    is sorted second: idx_in set), and behind an Int8 ties column (a later stable pass runs over its result); ascending and
    descending.  check(entry, descending) holds the main column's route entry."""
    n = sum(c.length for c in main)
    rng = np.random.default_rng(n)
    minor = chunked(rng.integers(-300, 300, n).astype(np.int16), dtype=A.I16, cuts=cuts)
    ties = chunked(rng.integers(0, 3, n).astype(np.int8), dtype=A.I8, cuts=cuts)
    for d in directions:
        note = run(api, [main], [d])
        assert len(note) == 1, (tag, note)
        check(note[0], d)
        note = run(api, [main, minor], [d, not d])
        assert len(note) == 2, (tag, note)
        want(note[0], "bytes", passes=2, nulls=0)
        check(note[1], d)
        note = run(api, [ties, main], [not d, d])
        assert len(note) == 2, (tag, note)
        check(note[0], d)
        want(note[1], "bytes", passes=1, nulls=0)


def int_column(seed, ladder, R_, npdt, n=None, nulls=0.0, cuts=(), offsets=None):
    rng = np.random.default_rng(seed)
    keys = S.bucket_keys(rng, S.bucket_sizes(rng, ladder, n), R_)
    vals, valid = S.with_nulls(rng, S.as_dtype(keys, npdt, R_ + 12), nulls)
    return chunked(vals, valid, A.dtype_code(npdt), cuts, offsets)


# ---------------------------------------------------------------- integer keys, buckets counted out

def test_bucket_size_ladder_every_lds_class_edge(api):
    """Buckets of exactly 0, 1, 2, 255 .. 4096 rows in one input: both sides of every len_lo / len_hi edge of
    launch_os_local's three launches and the one-row shortcut; every bucket holds ties (stability).  U64, R = 36."""
    for nulls in (0.0, 0.01):
        col = int_column(1, S.LADDER, 36, np.uint64, nulls=nulls)
        three_ways(api, col, lambda e, d: want(e, "top+lds", B=12, top=2, map="bits", nulls=int(nulls > 0), bucket=4096, lds=4096), "ladder")


@pytest.mark.parametrize("largest,lds", [(512, 512), (1024, 1024), (4096, 4096), (256, 256), (513, 1024), (1025, 2048)])
def test_each_launch_shape_of_the_lds_finish(api, largest, lds):
    """The largest bucket at 512 rows (one launch), 1024 (two), 4096 (three) — and one row past a class edge."""
    ladder = [s for s in S.LADDER if s <= largest] + ([largest] if largest not in S.LADDER else [])
    col = int_column(2, ladder, 36, np.int64, n=68_662)      # (the filler grows to keep the rows of the whole ladder's input)
    three_ways(api, col, lambda e, d: want(e, "top+lds", B=12, top=2, map="bits", nulls=0, bucket=largest, lds=lds), largest)


@pytest.mark.parametrize("nulls", [0.0, 0.01])
def test_late_fallback_after_two_top_passes(api, nulls):
    """One bucket of 4097 rows: the two top passes are spent, os_bounds finds the bucket, the byte passes sort the column
    from the order the top passes left — with NULLs, from a NULL tail that two passes leave in the current buffers."""
    ladder = S.LADDER[:-1] + [4097]
    col = int_column(3, ladder, 36, np.uint64, nulls=nulls)
    three_ways(api, col, lambda e, d: want(e, "top+bytes", B=12, top=2, map="bits", bucket=4097, then=True, passes=6, nulls=int(nulls > 0)), "late")


@pytest.mark.parametrize("R_,npdt", [(13, np.int64), (13, np.int32), (13, np.uint32), (20, np.uint32), (20, np.int32), (36, np.int64), (52, np.int64), (52, np.uint64)])
def test_remaining_bits_edges(api, R_, npdt):
    """R = 13 (25 bits vary: the narrowest keys the route takes), 20 (a 4-byte type's whole range), 36, and 52, where the LDS
    word (R bits << 12 | place) is exactly 64 bits: Int64 from its minimum to its maximum, UInt64 across 2^63."""
    col = int_column(4 + R_, S.LADDER, R_, npdt, nulls=0.01 if R_ in (13, 52) else 0.0)
    if R_ == 52:
        v = np.concatenate([R.chunk_values(c)[R.chunk_valid(c)] for c in col])
        assert int(v.min()) == np.iinfo(npdt).min and int(v.max()) == np.iinfo(npdt).max
    three_ways(api, col, lambda e, d: want(e, "top+lds", B=12, top=2, map="bits", bucket=4096, lds=4096), (R_, npdt))


def test_route_edge_controls(api):
    """24 bits at 65 536 rows, 25 bits at 65 535 rows and sort_msd = 0 all take the byte passes."""
    col = int_column(30, [], 12, np.int64, n=65536)
    three_ways(api, col, lambda e, d: want(e, "bytes", passes=3, nulls=0), "24 bits")
    col = int_column(31, [], 13, np.int64, n=65535)
    three_ways(api, col, lambda e, d: want(e, "bytes", passes=4, nulls=0), "65535 rows")
    col = int_column(32, [], 13, np.int64, n=65536)
    three_ways(api, col, lambda e, d: want(e, "top+lds", B=12, top=2, bucket=16, lds=256), "65536 rows, 25 bits")
    col = int_column(33, S.LADDER, 52, np.uint64, nulls=0.01)
    lib.set_option("sort_msd", 0)
    three_ways(api, col, lambda e, d: want(e, "bytes", passes=8, nulls=1), "sort_msd 0")


def test_chunked_input_with_offsets(api):
    """Chunks of 65 536, 1, 0 and 4 099 rows, every chunk with a value offset and a validity bit offset of its own."""
    sizes = S.bucket_sizes(np.random.default_rng(40), S.LADDER, n=68947)      # + 1 % NULL rows = 69 636
    rng = np.random.default_rng(41)
    vals, valid = S.with_nulls(rng, S.as_dtype(S.bucket_keys(rng, sizes, 36), np.int64, 48), 0.01)
    assert len(vals) == 65536 + 1 + 4099
    cuts = (65536, 65537, 65537)
    col = chunked(vals, valid, A.I64, cuts, offsets=[3, 64, 5, 1])
    assert [c.length for c in col] == [65536, 1, 0, 4099]
    three_ways(api, col, lambda e, d: want(e, "top+lds", B=12, top=2, map="bits", nulls=1, bucket=4096, lds=4096), "chunks", cuts=cuts)


# ---------------------------------------------------------------- every dtype just above the threshold

SPECIALS32 = np.array([0x7FC00000, 0xFFC00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("dt", [A.I8, A.U8, A.I16, A.U16, A.F32, A.U32, A.I32, A.U64, A.I64])
def test_every_dtype_between_65536_and_70000_rows(api, dt):
    """One- and two-byte types: one or two byte passes; Float32 with -NaN, -inf, -0.0, +0.0, denormals, +inf, +NaN: four
    byte passes, never the top-bits route; the 4- and 8-byte integers at full range: top bits, then the LDS finish."""
    npdt = np.dtype(A.NP_OF[dt])
    rng = np.random.default_rng(50 + dt)
    n = int(rng.integers(65536, 70001))
    if npdt.kind == "f":
        v = (rng.normal(size=n) * 1e3).astype(np.float32)
        v[rng.integers(0, n, 600)] = SPECIALS32[rng.integers(0, len(SPECIALS32), 600)]
    else:
        info = np.iinfo(npdt)
        v = rng.integers(info.min, info.max, n, dtype=npdt, endpoint=True)
        v[:2] = [info.min, info.max]
    size = npdt.itemsize
    for nulls in (False, True):
        valid = None
        if nulls:
            valid = rng.uniform(size=n) >= 0.02
            valid[:2] = True
        col = chunked(v, valid, dt)
        if size <= 2 or npdt.kind == "f":
            check = lambda e, d: want(e, "bytes", passes=size, nulls=int(nulls))       # noqa: E731
        else:
            check = lambda e, d: want(e, "top+lds", B=12, top=2, map="bits", nulls=int(nulls), lds=256)   # noqa: E731
        three_ways(api, col, check, (dt, nulls))


# ---------------------------------------------------------------- Float64: routes pinned by what the sample sees

def f64_column(name, nulls=0.0):
    v = S.f64_case(name)
    valid = S.null_mask_off_sample(np.random.default_rng(60), len(v), nulls) if nulls else None
    return chunked(v, valid, A.F64)


def f64_ways(api, col, check, tag):
    """a Float64 column's plan depends on the rows its sample reads, so it is sorted where it is read in its original order:
    alone, and as the first-sorted (last) criterion behind a ties column; ascending and descending (`flip`)."""
    n = sum(c.length for c in col)
    ties = chunked(np.random.default_rng(n).integers(0, 3, n).astype(np.int8), dtype=A.I8)
    for d in (False, True):
        note = run(api, [col], [d])
        assert len(note) == 1, (tag, note)
        check(note[0])
        note = run(api, [ties, col], [not d, d])
        assert len(note) == 2, (tag, note)
        check(note[0])
        want(note[1], "bytes", passes=1, nulls=0)


@pytest.mark.parametrize("name,map_,lds", [("uniform", "flat", 256), ("normal", "segments", 256), ("lognormal", "segments", 256),
                                           ("outliers_unseen", "segments", 256), ("nonfinite_unseen", "flat", 1024)])
@pytest.mark.parametrize("nulls", [0.0, 0.01])
def test_f64_value_buckets_then_lds_finish(api, name, map_, lds, nulls):
    """Uniform: the flat map; normal, lognormal: segments (with tails); Normal(100, 3) with +-inf, +-NaN, +-1e300, zeros of
    both signs and +-5e-324 on rows the sample does not read: still 12 bits, the outliers in the end buckets; uniform with
    1.5 % non-finite rows the sample does not meet: the flat map with its end buckets full, LDS class 1024."""
    col = f64_column(name, nulls)
    f64_ways(api, col, lambda e: want(e, "top+lds", B=12, top=2, map=map_, nulls=int(nulls > 0), lds=lds), name)


@pytest.mark.parametrize("nulls", [0.0, 0.01])
def test_f64_sentinel_met_by_the_sample_three_passes_then_bytes(api, nulls):
    """Normal(100, 3) with +1e300 and -1e300 on sampled rows, 70 001 rows: a 24-bit plan, three top passes, one bucket with
    nearly every row, then the byte passes.  With NULLs this is the input whose NULL tail the late fall-back used to leave
    behind: the NULLs-last pass puts the tail into one buffer pair, three top passes over the rows in front of it end in the
    OTHER pair, and the byte passes then ran over all n rows of that pair — stale keys and row numbers from the order
    before this column, or (first column sorted) arena memory nobody wrote, which the closing NULLs-last pass used as
    indices into the NULL flags.  Read in os_column_passes, fixed there (the tail is copied into the current pair, as the
    LDS branch always did) before this test ran on a device for the first time; the unfixed code was never run on it."""
    col = f64_column("outliers_seen", nulls)
    nv = sum(int(R.chunk_valid(c).sum()) for c in col)

    def check(e):
        want(e, "top+bytes", B=24, top=3, map="segments", then=True, passes=8, nulls=int(nulls > 0))
        assert nv - 40 <= e["bucket"] <= nv - 2, e        # everything but the planted specials

    f64_ways(api, col, check, "sentinel")


def test_f64_plans_refused(api):
    """10 % of the rows equal: refused, raw key bits, two top passes, a bucket of ~7000 rows, then the byte passes (with
    NULLs).  exp(1)^6 at 200 000 rows: refused, raw bits, finished by the narrow os_local_kernel on the bits of doubles.
    6 % non-finite at 200 000 rows: refused, and the top digit (~188 000 rows against a limit of 65 536) sends the column
    to the byte passes before any pass is spent."""
    def spike(e):
        want(e, "top+bytes", B=12, top=2, map="bits", then=True, passes=8, nulls=1)
        assert 6000 <= e["bucket"] <= 8500, e              # the 0.25s, 10 % of 70 001 rows +- 5 sigma, and their bucket's other rows
    f64_ways(api, f64_column("spike", 0.01), spike, "spike")
    for nulls in (0.0, 0.01):
        f64_ways(api, f64_column("exp6", nulls), lambda e: want(e, "top+lds", B=12, top=2, map="bits", nulls=int(nulls > 0), lds=1024), "exp6")

        def crowded(e):
            want(e, "crowded+bytes", B=12, top=2, map="bits", then=True, passes=8, nulls=int(nulls > 0))
            assert 180_000 <= e["digit"] <= 190_000, e     # the finite rows: 94 % of 200 000 (less the NULLs), all of one sign and seven exponents
        f64_ways(api, f64_column("nonfinite_6pct", nulls), crowded, "6 % non-finite")


@pytest.mark.parametrize("name", ["uniform", "normal"])
def test_f64_linear_map_without_the_sample(api, name):
    """sort_sample = 0: buckets linear over [min, max]."""
    lib.set_option("sort_sample", 0)
    for nulls in (0.0, 0.01):
        f64_ways(api, f64_column(name, nulls), lambda e: want(e, "top+lds", B=12, top=2, map="linear", nulls=int(nulls > 0), lds=256), name)


def test_all_null_and_single_value_columns(api):
    """65 536 rows, all NULL, and all NULL but one: no key bits vary, the NULLs-last pass is the whole sort."""
    rng = np.random.default_rng(70)
    n = 65536
    for dt, v in [(A.F64, rng.normal(size=n)), (A.I64, rng.integers(-2 ** 62, 2 ** 62, n))]:
        for keep in ([], [40_000]):
            valid = np.zeros(n, bool)
            valid[keep] = True
            col = chunked(v, valid, dt)
            three_ways(api, col, lambda e, d: want(e, "bytes", passes=0, nulls=1), (dt, keep))
    # and no NULLs, one value: nothing to do for a column that is not the only one; one pass writes the identity otherwise
    col = chunked(np.full(n, 7, dtype=np.int64), None, A.I64)
    ties = chunked(rng.integers(0, 3, n).astype(np.int8), dtype=A.I8)
    want(run(api, [col], [False])[0], "bytes", passes=1, nulls=0)
    note = run(api, [ties, col], [False, True])
    want(note[0], "none")
    want(note[1], "bytes", passes=1, nulls=0)
    note = run(api, [col, ties], [False, True])
    want(note[0], "bytes", passes=1, nulls=0)
    want(note[1], "none")
