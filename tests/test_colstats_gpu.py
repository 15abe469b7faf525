"""rdf_hist / rdf_uniques / rdf_utf8_uniques on the MI355X.  Everything is exact: histograms equal numpy.histogram in counts
AND edges, distinct values equal numpy.unique / set() of bytes as sets (the emission order is unspecified).  Every case
runs over host and device memory, every call is repeated once (same bytes / same set), and every distinct case runs on
the automatic route and with the sort / exact route forced."""
import csv
import os

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMS = ["host", "device"]
QNAN = 0x7FF8000000000000


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
    lib.set_option("uniques_route", 0)
    lib.set_option("uniques_table_bits", 24)


# ---------------------------------------------------------------- inputs

def num(values, valid=None, offset=0):
    return A.HostArray.from_numpy(np.asarray(values), valid, offset=offset)


def to_device(x):
    if isinstance(x, A.HostUtf8):
        return A.DeviceUtf8.from_host(x)
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def place(chunks, mem):
    return list(chunks) if mem == "host" else [to_device(c) for c in chunks]


def split(x, valid=None, cuts=(), offsets=None):
    """x cut at `cuts` into chunks of unequal length, chunk i behind offsets[i] junk elements."""
    bounds = [0] + list(cuts) + [len(x)]
    out = []
    for i in range(len(bounds) - 1):
        a, b = bounds[i], bounds[i + 1]
        out.append(num(x[a:b], None if valid is None else valid[a:b], offset=(offsets[i] if offsets else 0)))
    return out


def utf8(rows, row_offset=0, data_offset=0):
    """rows: bytes or None; row_offset junk rows and data_offset junk bytes in front make the chunk look like a slice."""
    enc = [b"j" * (i % 3 + 1) for i in range(row_offset)] + [b"" if r is None else r for r in rows]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in enc]) if enc else []
    data = np.frombuffer(b"\xee" * data_offset + b"".join(enc) + b"\0" * 8, dtype=np.uint8).copy()
    nulls = sum(r is None for r in rows)
    valid = None
    if nulls:
        valid = A.pack_bits(np.array([True] * row_offset + [r is not None for r in rows], dtype=bool))
    return A.HostUtf8(offs.astype(np.int32), data, valid, row_offset, len(rows), data_offset, nulls)


def utf8_fixed(mat):
    n, w = mat.shape
    offs = (np.arange(n + 1, dtype=np.int64) * w).astype(np.int32)
    data = np.concatenate([mat.reshape(-1), np.zeros(8, dtype=np.uint8)])
    return A.HostUtf8(offs, data, None, 0, n, 0, 0)


# ---------------------------------------------------------------- hist

def run_hist(api, chunks, nbins, rng, mem):
    """-> (counts, edges, counted), the call made twice and the two outputs compared byte for byte."""
    res = []
    for _ in range(2):
        c, e, counted = api.hist(place(chunks, mem), nbins, rng)
        assert c.length == nbins and e.length == nbins + 1
        res.append((api.stats_to_numpy(c), api.stats_to_numpy(e), counted))
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes() and res[0][2] == res[1][2]
    return res[0]


def check_hist(api, chunks, x_valid, nbins, rng=None):
    """x_valid: the valid rows' values (any order).  The reference is numpy on the rows without NaN."""
    x = np.asarray(x_valid)
    if x.dtype.kind == "f":
        x = x[~np.isnan(x)]
    if rng is None and len(x) == 0:
        ref_c, ref_e = np.histogram(np.zeros(0), bins=nbins)          # numpy's own empty rule: 0 .. 1
    else:
        ref_c, ref_e = np.histogram(x, bins=nbins, range=rng)
    out = {}
    for mem in MEMS:
        c, e, counted = run_hist(api, chunks, nbins, rng, mem)
        assert c.dtype == np.int64 and e.dtype == np.float64
        assert np.array_equal(e, ref_e), (mem, nbins, np.nonzero(e != ref_e)[0][:5])
        assert np.array_equal(c, ref_c), (mem, nbins, np.nonzero(c != ref_c)[0][:5], c[:8], ref_c[:8])
        assert counted == int(ref_c.sum())
        out[mem] = (c, e)
    assert out["host"][0].tobytes() == out["device"][0].tobytes() and out["host"][1].tobytes() == out["device"][1].tobytes()


ALL_BINS = [1, 2, 10, 1000, 4096, 4097, 100_000, 2**20]


@pytest.mark.parametrize("nbins", ALL_BINS)
def test_hist_uniform_normal_lognormal(api, nbins):
    rng = np.random.default_rng(nbins)
    n = 200_000
    for x in (rng.uniform(-3.0, 7.0, n), rng.normal(0.0, 1.0, n) * 1e6, rng.lognormal(0.0, 3.0, n)):
        check_hist(api, [num(x)], x, nbins)
    x = rng.normal(0.0, 1.0, n)
    check_hist(api, [num(x)], x, nbins, (-1.0, 0.5))          # both tails cut off
    check_hist(api, [num(x)], x, nbins, (0.25, 0.25))          # lo == hi


@pytest.mark.parametrize("nbins", [1, 2, 10, 1000, 4096, 4097, 100_000])
def test_hist_constant_edges_and_zeros(api, nbins):
    rng = np.random.default_rng(7)
    const = np.full(100_000, 3.25)
    check_hist(api, [num(const)], const, nbins)
    check_hist(api, [num(const)], const, nbins, (0.0, 6.5))
    # values rounded onto the bucket edges of [0, 1]
    edges = np.linspace(0.0, 1.0, nbins + 1)
    x = edges[rng.integers(0, nbins + 1, 100_000)]
    x[::3] = np.nextafter(x[::3], 2.0)
    x[1::3] = np.nextafter(x[1::3], -1.0)
    check_hist(api, [num(x)], x, nbins, (0.0, 1.0))
    check_hist(api, [num(x)], x, nbins)
    z = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0] * 1000)
    check_hist(api, [num(z)], z, nbins)
    check_hist(api, [num(z[:4])], z[:4], nbins)               # only +-0: lo == hi == 0


@pytest.mark.parametrize("nbins", [1, 10, 1000, 4097])
def test_hist_int64(api, nbins):
    rng = np.random.default_rng(11)
    x = rng.integers(-2**39, 2**39, 300_000, dtype=np.int64)
    check_hist(api, [num(x)], x, nbins)
    check_hist(api, [num(x)], x, nbins, (-2.0**38, 2.0**37))
    big = np.concatenate([2**62 - rng.integers(0, 5000, 50_000, dtype=np.int64), -2**62 + rng.integers(0, 5000, 50_000, dtype=np.int64),
                          np.array([2**62, -2**62, 2**62 - 1, 2**62 + 1, 2**53 + 1, -2**53 - 1], dtype=np.int64)])
    check_hist(api, [num(big)], big, nbins)                   # the `as f64` rounding
    check_hist(api, [num(big)], big, nbins, (2.0**62 - 2.0**40, 2.0**62))


@pytest.mark.parametrize("nbins", [2, 10, 4096, 4097])
def test_hist_nulls_chunks_and_offsets(api, nbins):
    rng = np.random.default_rng(13)
    n = 150_001
    x = rng.normal(5.0, 2.0, n)
    valid = rng.random(n) >= 0.1
    check_hist(api, [num(x, valid)], x[valid], nbins)
    check_hist(api, [num(x, valid, offset=5)], x[valid], nbins, (3.0, 6.0))
    chunks = split(x, valid, cuts=(1, 2049, 2049, 70_000, 140_003), offsets=(3, 0, 9, 64, 1, 17))
    check_hist(api, chunks, x[valid], nbins)
    check_hist(api, chunks, x[valid], nbins, (4.0, 9.0))
    xi = rng.integers(-1000, 1000, n, dtype=np.int64)
    check_hist(api, split(xi, valid, cuts=(77, 5000), offsets=(1, 2, 3)), xi[valid], nbins)
    none = np.zeros(n, dtype=bool)
    check_hist(api, [num(x, none)], x[:0], nbins)             # all NULL: 0 .. 1, nothing counted
    check_hist(api, [num(x, none)], x[:0], nbins, (1.0, 2.0))
    check_hist(api, [num(x[:0])], x[:0], nbins)               # empty column
    check_hist(api, [num(x[:0]), num(x[:0])], x[:0], nbins, (1.0, 2.0))


@pytest.mark.parametrize("nbins", [10, 5000])
def test_hist_nan_and_infinities(api, nbins):
    rng = np.random.default_rng(17)
    x = rng.uniform(0.0, 10.0, 50_000)
    x[::7] = np.nan
    x[3] = np.float64(np.frombuffer(np.uint64(0xFFF8000000000123).tobytes(), dtype=np.float64)[0])
    check_hist(api, [num(x)], x, nbins)
    check_hist(api, [num(x)], x, nbins, (2.0, 3.0))
    allnan = np.full(1000, np.nan)
    check_hist(api, [num(allnan)], allnan, nbins)             # nothing counted: 0 .. 1
    y = x.copy()
    y[11] = np.inf
    y[12] = -np.inf
    for mem in MEMS:
        with pytest.raises(A.RdfError) as ei:
            api.hist(place([num(y)], mem), nbins)
        assert ei.value.status == A.RDF_COMPUTE_ERROR and "range is not finite" in ei.value.message
    check_hist(api, [num(y)], y[np.isfinite(y)], nbins, (0.0, 10.0))   # ignored with an explicit range


@pytest.mark.parametrize("nbins", [1000, 4096])
def test_hist_1e8_rows_generated_on_the_device(api, nbins):
    """rdf_fill_uniform_f64(seed 42, column 0, first_row 0, lo 0, hi 1) binned over [0, 1]: every row is counted and every
    bucket lies within 6 sigma of rows / nbins (sigma^2 = rows p (1 - p), p = 1 / nbins).  The bound is a condition, not a
    measurement: the same generator run on the CPU and binned by numpy.histogram stays at 3.31 sigma (1000 buckets) and
    3.67 sigma (4096)."""
    rows = 100_000_000
    t = torch.empty(rows, dtype=torch.float64, device="cuda")
    lib.fill_uniform_f64(t.data_ptr(), rows, 42, 0, 0, 0.0, 1.0)
    col = [A.DeviceArray(t.data_ptr(), None, 0, rows, A.F64, 0, keep=t)]
    first = None
    for _ in range(2):
        c, e, counted = api.hist(col, nbins, (0.0, 1.0))
        c, e = api.stats_to_numpy(c), api.stats_to_numpy(e)
        assert int(c.sum()) == counted == rows
        assert np.array_equal(e, np.histogram(np.zeros(0), bins=nbins, range=(0.0, 1.0))[1])
        p = 1.0 / nbins
        sigma = (rows * p * (1.0 - p)) ** 0.5
        dev = np.abs(c - rows * p).max() / sigma
        print(f"hist 1e8 rows, {nbins} buckets: largest deviation {dev:.2f} sigma")
        assert dev <= 6.0, dev
        if first is not None:
            assert first == c.tobytes()
        first = c.tobytes()


# ---------------------------------------------------------------- uniques

def f64_key(x):
    """Float64 values as the set members the call promises: -0.0 -> +0.0, every NaN -> the quiet NaN, else the bits."""
    x = np.asarray(x, dtype=np.float64).copy()
    x[x == 0.0] = 0.0
    b = x.view(np.uint64).copy()
    b[np.isnan(x)] = QNAN
    return b


def run_uniques(api, chunks, mem):
    """-> the distinct values as sorted raw 64-bit words; the call is made twice (same count, same set), the count-only call
    agrees, and there are no duplicates."""
    res = []
    for _ in range(2):
        placed = place(chunks, mem)
        out = api.uniques(placed)
        v = api.stats_to_numpy(out)
        assert len(v) == out.length and out.null_count == 0
        res.append(np.sort(v.view(np.uint64)))
    assert np.array_equal(res[0], res[1])
    assert api.uniques(place(chunks, mem), count_only=True) == len(res[0])
    assert len(np.unique(res[0])) == len(res[0]), "a value was returned twice"
    return res[0]


def check_uniques(api, chunks, x_valid, routes=(0, 1)):
    x = np.asarray(x_valid)
    ref = np.unique(f64_key(x)) if x.dtype.kind == "f" else np.unique(x.view(np.uint64))
    for route in routes:
        lib.set_option("uniques_route", route)
        for mem in MEMS:
            got = run_uniques(api, chunks, mem)
            assert len(got) == len(ref), (route, mem, len(got), len(ref))
            assert np.array_equal(got, ref), (route, mem)
    lib.set_option("uniques_route", 0)


def test_uniques_cardinalities(api):
    rng = np.random.default_rng(23)
    n = 1_000_000
    for k in (1, 37, 1000):
        vals = rng.integers(-2**62, 2**62, k, dtype=np.int64)
        x = vals[rng.integers(0, k, n)]
        check_uniques(api, [num(x)], x)
        xf = (vals.astype(np.float64) / 3.0)[rng.integers(0, k, n)]
        check_uniques(api, [num(xf)], xf)
    x = rng.permutation(np.arange(n, dtype=np.int64) * 7919 - 12345)      # all rows distinct
    check_uniques(api, [num(x)], x)
    zipf = np.minimum(rng.zipf(1.3, n), 10**12).astype(np.int64)          # Zipf-like skew: a few hot values, a long tail
    check_uniques(api, [num(zipf)], zipf)
    u = rng.integers(0, 2**64 - 1, 5000, dtype=np.uint64)[rng.integers(0, 5000, 100_000)]
    check_uniques(api, [num(u)], u)


def test_uniques_1e6_distinct_among_1e7_rows(api):
    rng = np.random.default_rng(29)
    vals = rng.permutation(np.arange(1_000_000, dtype=np.int64)) * 1_000_003
    x = vals[rng.integers(0, 1_000_000, 10_000_000)]
    x[:1_000_000] = vals                                                   # every value occurs
    check_uniques(api, [num(x)], x)


def test_uniques_extremes_and_float_specials(api):
    i = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1, 1, -1, 0, np.iinfo(np.int64).min,
                  0, 0], dtype=np.int64)
    i[-2:] = np.array([0xFFF7A5A55A5A0001], dtype=np.uint64).view(np.int64)[0]    # the hash set's own free-slot word is a value too
    check_uniques(api, [num(np.tile(i, 500))], np.tile(i, 500))
    nan_payloads = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF7A5A55A5A0001, 0x7FFFFFFFFFFFFFFF],
                            dtype=np.uint64).view(np.float64)
    f = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072009e-308, 1.0, -1.0, 0.1, 0.1]),
                        nan_payloads])
    f = np.tile(f, 700)
    for route in (0, 1):
        lib.set_option("uniques_route", route)
        for mem in MEMS:
            got = run_uniques(api, [num(f)], mem)
            assert (got == QNAN).sum() == 1                                       # one NaN back, the canonical one
            assert np.isnan(got.view(np.float64)).sum() == 1
            assert (got == 0).sum() == 1 and (got == 0x8000000000000000).sum() == 0   # one +0.0 back
    check_uniques(api, [num(f)], f)
    nz = np.array([-0.0, -0.0, -0.0])
    check_uniques(api, [num(nz)], nz)
    assert run_uniques(api, [num(nz)], "host").tolist() == [0]


def test_uniques_nulls_chunks_and_offsets(api):
    rng = np.random.default_rng(31)
    n = 300_007
    x = rng.integers(0, 5000, n, dtype=np.int64) - 2500
    valid = rng.random(n) >= 0.1
    check_uniques(api, [num(x, valid)], x[valid])
    check_uniques(api, split(x, valid, cuts=(1, 2049, 2049, 100_000), offsets=(3, 0, 9, 64, 5)), x[valid])
    xf = rng.normal(0, 1, n).round(2)
    check_uniques(api, split(xf, valid, cuts=(12_345,), offsets=(7, 1)), xf[valid])
    # a value that only occurs in NULL rows is not returned
    y = x.copy()
    y[~valid] = 999_999
    check_uniques(api, [num(y, valid)], x[valid])
    none = np.zeros(n, dtype=bool)
    check_uniques(api, [num(x, none)], x[:0])                # all NULL: count 0
    check_uniques(api, [num(x[:0])], x[:0])                  # empty
    check_uniques(api, [num(x[:0]), num(x[:0])], x[:0])


def test_uniques_capacity_rules(api):
    x = np.array([4, 4, 2, 9, 2, 7], dtype=np.int64)
    for route in (0, 1):
        lib.set_option("uniques_route", route)
        for mem in MEMS:
            chunks = place([num(x)], mem)
            assert api.uniques(chunks, count_only=True) == 4
            short = api._stats_out(A.I64, 3, mem == "device")
            with pytest.raises(A.RdfError) as ei:
                api.uniques(chunks, out=short)
            assert ei.value.status == A.RDF_MEMORY_ERROR
            assert (api.stats_to_numpy(short) == 0).all(), "nothing is written on RDF_MEMORY_ERROR"
            for cap in (4, 6, 100):                          # exact, all rows, more
                out = api.uniques(chunks, out=api._stats_out(A.I64, cap, mem == "device"))
                assert sorted(api.stats_to_numpy(out).tolist()) == [2, 4, 7, 9]


def test_uniques_automatic_route_falls_back_to_the_sort(api):
    """The hash route's table has min(2^uniques_table_bits, 2 x rows rounded up to a power of two) slots and gives up beyond
    half of them (cs_table_slots / max_fill in rdf_capi_colstats.inc).  With the default budget of 2^24 slots it holds
    2^23 = 8 388 608 keys: 1e7 all-distinct rows cannot fit, so the automatic route itself must end on the sort route.
    The same with a budget of 2^12 slots (2048 keys) and 5000 distinct values."""
    rng = np.random.default_rng(37)
    x = rng.permutation(np.arange(10_000_000, dtype=np.int64)) * 3 - 7
    assert 10_000_000 > 2**23
    for mem in MEMS:
        out = api.uniques(place([num(x)], mem))
        assert "cs_runs_kernel" in lib.last_kernel()
        got = np.sort(api.stats_to_numpy(out))
        assert np.array_equal(got, np.sort(x))
    lib.set_option("uniques_table_bits", 12)
    y = rng.integers(0, 5000, 200_000, dtype=np.int64)
    check_uniques(api, [num(y)], y, routes=(0,))
    assert "cs_runs_kernel" in lib.last_kernel()
    z = rng.integers(0, 1500, 200_000, dtype=np.int64)       # 1500 <= 2048: stays on the hash route
    check_uniques(api, [num(z)], z, routes=(0,))
    assert "cs_distinct_kernel" in lib.last_kernel()


# ---------------------------------------------------------------- utf8_uniques

def run_utf8(api, chunks, mem):
    """-> the distinct strings as a list of bytes (the call made twice: same count, same set; no NULLs; no duplicates)."""
    res = []
    for _ in range(2):
        r = api.utf8_uniques(place(chunks, mem))
        h = r.to_host() if mem == "device" else r
        assert h.null_count == 0
        o = h.offsets[: h.length + 1].astype(np.int64)
        assert o[0] == 0
        raw = h.data.tobytes()
        vals = [raw[o[i]:o[i + 1]] for i in range(h.length)]
        assert len(set(vals)) == len(vals), "a value was returned twice"
        res.append(vals)
    assert len(res[0]) == len(res[1]) and set(res[0]) == set(res[1])
    return res[0]


def check_utf8(api, chunks, rows):
    ref = set(r for r in rows if r is not None)
    seen = {}
    for route in (0, 1):
        lib.set_option("uniques_route", route)
        for mem in MEMS:
            got = run_utf8(api, chunks, mem)
            assert len(got) == len(ref), (route, mem, len(got), len(ref))
            assert set(got) == ref, (route, mem)
            seen[(route, mem)] = set(got)
    lib.set_option("uniques_route", 0)
    assert seen[(0, "host")] == seen[(1, "host")] == seen[(0, "device")] == seen[(1, "device")]


def city_names():
    with open(os.path.join(ROOT, "tests", "golden", "uk_cities_with_headers.csv"), newline="") as f:
        rows = list(csv.reader(f))[1:]
    return [r[0].encode() for r in rows]


def test_utf8_city_names(api):
    names = city_names()
    assert len(set(names)) == 37
    check_utf8(api, [utf8(names)], names)
    check_utf8(api, [utf8(names * 50)], names * 50)


def test_utf8_small_edge_cases(api):
    long_a = b"x" * 65536
    rows = [b"", b"a", b"a\0", b"a\0b", b"b", None, b"", b"a", long_a, long_a[:-1] + b"y", long_a, long_a[:-1], b"\xc3\xa9",
            "é".encode(), "日本語".encode(), "日本".encode(), b"e\xcc\x81", None, b"\0", b"\0\0", b"a\0",
            b"p" * 511 + b"1", b"p" * 511 + b"2", b"p" * 512, b"p" * 511 + b"1", b"q" * 4000 + b"A", b"q" * 4000 + b"B", b"q" * 4000 + b"A"]
    check_utf8(api, [utf8(rows)], rows)
    check_utf8(api, [utf8(rows, row_offset=3, data_offset=5)], rows)
    check_utf8(api, [utf8(rows[:9], 1, 2), utf8(rows[9:20], 5, 0), utf8([]), utf8(rows[20:], 0, 9)], rows)
    check_utf8(api, [utf8([None, None, None])], [None] * 3)          # all NULL
    check_utf8(api, [utf8([])], [])                                      # empty
    check_utf8(api, [utf8([b""] * 100)], [b""])                         # the empty string is a value
    check_utf8(api, [utf8([None, b"", None])], [b""])


def test_utf8_1e6_rows_over_1000_values(api):
    rng = np.random.default_rng(41)
    vals = rng.integers(97, 123, size=(1000, 12), dtype=np.uint8)
    vals[:, :8] = np.frombuffer(b"prefix__", dtype=np.uint8)            # a shared prefix; they differ in the last bytes
    vals = np.unique(vals, axis=0)
    mat = vals[rng.integers(0, len(vals), 1_000_000)]
    ref = set(bytes(r) for r in np.unique(mat, axis=0))
    for route in (0, 1):
        lib.set_option("uniques_route", route)
        for mem in MEMS:
            got = run_utf8(api, [utf8_fixed(mat[:400_000]), utf8_fixed(mat[400_000:])], mem)
            assert len(got) == len(ref) and set(got) == ref, (route, mem)


def test_utf8_all_distinct(api):
    n = 300_000
    ids = np.arange(n, dtype=np.int64) * 2654435761 % (10**10)
    mat = np.zeros((n, 10), dtype=np.uint8)
    v = ids.copy()
    for k in range(9, -1, -1):
        mat[:, k] = 48 + v % 10
        v //= 10
    ref = set(bytes(r) for r in mat)
    assert len(ref) == n
    for route in (0, 1):
        lib.set_option("uniques_route", route)
        for mem in MEMS:
            got = run_utf8(api, [utf8_fixed(mat)], mem)
            assert len(got) == n and set(got) == ref, (route, mem)


def test_utf8_table_budget_sends_the_call_to_the_exact_route(api):
    """2^10 slots hold 512 hashes: 2000 distinct strings overflow the set, the exact route answers."""
    lib.set_option("uniques_table_bits", 10)
    rows = [b"value-%05d" % (i % 2000) for i in range(20_000)]
    for mem in MEMS:
        got = run_utf8(api, [utf8(rows)], mem)
        assert "cs_utf8_runs_kernel" in lib.last_kernel()
        assert set(got) == set(rows) and len(got) == 2000


def test_utf8_sizing_call_then_real_call(api):
    import ctypes as C
    so = lib.load()
    so.rdf_utf8_uniques.restype = C.c_int
    rows = [b"bb", b"a", None, b"bb", b"", b"ccc", b"a"]
    h = utf8(rows)
    carr = (A.rdf_utf8_array * 1)(h.c_struct())
    for route in (0, 1):
        lib.set_option("uniques_route", route)
        ob = np.zeros(len(rows) + 1, dtype=np.int32)
        oo = (A.rdf_out * 1)(A.rdf_out(ob.ctypes.data, None, len(rows) + 1, 0, 0, A.I32, A.MEM_HOST))
        od = (A.rdf_out * 1)(A.rdf_out(None, None, 0, 0, 0, A.U8, A.MEM_HOST))
        cnt = C.c_int64(-1)
        assert so.rdf_utf8_uniques(carr, C.c_int64(1), oo, od, C.byref(cnt)) == A.RDF_MEMORY_ERROR
        assert cnt.value == 4 and od[0].length == 6 and oo[0].length == 5
        db = np.zeros(od[0].length, dtype=np.uint8)
        od = (A.rdf_out * 1)(A.rdf_out(db.ctypes.data, None, len(db), 0, 0, A.U8, A.MEM_HOST))
        assert so.rdf_utf8_uniques(carr, C.c_int64(1), oo, od, C.byref(cnt)) == A.RDF_OK
        assert cnt.value == 4 and oo[0].length == 5 and od[0].length == 6 and oo[0].null_count == 0
        raw = db.tobytes()
        assert {raw[ob[i]:ob[i + 1]] for i in range(4)} == {b"bb", b"a", b"", b"ccc"}
