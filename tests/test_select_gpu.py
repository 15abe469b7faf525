"""rdf_null_test / rdf_coalesce / rdf_case_when / rdf_extremum / rdf_nanvl on the MI355X: every result equal, bit for bit, to
tests/select_ref.py — values, bitmap, length, NULL count.  Every case runs over host and over device memory, twice each, and
the four results are identical bytes; every output sits between guard bytes that must survive.  NULL rows hold 0 and the bits
past `length` in a bitmap's last byte are 0.

Shapes are the smallest at which each part of the kernels can go wrong: chunk lengths around one bitmap byte (8), one lane row
(64), one pass of every element size (64 V rows: 128 / 256 / 512 for 8 / 4 / 2-byte elements; 1-byte elements move 8 bytes a
lane, 512 rows; 1024 is kept as a length too), one wave tile (512) and one block tile (2048); every part and condition of a
call behind a different element / bit offset (which also decides, per part, between vector and element loads); and 200 003
rows in seven unequal chunks, one of a single row and one empty, with 10 % NULLs per part.

Bounds worked out here, not taken from the code under test: none — everything is compared for equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import select_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WAVE_TILE, TILE = 512, 2048          # kDtWaveTile, kCsTile: rows of one wave's and one block's tile
PASSES = [128, 256, 512, 1024]       # 64 V rows
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65] + [p + d for p in PASSES for d in (-1, 0, 1)] + [TILE - 1, TILE, TILE + 1]
OFFSETS = [0, 1, 3, 7, 9, 13, 64]
BIG = 200_003
CUTS = [1, 2049, 2049, 40_511, 100_000, 163_840]   # seven chunks: 1 row, 2048, EMPTY, 38 462, 59 489, 63 840, 36 163
CODES = {"i8": A.I8, "i16": A.I16, "i32": A.I32, "i64": A.I64, "u8": A.U8, "u16": A.U16, "u32": A.U32, "u64": A.U64, "f32": A.F32, "f64": A.F64}
NAMES = list(R.DTYPES)
GUARD = 64


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


def lengths_for(n):
    """LENGTHS repeated while rows last."""
    lens, at = [], 0
    while at < n:
        for k in LENGTHS:
            k = min(k, n - at)
            lens.append(k)
            at += k
            if at == n:
                break
    return lens


def chunks(v, m, lens, k, code):
    """Column k of a call: chunk i behind the element / bit offset OFFSETS[(i + k) % 7] — no two parts of a chunk share one."""
    out, at = [], 0
    for i, n in enumerate(lens):
        out.append(A.HostArray.from_numpy(v[at:at + n], None if m is None else m[at:at + n], offset=OFFSETS[(i + k) % 7], dtype=code))
        at += n
    return out


def es_of(code):
    return 1 if code == A.BOOL else np.dtype(A.NP_OF[code]).itemsize


def make_outs(code, lens, device, bitmap):
    """One output per chunk between guard bytes.  Host: exactly the bytes of the rows.  Device: room for the rows rounded up to
    64 (the header's rule), every second chunk 8 bytes off a 16-byte boundary, so vector and element stores mix."""
    outs = []
    for i, n in enumerate(lens):
        cap = (n + 63) // 64 * 64 if device else n
        vbytes = (cap + 7) // 8 if code == A.BOOL else max(cap, 1) * es_of(code)
        bbytes = (cap + 7) // 8
        g = GUARD + (8 if device and i % 2 else 0)
        if device:
            vt = torch.full((g + vbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            bt = torch.full((GUARD + max(bbytes, 8) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") if bitmap else None
            o = A.DeviceArray(vt.data_ptr() + g, bt.data_ptr() + GUARD if bitmap else None, 0, n, code, 0, keep=(vt, bt), capacity=n)
            o.spans = (g, vbytes, GUARD, bbytes)
        else:
            vb = np.full(g + vbytes + GUARD, 0xA5, dtype=np.uint8)
            bb = np.full(GUARD + bbytes + GUARD, 0xA5, dtype=np.uint8) if bitmap else None
            vals = vb[g:g + vbytes] if code == A.BOOL else vb[g:g + vbytes].view(A.NP_OF[code])
            o = A.HostArray(vals, bb[GUARD:GUARD + bbytes] if bitmap else None, 0, n, code, 0)
            o.whole = (vb, bb)
            o.spans = (g, vbytes, GUARD, bbytes)
        outs.append(o)
    return outs


def out_bytes(o):
    """(values bytes, bitmap bytes | None, length, NULL count) of one output chunk, wherever it lives; its guards are intact."""
    n = o.length
    g, vbytes, gb, bbytes = o.spans
    if isinstance(o, A.HostArray):
        vb, bb = o.whole
    else:
        vb, bb = o.keep[0].cpu().numpy(), (o.keep[1].cpu().numpy() if o.keep[1] is not None else None)
    assert (vb[:g] == 0xA5).all() and (vb[g + vbytes:] == 0xA5).all(), "values guard"
    if bb is not None:
        assert (bb[:gb] == 0xA5).all() and (bb[gb + max(bbytes, 8 if not isinstance(o, A.HostArray) else 0):] == 0xA5).all(), "bitmap guard"
    nv = (n + 7) // 8 if o.dtype == A.BOOL else n * es_of(o.dtype)
    return vb[g:g + nv].tobytes(), None if bb is None else bb[gb:gb + (n + 7) // 8].tobytes(), n, o.null_count


def four_ways(call, cols, code, lens, bitmap=True):
    """call(cols, outs) over host memory and over device memory, twice each: identical bytes -> [(values, valid mask | None)] per chunk."""
    dev = [[to_device(a) for a in c] for c in cols]
    runs = [call(c, make_outs(code, lens, d, bitmap)) for c, d in ((cols, False), (dev, True), (cols, False), (dev, True))]
    sig = [[out_bytes(o) for o in r] for r in runs]
    assert all(s == sig[0] for s in sig[1:]), "host / device / repeated runs differ"
    got = []
    for (vals, bits, n, nulls), want_n in zip(sig[0], lens):
        assert n == want_n
        if code == A.BOOL:
            v = A.unpack_bits(np.frombuffer(vals, dtype=np.uint8), 0, n)
            assert n % 8 == 0 or vals[-1] >> (n % 8) == 0, "bits past the length are 0"
        else:
            v = np.frombuffer(vals, dtype=A.NP_OF[code])
        m = None if bits is None else A.unpack_bits(np.frombuffer(bits, dtype=np.uint8), 0, n)
        if bits is not None and n % 8:
            assert bits[-1] >> (n % 8) == 0, "bits past the length are 0"
        assert nulls == (0 if m is None else int(n - m.sum()))
        got.append((v, m))
    return got


def expect(got, want, lens, what=""):
    """got: [(values, mask | None)] per chunk; want: the model's (values, valid) over the concatenated rows (NULL rows hold 0)."""
    wv, wm = want
    at = 0
    for i, ((v, m), n) in enumerate(zip(got, lens)):
        if m is None:
            assert wm[at:at + n].all(), (what, i)
        else:
            assert np.array_equal(m, wm[at:at + n]), (what, i, np.flatnonzero(m != wm[at:at + n])[:5])
        a, b = R.bits_of(v), R.bits_of(wv[at:at + n])
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)[:5]
            raise AssertionError(f"{what} chunk {i} ({n} rows): rows {bad}: got {v[bad]}, expected {wv[at:at + n][bad]}")
        at += n
    assert at == len(wv)


def as_part(p, cols):
    """('col', j) -> chunk list j; anything else is a literal."""
    return cols[p[1]] if isinstance(p, tuple) else p


def model_part(p, data):
    return data[p[1]] if isinstance(p, tuple) else p


@functools.lru_cache(maxsize=None)
def columns(name, k, n, null_share=0.35, seed=0):
    """k columns of n rows: (values, valid) with the edge values, ties and the full range of bit patterns mixed."""
    rng = np.random.default_rng(1000 * seed + 10 * k + len(name) + ord(name[0]) + int(name[1:]))
    return [(R.random_values(name, n, rng), rng.uniform(size=n) > null_share) for _ in range(k)]


N = sum(LENGTHS) + 700               # every length once, then a second round that ends inside it


# ---------------------------------------------------------------- null_test
@pytest.mark.parametrize("name", NAMES + ["bool"])
def test_is_null_and_is_not_null_of_every_dtype(api, name):
    rng = np.random.default_rng(5)
    code = A.BOOL if name == "bool" else CODES[name]
    v = rng.integers(0, 2, N).astype(bool) if name == "bool" else R.random_values(name, N, rng)
    lens = lengths_for(N)
    assert set(LENGTHS) <= set(lens)
    for m in (rng.uniform(size=N) > 0.3, None):
        col = chunks(v, m, lens, 0, code)
        assert m is None or {c.offset for c in col} == set(OFFSETS)
        for op, test in (("is_null", R.IS_NULL), ("is_not_null", R.IS_NOT_NULL)):
            for bitmap in (False, True):
                got = four_ways(lambda c, outs: api.null_test(op, c[0], outs=outs), [col], A.BOOL, lens, bitmap)
                expect(got, (R.null_test(test, v, m), np.ones(N, dtype=bool)), lens, f"{op} {name}")
                assert all(g[1] is None or g[1].all() for g in got)


@pytest.mark.parametrize("name", R.FLOATS)
def test_is_nan(api, name):
    rng = np.random.default_rng(6)
    v, m = R.random_values(name, N, rng), rng.uniform(size=N) > 0.3
    lens = lengths_for(N)
    for mask in (m, None):
        col = chunks(v, mask, lens, 3, CODES[name])
        got = four_ways(lambda c, outs: api.null_test("is_nan", c[0], outs=outs), [col], A.BOOL, lens, mask is not None)
        want = R.null_test(R.IS_NAN, v, mask)
        assert want.any() and not want.all()
        expect(got, (want, np.ones(N, dtype=bool)), lens, f"is_nan {name}")


def test_is_null_reads_no_values_and_takes_a_utf8_column(api):
    m = np.random.default_rng(7).uniform(size=1000) > 0.5
    col = [A.HostArray.from_numpy(np.zeros(1000, dtype=np.int32), m, offset=3)]
    struct = col[0].c_struct()
    struct.values = None                                                   # never read
    out = A.HostArray.empty_out(A.BOOL, 1000, False)
    carr = (A.rdf_out * 1)(out.out_struct())
    api._check(api._dt_fn("null_test")(C.c_int32(A.IS_NULL), (A.rdf_array * 1)(struct), C.c_int64(1), carr))
    assert np.array_equal(A.unpack_bits(out.values, 0, 1000), ~m)
    rows = [None if i % 3 == 0 else "x" * (i % 5) for i in range(300)]
    text = A.HostUtf8.from_pylist(rows, row_offset=5, data_offset=2)
    for t in (text, A.DeviceUtf8.from_host(text)):
        got = api.null_test("is_null", [t])[0]
        bits = got.values if isinstance(got, A.HostArray) else got.keep[0].cpu().numpy().view(np.uint8)
        assert A.unpack_bits(bits, 0, 300).tolist() == [r is None for r in rows]


# ---------------------------------------------------------------- coalesce
SHAPES = {1: [("col", 0)], 2: [("col", 0), ("col", 1)], 3: [("col", 0), ("col", 1), ("col", 2)], 8: [("col", j) for j in range(8)]}


@pytest.mark.parametrize("nparts", [1, 2, 3, 8])
@pytest.mark.parametrize("name", NAMES)
def test_coalesce_every_dtype_length_and_offset(api, name, nparts):
    code, dt = CODES[name], R.DTYPES[name]
    data = columns(name, nparts, N)
    lens = lengths_for(N)
    cols = [chunks(v, m, lens, k, code) for k, (v, m) in enumerate(data)]
    assert set(LENGTHS) <= set(lens) and all(len({c[i].offset for c in cols}) == min(nparts, 7) for i in range(7))
    got = four_ways(lambda c, outs: api.coalesce(c, outs=outs), cols, code, lens)
    expect(got, R.coalesce(list(data), dt), lens, f"coalesce {name} x{nparts}")


@pytest.mark.parametrize("name", NAMES)
def test_coalesce_with_literals_first_middle_last_and_the_null_literal(api, name):
    code, dt = CODES[name], R.DTYPES[name]
    data = columns(name, 3, N, seed=1)
    lens = lengths_for(N)
    cols = [chunks(v, m, lens, k + 2, code) for k, (v, m) in enumerate(data)]
    lit = np.array([R.edge_values(name)[-2]], dtype=dt)[0].item() if np.dtype(dt).kind != "f" else -0.0
    c = lambda j: ("col", j)
    for shape, bitmap in (([lit, c(0)], True), ([c(0), lit, c(1)], False), ([c(0), c(1), lit], False), ([c(0), None, c(1)], True), ([None, c(2), None], True),
                          ([c(0), c(1), c(2), None, lit], False), ([c(0), None], True)):
        got = four_ways(lambda cc, outs: api.coalesce([as_part(p, cc) for p in shape], outs=outs), cols, code, lens, bitmap)
        expect(got, R.coalesce([model_part(p, data) for p in shape], dt), lens, f"coalesce {name} {shape}")
        if not bitmap:
            assert all(m is None for _, m in got)


def skip_patterns(n, per_pass):
    """Validity of part 0 that exercises the skip of unneeded parts: (name, mask | None)."""
    one = lambda *rows: np.isin(np.arange(n), rows, invert=True)
    return [("no bitmap", None), ("all NULL", np.zeros(n, dtype=bool)), ("none NULL, with a bitmap", np.ones(n, dtype=bool)),
            ("one NULL at the first row of a pass", one(TILE + per_pass)), ("one NULL at the last row of a pass", one(TILE + 2 * per_pass - 1)),
            ("one NULL in the tile's last partial word", one(n - 3)), ("one NULL in the first and one in the last row", one(0, n - 1))]


@pytest.mark.parametrize("name", ["f64", "i32", "u16", "i8"])
def test_coalesce_null_patterns_that_decide_what_is_read(api, name):
    code, dt = CODES[name], R.DTYPES[name]
    per_pass = {8: 128, 4: 256, 2: 512, 1: 512}[np.dtype(dt).itemsize]
    n = 2 * TILE + WAVE_TILE + 70                                          # two block tiles, a full wave tile, a partial word
    (v0, _), (v1, m1), (v2, m2) = columns(name, 3, n, seed=2)
    lens = [n]
    for what, m0 in skip_patterns(n, per_pass):
        for second in (m1, None):
            data = [(v0, m0), (v1, second), (v2, m2)]
            cols = [chunks(v, m, lens, k, code) for k, (v, m) in enumerate(data)]
            got = four_ways(lambda c, outs: api.coalesce(c, outs=outs), cols, code, lens)
            expect(got, R.coalesce(data, dt), lens, f"coalesce {name}: {what}")
    # part 1 is needed by ONE row of a group of 64 V rows only; part 2 by one row in which both others are NULL
    m0 = np.ones(n, dtype=bool)
    m0[[per_pass + 5, TILE + 3 * per_pass - 1, n - 1]] = False
    m1 = np.ones(n, dtype=bool)
    m1[[TILE + 3 * per_pass - 1]] = False
    every = np.ones(n, dtype=bool)
    every[[17, n - 2]] = False                                             # rows in which EVERY part is NULL
    data = [(v0, m0 & every), (v1, m1 & every), (v2, m2 & every)]
    cols = [chunks(v, m, lens, k + 4, code) for k, (v, m) in enumerate(data)]
    got = four_ways(lambda c, outs: api.coalesce(c, outs=outs), cols, code, lens)
    want = R.coalesce(data, dt)
    assert not want[1][17] and not want[1][n - 2] and want[1].sum() >= n - 3
    expect(got, want, lens, f"coalesce {name}: single rows")


# ---------------------------------------------------------------- case_when
def conditions(nb, n, seed, share=0.3):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(size=n) < share, (rng.uniform(size=n) > 0.2) if k % 2 == 0 else None) for k in range(nb)]


@pytest.mark.parametrize("nb", [1, 2, 3, 8])
@pytest.mark.parametrize("name", NAMES)
def test_case_when_every_dtype_length_and_offset(api, name, nb):
    code, dt = CODES[name], R.DTYPES[name]
    data = columns(name, nb + 1, N, seed=3)
    conds = conditions(nb, N, nb)
    lens = lengths_for(N)
    cols = [chunks(v, m, lens, k, code) for k, (v, m) in enumerate(data)]
    ccols = [chunks(c, m, lens, k + 3, A.BOOL) for k, (c, m) in enumerate(conds)]
    for otherwise in (True, False):
        call = lambda c, outs: api.case_when(c[nb + 1:], c[:nb], c[nb] if otherwise else None, outs=outs)
        got = four_ways(call, cols + ccols, code, lens)
        expect(got, R.case_when(conds, list(data[:nb]), data[nb] if otherwise else None, dt), lens, f"case_when {name} x{nb} otherwise={otherwise}")


@pytest.mark.parametrize("name", ["f64", "i16", "u8"])
def test_case_when_literals_all_false_and_overlapping_conditions(api, name):
    code, dt = CODES[name], R.DTYPES[name]
    data = list(columns(name, 2, N, seed=4))
    data.append((data[0][0][::-1].copy(), None))                           # a column without a bitmap
    lens = lengths_for(N)
    cols = [chunks(v, m, lens, k + 1, code) for k, (v, m) in enumerate(data)]
    rng = np.random.default_rng(8)
    t = rng.uniform(size=N) < 0.5
    never, always = (np.zeros(N, dtype=bool), None), (np.ones(N, dtype=bool), None)
    c = lambda j: ("col", j)
    cases = [([(t, None)], [c(0)], c(1), "if_else"), ([(t, None)], [3], c(2), "if_else of a literal and a column without NULLs"), ([never, never], [c(0), 1], c(1), "all false, otherwise"),
             ([never, never], [c(0), 1], None, "all false, no otherwise"), ([always, always, (t, None)], [c(1), c(0), 5], 6, "overlapping: the first wins"),
             ([(t, None), always], [None, c(0)], None, "a NULL literal is chosen"), ([(t, rng.uniform(size=N) > 0.5), (t, None)], [1, 2], c(2), "a NULL condition falls through")]
    for conds, values, other, what in cases:
        ccols = [chunks(cv, cm, lens, k + 5, A.BOOL) for k, (cv, cm) in enumerate(conds)]
        need_bitmap = other is None or any(p is None or (isinstance(p, tuple) and data[p[1]][1] is not None) for p in values + [other])
        call = lambda cc, outs: api.case_when(cc[3:], [as_part(p, cc) for p in values], as_part(other, cc), outs=outs)
        got = four_ways(call, cols + ccols, code, lens, need_bitmap)
        expect(got, R.case_when(conds, [model_part(p, data) for p in values], model_part(other, data), dt), lens, f"case_when {name}: {what}")


# ---------------------------------------------------------------- extremum
@pytest.mark.parametrize("nparts", [2, 3, 8])
@pytest.mark.parametrize("name", NAMES)
def test_greatest_and_least_every_dtype_length_and_offset(api, name, nparts):
    code, dt = CODES[name], R.DTYPES[name]
    data = columns(name, nparts, N, seed=5)
    lens = lengths_for(N)
    cols = [chunks(v, m, lens, k + 1, code) for k, (v, m) in enumerate(data)]
    for greatest in (True, False):
        got = four_ways(lambda c, outs: api.extremum(greatest, c, outs=outs), cols, code, lens)
        expect(got, R.extremum(greatest, list(data), dt), lens, f"{'greatest' if greatest else 'least'} {name} x{nparts}")


@pytest.mark.parametrize("name", NAMES)
def test_extremum_ties_nan_signed_zero_and_unsigned_in_every_position(api, name):
    """Every ordered pair of the dtype's edge values (the extremes, UInt64 above 2^63, +-0, +-inf, NaNs of different payloads), the
    pair placed at every two positions of eight parts whose other parts are NULL or the literal NULL."""
    code, dt = CODES[name], R.DTYPES[name]
    e = R.edge_values(name)
    a, b = np.repeat(e, len(e)), np.tile(e, len(e))
    n = len(a)
    lens = [n]
    nulls = (np.zeros(n, dtype=dt), np.zeros(n, dtype=bool))
    for i, j in ((0, 1), (0, 7), (2, 5), (3, 4), (5, 2), (6, 7)):
        data = [nulls] * 8
        data[i], data[j] = (a, np.ones(n, dtype=bool)), (b, None)             # ((5, 2): b stands left of a)
        shape = [("col", k) if k in (i, j) or k % 2 else None for k in range(8)]
        cols = [chunks(v, m, lens, k, code) for k, (v, m) in enumerate(data)]
        for greatest in (True, False):
            got = four_ways(lambda c, outs: api.extremum(greatest, [as_part(p, c) for p in shape], outs=outs), cols, code, lens, False)
            want = R.extremum(greatest, [a_part if isinstance(p, tuple) else None for p, a_part in zip(shape, data)], dt)
            expect(got, want, lens, f"extremum {name} pairs at {i}, {j}")
    # a literal takes part like a column: first, middle, last
    lit = e[len(e) // 2].item()
    (v0, m0), (v1, m1) = columns(name, 2, 3000, seed=6)
    cols = [chunks(v0, m0, [3000], 1, code), chunks(v1, m1, [3000], 2, code)]
    for shape in ([lit, ("col", 0)], [("col", 0), lit, ("col", 1)], [("col", 0), ("col", 1), lit], [("col", 0), None]):
        for greatest in (True, False):
            got = four_ways(lambda c, outs: api.extremum(greatest, [as_part(p, c) for p in shape], outs=outs), cols, code, [3000])
            expect(got, R.extremum(greatest, [model_part(p, [(v0, m0), (v1, m1)]) for p in shape], dt), [3000], f"extremum {name} {shape}")


# ---------------------------------------------------------------- nanvl
@pytest.mark.parametrize("name", R.FLOATS)
def test_nanvl(api, name):
    code, dt = CODES[name], R.DTYPES[name]
    (av, am), (bv, bm) = columns(name, 2, N, seed=7)
    lens = lengths_for(N)
    nan = float("nan")
    for (a, b), bitmap in (((("col", 0), ("col", 1)), True), ((("col", 2), ("col", 3)), False), ((("col", 0), 123.0), True), ((("col", 2), 123.0), False),
                           ((("col", 0), None), True), ((nan, ("col", 1)), True), ((nan, ("col", 3)), False), ((1.5, ("col", 1)), True), ((("col", 2), ("col", 1)), True)):
        data = [(av, am), (bv, bm), (av, None), (bv, None)]
        cols = [chunks(v, m, lens, k + 2, code) for k, (v, m) in enumerate(data)]
        got = four_ways(lambda c, outs: api.nanvl(as_part(a, c), as_part(b, c), outs=outs), cols, code, lens, bitmap)
        expect(got, R.nanvl(model_part(a, data), model_part(b, data), dt), lens, f"nanvl {name} {a} {b}")


# ---------------------------------------------------------------- the long input
@functools.lru_cache(maxsize=None)
def big(name, k):
    rng = np.random.default_rng(40 + k)
    data = [(R.random_values(name, BIG, rng), rng.uniform(size=BIG) > 0.1) for _ in range(k)]
    bounds = [0] + CUTS + [BIG]
    return data, [b - a for a, b in zip(bounds[:-1], bounds[1:])]


@pytest.mark.parametrize("name", ["f64", "i32", "u8"])
def test_the_big_input_in_seven_unequal_chunks(api, name):
    code, dt = CODES[name], R.DTYPES[name]
    data, lens = big(name, 3)
    assert sorted(lens)[:2] == [0, 1] and len(lens) == 7 and sum(lens) == BIG
    cols = [chunks(v, m, lens, k, code) for k, (v, m) in enumerate(data)]
    expect(four_ways(lambda c, outs: api.coalesce(c, outs=outs), cols, code, lens), R.coalesce(data, dt), lens, f"coalesce {name} big")
    expect(four_ways(lambda c, outs: api.coalesce([c[0], 7], outs=outs), cols, code, lens), R.coalesce([data[0], 7], dt), lens, f"fill_null {name} big")
    for greatest in (True, False):
        expect(four_ways(lambda c, outs: api.extremum(greatest, c, outs=outs), cols, code, lens), R.extremum(greatest, data, dt), lens, f"extremum {name} big")
    conds = conditions(2, BIG, 9)
    ccols = [chunks(c, m, lens, k + 3, A.BOOL) for k, (c, m) in enumerate(conds)]
    got = four_ways(lambda c, outs: api.case_when(c[3:], c[:2], c[2], outs=outs), cols + ccols, code, lens)
    expect(got, R.case_when(conds, data[:2], data[2], dt), lens, f"case_when {name} big")
    if name == "f64":
        expect(four_ways(lambda c, outs: api.nanvl(c[0], c[1], outs=outs), cols, code, lens), R.nanvl(data[0], data[1], dt), lens, "nanvl big")
        mask = four_ways(lambda c, outs: api.null_test("is_nan", c[0], outs=outs), cols[:1], A.BOOL, lens, False)
        expect(mask, (R.null_test(R.IS_NAN, *data[0]), np.ones(BIG, dtype=bool)), lens, "is_nan big")


# ---------------------------------------------------------------- the results feed the calls that were there
def test_the_sign_of_a_nullable_column_as_group_by_key(api):
    """sign(x) = least(greatest(coalesce(x, 0), -1), 1) on device-resident chunks, each call fed by the one before, as the key of rdf_groupby_agg."""
    data, lens = big("i32", 3)
    v, m = data[0]
    x = [to_device(c) for c in chunks(v, m, lens, 0, A.I32)]
    sign = api.least([api.greatest([api.coalesce([x, 0]), -1]), 1])
    assert all(o.null_count == 0 for o in sign)
    keys, _, counts = api.groupby_agg([sign], None, "count", 16,
                                      outs=([api._window_out(A.I32, 18, True, True)], api._window_out(A.I64, 18, True, False), api._window_out(A.I64, 18, True, False)))
    k = keys[0].keep[0].cpu().numpy().view(np.int32)[:keys[0].length]
    c = counts.keep[0].cpu().numpy().view(np.int64)[:counts.length]
    want_k, want_c = np.unique(np.sign(np.where(m, v, 0)), return_counts=True)
    assert dict(zip(k.tolist(), c.tolist())) == dict(zip(want_k.tolist(), want_c.tolist()))
