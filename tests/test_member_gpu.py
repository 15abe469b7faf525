"""rdf_member_mask / rdf_first_occurrence on the MI355X, held to the pure-Python model tests/member_ref.py.  Every comparison
is bit for bit on each chunk's `length` bits (value and validity), plus null_count and *out_rows; every call is made twice
and the two answers' bytes compared; the count-only call must agree with the full one."""
import functools

import numpy as np
import pytest

import hash_fixtures as FX
import hash_models as H
import member_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KINDS = [R.SEMI, R.ANTI, R.IS_IN]
KEEPS = [R.FIRST, R.LAST, R.NONE]
LEFT_ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 7]
EMPTY = 0xFFF7A5A55A5A0001          # the free marker of a table of key words (a key equal to it is set aside in a flag)
MUL = 0x9E3779B97F4A7C15


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
    for name in ("member_route", "member_slots", "member_table_bits", "uniques_route"):
        lib.set_option(name, 0)
    lib.set_option("uniques_table_bits", 24)


# ---------------------------------------------------------------- inputs

def cuts_of(n, layout):
    """chunk lengths: the whole column, or (1, 63, 64, 65, 0, 130, ...) repeated until the rows are used up"""
    if layout == "one":
        return [n]
    out, left, pattern, i = [], n, (1, 63, 64, 65, 0, 130, 2048, 5, 700), 0
    while left > 0:
        c = min(left, pattern[i % len(pattern)])
        out.append(c)
        left -= c
        i += 1
    return out or [0]


def np_col(values, dtype):
    """python values (None = NULL) -> (numpy array of dtype, valid)"""
    valid = np.array([v is not None for v in values], dtype=bool)
    arr = np.array([0 if v is None else v for v in values], dtype=dtype) if len(values) else np.zeros(0, dtype=dtype)
    return arr, valid


def chunks(values, dtype, lens, sliced):
    """a python column as HostArray / HostUtf8 chunks of the given lengths; sliced: input offsets 0..9 (validity then starts at
    that bit: odd bit offsets included)"""
    out, at = [], 0
    for i, n in enumerate(lens):
        part = values[at:at + n]
        at += n
        off = (i * 3 + 1) % 10 if sliced else 0
        if dtype == "utf8":
            out.append(utf8(part, off))
            continue
        arr, valid = np_col(part, np.uint8 if dtype == "bool" else dtype)
        out.append(A.HostArray.from_numpy(arr.astype(bool) if dtype == "bool" else arr, None if valid.all() else valid, offset=off,
                                          dtype=A.BOOL if dtype == "bool" else None))
    return out


def utf8(rows, row_offset=0):
    enc = [b"j" * (i % 3 + 1) for i in range(row_offset)] + [b"" if r is None else r for r in rows]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in enc]) if enc else []
    data = np.frombuffer(b"\xee\xee\xee" + b"".join(enc) + b"\0" * 8, dtype=np.uint8).copy()
    nulls = sum(r is None for r in rows)
    valid = None
    if nulls:
        valid = A.pack_bits(np.array([(i % 2) == 0 for i in range(row_offset)] + [r is not None for r in rows], dtype=bool))
    return A.HostUtf8(offs.astype(np.int32), data, valid, row_offset, len(rows), 3, nulls)


def to_device(x):
    if isinstance(x, A.HostUtf8):
        return A.DeviceUtf8.from_host(x)
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def place(cols, mem):
    return [list(c) if mem == "host" else [to_device(x) for x in c] for c in cols]


def side(columns, dtypes, layout, mem):
    """columns: one python list per key -> the key columns as chunk lists in `mem`"""
    n = len(columns[0])
    lens = cuts_of(n, layout)
    return place([chunks(c, d, lens, layout != "one") for c, d in zip(columns, dtypes)], mem), lens


def model_rows(columns, dtypes):
    """the rows the model sees: float32 columns rounded as the column stores them"""
    cols = []
    for c, d in zip(columns, dtypes):
        if d == np.float32:
            c = [None if v is None else float(np.float32(v)) for v in c]
        elif d == "bool":
            c = [None if v is None else bool(v) for v in c]
        cols.append(c)
    return list(zip(*cols)) if cols and len(cols[0]) else []


# ---------------------------------------------------------------- outputs

def out_bytes(o):
    """(value bytes, validity bytes or None) of the chunk's `length` bits"""
    nb = (o.length + 7) // 8
    if isinstance(o, A.HostArray):
        return o.values[:nb].tobytes(), (o.validity[:nb].tobytes() if o.validity is not None else None)
    t, v = o.keep
    return t.cpu().numpy().view(np.uint8)[:nb].tobytes(), (v.cpu().numpy()[:nb].tobytes() if v is not None else None)


def read_mask(outs, lens):
    """-> the model's form: True / False / None per row, after checking lengths, the tail bits and null_count"""
    rows = []
    for o, n in zip(outs, lens):
        assert o.length == n
        vb, kb = out_bytes(o)
        bits = A.unpack_bits(np.frombuffer(vb, dtype=np.uint8), 0, n)
        valid = A.unpack_bits(np.frombuffer(kb, dtype=np.uint8), 0, n) if kb is not None else np.ones(n, dtype=bool)
        if n % 8:                                         # the tail of the last byte is masked
            assert vb[-1] >> (n % 8) == 0 and (kb is None or kb[-1] >> (n % 8) == 0)
        assert not (bits & ~valid).any()                  # the value bit of a NULL slot is 0
        assert o.null_count == int((~valid).sum())
        rows += [bool(b) if ok else None for b, ok in zip(bits, valid)]
    return rows


def check_member(api, lcols, rcols, dtypes, kind, layout="one", mem="device", rlayout=None, expect_kernel=None):
    want = R.member_mask(model_rows(lcols, dtypes), model_rows(rcols, dtypes), kind)
    L, lens = side(lcols, dtypes, layout, mem)
    Rr, _ = side(rcols, dtypes, rlayout or layout, mem)
    outs, rows = api.member_mask(L, Rr, kind)
    if expect_kernel and len(want):
        assert expect_kernel in lib.last_kernel(), lib.last_kernel()
    got = read_mask(outs, lens)
    assert got == want
    assert rows == R.true_rows(want)
    if kind != R.IS_IN:
        assert all(o.null_count == 0 for o in outs)
    outs2, rows2 = api.member_mask(L, Rr, kind)
    assert rows2 == rows and [out_bytes(o) for o in outs2] == [out_bytes(o) for o in outs]
    assert api.member_mask(L, Rr, kind, count_only=True) == rows
    return got


def check_first(api, cols, dtypes, keep, layout="one", mem="device"):
    want = R.first_occurrence(model_rows(cols, dtypes), keep)
    K, lens = side(cols, dtypes, layout, mem)
    outs, rows = api.first_occurrence(K, keep)
    got = read_mask(outs, lens)
    assert got == want
    assert rows == sum(want) and all(o.null_count == 0 for o in outs)
    if len(want):
        assert "member_fold_kernel + member_first_kernel" in lib.last_kernel()
    outs2, rows2 = api.first_occurrence(K, keep)
    assert rows2 == rows and [out_bytes(o) for o in outs2] == [out_bytes(o) for o in outs]
    assert api.first_occurrence(K, keep, count_only=True) == rows
    return got


def random_keys(rng, n, span, null_fraction):
    return [None if rng.random() < null_fraction else int(v) for v in rng.integers(-span, span, size=n)]


# ---------------------------------------------------------------- rows: the word writer's tail and the chunk walk

@pytest.mark.parametrize("layout", ["one", "cut"])
@pytest.mark.parametrize("n", LEFT_ROWS)
def test_left_rows_and_layouts(api, n, layout):
    rng = np.random.default_rng(n)
    left = random_keys(rng, n, 40, 0.15)
    right = random_keys(rng, 50, 40, 0.1)
    for kind in KINDS:
        check_member(api, [left], [right], [np.int64], kind, layout, "device", rlayout="one")
        if n <= 1025:
            check_member(api, [left], [right], [np.int64], kind, layout, "host", rlayout="cut")
    for keep in KEEPS:
        check_first(api, [left], [np.int64], keep, layout, "device")
        if n <= 1025:
            check_first(api, [left], [np.int64], keep, layout, "host")


# ---------------------------------------------------------------- the right side

def test_right_side_shapes(api):
    rng = np.random.default_rng(3)
    left = random_keys(rng, 700, 30, 0.1)
    for right in ([], [7], [None], [5] * 3000, [None] * 70, list(range(-20, 20)), list(range(3000))):
        for kind in KINDS:
            check_member(api, [left], [right], [np.int64], kind, "cut", "device")
    check_member(api, [left], [[]], [np.int64], R.IS_IN, "one", "host")          # NULL IN () is FALSE


@pytest.mark.parametrize("distinct", [31, 32, 33])
@pytest.mark.parametrize("route", [0, 1, 2])
def test_lds_capacity_boundary(api, distinct, route):
    """"member_slots" = 64: the LDS form holds 32 build rows.  Planned: LDS up to 32, HBM beyond; forced either way."""
    lib.set_option("member_slots", 64)
    lib.set_option("member_route", route)
    rng = np.random.default_rng(distinct)
    right = [int(v) for v in rng.permutation(200)[:distinct] * 977 - 50000]
    left = [None if rng.random() < 0.1 else int(v) * 977 - 50000 for v in rng.integers(0, 200, size=1300)]
    if route == 1 and distinct > 32:
        L, _ = side([left], [np.int64], "one", "device")
        Rr, _ = side([right], [np.int64], "one", "device")
        with pytest.raises(A.RdfError) as ei:
            api.member_mask(L, Rr, R.SEMI)
        assert ei.value.status == A.RDF_INVALID_ARGUMENT and "LDS route" in ei.value.message
        return
    lds = route == 1 or (route == 0 and distinct <= 32)
    for kind in KINDS:
        check_member(api, [left], [right], [np.int64], kind, "cut", "device", rlayout="one",
                     expect_kernel="member_probe_kernel<lds>" if lds else "member_probe_kernel<hbm>")


def test_planned_lds_table(api):
    """the planned LDS form at its own capacity (4096 build rows) and the HBM form just beyond"""
    rng = np.random.default_rng(8)
    left = [int(v) for v in rng.integers(0, 9000, size=5000)]
    check_member(api, [left], [list(range(0, 8192, 2))], [np.int64], R.SEMI, expect_kernel="<lds>")
    check_member(api, [left], [list(range(0, 8194, 2))], [np.int64], R.ANTI, expect_kernel="<hbm>")


def home(value, bits):
    """home slot of an Int64 key in a table of 2^bits slots"""
    word = (value + (1 << 63)) & (2**64 - 1)
    return ((word * MUL) & (2**64 - 1)) >> (64 - bits)


def test_shrunk_table_wraps_and_fills(api):
    lib.set_option("member_table_bits", 4)
    tail = [v for v in range(1, 4000) if home(v, 4) >= 14][:8]          # eight keys whose home is one of the last two slots
    assert len(tail) == 8
    absent = [v for v in range(4000, 9000) if home(v, 4) == 15][:5]
    left = tail + absent + [None, 0] + tail[::-1]
    for route in (1, 2):                                                 # probing wraps round the end, in LDS and in HBM
        lib.set_option("member_route", route)
        for kind in KINDS:
            check_member(api, [left], [tail], [np.int64], kind)
    lib.set_option("member_route", 0)
    for keep in KEEPS:
        check_first(api, [left], [np.int64], keep)
    # sixteen distinct keys fill the table to the last slot: a probe for an absent key still ends
    full = list(range(100, 116))
    check_member(api, [full + absent], [full], [np.int64], R.SEMI)
    # seventeen do not fit: RDF_MEMORY_ERROR, never a partial answer
    L, _ = side([left], [np.int64], "one", "device")
    Rr, _ = side([list(range(100, 117))], [np.int64], "one", "device")
    with pytest.raises(A.RdfError) as ei:
        api.member_mask(L, Rr, R.SEMI)
    assert ei.value.status == A.RDF_MEMORY_ERROR and "member_table_bits" in ei.value.message
    with pytest.raises(A.RdfError) as ei:
        api.first_occurrence(Rr, R.FIRST)
    assert ei.value.status == A.RDF_MEMORY_ERROR


# ---------------------------------------------------------------- keys

INT_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64]


@pytest.mark.parametrize("dtype", INT_DTYPES + [np.float32, np.float64, "bool"])
def test_every_dtype(api, dtype):
    rng = np.random.default_rng(11)
    if dtype == "bool":
        pool = [True, False]
    elif dtype in (np.float32, np.float64):
        pool = [0.0, -0.0, 1.5, -1.5, float("inf"), float("-inf"), 3.0e10, 1e-30]
    else:
        info = np.iinfo(dtype)
        pool = [int(info.min), int(info.max), 0, 1, int(info.max) - 1] + ([-1] if info.min < 0 else [int(info.max) // 2 + 1])
    left = [None if rng.random() < 0.2 else pool[int(i)] for i in rng.integers(0, len(pool), size=300)]
    for right in (pool[:1] if dtype == "bool" else pool[::2], pool[1:2] + [None]):
        for kind in KINDS:
            check_member(api, [left], [right], [dtype], kind, "cut", "device")
    for keep in KEEPS:
        check_first(api, [left], [dtype], keep, "cut", "device")
    check_member(api, [left], [pool[:2]], [dtype], R.SEMI, "cut", "host")


def test_free_marker_and_zero_keys(api):
    """the table's free marker and 0 as Int64 / UInt64 keys, on both sides and on one side only; UInt64 with the top bit set"""
    marker_u64 = EMPTY                      # UInt64 keys are their own key words
    marker_i64 = EMPTY - (1 << 63)          # Int64 key words have the sign bit flipped
    for dtype, marker, other in ((np.uint64, marker_u64, [0, 1 << 63, (1 << 64) - 1, EMPTY ^ 1]),
                                 (np.int64, marker_i64, [0, -(1 << 63), (1 << 63) - 1, marker_i64 + 1])):
        left = [marker, 0, None] + other + [marker, 0]
        for right in ([marker, 0], [marker], [0], other, [None, other[1]], []):
            for kind in KINDS:
                for route in (1, 2):
                    lib.set_option("member_route", route)
                    check_member(api, [left], [right], [dtype], kind)
        lib.set_option("member_route", 0)
        for keep in KEEPS:
            check_first(api, [left], [dtype], keep)


def f64(bits):
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


def test_float_zeros_and_nans(api):
    """-0.0 == +0.0, every NaN equals every NaN (sign and payload), NULLs on either side, all three kinds"""
    nans = [f64(0x7FF8000000000000), f64(0xFFF8000000000000), f64(0x7FF0000000000001), f64(0xFFFFFFFFFFFFFFFF), f64(0x7FF4A5A55A5A0001)]
    left = [0.0, -0.0, None, 1.0] + nans + [-1.0, float("inf")]
    for right in ([-0.0], [0.0, None], [nans[3]], [nans[0], -0.0], [1.0], [None]):
        for kind in KINDS:
            check_member(api, [left], [right], [np.float64], kind)
            check_member(api, [left], [right], [np.float64], kind, mem="host")
    for keep in KEEPS:
        assert check_first(api, [left], [np.float64], keep) == R.first_occurrence([(v,) for v in left], keep)
    # Float32: the same rule on the narrower type
    n32 = [float(np.array([b], dtype=np.uint32).view(np.float32)[0]) for b in (0x7FC00000, 0xFFC00001, 0x7F800001)]
    l32 = [0.0, -0.0, 2.5, None] + n32
    for kind in KINDS:
        check_member(api, [l32], [[-0.0, n32[2]]], [np.float32], kind)
    for keep in KEEPS:
        check_first(api, [l32], [np.float32], keep)


def test_utf8_keys(api):
    """\"\" next to NULL, a value only on the right, and pairs of different strings with one hash split between the sides"""
    left = [b"", None, b"a", b"b", b"", b"a\0", None, b"zz"]
    for right in ([b"", b"only-right"], [None, b"a"], [b"a\0", b""], []):
        for kind in KINDS:
            for mem in ("host", "device"):
                check_member(api, [left], [right], ["utf8"], kind, "cut" if mem == "device" else "one", mem)
    for keep in KEEPS:
        check_first(api, [left], ["utf8"], keep, "cut", "device")
        check_first(api, [left], ["utf8"], keep, "one", "host")
    fx = FX.utf8_fixtures()
    for name in ("adjacent", "tail_7_bytes", "lengths_15_16", "long_512", "free_word"):
        a, b = fx[name][0], fx[name][1]
        assert a != b
        got = check_member(api, [[a, b, a, None]], [[b, b"other"]], ["utf8"], R.SEMI)      # one of the pair left only, the other right only
        assert got == [False, True, False, False]
        check_member(api, [[a, a]], [[b]], ["utf8"], R.ANTI)
        assert check_first(api, [[a, b, a, b]], ["utf8"], R.FIRST) == [True, True, False, False]


NP_OF_H = {H.I32: np.int32, H.I64: np.int64, H.F64: np.float64, H.F32: np.float32}


def as_value(v, d):
    """a fixture component (float columns hold bits) as the python value of the column"""
    if d == H.F64:
        return f64(v)
    if d == H.F32:
        return float(np.array([v], dtype=np.uint32).view(np.float32)[0])
    return int(v)


@pytest.mark.parametrize("nk", [2, 3, 4])
def test_colliding_tuples(api, nk):
    """X != Y share the tuple hash: X on the right only, Y on the left only -> SEMI is FALSE for Y; Z's hash is the one the
    join gives NULL rows; for rdf_first_occurrence X and Y are two tuples"""
    dt, x, y, z = FX.tuple_fixtures()[nk]
    dtypes = [NP_OF_H[d] for d in dt]
    X, Y, Z = (tuple(as_value(v, d) for v, d in zip(t, dt)) for t in (x, y, z))
    assert len({R.canon_row(t) for t in (X, Y, Z)}) == 3
    nullrow = tuple([None] + list(X[1:]))

    def cols(rows):
        return [list(c) for c in zip(*rows)]

    left = [Y, X, Z, nullrow, Y]
    assert check_member(api, cols(left), cols([X, nullrow]), dtypes, R.SEMI) == [False, True, False, False, False]
    assert check_member(api, cols(left), cols([X, nullrow]), dtypes, R.ANTI) == [True, False, True, True, True]
    assert check_member(api, cols(left), cols([Z, Y]), dtypes, R.SEMI, mem="host") == [True, False, True, False, True]
    rows = [X, Y, X, Z, nullrow, Y, nullrow]
    assert check_first(api, cols(rows), dtypes, R.FIRST) == [True, True, False, True, True, False, False]
    assert check_first(api, cols(rows), dtypes, R.LAST) == [False, False, True, True, False, True, True]
    assert check_first(api, cols(rows), dtypes, R.NONE, mem="host") == [False, False, False, True, False, False, False]


def test_tuples_with_text_and_nulls(api):
    rng = np.random.default_rng(21)
    words = [b"", b"x", b"yy", None]
    n = 1500
    a = [words[int(i)] for i in rng.integers(0, 4, size=n)]
    b = [None if rng.random() < 0.2 else int(v) for v in rng.integers(0, 3, size=n)]
    for kind in (R.SEMI, R.ANTI):
        check_member(api, [a, b], [[b"x", b"", None, b"yy"], [1, None, 2, 2]], ["utf8", np.int32], kind, "cut", "device", rlayout="one")
        check_member(api, [a[:200], b[:200]], [[b"x", b""], [1, 0]], ["utf8", np.int32], kind, "one", "host")
    for keep in KEEPS:
        check_first(api, [a, b], ["utf8", np.int32], keep, "cut", "device")
        check_first(api, [a[:200], b[:200]], ["utf8", np.int32], keep, "one", "host")


# ---------------------------------------------------------------- rdf_first_occurrence

def test_first_occurrence_shapes(api):
    for keep, want in ((R.FIRST, [0]), (R.LAST, [1024]), (R.NONE, [])):               # all rows equal at 1025 rows
        for layout in ("one", "cut"):
            got = check_first(api, [[9] * 1025], [np.int64], keep, layout)
            assert [i for i, b in enumerate(got) if b] == want
    for keep in KEEPS:                                                                # all rows distinct
        assert all(check_first(api, [list(range(2000, 0, -1))], [np.int32], keep, "cut"))
    rows = [(None, None), (None, 1), (1, None), (None, None), (1, None), (1, 1)]      # NULL is a value, component-wise
    cols = [list(c) for c in zip(*rows)]
    assert check_first(api, cols, [np.int64, np.int8], R.FIRST) == [True, True, True, False, False, True]
    assert check_first(api, cols, [np.int64, np.int8], R.LAST) == [False, True, False, True, True, True]
    assert check_first(api, cols, [np.int64, np.int8], R.NONE) == [False, True, False, False, False, True]
    # the same rows cut into different chunkings give the same concatenated bits
    rng = np.random.default_rng(4)
    keys = random_keys(rng, 3079, 300, 0.05)
    for keep in KEEPS:
        assert check_first(api, [keys], [np.int64], keep, "one") == check_first(api, [keys], [np.int64], keep, "cut")


# ---------------------------------------------------------------- sizing and composition

def test_short_capacity_leaves_buffers_untouched(api):
    left = [list(range(100)), list(range(70))]
    L = [[to_device(A.HostArray.from_numpy(np.array(c, dtype=np.int64))) for c in left]]
    Rr = [[to_device(A.HostArray.from_numpy(np.arange(5, dtype=np.int64)))]]
    outs = [A.Api._window_out(A.BOOL, 100, True, True), A.Api._window_out(A.BOOL, 69, True, True)]
    for o in outs:
        o.keep[0].fill_(0x5A5A5A5A5A5A5A5A)
        o.keep[1].fill_(0xA5)
    before = [(o.keep[0].clone(), o.keep[1].clone()) for o in outs]
    with pytest.raises(A.RdfError) as ei:
        api.member_mask(L, Rr, R.IS_IN, outs=outs)
    assert ei.value.status == A.RDF_MEMORY_ERROR
    assert [o.length for o in outs] == [100, 70]
    assert all(torch.equal(o.keep[0], b[0]) and torch.equal(o.keep[1], b[1]) for o, b in zip(outs, before))
    with pytest.raises(A.RdfError) as ei:
        api.first_occurrence(L, R.FIRST, outs=outs)
    assert ei.value.status == A.RDF_MEMORY_ERROR and [o.length for o in outs] == [100, 70]
    assert all(torch.equal(o.keep[0], b[0]) and torch.equal(o.keep[1], b[1]) for o, b in zip(outs, before))


def test_semi_mask_feeds_filter_columns(api):
    rng = np.random.default_rng(17)
    n = 1500
    keys = random_keys(rng, n, 25, 0.1)
    payload = [float(i) for i in range(n)]
    right = [3, 4, 5, None, -7]
    lens = cuts_of(n, "cut")
    kc = chunks(keys, np.int64, lens, True)
    pc = chunks(payload, np.float64, lens, False)
    masks, rows = api.member_mask([kc], [[A.HostArray.from_numpy(np.array([0 if v is None else v for v in right], dtype=np.int64),
                                                                 [v is not None for v in right])]], R.SEMI)
    kept = api.filter_columns([kc, pc], masks)
    got_keys = [v for o in kept[0] for v in o.to_pylist()]
    got_pay = [v for o in kept[1] for v in o.to_pylist()]
    want = [i for i, b in enumerate(R.member_mask(keys, right, R.SEMI)) if b]
    assert rows == len(want)
    assert got_keys == [keys[i] for i in want] and got_pay == [payload[i] for i in want]
