"""rdf_utf8_dictionary_encode / rdf_groupby_agg_keys / rdf_equijoin_indices_keys on the MI355X, held to the pure-Python
reference tests/text_keys_ref.py.  Everything is exact: codes, validity and dictionary bytes equal factorize; GROUP BY results
are compared as sets of (key tuple, value, count) with integer-valued data (every order of addition is exact); joins as
multisets of pairs, and in the documented order for INNER and LEFT.  Every case runs over host and device memory, on the
automatic route and with the exact route forced, and every call is made twice with the two answers compared."""
import ctypes as C
import functools
from collections import Counter

import numpy as np
import pytest

import text_keys_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MEMS = ["host", "device"]
ROUTES = [0, 1]


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


# ---------------------------------------------------------------- inputs and outputs

def utf8(rows, row_offset=0, data_offset=0):
    """rows: bytes or None; row_offset junk rows (and validity bits) and data_offset junk bytes in front make the chunk look
    like a slice."""
    enc = [b"j" * (i % 3 + 1) for i in range(row_offset)] + [b"" if r is None else r for r in rows]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in enc]) if enc else []
    data = np.frombuffer(b"\xee" * data_offset + b"".join(enc) + b"\0" * 8, dtype=np.uint8).copy()
    nulls = sum(r is None for r in rows)
    valid = None
    if nulls:
        junk = [(i % 2) == 0 for i in range(row_offset)]
        valid = A.pack_bits(np.array(junk + [r is not None for r in rows], dtype=bool))
    return A.HostUtf8(offs.astype(np.int32), data, valid, row_offset, len(rows), data_offset, nulls)


def num(values, dtype, valid=None, offset=0):
    return A.HostArray.from_numpy(np.asarray(values, dtype=dtype), valid, offset=offset)


def num_col(values, dtype, cuts=()):
    """A python column (None = NULL) as chunks cut at `cuts`."""
    bounds = [0] + list(cuts) + [len(values)]
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        part = values[a:b]
        valid = [v is not None for v in part]
        out.append(num([0 if v is None else v for v in part], dtype, None if all(valid) else valid))
    return out


def text_col(values, cuts=(), offsets=None):
    bounds = [0] + list(cuts) + [len(values)]
    out = []
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        ro, do = offsets[i] if offsets else (0, 0)
        out.append(utf8(values[a:b], ro, do))
    return out


def to_device(x):
    if isinstance(x, A.HostUtf8):
        return A.DeviceUtf8.from_host(x)
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def place(chunks, mem):
    return list(chunks) if mem == "host" else [to_device(c) for c in chunks]


def text_rows(u):
    """A Utf8 result as a list of bytes (None = NULL)."""
    h = u.to_host() if isinstance(u, A.DeviceUtf8) else u
    o = h.offsets[h.offset:h.offset + h.length + 1].astype(np.int64) + h.data_offset
    raw = h.data.tobytes()
    return [raw[o[i]:o[i + 1]] if ok else None for i, ok in enumerate(h.valid_mask())]


def num_rows(arr):
    vals, valid = A.Api.window_agg_to_numpy(arr)
    return [v.item() if ok else None for v, ok in zip(vals, valid)]


# ---------------------------------------------------------------- encode

def encode_once(api, chunks):
    codes, dic, count = api.utf8_dictionary_encode(chunks)
    assert len(codes) == len(chunks)
    out = []
    for c, ch in zip(codes, chunks):
        vals, valid = A.Api.window_agg_to_numpy(c)
        assert c.length == ch.length and len(vals) == ch.length
        assert c.null_count == int((~valid).sum())
        assert (vals[~valid] == 0).all()                # a NULL code is value 0 under a clear bit
        out.append((vals.tobytes(), np.packbits(valid).tobytes()))
    d = text_rows(dic)
    assert count == len(d) and dic.null_count == 0
    h = dic.to_host() if isinstance(dic, A.DeviceUtf8) else dic
    assert h.length == 0 or int(h.offsets[0]) == 0       # the dictionary's offsets start at 0
    return out, d, [[v.item() if ok else None for v, ok in zip(*A.Api.window_agg_to_numpy(c))] for c in codes]


def run_encode(api, host_chunks, mem, route):
    lib.set_option("uniques_route", route)
    chunks = place(host_chunks, mem)
    raw1, d1, codes = encode_once(api, chunks)
    raw2, d2, _ = encode_once(api, chunks)
    assert raw1 == raw2 and d1 == d2                    # the same bytes, whatever the scheduling
    return codes, d1


def long_rows():
    rows = []
    for i, n in enumerate((0, 7, 8, 9, 511, 512, 513, 1100)):
        base = bytes((j * 7 + i) % 251 for j in range(n))
        rows.append(base)
        if n:
            rows.append(base[:-1] + bytes([(base[-1] + 1) % 256]))   # shares all but the last byte
            rows.append(base[:-1])                                  # differs only in length
        rows.append(base + b"\0")                                   # ... and by a trailing 0x00
        rows.append(base)                                           # a repeat far from its first occurrence
    return rows + rows[::-1]


def city_like(n, distinct, null_every, seed):
    rng = np.random.default_rng(seed)
    names = [("city-%d-%s" % (i, "x" * (i % 23))).encode() for i in range(distinct)]
    pick = rng.integers(0, distinct, size=n)
    rows = [names[j] for j in pick]
    if null_every:
        for i in rng.choice(n, size=n // null_every, replace=False):
            rows[i] = None
    return rows


@functools.lru_cache(maxsize=None)
def encode_case(name):
    """-> (host chunks, expected codes per chunk, expected dictionary); built and factorized once."""
    if name == "hand":
        lists = [[b"b", None, b"a", b"b", b""]]
        chunks = [utf8(lists[0])]
    elif name == "nul_bytes":
        lists = [[b"a", b"a\0", b"a\0b", b"a\0", b"a", b"a\0b"]]
        chunks = [utf8(lists[0])]
    elif name == "zero_chunks":
        lists, chunks = [], []
    elif name == "zero_rows":
        lists = [[]]
        chunks = [utf8([])]
    elif name == "empty_between":
        lists = [[], [b"x", None, b"y"], [], [], [b"y", b"x", b"z"], []]
        chunks = [utf8(x) for x in lists]
    elif name == "all_null":
        lists = [[None] * 70, [None] * 3]
        chunks = [utf8(x) for x in lists]
    elif name == "all_equal":
        lists = [[b"same"] * 300, [b"same"] * 45]
        chunks = [utf8(x) for x in lists]
    elif name == "all_distinct":
        lists = [[b"v%d" % i for i in range(600)]]
        chunks = [utf8(lists[0])]
    elif name == "slices":
        rows = city_like(37 + 5 + 295, 40, 5, 11)
        rows[0] = rows[36] = rows[38] = rows[41] = rows[42] = rows[-1] = None   # NULLs at both ends of every chunk
        lists = [rows[:37], rows[37:42], rows[42:]]
        assert all(None in x for x in lists)
        chunks = [utf8(lists[0], 0, 0), utf8(lists[1], 3, 13), utf8(lists[2], 7, 5)]   # validity at bit offsets 0, 3 and 7
    elif name == "long_rows":
        rows = long_rows()
        lists = [rows[:31], rows[31:]]
        chunks = [utf8(lists[0]), utf8(lists[1], 2, 3)]
    elif name == "cities_20001":
        rows = city_like(20001, 3000, 10, 5)
        lists = [rows[:7000], rows[7000:7001], rows[7001:]]
        chunks = [utf8(x) for x in lists]
    elif name == "distinct_20001":
        lists = [[b"row-%d" % i for i in range(20001)]]
        chunks = [utf8(lists[0])]
    elif name == "distinct_5000":
        rows = [b"k%d" % (i % 5000) for i in range(7001)]
        lists = [rows[:4000], rows[4000:]]
        chunks = [utf8(x) for x in lists]
    else:
        raise KeyError(name)
    codes, dic = R.factorize(lists)
    return chunks, codes, dic


ENCODE_CASES = ["hand", "nul_bytes", "zero_chunks", "zero_rows", "empty_between", "all_null", "all_equal", "all_distinct", "slices",
                "long_rows", "cities_20001", "distinct_20001"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("name", ENCODE_CASES)
def test_encode_equals_factorize(api, name, mem, route):
    chunks, exp_codes, exp_dict = encode_case(name)
    codes, dic = run_encode(api, chunks, mem, route)
    assert dic == exp_dict
    assert codes == exp_codes
    if name != "zero_chunks" and sum(c.length for c in chunks) > 0:
        assert ("lexsort" in lib.last_kernel()) == (route == 1), lib.last_kernel()


def test_hand_cases_spelled_out(api):
    codes, dic = run_encode(api, [utf8([b"b", None, b"a", b"b", b""])], "host", 0)
    assert codes == [[0, None, 1, 0, 2]] and dic == [b"b", b"a", b""]
    codes, dic = run_encode(api, [utf8([b"a", b"a\0", b"a\0b"])], "host", 0)
    assert codes == [[0, 1, 2]] and dic == [b"a", b"a\0", b"a\0b"]


@pytest.mark.parametrize("mem", MEMS)
def test_a_table_that_gives_up_hands_over_to_the_exact_route(api, mem):
    chunks, exp_codes, exp_dict = encode_case("distinct_5000")
    lib.set_option("uniques_table_bits", 10)            # 1024 slots, filled to half: 5000 values do not fit
    codes, dic = run_encode(api, chunks, mem, 0)
    assert "lexsort" in lib.last_kernel(), lib.last_kernel()
    assert dic == exp_dict and codes == exp_codes
    lib.set_option("uniques_table_bits", 24)
    codes2, dic2 = run_encode(api, chunks, mem, 0)
    assert "lexsort" not in lib.last_kernel()
    assert dic2 == dic and codes2 == codes


class RawEncode:
    """The entry point itself with caller-chosen capacities over sentinel-filled buffers (host or device memory)."""

    def __init__(self, chunks, mem, code_caps, offs_cap, data_cap):
        self.device = mem == "device"
        self.chunks = place(chunks, mem)
        self.bufs = []
        tag = A.MEM_DEVICE if self.device else A.MEM_HOST
        self.codes = (A.rdf_out * max(1, len(chunks)))()
        for i, cap in enumerate(code_caps):
            v, b = self._buf(cap * 4 + 8), self._buf(cap // 8 + 16)
            self.codes[i] = A.rdf_out(self._ptr(v), self._ptr(b), cap, -5, -5, A.U32, tag)
        ob = self._buf(offs_cap * 4 + 8)
        db = self._buf(data_cap + 8) if data_cap else None
        self.offs = (A.rdf_out * 1)(A.rdf_out(self._ptr(ob), None, offs_cap, -5, -5, A.I32, tag))
        self.data = (A.rdf_out * 1)(A.rdf_out(self._ptr(db) if db is not None else None, None, data_cap, -5, -5, A.U8, tag))
        self.count = C.c_int64(-5)

    def _buf(self, nbytes):
        b = np.full(nbytes, 0x5A, dtype=np.uint8)
        if self.device:
            b = torch.from_numpy(b).cuda()
        self.bufs.append(b)
        return b

    def _ptr(self, b):
        return b.data_ptr() if self.device else b.ctypes.data

    def untouched(self):
        return all(bool((b == 0x5A).all()) for b in self.bufs)

    def call(self):
        so = lib.load()
        so.rdf_utf8_dictionary_encode.restype = C.c_int
        carr = (A.rdf_utf8_array * max(1, len(self.chunks)))(*[c.c_struct() for c in self.chunks])
        return so.rdf_utf8_dictionary_encode(carr, C.c_int64(len(self.chunks)), self.codes, self.offs, self.data, C.byref(self.count))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
def test_sizing_call_and_short_capacities(api, mem, route):
    lib.set_option("uniques_route", route)
    chunks, exp_codes, exp_dict = encode_case("slices")
    rows = [c.length for c in chunks]
    nd, nb = len(exp_dict), sum(len(x) for x in exp_dict)
    # the sizing call: no data buffer at all
    r = RawEncode(chunks, mem, rows, nd + 1, 0)
    assert r.call() == A.RDF_MEMORY_ERROR
    assert r.count.value == nd and r.data[0].length == nb and r.offs[0].length == nd + 1
    assert [r.codes[i].length for i in range(3)] == rows
    assert r.untouched()
    # the real call into exactly those sizes
    r = RawEncode(chunks, mem, rows, nd + 1, nb)
    assert r.call() == A.RDF_OK
    assert r.count.value == nd and r.data[0].length == nb and r.offs[0].length == nd + 1
    assert [r.codes[i].length for i in range(3)] == rows
    assert [r.codes[i].null_count for i in range(3)] == [sum(v is None for v in x) for x in exp_codes]
    # each of the three outputs short in turn: lengths reported, nothing written
    for caps, oc, dc in (([rows[0], rows[1] - 1, rows[2]], nd + 1, nb), (rows, nd, nb), (rows, nd + 1, nb - 1)):
        r = RawEncode(chunks, mem, caps, oc, dc)
        assert r.call() == A.RDF_MEMORY_ERROR, (caps, oc, dc)
        assert r.count.value == nd and r.data[0].length == nb and r.offs[0].length == nd + 1
        assert [r.codes[i].length for i in range(3)] == rows
        assert r.untouched(), (caps, oc, dc)


# ---------------------------------------------------------------- GROUP BY

def groupby_once(api, key_chunks, value_chunks, agg, max_groups):
    keys, vals, counts = api.groupby_agg_keys(key_chunks, value_chunks, agg, max_groups)
    cols = [text_rows(k) if isinstance(k, (A.HostUtf8, A.DeviceUtf8)) else num_rows(k) for k in keys]
    v, c = num_rows(vals), num_rows(counts)
    if agg == "count" or value_chunks is None:   # rows are counted: the counts are the answer (the reference repeats them)
        v = c
    assert len(v) == len(c) and all(len(col) == len(v) for col in cols)
    rows = list(zip(zip(*cols), v, c))
    assert len(set(rows)) == len(rows)
    return set(rows)


def run_groupby(api, key_host, value_host, agg, max_groups, mem, route):
    lib.set_option("uniques_route", route)
    keys = [place(k, mem) for k in key_host]
    vals = place(value_host, mem) if value_host is not None else None
    a = groupby_once(api, keys, vals, agg, max_groups)
    b = groupby_once(api, keys, vals, agg, max_groups)
    assert a == b
    return a


def expected_groups(key_lists, values, agg):
    return {(k, v, c) for k, (v, c) in R.groupby(key_lists, values, agg).items()}


@functools.lru_cache(maxsize=None)
def groupby_data():
    rng = np.random.default_rng(3)
    n = 203
    names = [None, b"", b"leeds", b"york", b"bath", b"a\0", b"a", b"wells" * 120]
    text = [names[j] for j in rng.integers(0, len(names), size=n)]
    text2 = [(None, b"n", b"s", b"e")[j] for j in rng.integers(0, 4, size=n)]
    ints = [None if j == 0 else int(j) - 3 for j in rng.integers(0, 6, size=n)]
    vals = [None if j % 7 == 0 else int(j) - 40 for j in rng.integers(0, 90, size=n)]
    return text, text2, ints, vals


CUTS = (64, 65, 150)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("vdtype", [np.int64, np.float64])
@pytest.mark.parametrize("agg", ["sum", "min", "max", "count"])
def test_groupby_one_text_key(api, agg, vdtype, mem, route):
    text, _, _, vals = groupby_data()
    got = run_groupby(api, [text_col(text, CUTS, [(0, 0), (3, 2), (7, 9), (1, 0)])], num_col(vals, vdtype, CUTS), agg, 16, mem, route)
    assert got == expected_groups([text], vals, agg)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
def test_groupby_text_and_int32_keys(api, mem, route):
    text, _, ints, vals = groupby_data()
    got = run_groupby(api, [text_col(text, CUTS), num_col(ints, np.int32, CUTS)], num_col(vals, np.int64, CUTS), "sum", 64, mem, route)
    assert got == expected_groups([text, ints], vals, "sum")
    got = run_groupby(api, [num_col(ints, np.int32, CUTS), text_col(text, CUTS)], num_col(vals, np.int64, CUTS), "max", 64, mem, route)
    assert got == expected_groups([ints, text], vals, "max")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
def test_groupby_two_text_keys_and_row_counts(api, mem, route):
    text, text2, _, vals = groupby_data()
    got = run_groupby(api, [text_col(text, CUTS), text_col(text2, CUTS)], num_col(vals, np.float64, CUTS), "sum", 40, mem, route)
    assert got == expected_groups([text, text2], vals, "sum")
    got = run_groupby(api, [text_col(text, CUTS), text_col(text2, CUTS)], None, "sum", 40, mem, route)   # values == NULL: rows
    assert got == expected_groups([text, text2], None, "count")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
def test_groupby_max_groups_below_the_groups(api, mem, route):
    lib.set_option("uniques_route", route)
    text, _, _, vals = groupby_data()
    ngroups = len(set(text) - {None})   # as for rdf_groupby_agg, the NULL group does not count against max_groups
    with pytest.raises(A.RdfError) as ei:
        api.groupby_agg_keys([place(text_col(text, CUTS), mem)], place(num_col(vals, np.int64, CUTS), mem), "sum", ngroups - 1)
    assert ei.value.status == A.RDF_MEMORY_ERROR


@pytest.mark.parametrize("mem", MEMS)
def test_groupby_numeric_keys_only_is_groupby_agg(api, mem):
    _, _, ints, vals = groupby_data()
    wide = [None if v is None else v * 1000003 for v in ints]
    keys = [place(num_col(ints, np.int32, CUTS), mem), place(num_col(wide, np.int64, CUTS), mem)]
    values = place(num_col(vals, np.int64, CUTS), mem)
    got = groupby_once(api, keys, values, "sum", 32)
    ok, ov, oc = api.groupby_agg(keys, values, "sum", 32, outs=None if mem == "host" else (
        [A.Api._window_out(A.I32, 34, True, True), A.Api._window_out(A.I64, 34, True, True)], A.Api._window_out(A.I64, 34, True, False),
        A.Api._window_out(A.I64, 34, True, False)))
    plain = set(zip(zip(*[num_rows(k) for k in ok]), num_rows(ov), num_rows(oc)))
    assert got == plain == expected_groups([ints, wide], vals, "sum")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
def test_groupby_20001_rows_over_300_text_keys(api, mem, route):
    rows = city_like(20001, 300, 10, 9)
    rng = np.random.default_rng(4)
    vals = [None if j == 0 else int(j) for j in rng.integers(0, 50, size=20001)]
    cuts = (5000, 5001, 13000)
    got = run_groupby(api, [text_col(rows, cuts)], num_col(vals, np.float64, cuts), "sum", 400, mem, route)
    assert got == expected_groups([rows], vals, "sum")


# ---------------------------------------------------------------- join

def pairs_of(ol, orr):
    left, right = num_rows(ol), num_rows(orr)
    assert len(left) == len(right)
    return list(zip(left, right))


def run_join(api, left_host, right_host, how, mem, route):
    lib.set_option("uniques_route", route)
    left = [place(c, mem) for c in left_host]
    right = [place(c, mem) for c in right_host]
    a = pairs_of(*api.equijoin_indices_keys(left, right, how))
    b = pairs_of(*api.equijoin_indices_keys(left, right, how))
    assert Counter(a) == Counter(b)
    assert api.equijoin_indices_keys(left, right, how, count_only=True) == len(a)   # the count-only call
    return a


def check_join(pairs, left_lists, right_lists, how):
    assert Counter(pairs) == R.equijoin(left_lists, right_lists, how)
    if how in ("inner", "left"):
        assert pairs == R.ordered_pairs(left_lists, right_lists, how)   # probe rows ascending, partners ascending


@functools.lru_cache(maxsize=None)
def join_data():
    # duplicates on both sides, values on one side only ("left-only", "right-only", ""), NULLs on both sides
    left = [b"a", None, b"b", b"a", b"left-only", b"c", None, b"b", b"a\0", b"c" * 600, b"b"]
    right = [None, b"a", b"right-only", b"c", b"c", b"", b"a", None, b"c" * 600, b"a\0b"]
    return left, right


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("how", ["left", "right", "inner", "full"])
def test_join_on_one_text_pair(api, how, mem, route):
    left, right = join_data()
    # the two sides chunked differently, the right one behind junk rows and bytes
    pairs = run_join(api, [text_col(left, (4, 5))], [text_col(right, (7,), [(3, 4), (0, 0)])], how, mem, route)
    check_join(pairs, [left], [right], how)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("how", ["left", "right", "inner", "full"])
def test_join_with_an_empty_side(api, how, mem, route):
    left, _ = join_data()
    pairs = run_join(api, [text_col(left, (4,))], [text_col([])], how, mem, route)
    check_join(pairs, [left], [[]], how)
    pairs = run_join(api, [text_col([])], [text_col(left, (4,))], how, mem, route)
    check_join(pairs, [[]], [left], how)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("how", ["left", "right", "inner", "full"])
def test_join_on_a_text_and_an_int64_pair(api, how, mem, route):
    left, right = join_data()
    lnum = [1, 1, None, 2, 1, 1, 1, 2, 1, 1, 2]
    rnum = [1, 1, 1, 1, None, 1, 2, 1, 1, 1]
    pairs = run_join(api, [text_col(left, (4, 5)), num_col(lnum, np.int64, (4, 5))], [text_col(right, (7,)), num_col(rnum, np.int64, (7,))],
                     how, mem, route)
    check_join(pairs, [left, lnum], [right, rnum], how)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
def test_join_5000_by_2000_rows_over_500_values(api, mem, route):
    left = city_like(5000, 500, 10, 21)
    right = city_like(2000, 500, 10, 22)
    pairs = run_join(api, [text_col(left, (1234, 3000))], [text_col(right, (77,))], "left", mem, route)
    check_join(pairs, [left], [right], "left")
