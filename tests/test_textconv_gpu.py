"""rdf_utf8_parse / rdf_utf8_format on the MI355X, byte for byte against the model of tests/textconv_ref.py, behind guard bytes,
over host and device memory: values, validity bytes (the zero bits past `length` included), null_count and failed for parse;
offsets, data, validity and null_count under the sizing rule for format; both load forms of the parse kernel, the long rows,
the output widths up to the 256-byte cap, the round trip on the device, and determinism."""
import ctypes as C
import functools

import numpy as np
import pytest

import datetime_ref as D
import textconv_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu

MEMS = ["host", "device"]
CHUNK_ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
LAYOUTS = [(0, 0), (1, 0), (7, 3), (3, 1)]          # (row and validity-bit offset, leading junk bytes of the data buffer)
GUARD = 32
SHORT_ROW = 256       # kUtf8ShortRow of rdf_utf8.h: a longer row of a CAST grammar is taken by its wave
LDS_BYTES = 8192      # kTcLdsBytes of rdf_textconv.h: a tile whose byte span is at most this is staged in LDS
TILE = 256            # kTcTile: rows of one chunk a block takes
assert (SHORT_ROW, LDS_BYTES) == (R.SHORT_ROW, R.LDS_BYTES)
NP_OUT = dict(R.NP_DTYPES)


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    so = lib.load()
    so.rdf_utf8_parse.restype = C.c_int
    return a


class Buf:
    """nbytes bytes followed by GUARD guard bytes, in host or device memory, everything 0xAA; `shift` moves the pointer"""
    def __init__(self, nbytes, mem, shift=0):
        self.n, self.mem, self.shift = nbytes, mem, shift
        if mem == "device":
            import torch
            self.t = torch.full((nbytes + GUARD + shift + 16,), 0xAA, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()   # (the library writes on a stream of its own: the fill has to be there first)
            self.ptr = self.t.data_ptr() + shift
        else:
            self.t = np.full(nbytes + GUARD + shift + 16, 0xAA, dtype=np.uint8)
            self.ptr = self.t.ctypes.data + shift

    def read(self):
        raw = self.t.cpu().numpy() if self.mem == "device" else self.t
        body = raw[self.shift:self.shift + self.n].copy()
        return body, bool((raw[self.shift + self.n:] == 0xAA).all()) and bool((raw[:self.shift] == 0xAA).all())


def text_chunk(rows, valid=None, row_offset=0, data_offset=0):
    """A HostUtf8 of byte rows (any bytes, not only UTF-8).  valid: bool list or None (no validity buffer); row_offset junk rows
    and data_offset junk bytes in front make it a sliced array whose first value offset is not 0."""
    pre = [b"9" * (i % 3 + 1) for i in range(row_offset)]
    enc = pre + [bytes(r) for r in rows]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in enc]) if enc else []
    data = np.frombuffer(b"\xff" * data_offset + b"".join(enc) + b"\0" * 8, dtype=np.uint8).copy()
    vbuf, nulls = None, 0
    if valid is not None:
        vbuf = A.pack_bits(np.array([i % 2 == 0 for i in range(row_offset)] + list(valid), dtype=bool))
        nulls = int(len(valid) - sum(valid))
    return A.HostUtf8(offs.astype(np.int32), data, vbuf, row_offset, len(rows), data_offset, nulls)


def place(chunks, mem):
    return [A.DeviceUtf8.from_host(c) for c in chunks] if mem == "device" else list(chunks)


def to_device(x):
    import torch
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def out_dtype(kind, dtype):
    return {R.BOOL: A.BOOL, R.DATE: A.I32, R.TIMESTAMP: A.I64}.get(kind, dtype)


def run_parse(rows_per_chunk, valid_per_chunk, mem, kind, unit=R.S, dtype=R.I64, pattern=None, layout=(0, 0), expected=None):
    """One rdf_utf8_parse call into guarded buffers, checked against the model.  rows_per_chunk: lists of byte rows;
    valid_per_chunk: bool lists or None.  -> the raw output bytes (values, validity) of every chunk."""
    so = lib.load()
    hosts = [text_chunk(r, v, *layout) for r, v in zip(rows_per_chunk, valid_per_chunk)]
    ins = place(hosts, mem)
    n = len(ins)
    odt = out_dtype(kind, dtype)
    es = 0 if odt == A.BOOL else np.dtype(NP_OUT[odt]).itemsize
    m = A.MEM_DEVICE if mem == "device" else A.MEM_HOST
    co, keep = (A.rdf_out * max(1, n))(), []
    for i, h in enumerate(hosts):
        vb = Buf(h.length * es if es else (h.length + 7) // 8, mem)
        bb = Buf((h.length + 7) // 8, mem)
        co[i] = A.rdf_out(vb.ptr, bb.ptr, h.length, -7, -7, odt, m)
        keep.append((vb, bb))
    carr = (A.rdf_utf8_array * max(1, n))(*[c.c_struct() for c in ins])
    raw = b"" if pattern is None else pattern.encode()
    cp = (C.c_uint8 * max(1, len(raw))).from_buffer_copy(raw or b"\0")
    failed = (C.c_int64 * max(1, n))(*([-7] * max(1, n)))
    st = so.rdf_utf8_parse(carr, C.c_int64(n), C.c_int32(kind), C.c_int32(unit), cp if pattern is not None else None, C.c_int64(len(raw)), co, failed)
    assert st == A.RDF_OK, (st, so.rdf_last_error())
    toks = R.compile_pattern(pattern, True) if pattern is not None else None
    out = []
    for i, (rows, valid) in enumerate(zip(rows_per_chunk, valid_per_chunk)):
        nrows = len(rows)
        exp = expected[i] if expected is not None else [R.parse(kind, t, unit, dtype, toks) for t in rows]
        ok_in = [True] * nrows if valid is None else list(valid)
        good = np.array([a and e is not None for a, e in zip(ok_in, exp)], dtype=bool)
        vals, g1 = keep[i][0].read()
        bits, g2 = keep[i][1].read()
        what = f"kind {kind} unit {unit} dtype {dtype} pattern {pattern!r} {mem} chunk {i}"
        assert g1 and g2, what + ": guard bytes overwritten"
        assert co[i].length == nrows and co[i].null_count == int(nrows - good.sum()), (what, co[i].length, co[i].null_count)
        assert failed[i] == sum(a and e is None for a, e in zip(ok_in, exp)), (what, failed[i])
        want_bits = np.packbits(good.astype(np.uint8), bitorder="little")
        if not np.array_equal(bits, want_bits):
            at = int(np.flatnonzero(np.unpackbits(bits, bitorder="little")[:nrows] != good)[0]) if nrows and not np.array_equal(np.unpackbits(bits, bitorder="little")[:nrows], good) else -1
            raise AssertionError(f"{what}: validity differs at row {at}: {rows[at][:60] if at >= 0 else 'bits past the length'!r} expected {exp[at] if at >= 0 else 0}")
        if kind == R.BOOL:
            want = np.packbits(np.array([bool(g and e) for g, e in zip(good, exp)], dtype=np.uint8), bitorder="little")
        else:
            want = np.array([int(e) if g else 0 for g, e in zip(good, exp)], dtype=object)
            want = np.array([int(x) & (2 ** (8 * es) - 1) for x in want], dtype=np.uint64).astype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[es]).view(np.uint8)
        if not np.array_equal(vals, want):
            at = int(np.flatnonzero(vals != want)[0]) // max(es, 1) * (1 if es else 8)
            raise AssertionError(f"{what}: values differ near row {at}: {rows[min(at, nrows - 1)][:60]!r} expected {exp[min(at, nrows - 1)]}")
        out.append((vals.tobytes(), bits.tobytes()))
    return out


@functools.lru_cache(maxsize=None)
def corpus(kind, unit=R.S, dtype=R.I64, pattern=None):
    """(rows, the model's values): every branch case plus 1500 random rows, computed once per (kind, unit, dtype, pattern)."""
    toks = R.compile_pattern(pattern, True) if pattern is not None else None
    rows = ([] if pattern is not None else R.branch_cases(kind, dtype)) + R.random_cases(kind, 1500, 31 + 7 * kind + unit + 13 * dtype, unit, dtype, toks)
    return rows, [R.parse(kind, t, unit, dtype, toks) for t in rows]


def cut(rows, exp, lens, rng):
    """rows and expectations dealt into chunks of the given lengths (cycling through the corpus), validity on every other chunk"""
    out_rows, out_valid, out_exp, at = [], [], [], 0
    for i, n in enumerate(lens):
        idx = [(at + k) % len(rows) for k in range(n)]
        at += n
        out_rows.append([rows[k] for k in idx])
        out_exp.append([exp[k] for k in idx])
        out_valid.append(list(rng.uniform(size=n) > 0.2) if i % 2 == 0 else None)
    return out_rows, out_valid, out_exp


PARSE_CASES = [(R.BOOL, R.S, 10, None)] + [(R.INT, R.S, dt, None) for dt in R.INT_DTYPES] + [(R.DATE, R.S, R.I32, None), (R.DATE, R.S, R.I32, "yyyy-MM-dd"), (R.DATE, R.S, R.I32, "dd MMM yyyy")] + \
    [(R.TIMESTAMP, u, R.I64, None) for u in (R.S, R.MS, R.US, R.NS)] + [(R.TIMESTAMP, u, R.I64, p) for u, p in ((R.S, "yyyy-MM-dd"), (R.MS, "yyyy-MM-dd'T'HH:mm:ss.SSS"), (R.US, "MM/dd/yyyy hh:mm:ss a"), (R.NS, "yyyy-MM-dd HH:mm:ss.SSSSSSSSS"), (R.S, "yyyy DDD"))]


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("kind,unit,dtype,pattern", PARSE_CASES)
def test_parse_every_kind_dtype_and_unit(api, mem, kind, unit, dtype, pattern):
    rows, exp = corpus(kind, unit, dtype, pattern)
    r, v, e = cut(rows, exp, [0, 1000, 0, 1, 63, 64, 0, 65, 255, 256, 257], np.random.default_rng(5))
    first = run_parse(r, v, mem, kind, unit, dtype, pattern, expected=e)
    assert run_parse(r, v, mem, kind, unit, dtype, pattern, expected=e) == first, "two runs differ"


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("layout", LAYOUTS[1:])
def test_parse_sliced_layouts(api, mem, layout):
    for kind, unit, dtype in ((R.INT, R.S, R.I16), (R.TIMESTAMP, R.MS, R.I64), (R.BOOL, R.S, 10)):
        rows, exp = corpus(kind, unit, dtype)
        r, v, e = cut(rows, exp, [65, 0, 257, 64], np.random.default_rng(6))
        run_parse(r, v, mem, kind, unit, dtype, None, layout, expected=e)
        run_parse(r, [None if x is not None else [True] * len(rr) for x, rr in zip(v, r)], mem, kind, unit, dtype, None, layout, expected=e)


@pytest.mark.parametrize("span", [LDS_BYTES - 1, LDS_BYTES, LDS_BYTES + 1])
def test_parse_both_load_forms_give_the_same_bytes_at_the_lds_budget(api, span):
    """A tile whose rows hold exactly `span` bytes, between two ordinary tiles: staged at and below kTcLdsBytes, read from
    global memory above; with staging switched off every tile takes the fallback form.  All of it gives the model's bytes."""
    rng = np.random.default_rng(span)
    def tile(total):
        lens = np.full(TILE, total // TILE)
        lens[:total - lens.sum()] += 1
        return [(b" " * (int(n) - 6) + b"%6d" % int(rng.integers(-9999, 99999))) if rng.integers(5) else b"x" * int(n) for n in lens]
    rows = tile(2500) + tile(span) + tile(3000)[:100]
    assert sum(len(t) for t in rows[TILE:2 * TILE]) == span
    for layout in ((0, 0), (3, 5)):
        staged = run_parse([rows], [None], "device", R.INT, layout=layout)
        try:
            api._check(lib.load().rdf_set_option(b"textconv_stage", C.c_int64(0)))
            direct = run_parse([rows], [None], "device", R.INT, layout=layout)
        finally:
            api._check(lib.load().rdf_set_option(b"textconv_stage", C.c_int64(1)))
        assert staged == direct


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("kind", [R.BOOL, R.INT, R.DATE, R.TIMESTAMP])
def test_parse_long_rows_alone_in_a_wave_and_64_to_a_wave(api, mem, kind):
    longs = R.long_rows(kind)
    assert {len(t) for t in longs} >= {SHORT_ROW - 1, SHORT_ROW, SHORT_ROW + 1, 10000}
    short, _ = corpus(kind, R.MS, R.I64)
    alone = [[longs[k]] + short[k * 63:(k + 1) * 63] for k in range(len(longs))]          # one long row heading 63 short ones
    packed = [longs[(k + j) % len(longs)] for k in range(0, len(longs), 7) for j in range(64)][:256]   # 64 long rows to a wave
    rows = [[t for w in alone[:8] for t in w], packed, [t for w in alone[8:] for t in w]]
    run_parse(rows, [None, [i % 5 != 0 for i in range(len(packed))], None], mem, kind, R.MS, R.I64)
    if kind == R.INT:
        run_parse([packed], [None], mem, kind, R.S, R.U8)


# ------------------------------------------------------------------------------------------------------------------ format
def run_format(api, arrays, mem, kind, unit=R.S, pattern=None, shift=3):
    """The sizing call (it writes nothing and reports exact capacities), then the call into exactly sized, guarded buffers with
    a shifted data pointer -> per chunk (offsets, data bytes, validity bytes or None, null_count), checked against the model."""
    ins = [to_device(a) for a in arrays] if mem == "device" else list(arrays)
    call, _, nullable = api.utf8_format_call(ins, kind, unit, pattern)
    rows = [a.length for a in arrays]
    m = A.MEM_DEVICE if mem == "device" else A.MEM_HOST

    def buffers(caps, sh):
        co, cd, keep = (A.rdf_out * max(1, len(rows)))(), (A.rdf_out * max(1, len(rows)))(), []
        for i, r in enumerate(rows):
            ob, vb = Buf(4 * (r + 1), mem), (Buf((r + 7) // 8, mem) if nullable[i] else None)
            db = Buf(caps[i], mem, sh) if caps is not None and caps[i] > 0 else None
            co[i] = A.rdf_out(ob.ptr, vb.ptr if vb else None, r + 1, -7, -7, A.I32, m)
            cd[i] = A.rdf_out(db.ptr if db else None, None, caps[i] if db else 0, -7, -7, A.U8, m)
            keep.append((ob, vb, db))
        return co, cd, keep

    toks = R.compile_pattern(pattern, False) if pattern is not None else None
    exp = [[R.format(kind, v, unit, toks) if ok else None for v, ok in zip(a.to_numpy().tolist(), a.valid_mask())] for a in arrays]
    want_caps = [sum(len(t) for t in e if t is not None) for e in exp]
    co, cd, keep = buffers(None, 0)
    st = call(co, cd)
    assert st in (A.RDF_OK, A.RDF_MEMORY_ERROR), (st, lib.load().rdf_last_error())
    assert [cd[i].length for i in range(len(rows))] == want_caps and all(co[i].length == rows[i] + 1 for i in range(len(rows)))
    assert (st == A.RDF_OK) == (sum(want_caps) == 0)
    if st == A.RDF_MEMORY_ERROR:
        for ob, vb, _ in keep:
            assert (ob.read()[0] == 0xAA).all() and (vb is None or (vb.read()[0] == 0xAA).all()), "the sizing call wrote"
    co, cd, keep = buffers(want_caps, shift)
    st = call(co, cd)
    assert st == A.RDF_OK, (st, lib.load().rdf_last_error())
    out = []
    for i, (ob, vb, db) in enumerate(keep):
        what = f"kind {kind} unit {unit} pattern {pattern!r:.40} {mem} chunk {i}"
        offs, g1 = ob.read()
        valid, g2 = vb.read() if vb else (None, True)
        data, g3 = db.read() if db else (np.zeros(0, dtype=np.uint8), True)
        assert g1 and g2 and g3, f"{what}: guard bytes overwritten (offsets {g1}, validity {g2}, data {g3})"
        enc = [b"" if t is None else t for t in exp[i]]
        want_off = np.concatenate([[0], np.cumsum([len(b) for b in enc])]).astype(np.int32)
        assert np.array_equal(offs.view(np.int32), want_off), f"{what}: offsets differ"
        want = np.frombuffer(b"".join(enc), dtype=np.uint8)
        if not np.array_equal(data, want):
            at = int(np.flatnonzero(data != want)[0])
            row = int(np.searchsorted(want_off, at, side="right")) - 1
            raise AssertionError(f"{what}: bytes differ from byte {at} (row {row}): {bytes(data[at:at + 24])!r} vs {bytes(want[at:at + 24])!r}")
        assert co[i].null_count == sum(t is None for t in exp[i]) and cd[i].length == want_caps[i], what
        if valid is not None:
            assert np.array_equal(valid, np.packbits(np.array([t is not None for t in exp[i]], dtype=np.uint8), bitorder="little")), f"{what}: validity bits differ"
        out.append((offs.tobytes(), data.tobytes(), None if valid is None else valid.tobytes()))
    return out


def value_chunks(values, np_dtype, lens, rng, code=None):
    """values dealt into HostArray chunks of the given lengths, validity and an element offset on every other chunk"""
    out, at = [], 0
    for i, n in enumerate(lens):
        v = np.array([values[(at + k) % len(values)] for k in range(n)], dtype=np_dtype)
        at += n
        out.append(A.HostArray.from_numpy(v, valid=(rng.uniform(size=n) > 0.2) if i % 2 == 0 else None, offset=(0, 1, 7)[i % 3], dtype=code))
    return out


FORMAT_CASES = [("bool", None, R.S, None)] + [("int", dt, R.S, None) for dt in R.INT_DTYPES] + \
    [("date", R.I32, D.DAY, None), ("date", R.I64, R.MS, None), ("date", R.I32, D.DAY, "EEE, d MMM yyyy"), ("timestamp", R.I32, R.S, None), ("timestamp", R.I32, D.DAY, None)] + \
    [("timestamp", R.I64, u, None) for u in (R.S, R.MS, R.US, R.NS)] + \
    [("timestamp", R.I64, u, p) for u, p in ((R.S, "yyyy-MM-dd HH:mm:ss"), (R.MS, "yyyy-MM-dd'T'HH:mm:ss.SSS"), (R.US, "MM/dd/yy hh:mm:ss a SSSSSS"), (R.NS, "D DDD d dd M MM MMM H h a m s S yy EEE"))]


@functools.lru_cache(maxsize=None)
def format_values(kind, dtype, unit):
    rng = np.random.default_rng(50 + 3 * (dtype or 0) + unit)
    if kind == "bool":
        return [0, 1, 1, 0, 1]
    if kind == "int":
        lo, hi = R.int_limits(dtype)
        return R.edge_values(R.INT, dtype=dtype) + [int(x) for x in rng.integers(max(lo, -2 ** 62), min(hi, 2 ** 62), size=1500, endpoint=True)] + \
            [int(x) for x in rng.integers(max(lo, -1000), min(hi, 1000), size=500, endpoint=True)]
    if dtype == R.I32:
        return [int(x) for x in D.edge_days()] + [int(x) for x in rng.integers(D.I32_MIN, D.I32_MAX, size=1000)] + [int(x) for x in rng.integers(-40000, 60000, size=1000)]
    return R.edge_values(R.TIMESTAMP, unit) + [int(x) for x in rng.integers(D.I64_MIN, D.I64_MAX, size=700)] + \
        [int(x) for x in rng.integers(-10 ** 9, 4 * 10 ** 9, size=1300) * R.PER_SECOND[unit] + rng.integers(0, R.PER_SECOND[unit], size=1300)]


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("kind,dtype,unit,pattern", FORMAT_CASES)
def test_format_every_kind_dtype_and_unit(api, mem, kind, dtype, unit, pattern):
    vals = format_values(kind, dtype, unit)
    npdt, code = (bool, A.BOOL) if kind == "bool" else (NP_OUT[dtype], dtype)
    chunks = value_chunks(vals, npdt, [0, 1000, 0, 1, 63, 64, 65, 0, 255, 256, 257], np.random.default_rng(8), code)
    first = run_format(api, chunks, mem, R.KINDS.index(kind), unit, pattern)
    assert run_format(api, chunks, mem, R.KINDS.index(kind), unit, pattern) == first, "two runs differ"


@pytest.mark.parametrize("mem", MEMS)
def test_format_rows_from_zero_bytes_to_the_cap(api, mem):
    """NULL rows (0 bytes) beside rows of exactly 256 bytes: the literal-heavy pattern over Int64 seconds whose years have twelve
    digits.  Such a tile goes out in two passes of 128 rows."""
    vals = [D.I64_MIN, D.I64_MIN + 86399, D.I64_MAX, 0, -1, 1582979696]
    chunks = value_chunks(vals, np.int64, [300, 64, 1], np.random.default_rng(9))
    chunks[1] = A.HostArray.from_numpy(np.full(64, D.I64_MIN, dtype=np.int64), valid=np.zeros(64, dtype=bool))      # a wave of NULLs only
    res = run_format(api, chunks, mem, R.TIMESTAMP, R.S, R.CAP_PATTERN)
    offs = np.frombuffer(res[0][0], dtype=np.int32)
    assert int(np.diff(offs).max()) == R.MAX_ROW_BYTES and int(np.diff(offs).min()) == 0 and len(res[1][1]) == 0


@pytest.mark.parametrize("tail", [1, 15, 16, 17])
@pytest.mark.parametrize("shift", [0, 5])
def test_format_a_tile_whose_span_ends_inside_a_16_byte_piece(api, tail, shift):
    """The first tile's 256 rows hold 16 k + tail bytes: 255 one-digit rows and one of the digits that makes the sum."""
    last = {1: 2, 15: 16, 16: 1, 17: 18}[tail]
    vals = [7] * 255 + [int("1" * last)] + [12345] * 44
    assert sum(len(str(v)) for v in vals[:256]) % 16 == tail % 16
    run_format(api, [A.HostArray.from_numpy(np.array(vals, dtype=np.int64))], "device", R.INT, shift=shift)


@pytest.mark.parametrize("kind,dtype,unit", [("int", dt, R.S) for dt in R.INT_DTYPES] + [("date", R.I32, D.DAY)] + [("timestamp", R.I64, u) for u in (R.S, R.MS, R.US, R.NS)] + [("bool", None, R.S)])
def test_the_round_trip_on_the_device(api, kind, dtype, unit):
    """parse(format(x)) == x, device-resident end to end."""
    vals = format_values(kind, dtype, unit)
    if kind == "timestamp":
        lo, hi = int(D.days_from_civil(-999999, 1, 1)), int(D.days_from_civil(9999999, 12, 31))
        vals = [v for v in vals if lo <= v // (86400 * R.PER_SECOND[unit]) <= hi]
    npdt, code = (bool, A.BOOL) if kind == "bool" else (NP_OUT[dtype], dtype)
    x = np.array(vals, dtype=npdt)
    ins = [to_device(A.HostArray.from_numpy(x[:1000], dtype=code)), to_device(A.HostArray.from_numpy(x[1000:], dtype=code))]
    text = api.utf8_format(ins, kind, unit)
    assert all(isinstance(t, A.DeviceUtf8) for t in text)
    back, failed = api.utf8_parse(text, kind, None if kind != "timestamp" else unit, dtype=dtype)
    assert failed == [0, 0] and [b.null_count for b in back] == [0, 0]
    for b, part in zip(back, (x[:1000], x[1000:])):
        raw = b.keep[0].cpu().numpy().view(np.uint8)
        if kind == "bool":
            assert np.array_equal(np.unpackbits(raw, bitorder="little")[:len(part)].astype(bool), part)
        else:
            assert np.array_equal(raw[:len(part) * np.dtype(npdt).itemsize].view(npdt), part)
