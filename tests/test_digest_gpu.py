"""rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32 on the MI355X, exactly against the model of tests/digest_ref.py
(hashlib, zlib, Spark's Murmur3_x86_32, XXH64): values, offsets, hex bytes, validity bitmaps and NULL counts.  Every case
runs over host and device memory against ONE expectation, so both give the same bytes."""
import functools

import numpy as np
import pytest

import digest_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu

MEMS = ["host", "device"]
DIGESTS = list(R.DIGEST_NAMES)
M32, M64 = R.M32, R.M64


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


def to_device(x):
    if isinstance(x, A.HostUtf8):
        return A.DeviceUtf8.from_host(x)
    import torch
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def place(chunks, mem):
    return [to_device(c) for c in chunks] if mem == "device" else list(chunks)


def raw(out):
    """(value bytes, validity bytes or None) of a result array, wherever it lives"""
    if isinstance(out, A.HostArray):
        return out.values.view(np.uint8), out.validity
    t, v = out.keep
    return t.cpu().numpy().view(np.uint8), (v.cpu().numpy() if v is not None else None)


def bits(flags):
    return np.packbits(np.asarray(flags, dtype=np.uint8), bitorder="little") if len(flags) else np.zeros(0, dtype=np.uint8)


def chunk(rows, row_offset=0, first=0, exact_end=False, null_junk=b"", force_valid=False):
    """A Utf8 chunk of byte rows (None = NULL): row_offset junk rows ahead (the validity shares that bit offset), value
    offsets starting at `first`, NULL rows whose offsets span null_junk, no byte after the last row with exact_end."""
    pre = [b"j" * (i % 3 + 1) for i in range(row_offset)]
    buf = bytearray(b"\xee" * first)
    offs = [first]
    for r in pre + list(rows):
        buf += null_junk if r is None else r
        offs.append(len(buf))
    if not exact_end:
        buf += b"\0" * 8
    data = np.frombuffer(bytes(buf), dtype=np.uint8).copy() if buf else np.zeros(0, dtype=np.uint8)
    nulls = sum(r is None for r in rows)
    valid = None
    if nulls or force_valid:
        valid = A.pack_bits(np.array([True] * row_offset + [r is not None for r in rows], dtype=bool))
    return A.HostUtf8(np.array(offs, dtype=np.int32), data, valid, row_offset, len(rows), 0, nulls)


# ---------------------------------------------------------------- the nine functions over one Utf8 column
def expected(fn, rows, seed=42):
    """per row: bytes (digests), int or None (crc32), the unsigned hash (murmur3 / xxhash64: a NULL leaves the seed)"""
    if fn in DIGESTS:
        return [R.digest(DIGESTS.index(fn), r) for r in rows]
    if fn == "crc32":
        return [R.crc32(r) for r in rows]
    kind = R.MURMUR3_32 if fn == "murmur3" else R.XXHASH64
    return [R.hash_row(kind, ["utf8"], [r], seed) for r in rows]


def check_digest(res, rows, fn, nullable, what):
    h = res.to_host() if isinstance(res, A.DeviceUtf8) else res
    exp = expected(fn, rows)
    width = R.HEX_BYTES[DIGESTS.index(fn)]
    assert h.length == len(rows) and h.null_count == sum(e is None for e in exp), (what, h.length, h.null_count)
    want_offs = np.concatenate([[0], np.cumsum([0 if e is None else width for e in exp])]).astype(np.int32)
    got_offs = h.offsets[:len(rows) + 1]
    assert np.array_equal(got_offs, want_offs), f"{what}: offsets differ at {np.flatnonzero(got_offs != want_offs)[:5]}"
    want = b"".join(e for e in exp if e is not None)
    got = h.data[:len(want)].tobytes()
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i]) // width
        live = [i for i, e in enumerate(exp) if e is not None]
        raise AssertionError(f"{what}: hex differs at row {live[k]} (length {len(rows[live[k]])}): got {got[k * width:(k + 1) * width]}, expected {want[k * width:(k + 1) * width]}")
    assert (h.validity is not None) == nullable, what
    if nullable:
        assert np.array_equal(h.validity[:(len(rows) + 7) // 8], bits([e is not None for e in exp])), f"{what}: validity bits differ"


def check_values(out, exp, dtype, nullable, what):
    """exp: unsigned integers or None per row"""
    rows = len(exp)
    assert out.length == rows and out.dtype == dtype and out.null_count == sum(e is None for e in exp), (what, out.length, out.null_count)
    vals, valid = raw(out)
    npdt = np.uint32 if dtype == A.I32 else np.uint64
    got = vals[:rows * np.dtype(npdt).itemsize].view(npdt)
    want = np.array([0 if e is None else e for e in exp], dtype=npdt)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: values differ at rows {bad[:10]}: got {got[bad[:5]]}, expected {want[bad[:5]]}")
    assert (valid is not None) == nullable, what
    if nullable:
        assert np.array_equal(valid[:(rows + 7) // 8], bits([e is not None for e in exp])), f"{what}: validity bits differ"


def run_all_nine(api, chunks, rows_per_chunk, mem, what, expect=expected):
    placed = place(chunks, mem)
    nullable = [c.validity is not None for c in chunks]
    for fn in DIGESTS:
        res = api.utf8_digest(fn, placed)
        assert len(res) == len(chunks)
        for i, (r, rows) in enumerate(zip(res, rows_per_chunk)):
            check_digest(r, rows, fn, nullable[i], f"{what} {fn} {mem} chunk {i}")
    for i, (o, rows) in enumerate(zip(api.utf8_crc32(placed), rows_per_chunk)):
        check_values(o, expect("crc32", rows), A.I64, nullable[i], f"{what} crc32 {mem} chunk {i}")
    for fn, dt in (("murmur3", A.I32), ("xxhash64", A.I64)):
        for i, (o, rows) in enumerate(zip(api.hash_columns(fn, [placed]), rows_per_chunk)):
            check_values(o, expect(fn, rows), dt, False, f"{what} {fn} {mem} chunk {i}")


@functools.lru_cache(maxsize=None)
def ladder_rows():
    rng = np.random.default_rng(11)
    return tuple(rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in range(301))


@functools.lru_cache(maxsize=None)
def cached_expected(name, fn):
    return expected(fn, {"ladder": ladder_rows, "long": long_rows}[name]())


@pytest.mark.parametrize("mem", MEMS)
def test_length_ladder(api, mem):
    """One row of every length 0..300, random bytes (>= 0x80 among them): every padding boundary of the 64- and 128-byte
    blocks, XXH64's 32-byte stripes, Murmur3's 0..3 byte tails."""
    rows = list(ladder_rows())
    run_all_nine(api, [chunk(rows)], [rows], mem, "ladder", expect=lambda fn, _rows: cached_expected("ladder", fn))
    # the same call again gives the same bytes
    placed = place([chunk(rows)], mem)
    a, b = api.utf8_digest("sha256", placed)[0], api.utf8_digest("sha256", placed)[0]
    a, b = (x.to_host() if isinstance(x, A.DeviceUtf8) else x for x in (a, b))
    assert a.data[:301 * 64].tobytes() == b.data[:301 * 64].tobytes() and np.array_equal(a.offsets, b.offsets)


@functools.lru_cache(maxsize=None)
def long_rows():
    """300 rows: 1025 and 4097 bytes in one wave (rows 3 and 40), 70 001 and 4097 in two other waves of the same tile (rows
    70 and 200), 1025 as the last row of the chunk; short rows and NULLs around them."""
    rng = np.random.default_rng(12)
    rows = [None if i % 17 == 5 else rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8).tobytes() for i in range(300)]
    for at, n in ((3, 1025), (40, 4097), (70, 70_001), (200, 4097), (299, 1025)):
        rows[at] = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    return tuple(rows)


@pytest.mark.parametrize("mem", MEMS)
def test_long_rows_among_short_ones(api, mem):
    rows = list(long_rows())
    run_all_nine(api, [chunk(rows, exact_end=True)], [rows], mem, "long rows", expect=lambda fn, _rows: cached_expected("long", fn))


@pytest.mark.parametrize("mem", MEMS)
def test_layouts(api, mem):
    """Chunks of 0, 1 and 257 rows behind a row offset of 3 (the validity bits start at bit 3), value offsets that start at
    5, NULL rows whose offsets span bytes that must not be hashed, a last row that ends where the data ends; then a chunk
    without a data byte."""
    rng = np.random.default_rng(13)

    def rows_of(n):
        return [None if rng.random() < 0.2 else rng.integers(0, 256, size=int(rng.integers(0, 70)), dtype=np.uint8).tobytes() for _ in range(n)]

    per_chunk = [[], [b"Spark"], rows_of(257)]
    per_chunk[2][256] = b"the last row ends where the chunk's bytes end"
    chunks = [chunk(r, row_offset=3, first=5, exact_end=True, null_junk=b"NOT-A-ROW", force_valid=True) for r in per_chunk]
    run_all_nine(api, chunks, per_chunk, mem, "layout")
    nodata = [b"", None, b"", b"", None]
    c = chunk(nodata, exact_end=True)
    assert len(c.data) == 0
    run_all_nine(api, [c], [nodata], mem, "no data bytes")
    plain = [b"", b"", b""]
    run_all_nine(api, [chunk(plain, exact_end=True)], [plain], mem, "no data bytes, no validity")


# ---------------------------------------------------------------- rdf_hash_columns over many columns
NP = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64,
      "f32": np.float32, "f64": np.float64, "bool": np.bool_}
F32_EDGE = [0x00000000, 0x80000000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FA00000, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000]
F64_EDGE = [0, 1 << 63, 0x7FF8000000000000, 0xFFF8000000000123, 0x7FF0000000000001, 0x7FF4000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
            0x3FF0000000000000]


def numeric_column(dt, n, rng):
    """(numpy values, the model's values) of n rows: edges first, then random bits"""
    if dt == "bool":
        v = rng.integers(0, 2, size=n).astype(bool)
        return v, [bool(x) for x in v]
    if dt in ("f32", "f64"):
        ut, edge = (np.uint32, F32_EDGE) if dt == "f32" else (np.uint64, F64_EDGE)
        b = rng.integers(0, np.iinfo(ut).max, size=n, dtype=ut, endpoint=True)
        b[:len(edge)] = np.array(edge, dtype=ut)[:n]
        return b.view(NP[dt]), [("bits", int(x)) for x in b]
    info = np.iinfo(NP[dt])
    v = rng.integers(info.min, info.max, size=n, dtype=NP[dt], endpoint=True)
    v[:3] = [info.min, info.max, 0]
    return v, [int(x) for x in v]


@functools.lru_cache(maxsize=None)
def hash_frame(which):
    """Two frames of 8 columns over chunks of 44 and 257 rows, together all eleven fixed-width dtypes and Utf8, NULLs in
    different columns per row: -> (dtypes, per column the chunks' HostArray / HostUtf8, per chunk the rows as value lists)"""
    dtypes = (["bool", "i8", "i16", "i32", "i64", "u8", "u16", "utf8"], ["u32", "u64", "f32", "f64", "utf8", "i64", "f64", "i8"])[which]
    rng = np.random.default_rng(20 + which)
    cols, rows_per_chunk = [[] for _ in dtypes], []
    for ci, n in enumerate((44, 257)):
        model_cols = []
        for k, dt in enumerate(dtypes):
            valid = rng.random(n) > (0.0 if k == 3 else 0.25)          # (column 3 carries no validity bitmap)
            if dt == "utf8":
                vals = [rng.integers(0, 256, size=int(rng.integers(0, 30)), dtype=np.uint8).tobytes() for _ in range(n)]
                cols[k].append(chunk([v if ok else None for v, ok in zip(vals, valid)], row_offset=2, first=3, null_junk=b"xy"))
                model = vals
            else:
                arr, model = numeric_column(dt, n, rng)
                cols[k].append(A.HostArray.from_numpy(arr, valid=None if k == 3 else valid, offset=k % 4))
            model_cols.append([m if ok else None for m, ok in zip(model, valid)])
        rows_per_chunk.append(list(zip(*model_cols)))
    return dtypes, cols, rows_per_chunk


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("which", [0, 1])
def test_hash_columns_over_eight_columns(api, mem, which):
    dtypes, cols, rows_per_chunk = hash_frame(which)
    placed = [place(c, mem) for c in cols]
    for fn, kind, dt, mask in (("hash", R.MURMUR3_32, A.I32, M32), ("xxhash64", R.XXHASH64, A.I64, M64)):
        for seed in (0, 42, -1):
            outs = api.hash_columns(fn, placed, seed=seed)
            for i, (o, rows) in enumerate(zip(outs, rows_per_chunk)):
                check_values(o, [R.hash_row(kind, dtypes, r, seed) for r in rows], dt, False, f"{fn} seed {seed} {mem} chunk {i}")
    # one column alone, each of them
    for k, dtk in enumerate(dtypes):
        for fn, kind, dt in (("hash", R.MURMUR3_32, A.I32), ("xxhash64", R.XXHASH64, A.I64)):
            for i, (o, rows) in enumerate(zip(api.hash_columns(fn, [placed[k]]), rows_per_chunk)):
                check_values(o, [R.hash_row(kind, [dtk], [r[k]], 42) for r in rows], dt, False, f"{fn} of column {k} ({dtk}) alone {mem} chunk {i}")


@pytest.mark.parametrize("mem", MEMS)
def test_hash_columns_is_never_null(api, mem):
    """A validity buffer, if given, is written all ones (bits beyond the last row 0) and null_count is 0."""
    dtypes, cols, rows_per_chunk = hash_frame(0)
    placed = [place(c, mem) for c in cols]
    outs = [api._window_out(A.I32, len(rows), mem == "device", True) for rows in rows_per_chunk]
    for o in api.hash_columns("hash", placed, outs=outs):
        _, valid = raw(o)
        assert o.null_count == 0 and np.array_equal(valid[:(o.length + 7) // 8], bits([True] * o.length))
    # the Spark example through the device: hash('Spark', 123, 2) and xxhash64 of the same
    spark = [[chunk([b"Spark"])], [A.HostArray.from_numpy(np.array([123], dtype=np.int32))], [A.HostArray.from_numpy(np.array([2], dtype=np.int32))]]
    sp = [place(c, mem) for c in spark]
    assert raw(api.hash_columns("hash", sp)[0])[0][:4].view(np.int32)[0] == -1321691492
    assert raw(api.hash_columns("xxhash64", sp)[0])[0][:8].view(np.int64)[0] == 5602566077635097486


# ---------------------------------------------------------------- the sizing protocol of rdf_utf8_digest
@pytest.mark.parametrize("mem", MEMS)
def test_digest_sizing_protocol(api, mem):
    rows0, rows1 = [b"Spark", None, b"", b"abc"], [b"x" * 100] * 70 + [None] * 3
    chunks = [chunk(rows0), chunk(rows1)]
    placed = place(chunks, mem)
    device = mem == "device"
    need = [3 * 40, 70 * 40]

    def buffers(caps):
        co, cd, keep = api._utf8_outs(placed, [4, 73], [True, True], device, caps)
        for ob, db, vb in keep:                   # guard bytes everywhere
            for t in (ob, db, vb):
                if t is not None:
                    t[:] = 0x5A if device or t.dtype == np.uint8 else 0x5A5A5A5A
        return co, cd, keep

    def snapshot(keep):
        return [None if t is None else (t.cpu().numpy().copy() if device else t.copy()) for k in keep for t in k]

    call, _, _ = api.utf8_digest_call("sha1", placed)
    # the sizing call
    co, cd, keep = buffers(None)
    before = snapshot(keep)
    assert call(co, cd) == A.RDF_MEMORY_ERROR
    assert [cd[i].length for i in range(2)] == need and [co[i].length for i in range(2)] == [5, 74]
    assert all(a is None or np.array_equal(a, b) for a, b in zip(before, snapshot(keep)))
    # a capacity that is too small for the second chunk only: every length set, nothing written
    co, cd, keep = buffers([need[0], need[1] - 1])
    before = snapshot(keep)
    assert call(co, cd) == A.RDF_MEMORY_ERROR
    assert [cd[i].length for i in range(2)] == need
    assert all(a is None or np.array_equal(a, b) for a, b in zip(before, snapshot(keep)))
    # the exact capacity
    co, cd, keep = buffers(need)
    assert call(co, cd) == A.RDF_OK
    assert [cd[i].length for i in range(2)] == need and [co[i].null_count for i in range(2)] == [1, 3]
    for i, rows in enumerate((rows0, rows1)):
        ob, db, vb = (t.cpu().numpy() if device else t for t in keep[i])
        want = b"".join(R.digest(R.SHA1, r) for r in rows if r is not None)
        assert db[:need[i]].tobytes() == want
        assert np.all(db[need[i]:] == 0x5A), "bytes beyond the chunk's hex text were written"
        assert np.array_equal(ob[:len(rows) + 1], np.concatenate([[0], np.cumsum([0 if r is None else 40 for r in rows])]).astype(np.int32))
        assert np.array_equal(vb[:(len(rows) + 7) // 8], bits([r is not None for r in rows]))


@pytest.mark.parametrize("mem", MEMS)
def test_known_answers_on_the_device(api, mem):
    placed = place([chunk([b"Spark"])], mem)
    got = {fn: api.utf8_digest(fn, placed, as_arrow="pylist")[0][0] for fn in ("md5", "sha1", "sha256")}
    assert got == {"md5": "8cde774d6f7333752ed72cacddb05126", "sha1": "85f5955f4b27a9a4c2aab6ffe5d7189fc298b92c",
                   "sha256": "529bc3b07127ecb7e53a4dcf1991d9152c24537d919178022b2c42657f79a26b"}
    assert raw(api.utf8_crc32(placed)[0])[0][:8].view(np.int64)[0] == 1557323817
