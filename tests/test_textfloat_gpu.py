"""rdf_utf8_parse_float / rdf_utf8_format_float on the MI355X, bit for bit (NaN by its bits) and byte for byte against the model
of tests/textfloat_ref.py, behind guard bytes, over host and device memory: values, validity bytes, null_count and failed for
parse under the default routing, with every row on the exact path and with the global load form; the tile spans around the LDS
budget; the long rows; offsets, data, validity and null_count under the sizing rule for format; the round trip; determinism;
the smallest shapes that cross a wave, a tile and a chunk."""
import ctypes as C
import functools

import numpy as np
import pytest

import textfloat_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
from test_textconv_gpu import Buf, place, text_chunk, to_device

pytestmark = pytest.mark.gpu

MEMS = ["host", "device"]
TILE = 256
NP_BITS = {True: np.uint32, False: np.uint64}
NP_FLOAT = {True: np.float32, False: np.float64}
DT = {True: A.F32, False: A.F64}
assert (A.F32, A.F64) == (R.F32, R.F64)


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    so = lib.load()
    so.rdf_utf8_parse_float.restype = C.c_int
    so.rdf_utf8_format_float.restype = C.c_int
    yield a
    lib.set_option("textfloat_exact", 0)
    lib.set_option("textconv_stage", 1)


@functools.lru_cache(maxsize=None)
def model_parse(rows, f32):
    return tuple(R.parse(t, f32) for t in rows)


def run_parse(rows_per_chunk, valid_per_chunk, mem, f32, layout=(0, 0)):
    """One rdf_utf8_parse_float call into guarded buffers, checked against the model -> the raw output bytes of every chunk."""
    so = lib.load()
    hosts = [text_chunk(r, v, *layout) for r, v in zip(rows_per_chunk, valid_per_chunk)]
    ins = place(hosts, mem)
    n = len(ins)
    es = 4 if f32 else 8
    m = A.MEM_DEVICE if mem == "device" else A.MEM_HOST
    co, keep = (A.rdf_out * max(1, n))(), []
    for i, h in enumerate(hosts):
        vb = Buf(h.length * es, mem)
        bb = Buf((h.length + 7) // 8, mem)
        co[i] = A.rdf_out(vb.ptr, bb.ptr, h.length, -7, -7, DT[f32], m)
        keep.append((vb, bb))
    carr = (A.rdf_utf8_array * max(1, n))(*[c.c_struct() for c in ins])
    failed = (C.c_int64 * max(1, n))(*([-7] * max(1, n)))
    st = so.rdf_utf8_parse_float(carr, C.c_int64(n), co, failed)
    assert st == A.RDF_OK, (st, so.rdf_last_error())
    out = []
    for i, (rows, valid) in enumerate(zip(rows_per_chunk, valid_per_chunk)):
        nrows = len(rows)
        exp = model_parse(tuple(rows), f32)
        ok_in = [True] * nrows if valid is None else list(valid)
        good = np.array([a and e is not None for a, e in zip(ok_in, exp)], dtype=bool)
        vals, g1 = keep[i][0].read()
        bits, g2 = keep[i][1].read()
        what = f"f32 {f32} {mem} chunk {i}"
        assert g1 and g2, what + ": guard bytes overwritten"
        assert co[i].length == nrows and co[i].null_count == int(nrows - good.sum()), (what, co[i].length, co[i].null_count)
        assert failed[i] == sum(a and e is None for a, e in zip(ok_in, exp)), (what, failed[i])
        assert np.array_equal(bits, np.packbits(good.astype(np.uint8), bitorder="little")), what + ": validity differs"
        want = np.array([int(e) if g else 0 for g, e in zip(good, exp)], dtype=np.uint64).astype(NP_BITS[f32])
        got = vals.view(NP_BITS[f32])
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0])
            raise AssertionError(f"{what}: row {at} {rows[at][:60]!r}: got {int(got[at]):x}, expected {int(want[at]):x}")
        out.append((vals.tobytes(), bits.tobytes()))
    return out


@functools.lru_cache(maxsize=None)
def corpus(f32):
    rows = R.branch_cases() + [t for t, _, _ in R.hard_cases()]
    for k, fam in enumerate(R.FAMILIES):
        rows += R.random_cases(fam, 1500, 500 + k, f32)
    rng = np.random.default_rng(11)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    cut = [0, len(rows) // 3 + 17, 2 * len(rows) // 3 + 5, len(rows)]
    chunks = tuple(tuple(rows[cut[i]:cut[i + 1]]) for i in range(3))
    valids = tuple(tuple(bool(x) for x in rng.uniform(size=len(c)) > 0.1) for c in chunks)
    return chunks, valids


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("f32", [False, True])
def test_parse_corpus_under_every_routing(api, mem, f32):
    """branch cases, hard cases and 1500 rows of each random family over 3 sliced chunks with validity: the default routing, every
    row on the exact path, the global load form, and the default again: the same bytes four times"""
    chunks, valids = corpus(f32)
    runs = []
    try:
        for exact, stage in ((0, 1), (1, 1), (0, 0), (0, 1)):
            lib.set_option("textfloat_exact", exact)
            lib.set_option("textconv_stage", stage)
            runs.append(run_parse(chunks, valids, mem, f32, layout=(7, 3)))
            if exact:
                assert "resolve" in lib.last_kernel()
    finally:
        lib.set_option("textfloat_exact", 0)
        lib.set_option("textconv_stage", 1)
    assert runs[0] == runs[1] == runs[2] == runs[3]


def test_default_routing_reaches_the_resolve_kernel(api):
    """the long-digit ties are undecided by the fast path: the call's last kernel is the resolve kernel; human decimals are not"""
    ties = [t for t, f32, und in R.hard_cases() if und and not f32]
    assert len(ties) >= 10
    run_parse([ties], [None], "host", False)
    assert "resolve" in lib.last_kernel()
    run_parse([R.random_cases("human", 300, 3, False)], [None], "host", False)
    assert "resolve" not in lib.last_kernel()


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("span", [R.LDS_BYTES - 1, R.LDS_BYTES, R.LDS_BYTES + 1])
def test_tile_spans_around_the_lds_budget(api, f32, span):
    """a tile of 256 rows whose bytes are one below, at and one above the staging budget, then a short tile"""
    rows = R.random_cases("long", TILE, 21, f32)
    extra = span - sum(len(t) for t in rows)
    assert extra >= 0
    rows = [b" " * (extra // TILE + (k < extra % TILE)) + t for k, t in enumerate(rows)]      # (the trim set: the values stay)
    assert sum(len(t) for t in rows) == span
    rows += R.random_cases("human", 40, 5, f32)
    for mem in MEMS:
        run_parse([rows], [None], mem, f32)


@pytest.mark.parametrize("f32", [False, True])
def test_long_rows_alone_and_64_to_a_wave(api, f32):
    longs = R.long_rows()
    assert max(len(t) for t in longs) > 5000 and min(len(t) for t in longs) >= 300
    short = R.random_cases("human", 63, 9, f32)
    alone = []
    for t in longs[:12]:
        alone += [t] + short                  # one long row among 63 short ones
    run_parse([alone], [None], "device", f32)
    run_parse([longs[:64], longs[5:] + longs[:5]], [None, None], "host", f32)


SHAPES = [[1], [255], [256], [257], [64, 0, 65], [300, 0, 300]]


@pytest.mark.parametrize("rows", SHAPES)
def test_parse_small_shapes(api, rows):
    pool = R.random_cases("human", 400, 31, False) + R.branch_cases()
    chunks = [[pool[(7 * i + k) % len(pool)] for i in range(n)] for k, n in enumerate(rows)]
    for mem in MEMS:
        run_parse(chunks, [None] * len(rows), mem, False)
        run_parse(chunks, [[i % 3 != 0 for i in range(n)] for n in rows], mem, True, layout=(3, 1))
        run_parse(chunks, [[False] * n for n in rows], mem, False, layout=(1, 0))         # all NULL


# ----------------------------------------------------------------------------------------------------------------- format
@functools.lru_cache(maxsize=None)
def format_values(f32):
    vals = R.edge_values(f32) + R.hard_values(f32) + R.random_bits(3000, 91 + f32, f32)
    return tuple(vals)


@functools.lru_cache(maxsize=None)
def model_format(vals, f32):
    return tuple(R.fmt(b, f32) for b in vals)


def value_chunk(bits, f32, valid=None, offset=0):
    arr = np.array(list(bits), dtype=NP_BITS[f32]).view(NP_FLOAT[f32])
    return A.HostArray.from_numpy(arr, valid=None if valid is None else np.array(list(valid), dtype=bool), offset=offset)


def run_format(bits_per_chunk, valid_per_chunk, mem, f32, offset=0, short_by=0):
    """The sizing call, then the call into exactly sized guarded buffers (short_by: the first data buffer that many bytes too
    small: RDF_MEMORY_ERROR and nothing written) -> raw bytes per chunk"""
    so = lib.load()
    hosts = [value_chunk(b, f32, v, offset) for b, v in zip(bits_per_chunk, valid_per_chunk)]
    ins = [to_device(h) for h in hosts] if mem == "device" else hosts
    n = len(ins)
    m = A.MEM_DEVICE if mem == "device" else A.MEM_HOST
    carr = (A.rdf_array * max(1, n))(*[c.c_struct() for c in ins])
    exp = [[t if (v is None or v[i]) else b"" for i, t in enumerate(model_format(tuple(b), f32))] for b, v in zip(bits_per_chunk, valid_per_chunk)]
    need = [sum(len(t) for t in e) for e in exp]

    def outs(caps):
        co, cd, keep = (A.rdf_out * max(1, n))(), (A.rdf_out * max(1, n))(), []
        for i, b in enumerate(bits_per_chunk):
            ob, vb, db = Buf(4 * (len(b) + 1), mem), Buf((len(b) + 7) // 8, mem), Buf(caps[i], mem)
            co[i] = A.rdf_out(ob.ptr, vb.ptr if valid_per_chunk[i] is not None else None, len(b) + 1, -7, -7, A.I32, m)
            cd[i] = A.rdf_out(db.ptr if caps[i] else None, None, caps[i], -7, -7, A.U8, m)
            keep.append((ob, vb, db))
        return co, cd, keep

    co, cd, keep = outs([0] * n)
    st = so.rdf_utf8_format_float(carr, C.c_int64(n), co, cd)
    if sum(need):
        assert st == A.RDF_MEMORY_ERROR, (st, so.rdf_last_error())
        assert all(k[0].read()[0].tobytes() == b"\xaa" * k[0].n for k in keep), "the sizing call wrote offsets"
    assert [cd[i].length for i in range(n)] == need
    if short_by:
        caps = list(need)
        caps[0] -= short_by
        co, cd, keep = outs(caps)
        assert so.rdf_utf8_format_float(carr, C.c_int64(n), co, cd) == A.RDF_MEMORY_ERROR
        assert [cd[i].length for i in range(n)] == need
        assert all(k[2].read()[0].tobytes() == b"\xaa" * k[2].n and k[2].read()[1] for k in keep), "a call that does not fit wrote data"
        return None
    co, cd, keep = outs(need)
    st = so.rdf_utf8_format_float(carr, C.c_int64(n), co, cd)
    assert st == A.RDF_OK, (st, so.rdf_last_error())
    res = []
    for i, (b, v) in enumerate(zip(bits_per_chunk, valid_per_chunk)):
        offs, g1 = keep[i][0].read()
        vbits, g2 = keep[i][1].read()
        data, g3 = keep[i][2].read()
        assert g1 and g2 and g3, f"chunk {i}: guard bytes overwritten"
        want_offs = np.zeros(len(b) + 1, dtype=np.int32)
        want_offs[1:] = np.cumsum([len(t) for t in exp[i]]) if len(b) else []
        got_offs = offs.view(np.int32)
        if not np.array_equal(got_offs, want_offs) or data.tobytes() != b"".join(exp[i]):
            at = int(np.flatnonzero(got_offs != want_offs)[0]) - 1 if not np.array_equal(got_offs, want_offs) else \
                next(k for k in range(len(b)) if data.tobytes()[want_offs[k]:want_offs[k + 1]] != exp[i][k])
            at = max(at, 0)
            raise AssertionError(f"f32 {f32} {mem} chunk {i} row {at}: bits {b[at]:x} expected {exp[i][at]!r} got {data.tobytes()[got_offs[at]:got_offs[at + 1]]!r}")
        nulls = 0 if v is None else int(len(v) - sum(v))
        assert co[i].null_count == nulls and co[i].length == len(b) + 1 and cd[i].length == need[i]
        if v is not None:
            assert np.array_equal(vbits, np.packbits(np.array(v, dtype=np.uint8), bitorder="little"))
        res.append((offs.tobytes(), data.tobytes(), vbits.tobytes()))
    return res


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("f32", [False, True])
def test_format_byte_for_byte_and_the_sizing_rule(api, mem, f32):
    """hard cases' values, every power of ten and of two, the layout boundaries +- 1 ulp, subnormals, specials and 3000 random bit
    patterns over 3 chunks with an offset and validity; twice for the same bytes; a data buffer one byte too small"""
    vals = list(format_values(f32))
    rng = np.random.default_rng(5)
    vals = [vals[i] for i in rng.permutation(len(vals))]
    cut = [0, len(vals) // 3 + 11, 2 * len(vals) // 3 + 3, len(vals)]
    chunks = [vals[cut[i]:cut[i + 1]] for i in range(3)]
    valids = [[bool(x) for x in rng.uniform(size=len(c)) > 0.1] for c in chunks]
    a = run_format(chunks, valids, mem, f32, offset=5)
    b = run_format(chunks, valids, mem, f32, offset=5)
    assert a == b
    assert run_format(chunks, valids, mem, f32, offset=5, short_by=1) is None
    assert max(len(t) for t in model_format(tuple(vals), f32)) == R.MAX_ROW[f32]


@pytest.mark.parametrize("rows", SHAPES)
def test_format_small_shapes(api, rows):
    pool = format_values(False)
    pool32 = format_values(True)
    for mem in MEMS:
        run_format([[pool[(13 * i + k) % len(pool)] for i in range(n)] for k, n in enumerate(rows)], [None] * len(rows), mem, False)
        run_format([[pool32[(13 * i + k) % len(pool32)] for i in range(n)] for k, n in enumerate(rows)], [[i % 3 != 0 for i in range(n)] for n in rows], mem, True, offset=3)
        run_format([[pool[i % len(pool)] for i in range(n)] for n in rows], [[False] * n for n in rows], mem, False)


def host_bits(arr, f32):
    if isinstance(arr, A.DeviceArray):
        return arr.keep[0].cpu().numpy().view(NP_BITS[f32])[:arr.length].copy()
    return np.ascontiguousarray(arr.values).view(NP_BITS[f32])[:arr.length]


@pytest.mark.parametrize("f32", [False, True])
def test_round_trip_on_the_device(api, f32):
    """parse(format(x)) has the bits of x (NaN: the canonical one), through the Python front end, device memory"""
    F = R.FMT[f32]
    vals = list(format_values(f32))
    h = value_chunk(vals, f32)
    text = api.utf8_format_float([to_device(h)])
    assert isinstance(text[0], A.DeviceUtf8)
    back, failed = api.utf8_parse_float(text, dtype=DT[f32])
    assert failed == [0] and back[0].null_count == 0
    got = host_bits(back[0], f32)
    want = np.array([F.nan if (b & (F.sign - 1)) > F.inf else b for b in vals], dtype=np.uint64).astype(NP_BITS[f32])
    assert np.array_equal(got, want)
