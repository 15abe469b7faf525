"""rdf_utf8_concat / _pad / _repeat / _reverse / _substring_index on the MI355X, byte for byte against the model of
tests/utf8_build_ref.py: offsets, data, validity, null_count.  Every call here is made twice under the sizing rule (the
sizing call, then the call into exactly sized buffers) with guard bytes behind every buffer, over host and device memory."""
import numpy as np
import pytest

import utf8_build_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu

MEMS = ["host", "device"]
CHUNK_ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
LAYOUTS = [(0, 0), (3, 1), (5, 7), (1, 0)]
ALPHABET = ["a", "b", "c", "x", "é", "ß", "中", "😀", "%", "_", " "]
GUARD = 32
SHORT_ROW, COPY_TILE, WINDOW_ROWS = 256, 4096, 1024     # kUtf8ShortRow, kUtf8CopyTile, kUtf8WindowRows of rdf_utf8.h


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


def place(chunks, mem):
    return [A.DeviceUtf8.from_host(c) for c in chunks] if mem == "device" else list(chunks)


class Buf:
    """nbytes bytes followed by GUARD guard bytes, in host or device memory, everything 0xAA; `shift` moves the pointer"""
    def __init__(self, nbytes, mem, shift=0):
        self.n, self.mem, self.shift = nbytes, mem, shift
        if mem == "device":
            import torch
            self.t = torch.full((nbytes + GUARD + shift + 16,), 0xAA, dtype=torch.uint8, device="cuda")
            self.ptr = self.t.data_ptr() + shift
        else:
            self.t = np.full(nbytes + GUARD + shift + 16, 0xAA, dtype=np.uint8)
            self.ptr = self.t.ctypes.data + shift

    def read(self):
        """(the bytes, guard intact)"""
        raw = self.t.cpu().numpy() if self.mem == "device" else self.t
        body = raw[self.shift:self.shift + self.n].copy()
        return body, bool((raw[self.shift + self.n:] == 0xAA).all()) and bool((raw[:self.shift] == 0xAA).all())


def buffers(rows, nullable, mem, caps, shift=0):
    m = A.MEM_DEVICE if mem == "device" else A.MEM_HOST
    n = len(rows)
    co, cd, keep = (A.rdf_out * max(1, n))(), (A.rdf_out * max(1, n))(), []
    for i in range(n):
        ob = Buf(4 * (rows[i] + 1), mem)
        vb = Buf((rows[i] + 7) // 8, mem) if nullable[i] else None
        db = Buf(caps[i], mem, shift) if caps is not None and caps[i] > 0 else None
        co[i] = A.rdf_out(ob.ptr, vb.ptr if vb else None, rows[i] + 1, -7, -7, A.I32, m)
        cd[i] = A.rdf_out(db.ptr if db else None, None, caps[i] if db else 0, -7, -7, A.U8, m)
        keep.append((ob, vb, db))
    return co, cd, keep


def run_call(call, rows, nullable, mem, shift=0):
    """The sizing call, then the call into exactly sized, guarded buffers -> per chunk (offsets, data bytes, validity bytes or
    None, null_count).  The sizing call must leave every buffer untouched."""
    n = len(rows)
    co, cd, keep = buffers(rows, nullable, mem, None)
    st = call(co, cd)
    assert st in (A.RDF_OK, A.RDF_MEMORY_ERROR), (st, lib.load().rdf_last_error())
    caps = [cd[i].length for i in range(n)]
    assert all(c >= 0 for c in caps) and all(co[i].length == rows[i] + 1 for i in range(n))
    assert (st == A.RDF_OK) == (sum(caps) == 0)
    if st == A.RDF_MEMORY_ERROR:
        for ob, vb, _ in keep:
            assert (ob.read()[0] == 0xAA).all() and (vb is None or (vb.read()[0] == 0xAA).all()), "the sizing call wrote"
    co, cd, keep = buffers(rows, nullable, mem, caps, shift)
    st = call(co, cd)
    assert st == A.RDF_OK, (st, lib.load().rdf_last_error())
    out = []
    for i, (ob, vb, db) in enumerate(keep):
        assert co[i].length == rows[i] + 1 and cd[i].length == caps[i]
        offs, ok_o = ob.read()
        valid, ok_v = vb.read() if vb else (None, True)
        data, ok_d = db.read() if db else (np.zeros(0, dtype=np.uint8), True)
        assert ok_o and ok_v and ok_d, f"chunk {i}: guard bytes overwritten (offsets {ok_o}, validity {ok_v}, data {ok_d})"
        out.append((offs.view(np.int32), data, valid, co[i].null_count))
    return out


def _b(s):
    return s if isinstance(s, bytes) else s.encode("utf-8")


def check(res, expected, nullable, what=""):
    """expected[i]: the model's rows of chunk i (None = NULL)"""
    assert len(res) == len(expected), what
    for i, ((offs, data, valid, nulls), exp) in enumerate(zip(res, expected)):
        enc = [b"" if e is None else _b(e) for e in exp]
        want_off = np.concatenate([[0], np.cumsum([len(b) for b in enc])]).astype(np.int32)
        if not np.array_equal(offs, want_off):
            bad = int(np.flatnonzero(offs != want_off)[0])
            raise AssertionError(f"{what} chunk {i}: offsets differ from entry {bad}: {offs[bad - 1:bad + 2]} vs {want_off[bad - 1:bad + 2]}")
        want = np.frombuffer(b"".join(enc), dtype=np.uint8)
        if not np.array_equal(data, want):
            at = int(np.flatnonzero(data != want)[0])
            row = int(np.searchsorted(want_off, at, side="right")) - 1
            raise AssertionError(f"{what} chunk {i}: bytes differ from byte {at} (row {row}, byte {at - want_off[row]} of its {len(enc[row])}): "
                                 f"{bytes(data[at:at + 24])!r} vs {bytes(want[at:at + 24])!r}")
        assert nulls == sum(e is None for e in exp), (what, i, nulls)
        assert (valid is not None) == nullable[i], (what, i)
        if valid is not None:
            bits = np.packbits(np.array([e is not None for e in exp], dtype=np.uint8), bitorder="little")
            assert np.array_equal(valid, bits), f"{what} chunk {i}: validity bits differ"


def run_unary(api, op, col, mem, *args, shift=0, ins=None):
    ins = place(col, mem) if ins is None else ins
    call, _, nullable = api.utf8_build_call(op, ins, *args)
    res = run_call(call, [c.length for c in col], nullable, mem, shift)
    check(res, [[R.apply(op, s, *args) for s in c.to_pylist()] for c in col], nullable, f"{op} {args!r:.50} {mem}")
    return res


def run_concat(api, parts, mem, sep=None, shift=0):
    """parts: chunk lists (host) and str literals"""
    placed = [p if isinstance(p, str) else place(p, mem) for p in parts]
    call, shape, nullable = api.utf8_build_call(*(("concat", None, placed) if sep is None else ("concat_ws", None, placed, sep)))
    cols = [p for p in parts if not isinstance(p, str)]
    nch = len(cols[0])
    res = run_call(call, [c.length for c in cols[0]], nullable, mem, shift)
    exp = []
    for c in range(nch):
        lists = [[p] * cols[0][c].length if isinstance(p, str) else p[c].to_pylist() for p in parts]
        exp.append([R.concat(list(t)) if sep is None else R.concat_ws(sep, list(t)) for t in zip(*lists)] if lists[0] else [])
    assert nullable == [sep is None and any(p[c].validity is not None for p in cols) for c in range(nch)]
    check(res, exp, nullable, f"concat {len(parts)} parts sep {sep!r} {mem}")
    return res


def rand_rows(rng, n, null_frac, maxlen=14):
    return [None if rng.random() < null_frac else "".join(rng.choice(ALPHABET, size=rng.integers(0, maxlen + 1))) for _ in range(n)]


def column(rng, null_frac, ro, do, lens=CHUNK_ROWS):
    return [A.HostUtf8.from_pylist(rand_rows(rng, n, null_frac), row_offset=ro, data_offset=do) for n in lens]


def text(rows, **kw):
    return [A.HostUtf8.from_pylist(rows, **kw)]


# ---------------------------------------------------------------- every op over every layout
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("ro,do", LAYOUTS)
@pytest.mark.parametrize("null_frac", [0.0, 0.1])
def test_every_op_over_chunks_offsets_and_nulls(api, mem, ro, do, null_frac):
    rng = np.random.default_rng(100 * ro + do + int(null_frac * 10))
    a, b, c = column(rng, null_frac, ro, do), column(rng, null_frac, do % 4, ro), column(rng, null_frac * 2, 2, 3)
    for sep in (None, "中, "):
        run_concat(api, [a], mem, sep)
        run_concat(api, [a, "-é"], mem, sep)
        run_concat(api, ["<", b], mem, sep)
        run_concat(api, [a, ", ", b], mem, sep)
        run_concat(api, [a, b, c], mem, sep)
        run_concat(api, [a, "", b, "é", c, "the longer literal 中", a, b], mem, sep)
    run_concat(api, [a, b], mem, "")
    for op in ("lpad", "rpad"):
        for n, pad in ((10, "ab"), (5, "aé中😀"), (20, " ")):
            run_unary(api, op, a, mem, n, pad)
    run_unary(api, "repeat", a, mem, 3)
    run_unary(api, "reverse", a, mem)
    for delim, count in (("a", 2), ("é", -1), (" ", 1), ("ab", -2), ("😀", 3)):
        run_unary(api, "substring_index", a, mem, delim, count)


# ---------------------------------------------------------------- piece boundaries at every phase of a 16-byte store
@pytest.mark.parametrize("mem", MEMS)
def test_piece_boundaries_at_every_phase_of_a_store(api, mem):
    firsts = [("aé中😀" * 4).encode()[:n].decode("utf-8", "ignore") for n in range(40)]
    firsts = {len(s.encode()): s for s in firsts}
    firsts = [firsts[n] if n in firsts else "a" * n for n in range(34)]
    assert [len(s.encode()) for s in firsts] == list(range(34))
    left, right = [], []
    for s in firsts:
        for ph in range(16):            # a filler row moves the row's start over every byte of a store
            left += ["f" * ph, s]
            right += ["", "0123456789ABCDEFGHIJ"]
    starts = np.cumsum([0] + [len(x.encode()) + len(y) for x, y in zip(left, right)])[:-1]
    bounds = {(int(st) + len(x.encode())) % 16 for st, x in zip(starts[1::2], left[1::2])}
    assert bounds == set(range(16))
    run_concat(api, [text(left), text(right)], mem)
    run_concat(api, [text(left), text(right)], mem, "é")
    run_concat(api, [text(left, data_offset=3), "|", text(right, row_offset=2)], mem)
    # the pad / row boundary: rows of 0 .. 33 bytes padded to 40 code points; the boundary sits at byte 40 k + 40 - n (lpad)
    ascii_rows = ["r" * n for n in range(34)] * 2
    assert {(40 * k + 40 - len(r)) % 16 for k, r in enumerate(ascii_rows)} == set(range(16))
    assert {(40 * k + len(r)) % 16 for k, r in enumerate(ascii_rows)} == set(range(16))
    for op in ("lpad", "rpad"):
        run_unary(api, op, text(ascii_rows), mem, 40, "pq")
        run_unary(api, op, text(firsts), mem, 37, "aé中😀")


# ---------------------------------------------------------------- periods that do not divide 16
@pytest.mark.parametrize("mem", MEMS)
def test_periods_that_do_not_divide_16(api, mem):
    rows = ["a", "abc", "aébc", "中😀", None, ""]
    assert [len(r.encode()) for r in rows[:4]] == [1, 3, 5, 7]
    run_unary(api, "repeat", text(rows, data_offset=1), mem, 3000)
    pad = "aé中😀"
    assert len(pad.encode()) == 10
    for op in ("lpad", "rpad"):
        run_unary(api, op, text(["", "x", "中y", None, "éé😀"], row_offset=1), mem, 5000, pad)


# ---------------------------------------------------------------- long rows
def long_row(rng, n):
    pool = ["a", "é", "中", "😀", ".", "b"]
    return "".join(pool[k] for k in rng.integers(0, len(pool), size=n))


@pytest.mark.parametrize("mem", MEMS)
def test_one_row_of_10000_code_points_among_short_rows(api, mem):
    rng = np.random.default_rng(3)
    big, big2 = long_row(rng, 10000), long_row(rng, 10000)
    rows = rand_rows(rng, 70, 0.1) + [big] + rand_rows(rng, 70, 0.1) + [None, big2[:5000]]
    other = rand_rows(rng, 70, 0.1) + [big2] + rand_rows(rng, 72, 0.1)
    col, col2 = text(rows, row_offset=1, data_offset=5), text(other)
    run_unary(api, "reverse", col, mem)
    run_unary(api, "repeat", col, mem, 2)
    for op in ("lpad", "rpad"):
        run_unary(api, op, col, mem, 10007, "aé中😀")
        run_unary(api, op, col, mem, 4999, "x")           # the long rows are cut between code points of every width
        run_unary(api, op, col, mem, 10000, "x")
    for delim, count in ((".", 700), (".", -700), ("a.", 3), ("😀é", -2), ("b", 100000)):
        run_unary(api, "substring_index", col, mem, delim, count)
    run_concat(api, [col, ", ", col2], mem)
    run_concat(api, [col, col2, col], mem, "中")


def delimiter_rows(filler, d, width):
    """rows of about `width` bytes: the delimiter at every position, once alone and once with a second one at the row's start"""
    fb, db = len(filler.encode()), len(d.encode())
    one, two = (width - db) // fb, (width - 2 * db) // fb
    rows = [filler * i + d + filler * (one - i) for i in range(one + 1)]
    rows += [d + filler * i + d + filler * (two - i) for i in range(two + 1)]
    return rows


@pytest.fixture(scope="module")
def delimiter_columns():
    cols = {}
    for name, filler, d in (("ascii", "x", "ab"), ("wide", "中", "a中b")):
        rows = delimiter_rows(filler, d, 1000)
        assert max(len(r.encode()) for r in rows) <= 1000 and min(len(r.encode()) for r in rows) >= 990
        # a delimiter straddling kUtf8ShortRow, in rows just short and just long enough for either path
        for n in (SHORT_ROW - 1, SHORT_ROW, SHORT_ROW + 1, SHORT_ROW + 2):
            rows += ["y" * (SHORT_ROW - 1) + d[:n - (SHORT_ROW - 1)], "y" * (n - len(d.encode())) + d, d + "y" * (n - len(d.encode()))]
        half = len(rows) // 2
        cols[name] = (d, [A.HostUtf8.from_pylist(rows[:half], data_offset=1), A.HostUtf8.from_pylist(rows[half:] + [None], row_offset=1)])
    return cols


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("filler", ["ascii", "wide"])
def test_a_delimiter_at_every_position_of_1000_byte_rows(api, delimiter_columns, mem, filler):
    d, col = delimiter_columns[filler]
    ins = place(col, mem)
    for count in (1, -1, 2, -2, 3):
        run_unary(api, "substring_index", col, mem, d, count, ins=ins)
    run_unary(api, "substring_index", col, mem, d[0], -1, ins=ins)


# ---------------------------------------------------------------- tiles
@pytest.mark.parametrize("mem", MEMS)
def test_more_rows_than_the_window_in_one_copy_tile(api, mem):
    assert 3000 > WINDOW_ROWS
    rows = ["abc"] + [""] * 3000 + ["déf", None, "", "g"]
    col = text(rows, row_offset=1)
    run_unary(api, "reverse", col, mem)
    run_unary(api, "repeat", col, mem, 2)
    run_unary(api, "rpad", col, mem, 0, "x")              # every row empty
    run_unary(api, "substring_index", col, mem, "é", 1)
    run_concat(api, [col, "", col], mem)
    run_concat(api, [col, col], mem, "")
    empties = text([""] * 3004 + ["tail"])
    run_concat(api, [empties, col], mem)


@pytest.mark.parametrize("mem", MEMS)
def test_rows_that_end_on_and_around_a_tile_boundary(api, mem):
    rng = np.random.default_rng(9)
    lens = [COPY_TILE - 1, 1, COPY_TILE, 0, COPY_TILE + 1, COPY_TILE - 1, 7, 2 * COPY_TILE - 7, 3, COPY_TILE - 4]
    assert {sum(lens[:k]) % COPY_TILE for k in range(1, len(lens))} >= {0, 1, COPY_TILE - 1}
    rows = []
    for n in lens:
        s = long_row(rng, n)
        while len(s.encode()) > n:
            s = s[:-1]
        rows.append(s + "a" * (n - len(s.encode())))
    assert [len(r.encode()) for r in rows] == lens
    col = text(rows, data_offset=2)
    run_unary(api, "reverse", col, mem)
    run_unary(api, "repeat", col, mem, 1)
    run_concat(api, [col, ""], mem)
    run_unary(api, "substring_index", col, mem, "\x01", 1)     # no such byte: the whole row
    half = [s[:len(s) // 2] for s in rows], [s[len(s) // 2:] for s in rows]
    run_concat(api, [text(half[0]), text(half[1], row_offset=3)], mem)


# ---------------------------------------------------------------- truncating pads
@pytest.mark.parametrize("mem", MEMS)
def test_pads_that_truncate(api, mem):
    rows = ["aé中😀b", "中中中中中", "abcde", "😀é😀é😀", None, "é", ""]
    col = text(rows, row_offset=2, data_offset=1)
    for op in ("lpad", "rpad"):
        for n in (0, 1, 5, 4, -3, 2):
            run_unary(api, op, col, mem, n, "x")
            run_unary(api, op, col, mem, n, "中é")
        for n in (0, 3, 5, 9):
            run_unary(api, op, col, mem, n, "")          # pad_bytes == 0: never longer than the row
    big = text(["é" * 300 + "中" * 300, "a" * 700, None, "😀" * 257])
    for n in (0, 1, 256, 257, 299, 300, 301, 599, 600, 601):
        run_unary(api, "lpad", big, mem, n, "ab")
        run_unary(api, "rpad", big, mem, n, "")


# ---------------------------------------------------------------- bounds
@pytest.mark.parametrize("mem", MEMS)
def test_a_delimiter_is_never_completed_by_bytes_behind_the_chunk(api, mem):
    whole = A.HostUtf8.from_pylist(["xab", "cdefghijklmnop"])
    first = A.HostUtf8(whole.offsets[:2].copy(), whole.data, None, 0, 1, 0, 0)
    assert first.to_pylist() == ["xab"] and bytes(whole.data[3:6]) == b"cde"
    for d in ("abc", "abcdefgh", "xabc", "bc"):
        for count in (1, -1):
            res = run_unary(api, "substring_index", [first], mem, d, count)
            assert bytes(res[0][1]) == b"xab"
    long_row_ = "." * 700 + "ab"
    whole = A.HostUtf8.from_pylist([long_row_, "cdefghijklmnopqrstuvwxyz"])
    first = A.HostUtf8(whole.offsets[:2].copy(), whole.data, None, 0, 1, 0, 0)
    for d in ("abc", "abcdefghijklmnopq", "bc"):
        for count in (1, -1):
            res = run_unary(api, "substring_index", [first], mem, d, count)
            assert bytes(res[0][1]) == long_row_.encode()
    run_unary(api, "reverse", [first], mem)
    run_unary(api, "lpad", [first], mem, 800, "中")


def test_an_output_pointer_that_is_not_16_byte_aligned(api):
    rng = np.random.default_rng(13)
    col = column(rng, 0.1, 1, 2, [300, 77])
    for shift in (1, 7):
        run_unary(api, "reverse", col, "device", shift=shift)
        run_unary(api, "lpad", col, "device", 9, "é0", shift=shift)
        run_concat(api, [col, "-", col], "device", shift=shift)


def raw_column(rows):
    """a Utf8 chunk of arbitrary bytes"""
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    data = np.frombuffer(b"".join(rows) + b"\0" * 8, dtype=np.uint8).copy()
    return A.HostUtf8(offs, data, None, 0, len(rows), 0, 0)


@pytest.mark.parametrize("mem", MEMS)
def test_broken_utf8_keeps_lengths_and_bounds(api, mem):
    rng = np.random.default_rng(17)
    pool = [0x61, 0x80, 0xBF, 0xC3, 0xE4, 0xF0, 0xFF, 0xA9]
    rows = [bytes(rng.choice(pool, size=rng.integers(0, 40)).astype(np.uint8)) for _ in range(400)]
    rows += [bytes(rng.choice(pool, size=n).astype(np.uint8)) for n in (255, 256, 257, 1000, 5000)] + [b"\x80" * 600, b"\xf0" * 300]
    col = [raw_column(rows)]
    ins = place(col, mem)
    lens = np.array([len(r) for r in rows])
    call, _, nullable = api.utf8_build_call("reverse", ins)
    offs, data, _, nulls = run_call(call, [len(rows)], nullable, mem)[0]
    assert np.array_equal(np.diff(offs), lens) and nulls == 0           # every output row has its input row's length
    for op in ("lpad", "rpad"):
        for n, pad in ((20, b"\xc3"), (300, b"\x80\x80"), (7, b"a\x80\xe4"), (1000, b"\xf0\x9f")):
            call, _, nullable = api.utf8_build_call(op, ins, n, pad)
            offs, data, _, nulls = run_call(call, [len(rows)], nullable, mem)[0]       # (the guards are run_call's)
            assert offs[0] == 0 and (np.diff(offs) >= 0).all() and offs[-1] == len(data) and nulls == 0


# ---------------------------------------------------------------- sizing
@pytest.mark.parametrize("mem", MEMS)
def test_a_capacity_one_byte_short_is_refused_with_the_lengths_set(api, mem):
    rng = np.random.default_rng(19)
    col = column(rng, 0.1, 1, 1, [100, 0, 31])
    ins = place(col, mem)
    for op, args in (("reverse", ()), ("lpad", (20, "ab")), ("repeat", (3,)), ("substring_index", ("a", 1))):
        call, _, nullable = api.utf8_build_call(op, ins, *args)
        rows = [c.length for c in col]
        want = [sum(len(R.apply(op, s, *args).encode()) for s in c.to_pylist() if s is not None) for c in col]
        for short in (0, 2):
            caps = list(want)
            caps[short] -= 1
            co, cd, keep = buffers(rows, nullable, mem, caps)
            assert call(co, cd) == A.RDF_MEMORY_ERROR
            assert [cd[i].length for i in range(3)] == want and [co[i].length for i in range(3)] == [r + 1 for r in rows]
            for ob, vb, db in keep:
                for b in (ob, vb, db):
                    assert b is None or ((b.read()[0] == 0xAA).all() and b.read()[1]), "a refused call wrote"


@pytest.mark.parametrize("mem", MEMS)
def test_a_chunk_beyond_int32_offsets_is_a_compute_error_from_the_sizing_call(api, mem):
    col = text(["a" * 1000, "b" * 1000, None, "c" * 1000]) + text(["tiny"])
    ins = place(col, mem)
    for op, args in (("repeat", (1 << 21,)), ("repeat", (1 << 40,)), ("repeat", ((1 << 63) - 1,)), ("lpad", (1 << 31, "ab")), ("rpad", (1 << 62, "中"))):
        call, _, nullable = api.utf8_build_call(op, ins, *args)
        co, cd, keep = buffers([4, 1], nullable, mem, None)
        assert call(co, cd) == A.RDF_COMPUTE_ERROR, (op, args)
        assert "beyond the Int32 offsets" in lib.load().rdf_last_error().decode()
    # just below the limit it is only a matter of capacity: 2 x 1000 x 2^20 bytes
    call, _, nullable = api.utf8_build_call("repeat", place(text(["a" * 1000, "b" * 1000]), mem), 1 << 20)
    co, cd, keep = buffers([2], [False], mem, None)
    assert call(co, cd) == A.RDF_MEMORY_ERROR and cd[0].length == 2000 << 20


# ---------------------------------------------------------------- identities that tie the family together
def rows_of(res):
    return [bytes(data[offs[r]:offs[r + 1]]) for offs, data, _, _ in res for r in range(len(offs) - 1)]


def host_result(res, col):
    """the results of run_call as HostUtf8 chunks (the inputs' validity carried over)"""
    return [A.HostUtf8(offs.copy(), np.concatenate([data, np.zeros(8, dtype=np.uint8)]), None if valid is None else np.concatenate([valid, np.zeros(8, dtype=np.uint8)]),
                       0, c.length, 0, nulls) for (offs, data, valid, nulls), c in zip(res, col)]


@pytest.mark.parametrize("mem", MEMS)
def test_identities(api, mem):
    rng = np.random.default_rng(23)
    col = column(rng, 0.1, 2, 3, [500, 0, 129])
    col[0] = A.HostUtf8.from_pylist(col[0].to_pylist()[:-1] + [long_row(rng, 3000)], row_offset=2, data_offset=3)
    want = [b"" if s is None else s.encode() for c in col for s in c.to_pylist()]
    once = run_unary(api, "reverse", col, mem)
    back = host_result(once, col)
    assert rows_of(run_unary(api, "reverse", back, mem)) == want
    assert rows_of(run_concat(api, [col], mem)) == want
    assert rows_of(run_unary(api, "repeat", col, mem, 1)) == want
    # lpad(x, length(x), p) is x: columns whose rows all have n code points
    for n in (0, 1, 9):
        same = text([None if rng.random() < 0.1 else "".join(rng.choice(ALPHABET, size=n)) for _ in range(300)], data_offset=1)
        assert rows_of(run_unary(api, "lpad", same, mem, n, "pé")) == [b"" if s is None else s.encode() for s in same[0].to_pylist()]
    # length(lpad(x, n, p)) is n for every non-NULL row
    for n in (0, 1, 7, 40, 3001):
        padded = host_result(run_unary(api, "lpad", col, mem, n, "中a"), col)
        outs = api.utf8_measure("length", place(padded, mem))
        for o, c in zip(outs, col):
            t = o.to_numpy() if isinstance(o, A.HostArray) else o.keep[0].cpu().numpy().view(np.int32)[:o.length]
            assert (np.asarray(t)[:c.length][c.valid_mask()] == n).all()


# ---------------------------------------------------------------- the result is a key
@pytest.mark.parametrize("mem", MEMS)
def test_a_concatenated_column_is_a_group_by_key(api, mem):
    rng = np.random.default_rng(29)
    cities, countries = ["Paris", "Köln", "東京", "", "Lima"], ["FR", "DE", "日本", "PE", ""]
    lens = [700, 0, 333]
    city = [A.HostUtf8.from_pylist([None if rng.random() < 0.1 else cities[rng.integers(5)] for _ in range(n)], row_offset=1) for n in lens]
    country = [A.HostUtf8.from_pylist([None if rng.random() < 0.1 else countries[rng.integers(5)] for _ in range(n)], data_offset=2) for n in lens]
    raw_vals = [rng.integers(0, 100, n).astype(np.int64) for n in lens]
    vals = [A.HostArray.from_numpy(v) for v in raw_vals]
    key = host_result(run_concat(api, [city, country], mem, ", "), city)
    model = [R.concat_ws(", ", [x, y]) for a, b in zip(city, country) for x, y in zip(a.to_pylist(), b.to_pylist())]
    assert [s for k in key for s in k.to_pylist()] == model and all(k.validity is None for k in key)
    placed = place(key, mem)
    codes, dictionary, count = api.utf8_dictionary_encode(placed)
    words = (dictionary.to_host() if isinstance(dictionary, A.DeviceUtf8) else dictionary).to_pylist()
    first_seen = list(dict.fromkeys(model))
    assert count == len(first_seen) and words[:count] == first_seen
    if mem == "device":
        import torch
        dvals = [A.DeviceArray(t.data_ptr(), None, 0, v.length, A.I64, 0, keep=(t, None)) for v in vals for t in [torch.from_numpy(v.values).cuda()]]
    else:
        dvals = vals
    keys, sums, counts = api.groupby_agg_keys([placed], dvals, "sum", len(first_seen))
    k = keys[0].to_host() if isinstance(keys[0], A.DeviceUtf8) else keys[0]

    def nums(o):
        return (o.to_numpy() if isinstance(o, A.HostArray) else o.keep[0].cpu().numpy().view(np.int64))[:o.length].tolist()

    got = dict(zip(k.to_pylist(), zip(nums(sums), nums(counts))))
    want = {}
    allv = np.concatenate(raw_vals)
    for s, v in zip(model, allv):
        t = want.get(s, (0, 0))
        want[s] = (t[0] + int(v), t[1] + 1)
    assert got == want


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("mem", MEMS)
def test_the_same_call_and_another_chunking_give_the_same_bytes(api, mem):
    rng = np.random.default_rng(31)
    rows = rand_rows(rng, 1500, 0.1) + ["." * 900 + "ab", None, "ab" + "é" * 400]
    other = rand_rows(rng, 1503, 0.1)
    cuts = [(0, 1503)], [(0, 64), (64, 1000), (1000, 1503)]

    def col(src, cut, **kw):
        return [A.HostUtf8.from_pylist(src[a:b], **kw) for a, b in cut]

    for build in (lambda c: run_unary(api, "reverse", col(rows, c, row_offset=1), mem), lambda c: run_unary(api, "lpad", col(rows, c), mem, 30, "aé"),
                  lambda c: run_unary(api, "repeat", col(rows, c, data_offset=2), mem, 2), lambda c: run_unary(api, "substring_index", col(rows, c), mem, "a", -1),
                  lambda c: run_concat(api, [col(rows, c), ", ", col(other, c, row_offset=2)], mem), lambda c: run_concat(api, [col(rows, c), col(other, c)], mem, "中")):
        one, again, cut = build(cuts[0]), build(cuts[0]), build(cuts[1])
        for x, y in zip(one, again):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and (x[2] is None or np.array_equal(x[2], y[2]))
        assert rows_of(one) == rows_of(cut)
        assert b"".join(bytes(r[1]) for r in cut) == bytes(one[0][1])


def test_the_kernel_is_named_and_timed(api):
    col = text(["ab", None, "cde"] * 50)
    for f in (lambda: api.utf8_concat([col, "-", col]), lambda: api.utf8_build("lpad", col, 7, "0"), lambda: api.utf8_build("repeat", col, 2),
              lambda: api.utf8_build("reverse", col), lambda: api.utf8_build("substring_index", col, "b", 1)):
        lib.kernel_timing_reset(True)
        f()
        assert lib.last_kernel() == "utf8_build_size_kernel + utf8_build_copy_kernel"
        ms, launches = lib.kernel_timing_get()
        lib.kernel_timing_reset(False)
        assert launches >= 1 and ms > 0
    assert api.utf8_concat([col, "-", col], as_arrow="pylist") == [[None if s is None else s + "-" + s for s in col[0].to_pylist()]]
    assert api.utf8_build("substring_index", col, "d", 1, as_arrow="pylist")[0][:3] == ["ab", None, "c"]
