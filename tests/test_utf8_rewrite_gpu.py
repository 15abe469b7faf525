"""rdf_utf8_replace / _translate / _initcap / _split on the MI355X, byte for byte against the model of
tests/utf8_rewrite_ref.py: offsets, data, validity, null_count, and for split the list offsets and the child's offsets.
Every call here is made twice under the sizing rule (the sizing call, then the call into exactly sized buffers) with guard
bytes behind every buffer, over host and device memory.  The shapes are the smallest at which these kernels can go wrong."""
import numpy as np
import pytest

import utf8_rewrite_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
from test_utf8_build_gpu import Buf, place, run_call

pytestmark = pytest.mark.gpu

MEMS = ["host", "device"]
CHUNK_ROWS = [1, 63, 0, 64, 65, 255, 256, 257, 1000, 0]     # an empty chunk between two others, and one at the end
LAYOUTS = [(0, 0), (3, 1), (5, 7)]
ALPHABET = ["a", "b", "A", ",", " ", "-", "é", "ß", "Σ", "σ", "ǆ", "İ", "中", "😀", "\t"]
SHORT_ROW, COPY_TILE, WINDOW_ROWS = 256, 4096, 1024     # kUtf8ShortRow, kUtf8CopyTile, kUtf8WindowRows of rdf_utf8.h
IMAGE = 16384                                           # kUtf8RewriteImage of rdf_utf8.h: the output span a block assembles in LDS
LONG = 16 * 1024


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


def _b(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode("utf-8")


def utf8(rows, row_offset=0, data_offset=0):
    """A HostUtf8 of byte-string (or str) rows, None = NULL, behind row_offset junk rows and data_offset junk bytes"""
    enc = [b"j" * (i % 3 + 1) for i in range(row_offset)] + [b"" if r is None else _b(r) for r in rows]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in enc]) if enc else []
    data = np.frombuffer(b"\xff" * data_offset + b"".join(enc) + b"\0" * 8, dtype=np.uint8).copy()
    nulls = sum(r is None for r in rows)
    valid = A.pack_bits(np.array([True] * row_offset + [r is not None for r in rows], dtype=bool)) if nulls else None
    h = A.HostUtf8(offs.astype(np.int32), data, valid, row_offset, len(rows), data_offset, nulls)
    h.rows = [None if r is None else _b(r) for r in rows]
    return h


def rand_rows(rng, n, null_frac=0.2, maxlen=14):
    return [None if rng.random() < null_frac else "".join(rng.choice(ALPHABET, size=rng.integers(0, maxlen + 1))) for _ in range(n)]


def column(rng, ro=0, do=0, lens=CHUNK_ROWS, null_frac=0.2):
    return [utf8(rand_rows(rng, n, null_frac), ro, do) for n in lens]


def check_rows(res, expected, nullable, what):
    """res: run_call's per-chunk (offsets, data, validity, null_count); expected[i]: the model's rows of chunk i as bytes"""
    assert len(res) == len(expected), what
    for i, ((offs, data, valid, nulls), exp) in enumerate(zip(res, expected)):
        enc = [b"" if e is None else e for e in exp]
        want_off = np.concatenate([[0], np.cumsum([len(b) for b in enc])]).astype(np.int32)
        assert np.array_equal(offs, want_off), f"{what} chunk {i}: offsets differ from entry {int(np.flatnonzero(offs != want_off)[0])}"
        want = np.frombuffer(b"".join(enc), dtype=np.uint8)
        if not np.array_equal(data, want):
            at = int(np.flatnonzero(data != want)[0])
            row = int(np.searchsorted(want_off, at, side="right")) - 1
            raise AssertionError(f"{what} chunk {i}: bytes differ from byte {at} (row {row}, byte {at - want_off[row]} of its {len(enc[row])}): "
                                 f"{bytes(data[at:at + 24])!r} vs {bytes(want[at:at + 24])!r}")
        assert nulls == sum(e is None for e in exp), (what, i, nulls)
        assert (valid is not None) == nullable[i], (what, i)
        if valid is not None:
            assert np.array_equal(valid, np.packbits(np.array([e is not None for e in exp], dtype=np.uint8), bitorder="little")), f"{what} chunk {i}: validity"


MODEL = {"replace": R.replace, "translate": R.translate, "initcap": R.initcap}


def run_op(api, op, col, mem, *args, shift=0):
    ins = place(col, mem)
    call, _, nullable = getattr(api, f"utf8_{op}_call")(ins, *args)
    assert nullable == [c.validity is not None for c in col]
    res = run_call(call, [c.length for c in col], nullable, mem, shift)
    margs = [_b(a) for a in args]
    check_rows(res, [[MODEL[op](r, *margs) for r in c.rows] for c in col], nullable, f"{op} {args!r:.60} {mem}")
    return res


def run_split(api, col, mem, delim, limit, shift=0):
    """The sizing call (nothing written, all three lengths set), then the call into exactly sized, guarded buffers; list
    offsets, validity, null_count, child offsets and bytes against the model.  -> per chunk (list offsets, child offsets,
    data, validity bytes) and the model's lists"""
    ins = place(col, mem)
    call, _, nullable = api.utf8_split_call(ins, delim, limit)
    m = A.MEM_DEVICE if mem == "device" else A.MEM_HOST
    n = len(col)
    rows = [c.length for c in col]

    def buffers(ecaps, dcaps, sh=0):
        cl, ce, cd, keep = (A.rdf_out * n)(), (A.rdf_out * n)(), (A.rdf_out * n)(), []
        for i in range(n):
            lb = Buf(4 * (rows[i] + 1), mem)
            vb = Buf((rows[i] + 7) // 8, mem) if nullable[i] else None
            eb = Buf(4 * ecaps[i], mem) if ecaps[i] else None
            db = Buf(dcaps[i], mem, sh) if dcaps[i] else None
            cl[i] = A.rdf_out(lb.ptr, vb.ptr if vb else None, rows[i] + 1, -7, -7, A.I32, m)
            ce[i] = A.rdf_out(eb.ptr if eb else None, None, ecaps[i], -7, -7, A.I32, m)
            cd[i] = A.rdf_out(db.ptr if db else None, None, dcaps[i], -7, -7, A.U8, m)
            keep.append((lb, vb, eb, db))
        return cl, ce, cd, keep

    cl, ce, cd, keep = buffers([0] * n, [0] * n)
    assert call(cl, ce, cd) == A.RDF_MEMORY_ERROR, lib.load().rdf_last_error()
    for lb, vb, _, _ in keep:
        assert (lb.read()[0] == 0xAA).all() and (vb is None or (vb.read()[0] == 0xAA).all()), "the sizing call wrote"
    ecaps, dcaps = [ce[i].length for i in range(n)], [cd[i].length for i in range(n)]
    assert all(cl[i].length == rows[i] + 1 for i in range(n))
    cl, ce, cd, keep = buffers(ecaps, dcaps, shift)
    assert call(cl, ce, cd) == A.RDF_OK, lib.load().rdf_last_error()
    out, model = [], []
    for i, (lb, vb, eb, db) in enumerate(keep):
        what = f"split {delim!r} {limit} {mem} chunk {i}"
        exp = [R.split(r, _b(delim), limit) for r in col[i].rows]
        flat = [e for lst in exp if lst is not None for e in lst]
        assert cl[i].length == rows[i] + 1 and ce[i].length == len(flat) + 1 == ecaps[i] and cd[i].length == sum(len(e) for e in flat) == dcaps[i], what
        lo, ok_l = lb.read()
        valid, ok_v = vb.read() if vb else (None, True)
        eo, ok_e = eb.read()
        data, ok_d = db.read() if db else (np.zeros(0, dtype=np.uint8), True)
        assert ok_l and ok_v and ok_e and ok_d, f"{what}: guard bytes overwritten"
        lo, eo = lo.view(np.int32), eo.view(np.int32)
        assert np.array_equal(lo, np.concatenate([[0], np.cumsum([0 if lst is None else len(lst) for lst in exp])]).astype(np.int32)), f"{what}: list offsets"
        assert np.array_equal(eo, np.concatenate([[0], np.cumsum([len(e) for e in flat])]).astype(np.int32)), f"{what}: child offsets"
        assert bytes(data) == b"".join(flat), f"{what}: bytes"
        assert cl[i].null_count == sum(lst is None for lst in exp) and ce[i].null_count == 0, what
        if valid is not None:
            assert np.array_equal(valid, np.packbits(np.array([lst is not None for lst in exp], dtype=np.uint8), bitorder="little")), f"{what}: validity"
        out.append((lo, eo, data, valid))
        model.append(exp)
    return out, model


# ---------------------------------------------------------------- every op over every layout
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("ro,do", LAYOUTS)
def test_every_op_over_chunks_offsets_and_nulls(api, mem, ro, do):
    rng = np.random.default_rng(100 * ro + do)
    col = column(rng, ro, do)
    for search, rep in ((",", ""), ("a", "é中"), ("é", "e"), ("ab", "ab"), ("", "x"), ("中", "")):
        run_op(api, "replace", col, mem, search, rep)
    for matching, rep in (("ab,", "xy"), ("a", "中"), ("😀é", ""), ("aba", "123"), ("", "abc")):
        run_op(api, "translate", col, mem, matching, rep)
    run_op(api, "initcap", col, mem)
    for limit in (-1, 2):
        run_split(api, col, mem, ",", limit)
    run_split(api, col, mem, "é", 0)


@pytest.mark.parametrize("mem", MEMS)
def test_a_column_without_validity_needs_and_gets_none(api, mem):
    rng = np.random.default_rng(3)
    col = column(rng, 1, 2, lens=[65, 0, 300], null_frac=0.0)
    assert all(c.validity is None for c in col)
    run_op(api, "replace", col, mem, "a", "bb")
    run_op(api, "initcap", col, mem)
    run_split(api, col, mem, " ", -1)


# ---------------------------------------------------------------- row lengths: the lane's form, the wave's, the image, the direct rows
def long_rows(rng, unit_pool):
    rows = []
    for n in (0, 1, SHORT_ROW - 1, SHORT_ROW, SHORT_ROW + 1, 300, LONG):
        s = b""
        while len(s) < n:
            u = _b(unit_pool[rng.integers(len(unit_pool))])
            s += u if len(s) + len(u) <= n else b"x"
        rows.append(s)
    return rows


@pytest.mark.parametrize("mem", MEMS)
def test_row_lengths_around_the_short_row_and_a_16_kib_row(api, mem):
    rng = np.random.default_rng(5)
    rows = long_rows(rng, ["a", "b", ",", " ", "é", "Σ", "ǆ", "中", "😀", "A"])
    col = [utf8(rows + [None] + rows[::-1], 2, 3), utf8(rows[-1:] * 2 + ["a,b"])]
    run_op(api, "replace", col, mem, ",", "")
    run_op(api, "replace", col, mem, "a", "<a long replacement of a single byte>")      # the 16 KiB row's output exceeds the image: written directly
    run_op(api, "replace", col, mem, "é", "e")
    run_op(api, "translate", col, mem, "a,中😀", "中x")
    run_op(api, "initcap", col, mem)
    for limit in (-1, 5):
        run_split(api, col, mem, ",", limit)
    run_split(api, col, mem, "a", 0)


NEEDLES = [1, 2, 3, 5, 64, 65, 70]


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("m", NEEDLES)
def test_a_hit_across_the_waves_window(api, mem, m):
    """needles of m bytes with a hit that starts at bytes 62 .. 66 of a long row; r < m, r == m, r > m, r == 0"""
    needle = bytes((0x41 + (i * 7) % 26) for i in range(m))       # no self-overlap for m > 1
    rows = []
    for at in (62, 63, 64, 65, 66):
        rows.append(b"." * at + needle + b"." * 200 + needle + needle + b"." * 31 + needle)
        rows.append(b"." * at + needle)                              # the hit ends the row (short or long, by m)
        rows.append(b"." * at + needle[:-1] + b"." * 300 if m > 1 else b"." * (at + 300))   # no hit
    col = [utf8(rows[:7], 1, 1), utf8(rows[7:] + [None])]
    for rep in (b"", needle[:m // 2 + 0] if m > 1 else b"", b"#" * m, b"#" * (m + 3)):
        run_op(api, "replace", col, mem, needle, rep)
    for limit in (-1, 0, 1, 2, 5):
        run_split(api, col, mem, needle, limit)


@pytest.mark.parametrize("mem", MEMS)
def test_self_overlapping_needles(api, mem):
    rows = [b"a" * n for n in list(range(10)) + [257, 300]] + [b"ab" * 200 + b"a", b"aba" * 150, None]
    col = [utf8(rows, 3, 1)]
    for search, rep in ((b"aa", b"b"), (b"aa", b""), (b"aa", b"aaa"), (b"aba", b"x"), (b"abab", b"ab"), (b"a" * 65, b"-"), (b"ab" * 35, b"")):
        run_op(api, "replace", col, mem, search, rep)
    for d in (b"aa", b"aba", b"a" * 65):
        run_split(api, col, mem, d, -1)
        run_split(api, col, mem, d, 2)


@pytest.mark.parametrize("mem", MEMS)
def test_more_empty_rows_than_a_window_holds(api, mem):
    """replace('a', '') over 3000 rows 'a' (> kUtf8WindowRows consecutive rows without a byte), and a byte at last"""
    assert 3000 > WINDOW_ROWS
    col = [utf8([b"a"] * 3000 + [b"ab"]), utf8([b"a"] * 300)]
    run_op(api, "replace", col, mem, "a", "")
    out, _ = run_split(api, col, mem, "a", -1)       # 2 empty elements per row: offsets without bytes
    assert len(out[1][2]) == 0 and len(out[1][1]) == 601


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("edge", [COPY_TILE, IMAGE])
def test_chunk_lengths_on_the_tile_and_image_edges(api, mem, edge):
    """outputs whose chunk length falls on edge - 1, edge, edge + 1 bytes"""
    cols = []
    for total in (edge - 1, edge, edge + 1):
        rows, left = [], total
        while left > 0:
            n = min(left, 37)
            rows.append(b"ab" * (n // 2) + b"c" * (n % 2))
            left -= n
        cols.append(utf8(rows))
    res = run_op(api, "replace", cols, mem, "b", "d")
    assert [len(r[1]) for r in res] == [edge - 1, edge, edge + 1]
    run_op(api, "translate", cols, mem, "ab", "ba")
    res = run_op(api, "replace", cols, mem, "ab", "a")       # the INPUT falls on the edge, the output does not
    run_op(api, "initcap", cols, mem)
    # one row that fills the image exactly, one byte less, one byte more (the last is written directly)
    for n in (IMAGE - 1, IMAGE, IMAGE + 1):
        run_op(api, "replace", [utf8([b"x", b"ab" * (n // 2) + b"c" * (n % 2), b"y"])], mem, "b", "d")


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("shift", [1, 15])
def test_output_data_pointers_of_any_alignment(api, mem, shift):
    rng = np.random.default_rng(7 + shift)
    col = column(rng, 0, 0, lens=[257, 0, 1000])
    run_op(api, "replace", col, mem, "a", "中中", shift=shift)
    run_op(api, "translate", col, mem, "aé", "éa", shift=shift)
    run_op(api, "initcap", col, mem, shift=shift)
    run_split(api, col, mem, ",", -1, shift=shift)


# ---------------------------------------------------------------- translate
@pytest.mark.parametrize("mem", MEMS)
def test_translate_tables(api, mem):
    rng = np.random.default_rng(11)
    col = column(rng, 1, 0, lens=[300, 65]) + [utf8(long_rows(rng, ["a", "b", "é", "中", "😀", " "]))]
    for matching, rep in (("ab", "xy"),               # ASCII -> ASCII
                          ("a ", "中€"),               # ASCII -> 3 bytes
                          ("😀", ""),                  # 4 bytes -> deletion
                          ("aba", "123"),             # a duplicate key: its first position decides
                          ("a", "xyz"),               # replace longer than matching
                          ("", "abc"),                # an empty matching
                          ("é中😀ß", "e😀中"),           # wide keys, all widths; ß is dropped
                          ("".join(chr(0x400 + i) for i in range(500)) + "a", "b" * 500 + "中")):   # 501 keys: the sorted table at full size
        run_op(api, "translate", col, mem, matching, rep)


@pytest.mark.parametrize("mem", MEMS)
def test_broken_utf8_is_copied(api, mem):
    rows = [b"\x80a\xc3", b"\xe2\x82\xac\x80\x80 a", b"a\x80 b", b"\xf0\x9f\x98", b"\xff\xfe A\xce\xa3\xce", b"\xce\xa3" * 200 + b"\x80" * 100, None]
    col = [utf8(rows, 1, 1)]
    run_op(api, "translate", col, mem, b"a\x80\xe2\x82\xac", b"xyz")
    run_op(api, "initcap", col, mem)
    run_op(api, "replace", col, mem, b"\x80", b"\xc3\xa9")
    run_split(api, col, mem, b"\x80", -1)


# ---------------------------------------------------------------- initcap
@pytest.mark.parametrize("mem", MEMS)
def test_initcap_mappings_and_word_starts(api, mem):
    cps = [c for c in range(0x110000) if not 0xD800 <= c <= 0xDFFF]
    resized = [chr(c) for c in cps if R.title_simple(c) != c and len(chr(c).encode()) != len(chr(R.title_simple(c)).encode())]
    assert len(resized) == 31
    rows = [" ".join(resized), "x".join(resized), "ǆ ǅ Ǆ ǉ ǈ Ǉ ǌ ǋ Ǌ ǳ ǲ Ǳ", "İstanbul İ iİ", "ΑΣ Σ ΑΣ. ΑΣΑ Σ", "ΟΔΥΣΣΕΥΣ", "a  b   c", "a\tb\nc", " a", "  ", "",
            "sPark sql", "ǄX  ßa\tb ΑΣ Σ", "ſ ა ŉ ﬁ ß", None, ("ΑΣ " * 100) + "Σ", "ß" + "Ab " * 100, " ".join(resized) * 12]
    col = [utf8(rows, 2, 1)]
    res = run_op(api, "initcap", col, mem)
    offs, data = res[0][0], bytes(res[0][1])
    assert data[offs[11]:offs[12]].decode() == "Spark Sql" and data[offs[12]:offs[13]].decode() == "ǅx  ßa\tb Ας Σ"


# ---------------------------------------------------------------- split
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("limit", [-1, 0, 1, 2, 5])
def test_split_limits_and_explode_take(api, mem, limit):
    rng = np.random.default_rng(13)
    rows = ["a,b,,c,", "", ",", ",,,", "no hit", "a,", ",a", None, "é,中,😀", "x" * 300 + "," + "y" * 300 + ",", ",".join("ab" for _ in range(400))] + rand_rows(rng, 300)
    col = [utf8(rows, 1, 2)]
    out, model = run_split(api, col, mem, ",", limit)
    assert model[0][0] == ([b"a", b"b", b"", b"c", b""] if limit <= 0 or limit >= 5 else [[b"a,b,,c,"], [b"a", b"b,,c,"]][limit - 1])
    assert model[0][1] == [b""] and model[0][7] is None
    # through the public layer, then rdf_list_explode + rdf_utf8_take: the model's flattened list
    (lst, child), = api.utf8_split(place(col, mem), ",", limit)
    flat = [e.decode() for l in model[0] if l is not None for e in l]
    parents, idx, _ = api.list_explode(lst, raw=True)
    assert api.last_rows == len(flat)
    assert api.utf8_take([child], idx, as_arrow="pylist") == flat
    assert api.utf8_split(place(col, mem), ",", limit, as_arrow="pylist") == [[None if l is None else [e.decode() for e in l] for l in model[0]]]
    arrow = api.utf8_split(place(col, mem), ",", limit, as_arrow=True)[0]
    assert arrow.to_pylist() == [None if l is None else [e.decode() for e in l] for l in model[0]]


# ---------------------------------------------------------------- the result is a key
@pytest.mark.parametrize("mem", MEMS)
def test_a_replaced_column_is_a_group_by_key(api, mem):
    rng = np.random.default_rng(17)
    phones = ["555-12-34", "5551234", "555-1234", "-", "", "55-51-234", "044-1"]
    lens = [700, 0, 333]
    col = [utf8([None if rng.random() < 0.1 else phones[rng.integers(len(phones))] for _ in range(n)], 1, 1) for n in lens]
    res = run_op(api, "replace", col, mem, "-", "")
    key = [A.HostUtf8(offs.copy(), np.concatenate([data, np.zeros(8, dtype=np.uint8)]), None if valid is None else np.concatenate([valid, np.zeros(8, dtype=np.uint8)]),
                      0, c.length, 0, nulls) for (offs, data, valid, nulls), c in zip(res, col)]
    model = [None if r is None else R.replace(r, b"-", b"").decode() for c in col for r in c.rows]
    assert [s for k in key for s in k.to_pylist()] == model
    groups = list(dict.fromkeys(m for m in model if m is not None))
    keys, _, counts = api.groupby_agg_keys([place(key, mem)], None, "count", len(groups))
    k = keys[0].to_host() if isinstance(keys[0], A.DeviceUtf8) else keys[0]
    cnt = (counts.to_numpy() if isinstance(counts, A.HostArray) else counts.keep[0].cpu().numpy().view(np.int64))[:counts.length].tolist()
    got = dict(zip(k.to_pylist(), cnt))
    assert got.pop(None, model.count(None)) == model.count(None)      # (the NULL group, where the call reports one)
    assert got == {g: model.count(g) for g in groups}


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("mem", MEMS)
def test_the_same_call_and_another_chunking_give_the_same_bytes(api, mem):
    rng = np.random.default_rng(19)
    rows = rand_rows(rng, 1500, 0.1) + ["," * 900 + "ab", None, "ab" + "é" * 400]
    cuts = [(0, 1503)], [(0, 64), (64, 1000), (1000, 1503)]
    for build in (lambda c: run_op(api, "replace", c, mem, "a", "中"), lambda c: run_op(api, "translate", c, mem, "aé", "é"), lambda c: run_op(api, "initcap", c, mem)):
        one, again, cut = (build([utf8(rows[a:b]) for a, b in c]) for c in (cuts[0], cuts[0], cuts[1]))
        assert np.array_equal(one[0][0], again[0][0]) and np.array_equal(one[0][1], again[0][1]) and np.array_equal(one[0][2], again[0][2])
        assert b"".join(bytes(r[1]) for r in cut) == bytes(one[0][1])
    one, _ = run_split(api, [utf8(rows)], mem, ",", -1)
    cut, _ = run_split(api, [utf8(rows[a:b]) for a, b in cuts[1]], mem, ",", -1)
    assert b"".join(bytes(r[2]) for r in cut) == bytes(one[0][2]) and sum(len(r[1]) - 1 for r in cut) == len(one[0][1]) - 1


def test_the_kernel_is_named_and_timed(api):
    col = [utf8(["ab c", None, "c,de"] * 50)]
    for f in (lambda: api.utf8_replace(col, "a", "b"), lambda: api.utf8_translate(col, "a", "b"), lambda: api.utf8_initcap(col), lambda: api.utf8_split(col, ",")):
        lib.kernel_timing_reset(True)
        f()
        assert lib.last_kernel() == "utf8_rewrite_size_kernel + utf8_rewrite_write_kernel"
        ms, launches = lib.kernel_timing_get()
        lib.kernel_timing_reset(False)
        assert launches >= 1 and ms > 0
    assert api.utf8_initcap(col, as_arrow="pylist")[0][:3] == ["Ab C", None, "C,de"]
    assert api.utf8_replace(col, ",", "", as_arrow=True)[0].to_pylist()[:3] == ["ab c", None, "cde"]
