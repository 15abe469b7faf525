"""rdf_utf8_predicate / rdf_utf8_compare / rdf_utf8_measure on the MI355X, bit for bit against the model of
tests/utf8_pred_ref.py: the value and validity bitmaps byte by byte (NULL rows hold 0, bits beyond the last row are 0), the
Int32 values, the NULL counts.  Every case runs over host and device memory."""
import numpy as np
import pytest

import utf8_pred_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu

MEMS = ["host", "device"]
CHUNK_ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
LAYOUTS = [(0, 0), (3, 1), (5, 7), (1, 0)]
ALPHABET = ["a", "b", "c", "x", "é", "ß", "中", "😀", "%", "_", " "]


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


def as_host(out):
    """a result array as a HostArray"""
    if isinstance(out, A.HostArray):
        return out
    vals, valid = raw(out)
    return A.HostArray(vals if out.dtype == A.BOOL else vals.view(A.NP_OF[out.dtype]), valid, 0, out.length, out.dtype, out.null_count)


def bits(flags):
    return np.packbits(np.asarray(flags, dtype=np.uint8), bitorder="little") if len(flags) else np.zeros(0, dtype=np.uint8)


def check(outs, chunks, expected, boolean, what=""):
    """expected[i]: the model's list for chunk i (None = NULL)"""
    assert len(outs) == len(chunks) == len(expected), what
    for i, (o, c, exp) in enumerate(zip(outs, chunks, expected)):
        rows = len(exp)
        assert o.length == rows and o.dtype == (A.BOOL if boolean else A.I32), (what, i)
        assert o.null_count == sum(e is None for e in exp), (what, i, o.null_count)
        vals, valid = raw(o)
        nb = (rows + 7) // 8
        if boolean:
            want = bits([bool(e) for e in exp])
            got = vals[:nb]
            if not np.array_equal(got, want):
                bad = np.flatnonzero(np.unpackbits(got ^ want, bitorder="little")[:rows])
                raise AssertionError(f"{what} chunk {i}: value bits differ at rows {bad[:10]} of {rows}: "
                                     f"{[(int(r), c.to_pylist()[r][:40] if c.to_pylist()[r] is not None else None, exp[r]) for r in bad[:5]]}")
        else:
            want = np.array([0 if e is None else e for e in exp], dtype=np.int32)
            got = vals[:rows * 4].view(np.int32)
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError(f"{what} chunk {i}: values differ at rows {bad[:10]}: got {got[bad[:5]]}, expected {want[bad[:5]]}")
        nullable = c.validity is not None
        assert (valid is not None) == nullable, (what, i)
        if nullable:
            assert np.array_equal(valid[:nb], bits([e is not None for e in exp])), f"{what} chunk {i}: validity bits differ"


def rows_of(chunks):
    return [c.to_pylist() for c in chunks]


def run_pred(api, op, chunks, mem, pattern, escape=None):
    outs = api.utf8_predicate(op, place(chunks, mem), pattern, escape)
    check(outs, chunks, [[R.predicate(op, s, pattern, escape) for s in rows] for rows in rows_of(chunks)], True, f"{op} {pattern!r:.60} {mem}")
    return outs


def run_measure(api, what, chunks, mem, pattern="", pos=1):
    outs = api.utf8_measure(what, place(chunks, mem), pattern, pos)
    check(outs, chunks, [[R.measure(what, s, pattern, pos) for s in rows] for rows in rows_of(chunks)], False, f"{what} {pattern!r:.60} {pos} {mem}")
    return outs


def run_compare(api, op, a, b, mem):
    outs = api.utf8_compare(op, place(a, mem), place(b, mem))
    exp = [[R.compare(op, x, y) for x, y in zip(ra, rb)] for ra, rb in zip(rows_of(a), rows_of(b))]
    both = [x if x.validity is not None else y for x, y in zip(a, b)]     # (nullable if either side is)
    check(outs, both, exp, True, f"compare {op} {mem}")
    return outs


def rand_rows(rng, n, null_frac, maxlen=14):
    out = []
    for _ in range(n):
        if rng.random() < null_frac:
            out.append(None)
        else:
            out.append("".join(rng.choice(ALPHABET, size=rng.integers(0, maxlen + 1))))
    return out


def column(rng, null_frac, ro, do, lens=CHUNK_ROWS):
    return [A.HostUtf8.from_pylist(rand_rows(rng, n, null_frac), row_offset=ro, data_offset=do) for n in lens]


# ---------------------------------------------------------------- every op over every layout
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("ro,do", LAYOUTS)
@pytest.mark.parametrize("null_frac", [0.0, 0.1])
def test_every_op_over_chunks_offsets_and_nulls(api, mem, ro, do, null_frac):
    rng = np.random.default_rng(100 * ro + do + int(null_frac * 10))
    col = column(rng, null_frac, ro, do)
    other = column(rng, null_frac, do % 4, ro)
    # some rows of the other column are the first one's, so that eq / le / ge have something to find
    for c, o in zip(col, other):
        ra, rb = c.to_pylist(), o.to_pylist()
        for i in range(0, len(ra), 3):
            rb[i] = ra[i] if rb[i] is not None else None
        o2 = A.HostUtf8.from_pylist(rb, row_offset=o.offset, data_offset=o.data_offset)
        o.offsets, o.data, o.validity, o.null_count = o2.offsets, o2.data, o2.validity, o2.null_count
    for op in R.COMPARISONS:
        run_pred(api, op, col, mem, "ab")
        run_compare(api, op, col, other, mem)
    for op in ("starts_with", "ends_with", "contains"):
        for lit in ("", "a", "é", "ab"):
            run_pred(api, op, col, mem, lit)
    for pat in ("%", "a%", "%a", "%ab%", "_%b", "a_c%", "%a%b%", "%é_", "%\\%%", "__", ""):
        run_pred(api, "like", col, mem, pat, "\\")
    run_measure(api, "length", col, mem)
    run_measure(api, "octet_length", col, mem)
    for sub, pos in (("a", 1), ("ab", 2), ("é", 3), ("", 2), ("😀", 1), ("a", 0)):
        run_measure(api, "locate", col, mem, sub, pos)


@pytest.mark.parametrize("mem", MEMS)
def test_null_counts_the_host_does_not_know_are_counted(api, mem):
    rng = np.random.default_rng(5)
    col = column(rng, 0.3, 2, 3, [1000, 0, 300])
    other = column(rng, 0.2, 0, 0, [1000, 0, 300])
    for c in col:
        c.null_count = -1
    run_pred(api, "contains", col, mem, "a")
    run_measure(api, "length", col, mem)
    run_compare(api, "lt", col, other, mem)          # both sides nullable: counted although both counts are known
    plain = [A.HostUtf8.from_pylist([s or "" for s in c.to_pylist()]) for c in other]
    run_compare(api, "ge", plain, col, mem)          # validity on the right side only
    run_compare(api, "ge", col, plain, mem)


# ---------------------------------------------------------------- comparisons
@pytest.mark.parametrize("mem", MEMS)
def test_comparisons_in_unsigned_byte_order(api, mem):
    rows = R.COMPARE_ROWS
    col = [A.HostUtf8.from_pylist(rows), A.HostUtf8.from_pylist(rows + [None], row_offset=2, data_offset=5)]
    for lit in rows:
        for op in R.COMPARISONS:
            run_pred(api, op, col, mem, lit)
    assert R.compare("gt", "é", "z") and R.compare("lt", "a", "a\0") and R.compare("lt", "a\0", "a\0b")
    for k in range(1, len(rows)):
        rot = rows[k:] + rows[:k]
        a = [A.HostUtf8.from_pylist(rows + [None, "a", None])]
        b = [A.HostUtf8.from_pylist(rot + ["a", None, None], row_offset=1)]
        for op in R.COMPARISONS:
            run_compare(api, op, a, b, mem)


# ---------------------------------------------------------------- LIKE
@pytest.mark.parametrize("mem", MEMS)
def test_like_edge_list(api, mem):
    col = [A.HostUtf8.from_pylist(R.LIKE_ROWS + [None]), A.HostUtf8.from_pylist(R.LIKE_ROWS[::-1], row_offset=3, data_offset=2)]
    for pat in R.LIKE_PATTERNS:
        try:
            R.like_tokens(pat, "\\")
        except R.BadPattern:
            with pytest.raises(A.RdfError) as ei:
                api.utf8_predicate("like", place(col, mem), pat, "\\")
            assert ei.value.status == A.RDF_INVALID_ARGUMENT
            continue
        run_pred(api, "like", col, mem, pat, "\\")
        run_pred(api, "like", col, mem, pat.replace("\\", "#"), "#")
    for pat, esc in R.LIKE_HASH:
        run_pred(api, "like", col, mem, pat, esc)
    one = [A.HostUtf8.from_pylist(["é", "😀", "éé", "", "a", "中"])]
    run_pred(api, "like", one, mem, "_")
    run_pred(api, "like", one, mem, "_", "\\")
    # without an escape the backslash is an ordinary character
    run_pred(api, "like", col, mem, "a\\b")
    run_pred(api, "like", col, mem, "a\\%")


# ---------------------------------------------------------------- rows do not leak into each other
@pytest.mark.parametrize("mem", MEMS)
def test_a_match_never_extends_past_its_row(api, mem):
    col = [A.HostUtf8.from_pylist(["xab", "cx", "ab", "c", "", "abc"])]
    outs = run_pred(api, "contains", col, mem, "abc")
    assert list(np.unpackbits(raw(outs[0])[0][:1], bitorder="little")[:6]) == [0, 0, 0, 0, 0, 1]
    run_pred(api, "like", col, mem, "%abc%")
    run_pred(api, "like", col, mem, "%ab_")
    run_pred(api, "ends_with", col, mem, "abc")
    run_pred(api, "starts_with", col, mem, "cx")
    run_measure(api, "locate", col, mem, "abc")
    run_measure(api, "locate", col, mem, "bc")
    # the chunk ends at "xab" (hi = 3) and the bytes that would complete the needle follow inside the same data buffer
    whole = A.HostUtf8.from_pylist(["xab", "cdefghijklmnop"])
    first = A.HostUtf8(whole.offsets[:2].copy(), whole.data, None, 0, 1, 0, 0)
    assert first.to_pylist() == ["xab"] and bytes(whole.data[3:6]) == b"cde"
    for needle in ("abc", "abcdefgh", "xabc"):
        run_pred(api, "contains", [first], mem, needle)
        run_pred(api, "like", [first], mem, "%" + needle + "%")
        run_pred(api, "like", [first], mem, "xa_" + "_")
        run_pred(api, "starts_with", [first], mem, "xabc")
        run_pred(api, "ge", [first], mem, "xabc")
        run_measure(api, "locate", [first], mem, needle)
    run_measure(api, "length", [first], mem)
    run_compare(api, "eq", [first], [A.HostUtf8.from_pylist(["xabc"])], mem)
    # the same with a long row, which the wave takes
    long_row = "." * 700 + "ab"
    whole = A.HostUtf8.from_pylist([long_row, "cdefghijklmnopqrstuvwxyz"])
    first = A.HostUtf8(whole.offsets[:2].copy(), whole.data, None, 0, 1, 0, 0)
    for needle in ("abc", "abcdefghijklmnopq", "b" + "c"):
        run_pred(api, "contains", [first], mem, needle)
        run_pred(api, "like", [first], mem, "%" + needle + "%")
        run_pred(api, "like", [first], mem, "%ab_")
        run_measure(api, "locate", [first], mem, needle)
    run_measure(api, "length", [first], mem)
    run_compare(api, "lt", [first], [A.HostUtf8.from_pylist([long_row + "c"])], mem)


# ---------------------------------------------------------------- the short / long boundary and the wave's pieces
def boundary_rows():
    rows = []
    for n in (255, 256, 257, 1023, 1024, 1025):
        rows += ["." * (n - 3) + "abc", "abc" + "." * (n - 3), "." * n, "x" + "." * (n - 5) + "abcy", "." * (n // 2) + "abc" + "." * (n - 3 - n // 2)]
        k = (n - 3) // 2
        rows += ["é" * k + "." * (n - 3 - 2 * k) + "abc", "abc" + "é" * k + "." * (n - 3 - 2 * k), "😀" * (n // 4) + "." * (n % 4)]
    assert sorted({len(r.encode()) for r in rows}) == [255, 256, 257, 1023, 1024, 1025]
    return rows


@pytest.mark.parametrize("mem", MEMS)
def test_rows_around_the_short_row_limit(api, mem):
    rows = boundary_rows()
    col = [A.HostUtf8.from_pylist(rows, data_offset=3), A.HostUtf8.from_pylist(rows[::-1] + [None], row_offset=1)]
    for op, lit in (("contains", "abc"), ("contains", "abcd"), ("contains", "."), ("starts_with", "abc"), ("ends_with", "abc"), ("eq", rows[0]), ("lt", "." * 300),
                    ("ge", "abc" + "." * 252)):
        run_pred(api, op, col, mem, lit)
    for pat in ("%abc%", "x%abc%y", "%abc", "abc%", "%a_c%", "_%abc", "%.abc.%", "%é.%abc", "%" + "_" * 255, "_" * 256, "%" + "." * 200 + "%abc"):
        run_pred(api, "like", col, mem, pat)
    run_measure(api, "length", col, mem)
    run_measure(api, "octet_length", col, mem)
    for sub, pos in (("abc", 1), ("abc", 2), ("abc", 200), ("c", 128), ("", 256), ("", 1026), ("é.", 1), ("😀", 60)):
        run_measure(api, "locate", col, mem, sub, pos)
    other = [A.HostUtf8.from_pylist(rows[1:] + rows[:1]), A.HostUtf8.from_pylist(rows[::-1] + ["a"], row_offset=4)]
    for op in R.COMPARISONS:
        run_compare(api, op, col, other, mem)


def needle_rows(filler, width):
    """rows of `width` characters: x, filler, the needle at every position, filler, y; one row per position and needle"""
    rows = []
    for m in (1, 3, 17):
        needle = "abcdefghijklmnopq"[:m]
        room = width - 2 - m
        rows += ["x" + filler * i + needle + filler * (room - i) + "y" for i in range(room + 1)]
    return rows


@pytest.fixture(scope="module")
def needle_columns():
    ascii_rows = needle_rows(".", 2200)
    assert all(len(r) == 2200 for r in ascii_rows[::97])
    wide_rows = needle_rows("中", 735)            # 3-byte filler: code-point and byte positions differ; about 2200 bytes
    cols = {}
    for name, rows in (("ascii", ascii_rows), ("wide", wide_rows)):
        half = len(rows) // 2
        host = [A.HostUtf8.from_pylist(rows[:half], data_offset=1), A.HostUtf8.from_pylist(rows[half:], row_offset=1)]
        cols[name] = {"host": host, "rows": [rows[:half], rows[half:]]}
    return cols


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("filler", ["ascii", "wide"])
def test_a_needle_at_every_position_of_long_rows(api, needle_columns, mem, filler):
    entry = needle_columns[filler]
    col, rows = entry["host"], entry["rows"]
    ins = place(col, mem)
    if mem == "device":
        entry["device"] = ins

    def pred(op, pattern, model):
        outs = api.utf8_predicate(op, ins, pattern)
        check(outs, col, [[model(s) for s in r] for r in rows], True, f"{op} {pattern} {filler} {mem}")

    def locate(sub, pos):
        outs = api.utf8_measure("locate", ins, sub, pos)
        check(outs, col, [[R.locate(sub, s, pos) for s in r] for r in rows], False, f"locate {sub} {pos} {filler} {mem}")

    for m in (1, 3, 17):
        needle = "abcdefghijklmnopq"[:m]
        pred("contains", needle, lambda s: needle in s)
        pred("like", "%" + needle + "%", lambda s: needle in s)
        # x%needle%y: every row begins with x and ends with y, so the row matches iff it holds the needle between them
        pred("like", "x%" + needle + "%y", lambda s: needle in s[1:-1])
        pred("like", "%" + needle[:-1] + "_" + "%", lambda s: needle in s or (m > 1 and needle[:-1] in s))
        locate(needle, 1)
        locate(needle, len(rows[0][0]) // 2)          # past the hit for half of the positions
        locate(needle, 2)
    outs = api.utf8_measure("length", ins)
    check(outs, col, [[len(s) for s in r] for r in rows], False, f"length {filler} {mem}")


@pytest.mark.parametrize("mem", MEMS)
def test_length_of_rows_of_5000_mixed_width_code_points(api, mem):
    rng = np.random.default_rng(11)
    pool = ["a", "é", "中", "😀", "\0"]          # (picked by index: a numpy string array would drop the NUL)
    rows = ["".join(pool[k] for k in rng.integers(0, len(pool), size=5000)) for _ in range(7)] + ["", None, "é" * 5000, "a" * 5000 + "😀"]
    col = [A.HostUtf8.from_pylist(rows, row_offset=2, data_offset=5)]
    outs = run_measure(api, "length", col, mem)
    assert raw(outs[0])[0][:44].view(np.int32)[:7].tolist() == [5000] * 7
    run_measure(api, "octet_length", col, mem)
    run_measure(api, "locate", col, mem, "😀a", 2500)
    run_measure(api, "locate", col, mem, "", 5001)
    run_measure(api, "locate", col, mem, "", 5002)


@pytest.mark.parametrize("mem", MEMS)
def test_compare_of_long_rows_that_differ_in_one_byte(api, mem):
    base = "".join(chr(ord("a") + i % 23) for i in range(4000))
    a_rows, b_rows = [], []
    for k in (0, 15, 16, 1023, 1024, 3999):
        hi = base[:k] + "~" + base[k + 1:]
        lo = base[:k] + "!" + base[k + 1:]
        a_rows += [base, hi, lo, base]
        b_rows += [hi, base, base, lo]
    for n in (0, 1, 255, 256, 257, 1024, 3999):       # one row a proper prefix of the other
        a_rows += [base[:n], base]
        b_rows += [base, base[:n]]
    a_rows += [base, None, base]
    b_rows += [base, base, None]
    a = [A.HostUtf8.from_pylist(a_rows, data_offset=1)]
    b = [A.HostUtf8.from_pylist(b_rows, row_offset=3, data_offset=2)]
    for op in R.COMPARISONS:
        run_compare(api, op, a, b, mem)


# ---------------------------------------------------------------- outputs: nothing beyond (rows + 7) / 8 bytes
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("rows", [1, 7, 8, 63, 64, 65, 250, 256, 321])
def test_nothing_is_written_past_the_bitmaps(api, mem, rows):
    rng = np.random.default_rng(rows)
    col = [A.HostUtf8.from_pylist(rand_rows(rng, rows, 0.2) + [None], row_offset=1)]      # (always nullable)
    n = rows + 1
    nb = (n + 7) // 8
    if mem == "device":
        import torch
        vt = torch.full((nb + 16,), 0xAA, dtype=torch.uint8, device="cuda")
        bt = torch.full((nb + 16,), 0xAA, dtype=torch.uint8, device="cuda")
        out = A.DeviceArray(vt.data_ptr(), bt.data_ptr(), 0, n, A.BOOL, 0, keep=(vt, bt), capacity=n)
    else:
        out = A.HostArray(np.full(nb + 16, 0xAA, dtype=np.uint8), np.full(nb + 16, 0xAA, dtype=np.uint8), 0, n, A.BOOL, 0)
    outs = api.utf8_predicate("contains", place(col, mem), "a", outs=[out])
    check(outs, col, [[R.predicate("contains", s, "a") for s in col[0].to_pylist()]], True, f"{rows} rows {mem}")
    vals, valid = raw(outs[0])
    assert (vals[nb:nb + 16] == 0xAA).all() and (valid[nb:nb + 16] == 0xAA).all()


# ---------------------------------------------------------------- chaining
@pytest.mark.parametrize("mem", MEMS)
def test_the_mask_filters_text_and_numbers_and_joins_a_predicate(api, mem):
    from oracle import oracle
    rng = np.random.default_rng(21)
    lens = [300, 0, 77]
    col = column(rng, 0.1, 1, 2, lens)
    nums = [A.HostArray.from_numpy(rng.integers(0, 100, n).astype(np.int64), valid=rng.uniform(size=n) > 0.1) for n in lens]
    ins, dnums = place(col, mem), place(nums, mem)
    mask = api.utf8_predicate("like", ins, "%a%")
    model = [[R.like(s, "%a%") for s in rows] for rows in rows_of(col)]
    # Column::filter keeps the rows whose mask bit is set and valid
    kept = api.utf8_filter(ins, mask, as_arrow="pylist")
    assert kept == [[s for s, m in zip(rows, mm) if m] for rows, mm in zip(rows_of(col), model)]
    counts = [sum(bool(m) for m in mm) for mm in model]
    got = api.filter(dnums, mask, outs=[api._window_out(A.I64, k, True, True) for k in counts] if mem == "device" else None)
    for g, x, mm in zip(got, nums, model):
        assert as_host(g).to_pylist() == [v for v, m in zip(x.to_pylist(), mm) if m]
    # the mask as a Boolean input column of rdf_predicate under `and` with a numeric comparison: rdf_predicate's own rule
    # for NULLs, taken from the oracle fed with the MODEL's mask
    e = A.Expr()
    root = e.op("and", e.col(0), e.op("gt", e.col(1), e.scalar(50, A.I64)))
    model_mask = [A.HostArray.from_numpy(np.array([bool(m) for m in mm], dtype=bool), valid=np.array([m is not None for m in mm], dtype=bool), dtype=A.BOOL)
                  if c.validity is not None else A.HostArray.from_numpy(np.array([bool(m) for m in mm], dtype=bool), dtype=A.BOOL)
                  for mm, c in zip(model, col)]
    want = oracle.api().predicate(e, root, [model_mask, nums])
    res = api.predicate(e, root, [mask, dnums], outs=[api._window_out(A.BOOL, n, True, True) for n in lens] if mem == "device" else None)
    for g, w in zip(res, want):
        g = as_host(g)
        assert g.length == w.length and g.null_count == w.null_count
        assert np.array_equal(g.valid_mask(), w.valid_mask())
        assert np.array_equal(g.to_numpy()[w.valid_mask()], w.to_numpy()[w.valid_mask()])
    for w, mm, x in zip(want, model, nums):        # and the oracle's conjunction is the model's where both sides are known
        for r, (m, v, ok) in enumerate(zip(mm, x.to_pylist(), w.valid_mask())):
            if m is not None and v is not None:
                assert ok and bool(w.to_numpy()[r]) == (m and v > 50)


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("mem", MEMS)
def test_the_same_call_and_another_chunking_give_the_same_bytes(api, mem):
    rng = np.random.default_rng(31)
    rows = rand_rows(rng, 1500, 0.1) + ["." * 900 + "ab", None, "ab" + "é" * 400]
    one = [A.HostUtf8.from_pylist(rows)]
    cut = [A.HostUtf8.from_pylist(rows[:64]), A.HostUtf8.from_pylist(rows[64:1000], row_offset=2), A.HostUtf8.from_pylist(rows[1000:] + [None], data_offset=3)]
    rows2 = rows + [None]

    def flat(outs, n, boolean):
        vals, valid = [], []
        for o in outs:
            v, b = raw(o)
            vals += list(np.unpackbits(v[:(o.length + 7) // 8], bitorder="little")[:o.length]) if boolean else list(v[:o.length * 4].view(np.int32))
            valid += list(np.unpackbits(b[:(o.length + 7) // 8], bitorder="little")[:o.length])
        return vals[:n], valid[:n]

    for call, boolean in ((lambda c: api.utf8_predicate("like", c, "%a_%b%"), True), (lambda c: api.utf8_predicate("contains", c, "ab"), True),
                          (lambda c: api.utf8_measure("locate", c, "ab", 2), False), (lambda c: api.utf8_measure("length", c), False),
                          (lambda c: api.utf8_compare("le", c, c), True)):
        a1 = call(place(one, mem))
        a2 = call(place(one, mem))
        assert all(np.array_equal(raw(x)[0], raw(y)[0]) and np.array_equal(raw(x)[1], raw(y)[1]) for x, y in zip(a1, a2))
        assert flat(a1, len(rows), boolean) == flat(call(place(cut, mem)), len(rows), boolean)
    assert len(rows2) == sum(c.length for c in cut)


def test_the_kernel_is_named_and_timed(api):
    col = [A.HostUtf8.from_pylist(["ab", None, "cde"] * 50)]
    lib.kernel_timing_reset(True)
    api.utf8_predicate("like", col, "%b%")
    assert lib.last_kernel() == "utf8_pred_kernel"
    ms, launches = lib.kernel_timing_get()
    lib.kernel_timing_reset(False)
    assert launches >= 1 and ms > 0
