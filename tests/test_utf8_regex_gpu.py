"""rdf_utf8_regexp_match / _count / _extract / _replace / _split on the MI355X, bit for bit against the backtracking model of
tests/utf8_regex_ref.py, through the ABI, over host and device memory.  The text operations are called twice under the
sizing rule with guard bytes behind every buffer (run_call of the builders' tests).  The shapes are the smallest at which
these kernels can go wrong: several chunks with an empty one, row and value offsets, validity at odd bit offsets and a column
without it, rows of 0, 1, kUtf8ShortRow - 1 .. + 1 and 16 KiB + 1 bytes, output pointers at every alignment."""
import sys

import numpy as np
import pytest

import utf8_regex_ref as R
import utf8_rewrite_ref as RW
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
from test_utf8_build_gpu import place, run_call
from test_utf8_pred_gpu import check
from test_utf8_rewrite_gpu import check_rows, utf8

pytestmark = pytest.mark.gpu

MEMS = ["host", "device"]
SHORT_ROW, IMAGE = 256, 16384     # kUtf8ShortRow, kUtf8RewriteImage of rdf_utf8.h
ALPHABET = ["a", "b", "c", "A", "7", " ", ",", "\n", "é", "中", "😀"]
GROUP_LOOPS = ["(a|b)*?c", "(?:ab|c)+7", "(?i)(?:a |b)*"]     # the model recurses once per iteration: short rows only
PATTERNS = ["a", "a|ab", "a+?", "a*", "x*", "", "^a", "a$", "\\Aab|c\\z", "(?i)a+b", "(?s).", ".", "[^a]", "\\s+", "[^0-9]", "\\s*,\\s*",
            "(?:a|ab)(?:c|bcd)", "a{2,3}?", "a{2,3}", "[a-c]{2}7?", "\\W", "é|中+", "😀", "abc", "^", "$", "^$", "(?i)[^A]"]


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


def rand_rows(rng, n, null_frac=0.2, maxlen=14):
    return [None if rng.random() < null_frac else "".join(rng.choice(ALPHABET, size=rng.integers(0, maxlen + 1))) for _ in range(n)]


@pytest.fixture(scope="module")
def col():
    rng = np.random.default_rng(5)
    edge = ["", "a", "ab", "c", "abcd", "aaa", "baaac", "b" * (SHORT_ROW - 1) + "a", "a" + "b" * (SHORT_ROW - 1), "a" + "b" * (SHORT_ROW - 1) + "a",
            "é" * 128 + "a", None, b"a\x80\xffb", b"\xe4\xb8x", b"\x80a", b"\xf0\x9f\x98", "a\n\r\u0085 b", "AB12", " a , b,c "]
    long_row = ("ab c,7" * 2731)[:16384] + "a"      # 16 KiB + 1
    return [utf8(rand_rows(rng, 63) + edge, 3, 1), utf8([], 0, 0), utf8(rand_rows(rng, 257, 0.0), 5, 7), utf8([long_row, None, "a" * 600, "x"], 1, 2),
            utf8(rand_rows(rng, 256), 0, 0), utf8(rand_rows(rng, 65) + ["b" * 300 + "a"] * 70, 0, 3)]


def rows_of(col):
    return [c.rows for c in col]


@pytest.mark.parametrize("mem", MEMS)
def test_rlike_and_count_against_the_model(api, col, mem):
    ins = place(col, mem)
    for p in PATTERNS:
        check(api.utf8_regexp_match(ins, p), col, [[R.rlike(r, p) for r in rows] for rows in rows_of(col)], True, f"rlike {p!r} {mem}")
        check(api.utf8_regexp_count(ins, p), col, [[R.count(r, p) for r in rows] for rows in rows_of(col)], False, f"count {p!r} {mem}")
    short = [col[2], col[4]]
    for p in GROUP_LOOPS:
        check(api.utf8_regexp_count(place(short, mem), p), short, [[R.count(r, p) for r in rows] for rows in rows_of(short)], False, f"count {p!r} {mem}")
        text_op(api, "replace", short, mem, p, "-")
        text_op(api, "extract", short, mem, p)


def text_op(api, op, col, mem, *args, shift=0):
    call, _, nullable = getattr(api, f"utf8_regexp_{op}_call")(place(col, mem), *args)
    res = run_call(call, [c.length for c in col], nullable, mem, shift)
    model = {"extract": R.extract, "replace": R.replace}[op]
    check_rows(res, [[model(r, *args) for r in c.rows] for c in col], nullable, f"{op} {args!r:.60} {mem}")
    return res


@pytest.mark.parametrize("mem", MEMS)
def test_extract_and_replace_against_the_model(api, col, mem):
    for p in PATTERNS:
        text_op(api, "extract", col, mem, p)
        text_op(api, "replace", col, mem, p, "<é>")
    text_op(api, "replace", col, mem, "[^0-9]", "")
    text_op(api, "replace", col, mem, "a", "\\$\\\\")
    text_op(api, "replace", col, mem, "b", "x" * 100)      # the long rows grow past the image: written to HBM directly
    a = text_op(api, "replace", col, mem, "\\s+", " ")
    b = text_op(api, "replace", col, mem, "\\s+", " ")     # the same call twice
    one = [utf8([r for c in col for r in c.rows], 2, 3)]   # another chunking
    c = text_op(api, "replace", one, mem, "\\s+", " ")
    assert all(np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    assert np.array_equal(np.concatenate([x[1] for x in a]), c[0][1])


def test_output_pointers_at_every_alignment(api, col):
    for shift in range(16):
        text_op(api, "replace", col[3:5], "device", "a|,", "--", shift=shift)
        text_op(api, "extract", col[:1], "device", "[a-c]+", shift=shift)


@pytest.mark.parametrize("mem", MEMS)
def test_split_against_the_model_then_explode_and_take(api, col, mem):
    valid = [c for c in col if all(r is None or b"\x80" not in r and b"\xe4\xb8x" != r and b"\xf0\x9f\x98" != r for r in c.rows)]
    ins = place(valid, mem)
    for p in [",", "\\s*,\\s*", "", "x*", "a|b", " "]:
        for limit in (-1, 0, 1, 2, 5):
            got = api.utf8_regexp_split(ins, p, limit, as_arrow="pylist")
            want = [[None if r is None else [x.decode() for x in R.split(r, p, limit)] for r in c.rows] for c in valid]
            assert got == want, (p, limit, mem)
    # a regex-escaped literal splits like the literal operation
    a, b = api.utf8_regexp_split(ins, "\\,", 3, as_arrow="pylist"), api.utf8_split(ins, ",", 3, as_arrow="pylist")
    assert a == b
    # rdf_list_explode + rdf_utf8_take take the result as they take rdf_utf8_split's: the model's flattened list
    (lst, child), = api.utf8_regexp_split(ins[:1], "\\s*,\\s*", -1)
    flat = [x.decode() for r in valid[0].rows if r is not None for x in R.split(r, "\\s*,\\s*", -1)]
    parents, idx, _ = api.list_explode(lst, raw=True)
    assert api.last_rows == len(flat)
    assert api.utf8_take([child], idx, as_arrow="pylist") == flat


@pytest.mark.parametrize("mem", MEMS)
def test_escaped_literals_agree_with_the_literal_operations(api, col, mem):
    ins = place(col, mem)
    call, _, nullable = api.utf8_regexp_replace_call(ins, "\\,", "")
    a = run_call(call, [c.length for c in col], nullable, mem)
    call, _, nullable = api.utf8_replace_call(ins, ",", "")
    b = run_call(call, [c.length for c in col], nullable, mem)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    m1, m2 = api.utf8_regexp_match(ins, "ab c"), api.utf8_predicate("contains", ins, "ab c")
    from test_utf8_pred_gpu import raw
    for x, y, c in zip(m1, m2, col):
        assert np.array_equal(raw(x)[0][:(c.length + 7) // 8], raw(y)[0][:(c.length + 7) // 8])
    # the rlike mask drives rdf_utf8_filter
    got = api.utf8_filter(ins, m1, as_arrow=False)
    for g, c in zip(got, col):
        h = g.to_host() if mem == "device" else g
        assert h.length == sum(r is not None and b"ab c" in r for r in c.rows)


# One pattern just under each cap of rdf_utf8_regex.h, with what rdf_utf8_regexp_info must report of it:
#   states   2048 forward states of kUtf8RegexMaxStates = 2048 (c{509} in its place is refused)
#   program  4070 instructions of kUtf8RegexMaxProgram = 4096 ({84} is refused)
#   table    261 984 table bytes of kUtf8RegexMaxTableBytes = 262 144 (z{186} is refused), walked out of HBM
WIDE_STAR = "(?:" + "|".join("acegikmoqsuwyACEGIKMOQSUWY02468") + ")*a(?:a|c){8}"
UNDER_A_CAP = [
    ("(?:a|b)*a(?:a|b){8}|c{508}", "(?:a|b)*a(?:a|b){8}|c{509}", "forward_states", 2048, 2048),
    ("^(?:é|中|😀|[^a]){83}$", "^(?:é|中|😀|[^a]){84}$", "program_len", 4070, 4096),
    (WIDE_STAR + "|z{185}", WIDE_STAR + "|z{186}", "table_bytes", 261984, 256 * 1024),
]


@pytest.mark.parametrize("pattern,beyond,field,value,cap", UNDER_A_CAP)
def test_a_pattern_just_under_each_cap(api, pattern, beyond, field, value, cap):
    info = api.utf8_regexp_info(pattern)
    assert info[field] == value and cap * 0.99 <= value <= cap
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(20000)      # the model recurses once per counted atom: c{508} is 508 deep
    try:
        under_a_cap(api, pattern, beyond)
    finally:
        sys.setrecursionlimit(limit)


def under_a_cap(api, pattern, beyond):
    with pytest.raises(A.RdfError) as e:
        api.utf8_regexp_info(beyond)
    assert e.value.status == A.RDF_INVALID_ARGUMENT
    rng = np.random.default_rng(11)
    rows = ["".join(rng.choice(["a", "b", "c"], size=k % 40)) for k in range(70)]
    rows += ["".join(rng.choice(["a", "c", "e", "8", "Y", "z"], size=k % 40)) for k in range(70)]
    rows += ["c" * 507, "c" * 508, "b" + "c" * 1020 + "ab", "z" * 184, "az" * 9 + "z" * 185, "z" * 400, None]
    rows += [s * 83 for s in ("é", "中", "😀", "b")] + ["é" * 82, "中" * 84, "é" * 40 + "a" + "😀" * 42, "é" * 40 + "\n" + "😀" * 42, b"b" * 82 + b"\x80", b"\xf0\x9f\x98" + b"b" * 82]
    chunks = [utf8(rows[:100], 1, 3), utf8(rows[100:], 2, 0)]
    want = [[R.count(r, pattern) for r in c.rows] for c in chunks]
    assert sum(x or 0 for w in want for x in w) > 3
    for mem in MEMS:
        check(api.utf8_regexp_count(place(chunks, mem), pattern), chunks, want, False, pattern)
        check(api.utf8_regexp_match(place(chunks, mem), pattern), chunks, [[R.rlike(r, pattern) for r in c.rows] for c in chunks], True, pattern)
        text_op(api, "replace", chunks, mem, pattern, "<é>")
        text_op(api, "extract", chunks, mem, pattern)


@pytest.mark.parametrize("mem", MEMS)
def test_split_of_rows_with_broken_utf8(api, col, mem):
    """the child's offsets and bytes against the model, bytes as they are: a broken row is never matched inside a broken sequence"""
    ins = place(col, mem)
    for p, limit in ((",", -1), ("", -1), ("x*", 3), (".", -1), ("[^a]", 0), ("\\s*,\\s*", 2)):
        for (lst, child), c in zip(api.utf8_regexp_split(ins, p, limit), col):
            want = [None if r is None else R.split(r, p, limit) for r in c.rows]
            flat = [x for w in want if w is not None for x in w]
            h = child.to_host() if mem == "device" else child
            assert h.length == len(flat), (p, limit)
            o = h.offsets[:h.length + 1].astype(np.int64)
            raw = h.data.tobytes()
            assert [raw[o[i]:o[i + 1]] for i in range(h.length)] == [bytes(x) for x in flat], (p, limit)
            if mem == "host":
                lo = lst.offsets[:c.length + 1]
                assert list(np.diff(lo)) == [0 if w is None else len(w) for w in want], (p, limit)


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("edge", [4096, IMAGE])     # kUtf8CopyTile, kUtf8RewriteImage of rdf_utf8.h
def test_chunk_lengths_on_the_tile_and_image_edges(api, mem, edge):
    """outputs, then inputs, whose chunk length falls on edge - 1, edge, edge + 1 bytes; one row around the image's size"""
    cols = []
    for total in (edge - 1, edge, edge + 1):
        rows, left = [], total
        while left > 0:
            n = min(left, 37)
            rows.append(b"ab" * (n // 2) + b"c" * (n % 2))
            left -= n
        cols.append(utf8(rows))
    res = text_op(api, "replace", cols, mem, "[b]", "d")
    assert [len(r[1]) for r in res] == [edge - 1, edge, edge + 1]
    text_op(api, "replace", cols, mem, "ab?", "a")          # the INPUT falls on the edge, the output does not
    text_op(api, "extract", cols, mem, "(?:ab)+")
    for n in (IMAGE - 1, IMAGE, IMAGE + 1):                 # (the last is written directly)
        text_op(api, "replace", [utf8([b"x", b"ab" * (n // 2) + b"c" * (n % 2), b"y"])], mem, "b|c$", "d")


def test_patterns_near_the_caps_and_the_kernels_by_name(api, col):
    info = api.utf8_regexp_info("a{200}")
    assert info["forward_states"] >= 200 and info["table_bytes"] <= 32 * 1024 and not info["can_match_empty"]
    big = api.utf8_regexp_info("(?:a|b|c|e|g|i|k|m|o)*a(?:a|b){8}")        # 1540 forward states of 21 classes: the tables stay in HBM
    assert 1024 < big["forward_states"] <= 2048 and 32 * 1024 < big["table_bytes"] <= 256 * 1024
    lds = api.utf8_regexp_info("(?:a|b)*a(?:a|b){8}")                       # as many states of 8 classes: just under the LDS budget
    assert lds["forward_states"] > 1024 and 24 * 1024 < lds["table_bytes"] <= 32 * 1024
    with pytest.raises(A.RdfError) as e:
        api.utf8_regexp_info("(a|b)*a(a|b){12}")
    assert e.value.status == A.RDF_INVALID_ARGUMENT and "states" in str(e.value)
    ab = [utf8(["".join(np.random.default_rng(k).choice(["a", "b"], size=k % 40)) for k in range(300)] + ["ab" * 40], 1, 1)]
    long_a = [utf8(["a" * 450, "a" * 199, "b" + "a" * 200, None], 0, 1)]     # (the model recurses per iteration of a group: a{200} alone gets the long rows)
    for mem in MEMS:
        check(api.utf8_regexp_count(place(long_a, mem), "a{200}"), long_a, [[R.count(r, "a{200}") for r in long_a[0].rows]], False, "a{200}")
        text_op(api, "replace", long_a, mem, "a{200}", "-")
    for p in ("a{200}", "(?:a|b|c|e|g|i|k|m|o)*a(?:a|b){8}", "(?:a|b)*a(?:a|b){8}", "b(?:a|b){9}$"):
        for mem in MEMS:
            check(api.utf8_regexp_count(place(ab, mem), p), ab, [[R.count(r, p) for r in ab[0].rows]], False, p)
            text_op(api, "replace", ab, mem, p, "-")
    for f, name in ((lambda: api.utf8_regexp_match(col, "a"), "utf8_regex_measure_kernel"),
                    (lambda: api.utf8_regexp_replace(col, "a", "b"), "utf8_regex_size_kernel + utf8_regex_write_kernel"),
                    (lambda: api.utf8_regexp_split(col, ","), "utf8_regex_size_kernel + utf8_regex_write_kernel")):
        lib.kernel_timing_reset(True)
        f()
        assert lib.last_kernel() == name
        ms, launches = lib.kernel_timing_get()
        lib.kernel_timing_reset(False)
        assert launches >= 1 and ms > 0
    assert api.utf8_regexp_replace([utf8(["aaa", "ab", "c"])], "^a", "x", as_arrow="pylist")[0] == ["xaa", "xb", "c"]
    assert api.utf8_regexp_match([utf8(["ab", "c"])], "abc")[0].values[0] & 3 == 0      # a match never completes in the next row
