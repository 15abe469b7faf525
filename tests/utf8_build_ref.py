"""The executable model of rdf_utf8_concat / _pad / _repeat / _reverse / _substring_index: pure Python, a row at a time.
The reference declares concat, concat_ws, lpad, rpad, repeat, reverse and substring_index with empty bodies, so Spark 3's
semantics are defined HERE; tests/test_utf8_build_ref.py holds this file to pyarrow.compute where pyarrow means the same
thing, and to a hand-written table of Spark's examples.

None -> None everywhere (concat_ws skips None parts and never returns None).  Rows are str or bytes; a result has the type
of its row.  Everything is computed on UTF-8 bytes: a code point begins at every byte that is not a continuation byte
(10xxxxxx), which on valid UTF-8 is Python's own count of a str.
"""
import random

PARTS_MAX = 8
PATTERN_MAX = 1024
CLAMP = 1 << 31


def _b(s):
    return bytes(s) if isinstance(s, (bytes, bytearray)) else s.encode("utf-8")


def _like(row, b):
    """b as the type of row"""
    return b if isinstance(row, (bytes, bytearray)) else b.decode("utf-8")


def code_points(b):
    """The code points of a byte string as a list of byte strings (bytes before the first start byte go with the first)."""
    out = []
    for i, c in enumerate(b):
        if (c & 0xC0) != 0x80 or i == 0:
            out.append(bytearray())
        out[-1].append(c)
    return [bytes(x) for x in out]


def concat(parts):
    """parts: str / bytes / None.  NULL if any part is NULL."""
    if any(p is None for p in parts):
        return None
    return _like(parts[0], b"".join(_b(p) for p in parts))


def concat_ws(sep, parts):
    """NULL parts are skipped, empty strings are not; never NULL."""
    kept = [_b(p) for p in parts if p is not None]
    return _like(sep, _b(sep).join(kept))


def _pad(side, s, n, pad):
    if s is None:
        return None
    row, p = code_points(_b(s)), code_points(_b(pad))
    n = max(0, min(int(n), CLAMP))
    if len(row) >= n or not p:
        return _like(s, b"".join(row[:n]))
    fill = n - len(row)
    padding = b"".join(p) * (fill // len(p)) + b"".join(p[:fill % len(p)])
    return _like(s, padding + _b(s) if side == 0 else _b(s) + padding)


def lpad(s, n, pad):
    return _pad(0, s, n, pad)


def rpad(s, n, pad):
    return _pad(1, s, n, pad)


def repeat(s, times):
    return None if s is None else _like(s, _b(s) * max(0, int(times)))


def reverse(s):
    """Code points in reverse order, each one's bytes kept in order."""
    return None if s is None else _like(s, b"".join(reversed(code_points(_b(s)))))


def substring_index(s, delim, count):
    """Spark's UTF8String.subStringIndex, on bytes: each search resumes one byte after (before) the START of the last hit."""
    if s is None:
        return None
    x, d = _b(s), _b(delim)
    if not d or count == 0:
        return _like(s, b"")
    if count > 0:
        idx = -1
        for _ in range(min(count, len(x) + 1)):
            idx = x.find(d, idx + 1)
            if idx < 0:
                return s
        return _like(s, x[:idx])
    idx = len(x) - len(d) + 1
    for _ in range(min(-count, len(x) + 1)):
        if idx - 1 < 0:
            return s
        idx = x.rfind(d, 0, idx - 1 + len(d))      # the rightmost start <= idx - 1
        if idx < 0:
            return s
    return _like(s, x[idx + len(d):])


def apply(op, row, *args):
    """One row of a one-column op by name: ("lpad", n, pad), ("rpad", n, pad), ("repeat", times), ("reverse",),
    ("substring_index", delim, count)."""
    return {"lpad": lpad, "rpad": rpad, "repeat": repeat, "reverse": reverse, "substring_index": substring_index}[op](row, *args)


# ---------------------------------------------------------------- the lists the tests share
ALPHABET = ["a", "b", "c", ".", "é", "ß", "中", "😀", " "]

# (function, arguments, expected): Spark's documented examples and the edges of the contract
SPARK_TABLE = [
    (concat, (["Spark", "SQL"],), "SparkSQL"),
    (concat, (["a", None, "b"],), None),
    (concat, ([""],), ""),
    (concat_ws, (" ", ["Spark", "SQL"]), "Spark SQL"),
    (concat_ws, ("-", ["", ""]), "-"),
    (concat_ws, ("-", ["a", None, "b"]), "a-b"),
    (concat_ws, ("-", [None, None]), ""),
    (concat_ws, ("-", [None, "a"]), "a"),
    (concat_ws, ("-", ["a", None]), "a"),
    (concat_ws, ("", ["a", "b"]), "ab"),
    (concat_ws, ("中", ["a", "", "b"]), "a中中b"),
    (lpad, ("hi", 5, "??"), "???hi"),
    (lpad, ("hi", 1, "??"), "h"),
    (lpad, ("hi", 5, ""), "hi"),
    (lpad, ("hi", 0, "x"), ""),
    (lpad, ("hi", -3, "x"), ""),
    (lpad, ("hi", 2, "x"), "hi"),
    (lpad, (None, 5, "x"), None),
    (lpad, ("é中", 1, "x"), "é"),
    (lpad, ("", 3, "ab"), "aba"),
    (rpad, ("hi", 5, "??"), "hi???"),
    (rpad, ("hi", 1, "??"), "h"),
    (rpad, ("hi", 6, "ab"), "hiabab"),
    (rpad, ("hi", 7, "abc"), "hiabcab"),
    # multi-byte pads whose partial repetition ends between code points of different widths
    (lpad, ("x", 2, "aé中😀"), "ax"),
    (lpad, ("x", 3, "aé中😀"), "aéx"),
    (lpad, ("x", 4, "aé中😀"), "aé中x"),
    (lpad, ("x", 5, "aé中😀"), "aé中😀x"),
    (lpad, ("x", 6, "aé中😀"), "aé中😀ax"),
    (lpad, ("x", 8, "aé中😀"), "aé中😀aé中x"),
    (rpad, ("中", 4, "😀é"), "中😀é😀"),
    (rpad, ("😀😀", 3, "éa"), "😀😀é"),
    (repeat, ("123", 2), "123123"),
    (repeat, ("ab", 0), ""),
    (repeat, ("ab", -1), ""),
    (repeat, ("", 5), ""),
    (repeat, (None, 2), None),
    (reverse, ("Spark SQL",), "LQS krapS"),
    (reverse, ("aé中😀",), "😀中éa"),
    (reverse, ("",), ""),
    (reverse, (None,), None),
    (substring_index, ("www.apache.org", ".", 2), "www.apache"),
    (substring_index, ("www.apache.org", ".", -2), "apache.org"),
    (substring_index, ("www.apache.org", ".", 5), "www.apache.org"),
    (substring_index, ("www.apache.org", ".", -5), "www.apache.org"),
    (substring_index, ("www.apache.org", ".", 1), "www"),
    (substring_index, ("www.apache.org", ".", -1), "org"),
    (substring_index, ("www.apache.org", "", 1), ""),
    (substring_index, ("www.apache.org", ".", 0), ""),
    (substring_index, ("aaaa", "aa", 1), ""),
    (substring_index, ("aaaa", "aa", 2), "a"),
    (substring_index, ("aaaa", "aa", 3), "aa"),
    (substring_index, ("aaaa", "aa", 4), "aaaa"),
    (substring_index, ("aaaa", "aa", -1), ""),
    (substring_index, ("aaaa", "aa", -2), "a"),
    (substring_index, ("aaaa", "aa", -3), "aa"),
    (substring_index, ("aaaa", "aa", -4), "aaaa"),
    (substring_index, (".a", ".", 1), ""),
    (substring_index, ("a.", ".", -1), ""),
    (substring_index, ("a", "ab", 1), "a"),
    (substring_index, ("", ".", 1), ""),
    (substring_index, (None, ".", 1), None),
    (substring_index, ("a中b中c", "中", 2), "a中b"),
    (substring_index, ("a中b中c", "中", -1), "c"),
]


def rand_text(rng, maxlen=12, alphabet=ALPHABET):
    return "".join(rng.choice(alphabet) for _ in range(rng.randrange(maxlen + 1)))


def random_cases(op, n, seed=1):
    """n tuples (row, *arguments) for apply(op, ...), rows of the mixed-width alphabet, one in ten longer than a lane's
    16-byte piece; for "concat": (with_separator, sep, parts) with None parts among them."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        row = rand_text(rng, 40 if rng.random() < 0.1 else 12)
        if op == "concat":
            k = rng.randrange(1, PARTS_MAX + 1)
            parts = [None if rng.random() < 0.1 else rand_text(rng, 9) for _ in range(k)]
            ws = rng.random() < 0.5
            out.append((ws, rng.choice(["", ",", ", ", "中", "é-"]) if ws else "", parts))
        elif op in ("lpad", "rpad"):
            out.append((row, rng.randrange(-1, 30), rng.choice(["", " ", "0", "ab", "é", "aé中😀", "中😀"])))
        elif op == "repeat":
            out.append((row, rng.randrange(-1, 6)))
        elif op == "reverse":
            out.append((row,))
        else:
            delim = rng.choice([".", "a", "aa", "ab", "é", "中", " .", "😀"])
            if rng.random() < 0.5:
                row = (delim if rng.random() < 0.3 else "").join(rand_text(rng, 4, ALPHABET[:4]) for _ in range(rng.randrange(1, 6)))
            out.append((row, delim, rng.choice([-3, -2, -1, 1, 2, 3, 0, 7, -7])))
    return out


def write_host_table(path, nrows=100_000):
    """The table tests/cpp/test_utf8_build_host.cpp reads, a case a line, byte strings as hex ('-' = empty, 'N' = NULL):
         pad <side> <len> <pad> <row> <expected>        repeat <times> <row> <expected>       reverse <row> <expected>
         subidx <count> <delim> <row> <expected>        concat <ws> <sep> <expected> <part> ...
       expected '*' (broken UTF-8): only the output's length and the bounds are checked."""
    def hx(b):
        return "N" if b is None else (_b(b).hex() or "-")

    lines = []
    for fn, args, exp in SPARK_TABLE:
        if args[0] is None:
            continue
        if fn in (lpad, rpad):
            lines.append(f"pad {int(fn is rpad)} {args[1]} {hx(args[2])} {hx(args[0])} {hx(exp)}")
        elif fn is repeat:
            lines.append(f"repeat {args[1]} {hx(args[0])} {hx(exp)}")
        elif fn is reverse:
            lines.append(f"reverse {hx(args[0])} {hx(exp)}")
        elif fn is substring_index:
            lines.append(f"subidx {args[2]} {hx(args[1])} {hx(args[0])} {hx(exp)}")
        elif fn is concat:
            lines.append(f"concat 0 - {hx(exp)} " + " ".join(hx(p) for p in args[0]))
        else:
            lines.append(f"concat 1 {hx(args[0])} {hx(exp)} " + " ".join(hx(p) for p in args[1]))
    for side, op in enumerate(("lpad", "rpad")):
        for row, n, pad in random_cases(op, nrows // 2, seed=side + 1):
            lines.append(f"pad {side} {n} {hx(pad)} {hx(row)} {hx(apply(op, row, n, pad))}")
    for row, times in random_cases("repeat", nrows, 3):
        lines.append(f"repeat {times} {hx(row)} {hx(repeat(row, times))}")
    for (row,) in random_cases("reverse", nrows, 4):
        lines.append(f"reverse {hx(row)} {hx(reverse(row))}")
    for row, delim, count in random_cases("substring_index", nrows, 5):
        lines.append(f"subidx {count} {hx(delim)} {hx(row)} {hx(substring_index(row, delim, count))}")
    for ws, sep, parts in random_cases("concat", nrows, 6):
        exp = concat_ws(sep, parts) if ws else concat(parts)
        lines.append(f"concat {int(ws)} {hx(sep)} {hx(exp)} " + " ".join(hx(p) for p in parts))
    # long rows: more than one 16-byte piece, periods that do not divide 16, a delimiter at many positions
    rng = random.Random(7)
    for _ in range(200):
        row = rand_text(rng, 300)
        lines.append(f"reverse {hx(row)} {hx(reverse(row))}")
        for pad in ("aé中😀", "0"):
            lines.append(f"pad 0 400 {hx(pad)} {hx(row)} {hx(lpad(row, 400, pad))}")
            lines.append(f"pad 1 400 {hx(pad)} {hx(row)} {hx(rpad(row, 400, pad))}")
        lines.append(f"pad 1 {len(row) - 1} {hx('x')} {hx(row)} {hx(rpad(row, len(row) - 1, 'x'))}")
        lines.append(f"repeat 37 {hx(row[:7])} {hx(repeat(row[:7], 37))}")
        for count in (1, -1, 3, -3):
            lines.append(f"subidx {count} {hx('.a')} {hx(row)} {hx(substring_index(row, '.a', count))}")
    # broken UTF-8: bounds and lengths only
    for _ in range(2000):
        row = bytes(rng.choice([0x61, 0x80, 0xBF, 0xC3, 0xE4, 0xF0, 0xFF, 0xA9]) for _ in range(rng.randrange(40)))
        lines.append(f"reverse {hx(row)} *")
        lines.append(f"pad {rng.randrange(2)} {rng.randrange(50)} {hx(bytes([0xC3, 0x80, 0x80, 0x61][:rng.randrange(5)]))} {hx(row)} *")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)
