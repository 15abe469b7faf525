"""The executable model of rdf_utf8_predicate / rdf_utf8_compare / rdf_utf8_measure: pure Python on str / bytes, a row at a
time.  The reference declares length, locate, ... as empty stubs and compares strings as Float64, so SQL / Spark semantics
are defined HERE; tests/test_utf8_pred_ref.py holds this file to pyarrow.compute and to an independent LIKE matcher.

None -> None everywhere.  Rows and patterns are str; comparisons, starts_with / ends_with / contains look at their UTF-8
bytes, LIKE / length / locate at their code points.
"""
import random
import re

PRED_OPS = ("eq", "ne", "lt", "le", "gt", "ge", "starts_with", "ends_with", "contains", "like")
COMPARISONS = PRED_OPS[:6]
MEASURE_OPS = ("length", "octet_length", "locate")
PATTERN_MAX = 1024
MAX_SEGMENTS = 32


def _b(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode("utf-8")


def compare(op, a, b):
    """One of the six comparisons in unsigned byte order (Python's bytes order: a proper prefix sorts first)."""
    if a is None or b is None:
        return None
    x, y = _b(a), _b(b)
    return {"eq": x == y, "ne": x != y, "lt": x < y, "le": x <= y, "gt": x > y, "ge": x >= y}[op]


class BadPattern(ValueError):
    pass


def check_escape(escape):
    if escape is None:
        return
    if not isinstance(escape, str) or len(escape) != 1 or not (1 <= ord(escape) <= 127) or escape in "%_":
        raise BadPattern(f"bad escape {escape!r}")


def like_tokens(pattern, escape=None):
    """[('lit', ch) | ('one',) | ('any',)] of a LIKE pattern; the escape followed by any character is that character."""
    check_escape(escape)
    toks, i = [], 0
    while i < len(pattern):
        ch = pattern[i]
        if escape is not None and ch == escape:
            if i + 1 >= len(pattern):
                raise BadPattern("the pattern ends in a lone escape")
            toks.append(("lit", pattern[i + 1]))
            i += 2
            continue
        toks.append(("any",) if ch == "%" else ("one",) if ch == "_" else ("lit", ch))
        i += 1
    return toks


def like_segments(pattern, escape=None):
    """The non-empty runs between the unescaped '%' (the library takes at most MAX_SEGMENTS)."""
    n, run = 0, False
    for t in like_tokens(pattern, escape):
        if t[0] == "any":
            run = False
        elif not run:
            run, n = True, n + 1
    return n


def like_regex(pattern, escape=None):
    out = []
    for t in like_tokens(pattern, escape):
        out.append(".*" if t[0] == "any" else "." if t[0] == "one" else re.escape(t[1]))
    return re.compile("".join(out), re.S)


def like(s, pattern, escape=None):
    """SQL LIKE over code points: '%' any run, '_' exactly one, the whole row must match."""
    rx = pattern if isinstance(pattern, re.Pattern) else like_regex(pattern, escape)
    return None if s is None else rx.fullmatch(s) is not None


def like_table(s, pattern, escape=None):
    """The same by a table over (tokens, code points): no backtracking, for patterns of many '%' that a regex engine
    takes exponential time to refuse."""
    if s is None:
        return None
    toks = like_tokens(pattern, escape)
    reach = [True] + [False] * len(s)          # reach[j]: the tokens so far can match s[:j]
    for t in toks:
        if t[0] == "any":
            seen = False
            for j in range(len(s) + 1):
                seen = seen or reach[j]
                reach[j] = seen
        else:
            reach = [False] + [reach[j] and (t[0] == "one" or s[j] == t[1]) for j in range(len(s))]
    return reach[len(s)]


def predicate(op, s, pattern, escape=None):
    check_escape(escape)
    if op in COMPARISONS:
        return compare(op, s, pattern)
    if op == "like":
        return like(s, pattern, escape)
    if s is None:
        return None
    x, p = _b(s), _b(pattern)
    return {"starts_with": x.startswith(p), "ends_with": x.endswith(p), "contains": p in x}[op]


def length(s):
    return None if s is None else len(s)


def octet_length(s):
    return None if s is None else len(_b(s))


def locate(sub, s, pos=1):
    """The 1-based code-point position of the first `sub` at or after position pos; 0: none, or pos < 1."""
    if s is None:
        return None
    return s.find(sub, pos - 1) + 1 if pos >= 1 else 0


def measure(what, s, pattern="", pos=1):
    return length(s) if what == "length" else octet_length(s) if what == "octet_length" else locate(pattern, s, pos)


# ---------------------------------------------------------------- the lists the tests share
COMPARE_ROWS = ["", "a", "a\0", "a\0b", "b", "é", "z", "zz"]
LIKE_ROWS = ["", "a", "ab", "abab", "aab", "aaab", "a%b", "a_b", "a\\b", "é", "😀b", "aé😀"]
LIKE_PATTERNS = ["", "%", "%%", "_", "__", "a%", "%a", "%a%", "a%b", "a_b", "%a_b%", "_%", "%_", "a%b%c", "%ab%ab", "a%a", "%aab",
                 "\\%", "a\\%b", "a\\_b", "\\\\"]     # with escape '\\'
LIKE_HASH = [("a#%b", "#")]
ALPHABET = ["a", "b", "é", "😀", "%", "_", "\\"]


def random_like_pairs(n, seed=1):
    """(pattern, escape, row) over ALPHABET: patterns of 0-7 items, escaped ones among them (escape '\\' or none)."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        escape = "\\" if rng.random() < 0.7 else None
        items = []
        for _ in range(rng.randrange(8)):
            ch = rng.choice(ALPHABET)
            if escape is not None and ch == escape:
                ch = escape + rng.choice(ALPHABET)     # an escaped character; never a lone escape
            elif escape is not None and rng.random() < 0.1:
                ch = escape + ch
            items.append(ch)
        row = "".join(rng.choice(ALPHABET[:4] if rng.random() < 0.8 else ALPHABET) for _ in range(rng.randrange(9)))
        out.append(("".join(items), escape, row))
    return out


def write_host_table(path, npairs=100_000):
    """The table tests/cpp/test_utf8_pattern_host.cpp reads: one case a line, `kind op escape pos pattern row expected` with
    pattern and row as hex ('-' = empty); expected is 0 / 1 / an integer, or E where the pattern must not compile."""
    def hx(b):
        return _b(b).hex() or "-"

    lines = []

    def pred(op, pat, esc, row, model=predicate):
        try:
            exp = str(int(model(op, row, pat, esc)))
            if op == "like" and like_segments(pat, esc) > MAX_SEGMENTS:
                exp = "E"
        except BadPattern:
            exp = "E"
        if len(_b(pat)) > PATTERN_MAX:
            exp = "E"
        e = -1 if esc is None else (ord(esc) if isinstance(esc, str) and len(esc) == 1 else esc)
        lines.append(f"pred {op} {e} 0 {hx(pat)} {hx(row)} {exp}")

    for pat, esc, row in random_like_pairs(npairs):
        pred("like", pat, esc, row)
    for pat in LIKE_PATTERNS:
        for row in LIKE_ROWS:
            pred("like", pat, "\\", row)
    for pat, esc in LIKE_HASH:
        for row in LIKE_ROWS:
            pred("like", pat, esc, row)
    for row in ("é", "😀", "", "éé"):
        pred("like", "_", None, row)
    for op in PRED_OPS[:9]:
        for lit in COMPARE_ROWS + ["ab", "abcdefgh", "abcdefghi"]:
            for row in COMPARE_ROWS + LIKE_ROWS + ["abcdefgh", "abcdefghij", "xabcdefghi"]:
                pred(op, lit, None, row)
    # 32 and 33 segments; 1024 and 1025 bytes; the bad escapes
    for nseg in (32, 33):
        pat = "%".join("a" * nseg)
        for row in ("a" * nseg, "a" * (nseg - 1), "ba" * nseg):
            pred("like", pat, None, row, lambda op, s, p, e: like_table(s, p, e))
            pred("like", "%" + pat + "%", None, row, lambda op, s, p, e: like_table(s, p, e))
    for nbytes in (1024, 1025):
        for row in ("a" * nbytes, "a" * 1024 + "b", "a" * 1023):
            pred("like", "a" * nbytes, None, row)
            pred("like", "%" + "a" * (nbytes - 2) + "_", None, row)
            pred("eq", "a" * nbytes, None, row)
    for esc in ("%", "_", 0, 128, 200, -2):
        lines.append(f"pred like {ord(esc) if isinstance(esc, str) else esc} 0 {hx('a')} {hx('a')} E")
    pred("like", "a\\", "\\", "a")
    pred("like", "\\", "\\", "")
    pred("like", "a#", "#", "a#")
    # column against column, counts, locate
    rows = COMPARE_ROWS + LIKE_ROWS + ["abcdefgh" * 3, "abcdefgh" * 3 + "é", "abcdefgh" * 2 + "abcdefgz"]
    for a in rows:
        for b in rows:
            x, y = _b(a), _b(b)
            lines.append(f"cmp - -1 0 {hx(b)} {hx(a)} {(x > y) - (x < y)}")
    for row in rows + ["aé😀" * 7, "😀" * 9]:
        lines.append(f"length - -1 0 - {hx(row)} {len(row)}")
        for sub in ("", "a", "b", "ab", "é", "😀b", "é😀a"):
            for pos in (-1, 0, 1, 2, 3, len(row), len(row) + 1, len(row) + 2):
                lines.append(f"locate - -1 {pos} {hx(sub)} {hx(row)} {locate(sub, row, pos)}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)
