"""The executable model of rdf_utf8_replace / _translate / _initcap / _split: pure Python, a row at a time.
The reference declares initcap, translate and split with empty bodies (src/functions/scalar.rs) and has no replace, so Spark 3's
semantics are defined HERE, from Spark's documentation and UTF8String's source as published.  Spark itself was NOT run:
tests/test_utf8_rewrite_ref.py holds this file to what this machine has — pyarrow.compute.replace_substring and
split_pattern, Python's str.translate / str.lower / str.title — and to a hand-written table of Spark's documented examples.

None -> None everywhere.  Rows are str or bytes; a result has the type of its row (split: a list of them).  Everything is
computed on UTF-8 bytes and nothing is validated.

  hits    replace and split find the occurrences of a literal byte-wise from the left; each search resumes at the END of
          the previous hit ('aaaaa', 'aa' -> hits at 0 and 2).
  units   translate and initcap work on units: a unit begins at every byte that is not a continuation byte (10xxxxxx) and
          runs over the continuation bytes that follow; continuation bytes at the start of a row stand alone.  A unit is
          well-formed when its length is what its first byte announces (0xxxxxxx 1, 110xxxxx 2, 1110xxxx 3, 1111xxxx 4).  A
          unit that is not well-formed — a stray continuation byte, a lead byte with too few or too many continuation bytes
          — never matches, is never mapped, and is copied.  On valid UTF-8 the units are the code points.

replace(row, search, replacement): every hit replaced; an empty search gives the row unchanged (UTF8String.replace).
translate(row, matching, replace): unit i of matching maps to unit i of replace, to nothing when replace has fewer units; the
    first position of a unit in matching decides; units of replace beyond matching's count are ignored.  A unit of matching
    that is not well-formed keeps its position and matches nothing; a replacement unit longer than 4 bytes (never
    well-formed) leaves its key mapped to itself.
initcap(row) = title_words(lower(row)): lower is rdf_utf8_lower's mapping (str.lower's: one-to-many mappings and Final_Sigma,
    both decided on the original row); a word begins at the first unit of the row and after every byte 0x20 — no other white
    space starts a word (UTF8String.toTitleCase); the first code point of a word is replaced by its SIMPLE title mapping
    (t = c.title(); t if len(t) == 1 else c).
split(row, delim, limit): delim is a LITERAL (Spark takes a regular expression; a delimiter without metacharacters means the
    same in both).  limit > 0: at most limit elements, the last one holds the rest; limit <= 0: every hit splits.  Trailing
    empty strings are kept ('a,b,,c,' -> ['a','b','','c','']); the empty row gives ['']; an empty delim is refused.
"""
import functools
import random

PATTERN_MAX = 1024
CLAMP = 1 << 31


def _b(s):
    return bytes(s) if isinstance(s, (bytes, bytearray)) else s.encode("utf-8")


def _like(row, b):
    return b if isinstance(row, (bytes, bytearray)) else b.decode("utf-8")


def lead_len(c):
    return 1 if c < 0x80 else 0 if c < 0xC0 else 2 if c < 0xE0 else 3 if c < 0xF0 else 4


def units(b):
    """[(start, end, well_formed)] of a byte string"""
    out = []
    i, n = 0, len(b)
    while i < n:
        j = i + 1
        while j < n and (b[j] & 0xC0) == 0x80:
            j += 1
        out.append((i, j, lead_len(b[i]) == j - i))
        i = j
    return out


def hits(b, d, maxhits=None):
    """starts of the non-overlapping occurrences of d in b, from the left"""
    out = []
    if not d:
        return out
    pos = 0
    while maxhits is None or len(out) < maxhits:
        h = b.find(d, pos)
        if h < 0:
            break
        out.append(h)
        pos = h + len(d)
    return out


def replace(s, search, replacement):
    if s is None:
        return None
    b, d, r = _b(s), _b(search), _b(replacement)
    out, pos = bytearray(), 0
    for h in hits(b, d):
        out += b[pos:h] + r
        pos = h + len(d)
    out += b[pos:]
    return _like(s, bytes(out))


def translate_table(matching, rep):
    """{key unit: replacement bytes}"""
    m, r = _b(matching), _b(rep)
    mu, ru = units(m), units(r)
    table = {}
    for i, (s, e, wf) in enumerate(mu):
        if not wf:
            continue
        key = m[s:e]
        val = b""
        if i < len(ru):
            val = r[ru[i][0]:ru[i][1]]
            if len(val) > 4:
                val = key
        table.setdefault(key, val)
    return table


def translate(s, matching, rep, table=None):
    if s is None:
        return None
    b = _b(s)
    if table is None:
        table = translate_table(matching, rep)
    out = bytearray()
    for st, en, wf in units(b):
        u = b[st:en]
        out += table.get(u, u) if wf else u
    return _like(s, bytes(out))


def _decode(u):
    if len(u) == 1:
        return u[0]
    cp = u[0] & (0x07 if len(u) == 4 else 0x0F if len(u) == 3 else 0x1F)
    for c in u[1:]:
        cp = (cp << 6) | (c & 0x3F)
    return cp


def _encode(cp):
    if cp < 0x80:
        return bytes([cp])
    if cp < 0x800:
        return bytes([0xC0 | (cp >> 6), 0x80 | (cp & 0x3F)])
    if cp < 0x10000:
        return bytes([0xE0 | (cp >> 12), 0x80 | ((cp >> 6) & 0x3F), 0x80 | (cp & 0x3F)])
    return bytes([0xF0 | ((cp >> 18) & 7), 0x80 | ((cp >> 12) & 0x3F), 0x80 | ((cp >> 6) & 0x3F), 0x80 | (cp & 0x3F)])


def _scalar(cp):
    return cp < 0x110000 and not 0xD800 <= cp <= 0xDFFF


@functools.lru_cache(maxsize=None)
def _lower_cp(cp):
    return tuple(ord(x) for x in chr(cp).lower()) if _scalar(cp) else (cp,)


@functools.lru_cache(maxsize=None)
def title_simple(cp):
    if not _scalar(cp):
        return cp
    t = chr(cp).title()
    return ord(t) if len(t) == 1 else cp


@functools.lru_cache(maxsize=None)
def _cased(cp):
    """Cased and not Case_Ignorable, probed off this interpreter's Final_Sigma rule (tools/gen_unicode_case.py's way)"""
    return _scalar(cp) and (chr(cp) + "Σ").lower()[-1] == "ς"


@functools.lru_cache(maxsize=None)
def _ignorable(cp):
    return _scalar(cp) and not _cased(cp) and ("A" + chr(cp) + "Σ").lower()[-1] == "ς"


def _final_sigma(b, us, i):
    before = False
    for s, e, wf in reversed(us[:i]):
        if not wf:
            break
        c = _decode(b[s:e])
        if _ignorable(c):
            continue
        before = _cased(c)
        break
    if not before:
        return False
    for s, e, wf in us[i + 1:]:
        if not wf:
            return True
        c = _decode(b[s:e])
        if _ignorable(c):
            continue
        return not _cased(c)
    return True


def initcap(s):
    if s is None:
        return None
    b = _b(s)
    us = units(b)
    out = bytearray()
    for i, (st, en, wf) in enumerate(us):
        u = b[st:en]
        if not wf:
            out += u
            continue
        cp = _decode(u)
        word = st == 0 or b[st - 1] == 0x20
        if cp == 0x3A3:
            m = [0x3C2 if _final_sigma(b, us, i) else 0x3C3]
        else:
            m = list(_lower_cp(cp))
        if word:
            m[0] = title_simple(m[0])
        out += u if m == [cp] else b"".join(_encode(x) for x in m)
    return _like(s, bytes(out))


def split(s, delim, limit=-1):
    if s is None:
        return None
    b, d = _b(s), _b(delim)
    if not d:
        raise ValueError("split: an empty delimiter")
    out, pos = [], 0
    for h in hits(b, d, limit - 1 if limit > 0 else None):
        out.append(b[pos:h])
        pos = h + len(d)
    out.append(b[pos:])
    return [_like(s, x) for x in out]


# ---- sizes, as the header states them
def replace_bytes(n, k, m, r):
    return max(0, min(CLAMP, n + k * (r - m)))


# ---- random rows
ALPHABET = ["a", "b", "A", "Z", " ", ",", "-", "é", "ß", "Σ", "σ", "ǆ", "Ǆ", "İ", "ა", "中", "€", "ﬁ", "\U0001F600", "\U00010400", "\t", "."]
BROKEN = [0x61, 0x20, 0x2C, 0x80, 0xBF, 0xC3, 0xA9, 0xE2, 0x82, 0xAC, 0xF0, 0x9F, 0x98, 0x80, 0xFF, 0xCE, 0xA3]


def random_row(rng, max_cp=24, broken=0.1):
    if rng.random() < broken:
        return bytes(rng.choice(BROKEN) for _ in range(rng.randrange(0, max_cp + 1)))
    return "".join(rng.choice(ALPHABET) for _ in range(rng.randrange(0, max_cp + 1))).encode("utf-8")


def _hex(b):
    return b.hex() if b else "-"


def write_host_table(path, rows_per_op=100_000, seed=23):
    """The case table of tests/cpp/test_utf8_rewrite_host.cpp, one case a line (byte strings as hex, '-' = empty):
        replace <search> <replacement> <row> <expected>      translate <matching> <replace> <row> <expected>
        initcap <row> <expected>                             split <limit> <delim> <row> <expected bytes> <offset,offset,...>
    Returns the number of cases."""
    rng = random.Random(seed)
    needles = [b",", b" ", b"aa", b"ab", b"aba", b"abab", b", ", "é".encode(), "中".encode(), b"a", b"\x80", b"-,-"]
    n = 0

    def long_row():
        return random_row(rng, max_cp=rng.choice([300, 700, 2000]), broken=0.2)

    def needle_for(row):
        k = rng.random()
        if k < 0.6 or len(row) < 2:
            return rng.choice(needles)
        if k < 0.7 and len(row) > 200:   # longer than a wave's window, taken from the row so that it occurs
            m = rng.randrange(65, 120)
            at = rng.randrange(0, len(row) - m)
            return row[at:at + m]
        m = rng.randrange(1, min(6, len(row)))
        at = rng.randrange(0, len(row) - m + 1)
        return row[at:at + m]

    with open(path, "w") as f:
        for i in range(rows_per_op):
            row = long_row() if i % 500 == 0 else random_row(rng)
            if i % 97 == 0:
                row = b"a" * rng.randrange(0, 12) if i % 2 else b"ab" * rng.randrange(0, 200) + b"a"
            d = needle_for(row)
            r = rng.choice([b"", b"b", b"aa", d, d + d, "é".encode(), b"0123456789" * 3])
            f.write(f"replace {_hex(d)} {_hex(r)} {_hex(row)} {_hex(replace(row, d, r))}\n")
            limit = rng.choice([-1, 0, 1, 2, 3, 5])
            parts = split(row, d, limit)
            offs, at = [0], 0
            for p in parts:
                at += len(p)
                offs.append(at)
            f.write(f"split {limit} {_hex(d)} {_hex(row)} {_hex(b''.join(parts))} {','.join(str(o) for o in offs)}\n")
            n += 2
        tables = []
        for _ in range(40):
            m = random_row(rng, max_cp=rng.choice([0, 1, 4, 12]), broken=0.15)
            r = random_row(rng, max_cp=rng.choice([0, 1, 4, 16]), broken=0.15)
            tables.append((m, r, translate_table(m, r)))
        tables.append(("abé€\U0001F600a".encode(), "x中".encode(), None))
        for i in range(rows_per_op):
            row = long_row() if i % 500 == 0 else random_row(rng)
            m, r, t = tables[i % len(tables)]
            f.write(f"translate {_hex(m)} {_hex(r)} {_hex(row)} {_hex(translate(row, m, r, t))}\n")
            f.write(f"initcap {_hex(row)} {_hex(initcap(row))}\n")
            n += 2
    return n
