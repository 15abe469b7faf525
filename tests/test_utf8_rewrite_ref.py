"""tests/utf8_rewrite_ref.py — the model the GPU tests compare against — held to what this machine has: pyarrow.compute
(replace_substring, split_pattern), Python's str.translate / str.lower / str.title, and Spark's documented examples.  Spark
itself was not run."""
import random
import unicodedata

import pyarrow as pa
import pyarrow.compute as pc
import pytest

import utf8_rewrite_ref as R

NEEDLES = [",", " ", "aa", "ab", "é", "中", ", ", "a", "-,-", "\U0001F600"]


def rows(seed, n=4000):
    rng = random.Random(seed)
    out = [R.random_row(rng, broken=0.0).decode("utf-8") for _ in range(n)]
    out += ["", "a", "aaaaa", "a,b,,c,", ",", ",,", "aa" * 40 + "a"]
    return out


def test_unicode_version_is_the_case_tables():
    assert unicodedata.unidata_version == "13.0.0"


def test_replace_against_pyarrow_and_python():
    xs = rows(1)
    for d in NEEDLES:
        for r in ["", "b", d + d, "é"]:
            got = [R.replace(x, d, r) for x in xs]
            assert got == pc.replace_substring(pa.array(xs), d, r).to_pylist()
            assert got == [x.replace(d, r) for x in xs]
    assert R.replace("aaaaa", "aa", "b") == "bba"
    assert R.replace("abc", "", "x") == "abc"            # UTF8String.replace: an empty search changes nothing
    assert R.replace("ABCabc", "abc", "DEF") == "ABCDEF"  # Spark's example
    assert R.replace("ABCabc", "abc", "") == "ABC"
    assert R.replace(None, "a", "b") is None


def test_split_against_pyarrow():
    xs = rows(2)
    for d in NEEDLES:
        assert [R.split(x, d, -1) for x in xs] == pc.split_pattern(pa.array(xs), d).to_pylist()
        assert [R.split(x, d, 0) for x in xs] == [x.split(d) for x in xs]
        for limit in (1, 2, 5):
            assert [R.split(x, d, limit) for x in xs] == pc.split_pattern(pa.array(xs), d, max_splits=limit - 1).to_pylist()
            assert [R.split(x, d, limit) for x in xs] == [x.split(d, limit - 1) for x in xs]
    assert R.split("a,b,,c,", ",") == ["a", "b", "", "c", ""]
    assert R.split("", ",") == [""]
    assert R.split("oneAtwoBthreeC", "A", -1) == ["one", "twoBthreeC"]
    assert R.split("oneAtwoAthreeA", "A", 2) == ["one", "twoAthreeA"]   # Spark's examples with a literal delimiter
    assert R.split("oneAtwoAthreeA", "A", -1) == ["one", "two", "three", ""]
    assert R.split(None, ",") is None
    with pytest.raises(ValueError):
        R.split("a", "")


def test_translate_against_python():
    xs = rows(3)
    for m, r in [("ab", "xy"), ("aé", "中"), ("\U0001F600 ", ""), ("aba", "123"), ("a", "xyz"), ("", "abc"), ("áé", "ae"), ("abé", "é中\U0001F600")]:
        table = {}
        for i, c in enumerate(m):
            table.setdefault(ord(c), r[i] if i < len(r) else None)
        assert [R.translate(x, m, r) for x in xs] == [x.translate(table) for x in xs], (m, r)
    assert R.translate("AaBbCc", "abc", "123") == "A1B2C3"     # Spark's example
    assert R.translate("translate", "rnlt", "123") == "1a2s3ae"
    assert R.translate(None, "a", "b") is None
    # broken UTF-8: never matched, copied
    assert R.translate(b"\x80a\xc3", b"\x80a", b"xy") == b"\x80y\xc3"   # the stray byte keeps its position in matching
    assert R.translate(b"\xe2\x82\xac\x80\x80", "€".encode(), b"E") == b"\xe2\x82\xac\x80\x80"
    assert R.translate(b"a\x80", b"a", b"x") == b"a\x80"       # the unit is 'a' with its stray byte


def title_words(s):
    out, word = [], True
    for c in s:
        t = c.title()
        out.append(t if word and len(t) == 1 else c)
        word = c == " "
    return "".join(out)


def test_initcap_against_python():
    xs = rows(4) + ["sPark sql", "ǄX  ßa\tb ΑΣ Σ", " a", "İstanbul iİ", "ΟΔΥΣΣΕΥΣ ΣΑΣ", "ǆ ǉ ǌ ǳ", "ſ ა ŉ ﬁ", "áΣ", "Σ", "aΣ.", "a Σ"]
    for x in xs:
        assert R.initcap(x) == title_words(x.lower()), x
    assert R.initcap("sPark sql") == "Spark Sql"                # Spark's example
    assert R.initcap("ǄX  ßa\tb ΑΣ Σ") == "ǅx  ßa\tb Ας Σ"
    assert R.initcap("ǆ") == "ǅ" and R.initcap("ſ") == "S" and R.initcap("ა") == "ა" and R.initcap("ß") == "ß"
    assert R.initcap(None) is None
    assert R.initcap(b"\x80abc \xc3") == b"\x80abc \xc3"        # 'a' follows a stray byte, not a word's start... and is lower already
    assert R.initcap(b"\x80Abc D\x80") == b"\x80abc D\x80"      # 'D' with its stray byte is no well-formed unit


def test_initcap_lowers_back():
    """initcap(s).lower() == s.lower() wherever no title mapping changes under lower (ǅ lowers to ǆ again; 'İ' -> 'i̇' does not round-trip a second time through the dotted I)"""
    for x in rows(5):
        y = R.initcap(x)
        if all(R.title_simple(ord(c)) == ord(c) or chr(R.title_simple(ord(c))).lower() == c for c in x.lower()):
            assert y.lower() == x.lower(), x


def test_title_mapping_counts():
    cps = [c for c in range(0x110000) if not 0xD800 <= c <= 0xDFFF]
    mapped = [c for c in cps if R.title_simple(c) != c]
    upper1 = lambda c: ord(chr(c).upper()) if len(chr(c).upper()) == 1 else c
    assert len(mapped) == 1364
    assert sum(1 for c in cps if R.title_simple(c) != upper1(c)) == 85
    assert sum(1 for c in mapped if len(chr(c).encode()) != len(chr(R.title_simple(c)).encode())) == 31


def test_the_generated_title_header_is_up_to_date():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, os.path.join(root, "tools", "gen_unicode_title.py"), "--check"]).returncode == 0
