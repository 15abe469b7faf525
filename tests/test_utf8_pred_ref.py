"""Holds the model of the Utf8 predicates (tests/utf8_pred_ref.py) to what others compute: pyarrow.compute where pyarrow is
importable, and for LIKE an independent naive recursive matcher over 10^5 random (pattern, row) pairs."""
import functools

import pytest

import utf8_pred_ref as R

ROWS = R.COMPARE_ROWS + R.LIKE_ROWS + ["abc", "xabcx", "éa", "a" * 300, None]


def naive_like(row, pattern, escape):
    """match(i, j): pattern[i:] against row[j:], straight from the definition."""
    @functools.lru_cache(maxsize=None)
    def match(i, j):
        if i == len(pattern):
            return j == len(row)
        ch = pattern[i]
        if escape is not None and ch == escape:
            return j < len(row) and row[j] == pattern[i + 1] and match(i + 2, j + 1)
        if ch == "%":
            return match(i + 1, j) or (j < len(row) and match(i, j + 1))
        if ch == "_":
            return j < len(row) and match(i + 1, j + 1)
        return j < len(row) and row[j] == ch and match(i + 1, j + 1)
    return match(0, 0)


def test_like_against_a_naive_matcher_on_random_pairs():
    pairs = R.random_like_pairs(100_000, seed=2)
    assert len(pairs) >= 100_000
    hits = 0
    cache = {}
    for pat, esc, row in pairs:
        rx = cache.get((pat, esc))
        if rx is None:
            rx = cache[(pat, esc)] = R.like_regex(pat, esc)
        got = R.like(row, rx)
        assert got == naive_like(row, pat, esc), (pat, esc, row)
        hits += got
    assert 5_000 < hits < 95_000          # both answers are exercised


def test_like_table_form_agrees_with_the_regex():
    for pat, esc, row in R.random_like_pairs(20_000, seed=3):
        assert R.like_table(row, pat, esc) == R.like(row, pat, esc), (pat, esc, row)
    assert R.like_table("ab", "%ab%ab") is False and R.like_table("a", "a%a") is False


def test_like_edge_list_and_refusals():
    assert R.like("ab", "%ab%ab") is False and R.like("abab", "%ab%ab") is True
    assert R.like("a", "a%a") is False and R.like("aa", "a%a") is True
    assert R.like("é", "_") and R.like("😀", "_") and not R.like("éé", "_")
    assert R.like("a%b", "a#%b", "#") and not R.like("axb", "a#%b", "#")
    assert R.like("\\", "\\\\", "\\") and R.like("%", "\\%", "\\")
    assert R.like(None, "%") is None
    for pat, esc in (("a\\", "\\"), ("\\", "\\"), ("a", "%"), ("a", "_"), ("a", "\0"), ("a", "é"), ("a", "ab")):
        with pytest.raises(R.BadPattern):
            R.like("a", pat, esc)
    assert R.like_segments("%".join("a" * 33)) == 33 and R.like_segments("%%a%%b_%") == 2


def test_locate_and_lengths():
    assert R.locate("", "abc", 4) == 4 and R.locate("", "abc", 5) == 0 and R.locate("", "", 1) == 1
    assert R.locate("b", "abcb", 1) == 2 and R.locate("b", "abcb", 3) == 4 and R.locate("b", "abcb", 5) == 0
    assert R.locate("b", "abcb", 0) == 0 and R.locate("b", "abcb", -3) == 0
    assert R.locate("😀", "aé😀", 1) == 3 and R.locate("a", None, 1) is None
    assert R.length("aé😀") == 3 and R.octet_length("aé😀") == 7 and R.length(None) is None
    assert R.compare("gt", "é", "z") and R.compare("lt", "a", "a\0") and R.compare("lt", "a\0", "a\0b") and R.compare("eq", None, "a") is None


def test_model_against_pyarrow():
    pa = pytest.importorskip("pyarrow")
    pc = pytest.importorskip("pyarrow.compute")
    arr = pa.array(ROWS, type=pa.string())
    for lit in R.COMPARE_ROWS + ["ab", "a" * 300]:
        for op, fn in (("eq", pc.equal), ("ne", pc.not_equal), ("lt", pc.less), ("le", pc.less_equal), ("gt", pc.greater), ("ge", pc.greater_equal)):
            assert fn(arr, pa.scalar(lit, type=pa.string())).to_pylist() == [R.compare(op, r, lit) for r in ROWS], (op, lit)
        for op, fn in (("starts_with", pc.starts_with), ("ends_with", pc.ends_with), ("contains", pc.match_substring)):
            assert fn(arr, lit).to_pylist() == [R.predicate(op, r, lit) for r in ROWS], (op, lit)
    for pat in R.LIKE_PATTERNS:       # pyarrow's match_like escapes with a backslash
        try:
            R.like_tokens(pat, "\\")
        except R.BadPattern:
            continue
        assert pc.match_like(arr, pat).to_pylist() == [R.like(r, pat, "\\") for r in ROWS], pat
    assert pc.utf8_length(arr).to_pylist() == [R.length(r) for r in ROWS]
    assert pc.binary_length(arr).to_pylist() == [R.octet_length(r) for r in ROWS]
    for sub in ("a", "ab", "é", "😀b"):      # find_substring: 0-based BYTE index of the first occurrence, -1 = none
        exp = []
        for r in ROWS:
            k = R.locate(sub, r, 1)
            exp.append(None if r is None else (-1 if k == 0 else len(r[:k - 1].encode())))
        assert pc.find_substring(arr, sub).to_pylist() == exp, sub
