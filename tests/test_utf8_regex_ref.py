"""tests/utf8_regex_ref.py held to Python's `re` (re.ASCII) wherever Java and Python agree, and to hand-written tables where
they do not.  Python's finditer differs from Matcher.find in ONE way that matters here: after an empty match at p it searches
again AT p for a non-empty match, where Java moves on to p + 1.  So the model's spans are held to Matcher.find's loop run over
re.search, for every generated pair; and to re.finditer, re.sub and re.split on every pair where finditer agrees with that
loop (nearly all of them).  No generated pattern may be refused by either side."""
import random
import re

import pytest

import utf8_regex_ref as R


def _byte_offsets(row):
    offs = [0]
    for ch in row:
        offs.append(offs[-1] + len(ch.encode()))
    return offs


def _java_find_all(rx, row):
    out, at = [], 0
    while at <= len(row):
        m = rx.search(row, at)
        if m is None:
            break
        out.append((m.start(), m.end()))
        at = m.end() if m.end() > m.start() else m.end() + 1
    return out


def test_generated_patterns_against_python_re():
    rng = random.Random(7)
    pairs = agreed = splits = 0
    for _ in range(1500):
        ours, py, _ = R.gen_pattern(rng)
        rx = re.compile(py, re.ASCII)          # a pattern Python cannot take means the generator is wrong
        rs = re.compile(re.sub(r"\((?!\?)", "(?:", py), re.ASCII)   # (re.split would return the groups too)
        model = R.compiled(ours)
        for _ in range(8):
            row = R.gen_row(rng)
            offs = _byte_offsets(row)
            want = _java_find_all(rx, row)
            got = R.spans(row, ours)
            assert got == [(offs[s], offs[e]) for s, e in want], (ours, row)
            assert R.count(row, ours) == len(want)
            assert R.rlike(row, ours) == bool(want)
            pairs += 1
            if want == [m.span() for m in rx.finditer(row)]:
                agreed += 1
                assert R.replace(row, ours, "<é>") == rx.sub(lambda m: "<é>", row), (ours, row)
                if not model.can_match_empty:
                    splits += 1
                    assert R.split(row, ours, -1) == rs.split(row), (ours, row)
                    assert R.split(row, ours, 3) == rs.split(row, maxsplit=2), (ours, row)
    assert pairs == 12000 and agreed > 0.9 * pairs and splits > 2000, (pairs, agreed, splits)


@pytest.mark.parametrize("pattern,row,spans", R.HAND_SPANS)
def test_hand_written_spans(pattern, row, spans):
    assert R.spans(row, pattern) == spans


@pytest.mark.parametrize("pattern,limit,row,expected", R.HAND_SPLIT)
def test_javadoc_split_examples(pattern, limit, row, expected):
    assert R.split(row, pattern, limit) == expected


@pytest.mark.parametrize("pattern,what,pos", R.HAND_REFUSED)
def test_refused_constructs_and_their_positions(pattern, what, pos):
    with pytest.raises(R.Refused) as e:
        R.parse(pattern)
    assert (e.value.what, e.value.pos) == (what, pos)


def test_the_operations():
    assert R.replace("baaac", "a*", "-") == "-b--c-"          # Java and Python; RE2 gives -b-c-
    assert R.replace("aaa", "^a", "x") == "xaa"
    assert R.replace("a1b22", "[^0-9]", "") == "122"
    assert R.replace("a  b \t c", "\\s+", " ") == "a b c"
    assert R.replace("ab", "b", "\\$\\\\") == "a$\\"
    assert R.extract("xx123y", "\\d+") == "123" and R.extract("xy", "\\d+") == ""
    assert R.count("abab", "a|ab") == 2 and R.rlike("AB12", "^[A-Z]{2}\\d+")
    assert R.rlike(None, "a") is None and R.split(None, "a") is None and R.replace(None, "a", "") is None
    for rep, what in (("a\\", "a trailing backslash in the replacement"), ("$1", "an unescaped $ in the replacement")):
        with pytest.raises(R.Refused) as e:
            R.replace("a", "a", rep)
        assert e.value.what == what
    with pytest.raises(R.Refused):
        R.extract("a", "a", 1)
    # broken UTF-8 is matched by no element and copied; a match begins at no continuation byte
    assert R.spans(b"a\x80\xffb", ".") == [(0, 1), (3, 4)]
    assert R.spans(b"\x80a", "") == [(1, 1), (2, 2)]
    assert R.replace(b"\xe4\xb8x", "[^a]", "-") == b"\xe4\xb8-"
