"""The model of tests/utf8_build_ref.py against pyarrow.compute where pyarrow means the same thing, and against the table of
Spark's examples and the contract's edge cases.  No GPU: these tests define what the kernels are held to."""
import random

import pytest

import utf8_build_ref as R


def test_the_table_of_spark_examples_and_edges():
    for fn, args, exp in R.SPARK_TABLE:
        assert fn(*args) == exp, (fn.__name__, args, fn(*args), exp)


def test_bytes_in_bytes_out_and_str_in_str_out():
    assert R.reverse("aé") == "éa" and R.reverse("aé".encode()) == "éa".encode()
    assert R.lpad(b"x", 3, b"ab") == b"abx" and R.substring_index(b"a.b", b".", 1) == b"a"
    assert R.repeat(b"ab", 2) == b"abab" and R.concat([b"a", b"b"]) == b"ab" and R.concat_ws(b"-", [b"a", None, b""]) == b"a-"


def test_overlapping_delimiters_follow_spark_and_differ_from_split():
    # str.split finds non-overlapping occurrences: 'aaaa'.split('aa') has 2 of them, Spark's search finds 3
    assert [R.substring_index("aaaa", "aa", k) for k in (1, 2, 3, 4)] == ["", "a", "aa", "aaaa"]
    assert [R.substring_index("aaaa", "aa", -k) for k in (1, 2, 3, 4)] == ["", "a", "aa", "aaaa"]
    assert R.substring_index("abababa", "aba", 2) == "ab" and R.substring_index("abababa", "aba", -2) == "ba"
    # without overlaps it is split / join
    rng = random.Random(3)
    for _ in range(2000):
        row = ".".join(R.rand_text(rng, 4, "abé中") for _ in range(rng.randrange(1, 6)))
        for k in (1, 2, 3, 9):
            assert R.substring_index(row, ".", k) == ".".join(row.split(".")[:k])
            assert R.substring_index(row, ".", -k) == ".".join(row.split(".")[-k:])


def test_pads_that_end_between_code_points_of_different_widths():
    pad = "aé中😀"
    for n in range(0, 14):
        for row in ("", "x", "中y"):
            got = R.lpad(row, n, pad)
            assert len(got) == (n if n > len(row) else min(n, len(row)))
            if n > len(row):
                assert got == (pad * 4)[:n - len(row)] + row and R.rpad(row, n, pad) == row + (pad * 4)[:n - len(row)]
            else:
                assert got == row[:n] == R.rpad(row, n, pad)


def rows(n, seed, null_frac=0.1):
    rng = random.Random(seed)
    return [None if rng.random() < null_frac else R.rand_text(rng, 12) for _ in range(n)]


def test_against_pyarrow_where_it_means_the_same():
    pa = pytest.importorskip("pyarrow")
    pc = pytest.importorskip("pyarrow.compute")
    a, b, c = rows(3000, 1), rows(3000, 2), rows(3000, 3, 0.3)
    for sep in ("", ", ", "中"):
        emit = pc.binary_join_element_wise(pa.array(a, pa.string()), pa.array(b, pa.string()), pa.array(c, pa.string()), pa.scalar(sep), null_handling="emit_null").to_pylist()
        # (a row without one non-NULL part is the empty string in Spark; pyarrow 25 drops such a row from its result, so the
        # comparison gives every row at least one part)
        c1 = ["" if x is None and y is None and z is None else z for x, y, z in zip(a, b, c)]
        assert 0 < sum(x != y for x, y in zip(c, c1)) < 100
        skip = pc.binary_join_element_wise(pa.array(a, pa.string()), pa.array(b, pa.string()), pa.array(c1, pa.string()), pa.scalar(sep), null_handling="skip").to_pylist()
        assert skip == [R.concat_ws(sep, list(p)) for p in zip(a, b, c1)]
        if sep == "":
            assert emit == [R.concat(list(p)) for p in zip(a, b, c)]
        else:      # concat with the separator as literal parts
            assert emit == [R.concat([x, sep, y, sep, z]) if None not in (x, y, z) else None for x, y, z in zip(a, b, c)]
    arr = pa.array(a, pa.string())
    for times in (0, 1, 3):
        assert pc.binary_repeat(arr, times).to_pylist() == [R.repeat(s, times) for s in a]
    assert pc.utf8_reverse(arr).to_pylist() == [R.reverse(s) for s in a]
    # pyarrow neither truncates nor cycles a longer pad: one-code-point pads and len >= the row's length only
    for pad in (" ", "é", "😀"):
        for n in (12, 13, 40):
            assert pc.utf8_lpad(arr, n, pad).to_pylist() == [R.lpad(s, n, pad) for s in a]
            assert pc.utf8_rpad(arr, n, pad).to_pylist() == [R.rpad(s, n, pad) for s in a]


def test_the_host_table_is_written_and_counts_its_rows(tmp_path):
    n = R.write_host_table(str(tmp_path / "t.txt"), nrows=200)
    lines = (tmp_path / "t.txt").read_text().splitlines()
    assert n == len(lines) and {ln.split()[0] for ln in lines} == {"pad", "repeat", "reverse", "subidx", "concat"}
