"""tests/textfloat_ref.py, the executable model of rdf_utf8_parse_float / rdf_utf8_format_float, held to what this machine knows
without running the reference: float() (correctly rounded) for Float64 parsing, repr() / numpy.format_float_scientific(unique=True)
for the digits wherever the shortest length is at least 2, exact Fraction rounding for Float32, the known answers of the JDK's
specification, and parse(format(x)) having the bits of x.  No GPU, no library."""
import re
import struct
from fractions import Fraction

import numpy as np
import pytest

import textfloat_ref as R


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def bits_f64(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def bits_f32(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


def fraction_round_f32(fr):
    """the Float32 nearest to a positive Fraction, ties to even, by exact arithmetic on the candidates -> bits"""
    if fr == 0:
        return 0
    e = 0
    while Fraction(2) ** (e + 1) <= fr:
        e += 1
    while Fraction(2) ** e > fr:
        e -= 1
    if e > 127:
        return 0x7F800000
    ulp = Fraction(2) ** (max(e, -126) - 23)
    q = fr / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    if n * ulp >= Fraction(2) ** 128:
        return 0x7F800000
    return f32_bits(float(n * ulp))        # n * ulp is a Float32 exactly, so a Float64 exactly too


DIFFERS_FROM_PYTHON = {b"\x1c3.14\x1f", b"1_0", b"+nan", b"-nan", "\xa01".encode(), "١".encode(), "１".encode()}


def test_branch_cases_against_float():
    """every grammar arm and refusal; where the grammar knowingly differs from Python's the model's answer is pinned here"""
    for t in R.branch_cases():
        m = R.parse(t, False)
        if t in DIFFERS_FROM_PYTHON:
            continue
        try:
            py = float(t.decode("utf-8"))
        except (ValueError, UnicodeDecodeError):
            py = None
        assert (m is None) == (py is None), t
        if m is not None:
            assert m == (R.FMT[False].nan if py != py else f64_bits(py)), t
    assert R.parse(b"\x1c3.14\x1f", False) == f64_bits(3.14)      # the CAST grammars' trim set
    for t in (b"1_0", b"+nan", b"-nan", b".", b"e5", b"1e", b"1e+", b"0x10", b"1d", b"1f", b"", b" "):
        assert R.parse(t, False) is None and R.parse(t, True) is None, t
    for t in (b"5.", b".5", b"1e5", b"nan", b"NaN", b"inf", b"-Infinity", b"+INF"):
        assert R.parse(t, False) is not None and R.parse(t, True) is not None, t
    assert R.parse(b"-0", False) == R.parse(b"-0.0", False) == R.parse(b"-1e-999", False) == 1 << 63
    assert R.parse(b"-0", True) == R.parse(b"-1e-999", True) == 1 << 31
    assert R.parse(b"nan", False) == 0x7FF8000000000000 and R.parse(b"NAN", True) == 0x7FC00000
    assert R.parse(b"1e999", False) == 0x7FF0000000000000 and R.parse(b"-1e39", True) == 0xFF800000


@pytest.mark.parametrize("family", R.FAMILIES)
def test_float64_parse_is_float(family):
    for t in R.random_cases(family, 4000, 7, False):
        assert R.parse(t, False) == f64_bits(float(t.decode())), t


def test_hard_cases_and_long_rows_against_float_and_fractions():
    hc = R.hard_cases()
    texts = {t for t, _, _ in hc}
    two53 = b"9007199254740993"
    assert two53 in texts and two53 + b"." + b"0" * 30 + b"1" in texts
    assert b"2.4703282292062327e-324" in texts and b"2.4703282292062328e-324" in texts
    assert R.parse(two53, False) == f64_bits(9007199254740992.0)
    assert R.parse(two53 + b"." + b"0" * 30 + b"1", False) == f64_bits(9007199254740994.0)
    tie = [t for t in texts if 1070 <= len(t) <= 1090 and t.startswith(b"0.000")]
    assert sorted(R.parse(t, False) for t in tie) == [0, 0, 1]          # the tie and the decimal below it give 0.0, the one above 5e-324
    assert R.parse(b"2.4703282292062327e-324", False) == 0 and R.parse(b"2.4703282292062328e-324", False) == 1
    assert R.parse(b"1.7976931348623157e308", False) == 0x7FEFFFFFFFFFFFFF
    assert R.parse(str((1 << 1024) - (1 << 970)).encode(), False) == 0x7FF0000000000000
    assert R.parse(str((1 << 1024) - (1 << 970) - 1).encode(), False) == 0x7FEFFFFFFFFFFFFF
    assert sum(und for _, _, und in hc) >= 40
    for t, f32, und in hc:
        if f32:
            s = R.scan(t)
            fr = Fraction(s[2]) * Fraction(10) ** s[3]
            assert R.parse(t, True) == fraction_round_f32(fr), t
            # the double-rounding trap: some of these differ from rounding through Float64
        else:
            assert R.parse(t, False) == f64_bits(float(t.decode())), t[:40]
        if und:
            assert len(t) > 19
    # the listed long-digit ties and near-ties are flagged for the exact path
    flagged = {t for t, _, und in hc if und}
    assert two53 + b"." + b"0" * 30 + b"1" in flagged and all(t in flagged for t in tie)
    assert sum(1 for t, f32, und in hc if f32 and und) >= 10
    with np.errstate(over="ignore"):
        trap = sum(1 for t, f32, _ in hc if f32 and R.parse(t, True) != f32_bits(np.float32(float(t.decode()))))
    assert trap >= 1, "no Float32 case here differs from rounding through Float64"
    for t in R.long_rows():
        try:
            py = float(t.decode())
        except ValueError:
            py = None
        m = R.parse(t, False)
        assert (m is None) == (py is None) and (m is None or m == f64_bits(py)), t[:30]
        assert 300 <= len(t)
    assert max(len(t) for t in R.long_rows()) >= 5000


def test_float32_parse_is_the_exact_fraction_rounded_once():
    for fam in R.FAMILIES:
        for t in R.random_cases(fam, 700, 13, True):
            s = R.scan(t)
            if s is None or s[0] != "num":
                want = R.parse(t, True)
            else:
                want = fraction_round_f32(Fraction(s[2]) * Fraction(10) ** s[3]) | (0x80000000 if s[1] else 0)
            assert R.parse(t, True) == want, t


def digits_of(text):
    """the significant digits and the scientific exponent of a printed number"""
    t = text.lstrip("-")
    mant, _, ex = t.replace("E", "e").partition("e")
    ip, _, fp = mant.partition(".")
    digits = (ip + fp).lstrip("0")
    lead_zeros = len(ip + fp) - len(digits)
    e = (int(ex) if ex else 0) + len(ip) - 1 - lead_zeros
    return digits.rstrip("0") or "0", e


def test_format_digits_are_repr_and_numpy():
    for b in R.random_bits(6000, 3, False) + R.edge_values(False):
        F = R.FMT[False]
        mag = b & (F.sign - 1)
        if mag >= F.inf or mag == 0:
            continue
        x = bits_f64(b)
        ours = digits_of(R.fmt(b, False).decode())
        theirs = digits_of(repr(x))
        if len(theirs[0]) >= 2:
            assert ours == theirs, (hex(b), R.fmt(b, False), repr(x))
            assert ours == digits_of(np.format_float_scientific(np.float64(x), unique=True)), hex(b)
        else:
            assert ours[1] == theirs[1] or len(ours[0]) == 2, hex(b)
            assert len(ours[0]) <= 2
    for b in R.random_bits(6000, 4, True) + R.edge_values(True):
        F = R.FMT[True]
        mag = b & (F.sign - 1)
        if mag >= F.inf or mag == 0:
            continue
        theirs = digits_of(np.format_float_scientific(np.float32(bits_f32(b)), unique=True))
        if len(theirs[0]) >= 2:
            assert digits_of(R.fmt(b, True).decode()) == theirs, hex(b)


def test_known_answers_and_the_layout():
    known = [(1.0, "1.0"), (123.456, "123.456"), (0.001, "0.001"), (9999999.999999998, "9999999.999999998"), (1e7, "1.0E7"), (1e23, "1.0E23"),
             (5.684341886080802e-14, "5.684341886080802E-14"), (1.7976931348623157e308, "1.7976931348623157E308"), (5e-324, "4.9E-324"),
             (1e-323, "9.9E-324"), (-0.0, "-0.0"), (0.0, "0.0"), (float("inf"), "Infinity"), (float("-inf"), "-Infinity"), (100.0, "100.0"),
             (1234567.0, "1234567.0"), (12345678.0, "1.2345678E7"), (9.999e-4, "9.999E-4"), (0.00123, "0.00123"), (2e-3, "0.002"), (-2.5, "-2.5"),
             (1e21, "1.0E21"), (1e22, "1.0E22"), (2.2250738585072014e-308, "2.2250738585072014E-308"), (4.35, "4.35"), (0.3, "0.3"), (2 ** 53 + 0.0, "9.007199254740992E15")]
    for x, t in known:
        assert R.fmt(f64_bits(x), False) == t.encode(), (x, R.fmt(f64_bits(x), False))
    assert R.fmt(0x7FF8000000000000, False) == R.fmt(0xFFF0000000000001, False) == R.fmt(0x7FC00001, True) == b"NaN"
    known32 = [(1, "1.4E-45"), (2, "2.8E-45"), (7, "9.8E-45"), (71, "9.9E-44"), (f32_bits(1.0), "1.0"), (f32_bits(0.1), "0.1"), (f32_bits(3.4028235e38), "3.4028235E38"),
               (f32_bits(1e7), "1.0E7"), (f32_bits(16777216.0), "1.6777216E7"), (f32_bits(0.001), "0.001"), (f32_bits(1.17549435e-38), "1.1754944E-38"), (0x80000000, "-0.0")]
    for b, t in known32:
        assert R.fmt(b, True) == t.encode(), (hex(b), R.fmt(b, True))
    assert max(len(R.fmt(b, False)) for b in R.edge_values(False) + R.random_bits(3000, 8, False)) == 24 == R.MAX_ROW[False]
    assert max(len(R.fmt(b, True)) for b in R.edge_values(True) + R.random_bits(3000, 8, True)) == 15 == R.MAX_ROW[True]
    for b in R.random_bits(2000, 9, False):
        t = R.fmt(b, False).decode()
        if "N" in t or "I" in t:
            continue
        x = abs(bits_f64(b))
        assert ("E" in t) == (not (1e-3 <= x < 1e7) and x != 0), t
        assert re.fullmatch(r"-?(\d+\.\d+|\d\.\d+E-?\d+)", t), t


@pytest.mark.parametrize("f32", [False, True])
def test_round_trip_of_random_bit_patterns(f32):
    F = R.FMT[f32]
    for b in R.random_bits(8000, 21, f32) + R.edge_values(f32) + R.hard_values(f32):
        want = F.nan if (b & (F.sign - 1)) > F.inf else b
        assert R.parse(R.fmt(b, f32), f32) == want, hex(b)


def test_the_interval_test_is_the_round_back_test():
    """the model finds the digits by an interval of midpoints; a decimal lies in it exactly when it parses back to the value"""
    for f32 in (False, True):
        for b in R.random_bits(300, 33, f32) + [1, 2, 3, R.FMT[f32].inf - 1, 1 << (R.FMT[f32].mant - 1)]:
            F = R.FMT[f32]
            mag = b & (F.sign - 1)
            if mag >= F.inf or mag == 0:
                continue
            d, p = R.shortest(mag, f32)
            for dd in (d - 1, d, d + 1, d * 10 - 1, d * 10 + 1, d * 10 + 5, d * 10 - 5):
                if dd <= 0:
                    continue
                pp = p if dd < d * 5 else p - 1
                iv = R._interval(mag, f32)
                inside = R._rounds_back(dd * 10 ** pp, 1, iv) if pp >= 0 else R._rounds_back(dd, 10 ** -pp, iv)
                assert inside == (R.parse(f"{dd}e{pp}".encode(), f32) == mag), (hex(b), dd, pp)
