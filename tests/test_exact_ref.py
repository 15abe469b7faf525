"""The references of the float accuracy tests (tests/exact_ref.py) checked on the host: the long double path against mpmath
at 200 bits, and the ulp distance on binade edges, subnormals, zeros, infinities and NaN.  No GPU needed."""
import math

import numpy as np
import pytest

import exact_ref as X

# the worst points of the host restatement of the device trig code below 1e5 (f64 sin / cos / tan)
WORST = [-75885.045330917957, 63600.224891491329, 46639.304862655372]


def _points(rng):
    k = rng.integers(-63_000, 63_000, 600)
    near = (k * (np.pi / 2)).astype(np.float64)
    steps = rng.integers(-3, 4, 600)
    near = np.array([x + s * np.spacing(x) for x, s in zip(near, steps)])
    return np.concatenate([near, rng.uniform(-1e5, 1e5, 600), np.exp(rng.uniform(-60, 60, 400)) * rng.choice([-1, 1], 400),
                           np.array(WORST + [0.0, -0.0, 5e-324, -1e-310, 2.0 ** -26, 1e5, np.nextafter(1e5, 0)])])


@pytest.mark.skipif(not X.HAVE_LONGDOUBLE, reason="no x86 extended precision here: the mpmath path is the reference itself")
@pytest.mark.parametrize("op", ["sin", "cos", "tan", "cot", "sec", "csc"])
def test_longdouble_matches_mpmath_trig(op):
    rng = np.random.default_rng(1)
    x = _points(rng)
    h, l = X.exact_unary(op, x)
    hm, lm = X.exact_unary(op, x, use_mpmath=True)
    fin = np.isfinite(hm)
    assert np.array_equal(np.isnan(h), np.isnan(hm)) and np.array_equal(h[~fin & ~np.isnan(hm)], hm[~fin & ~np.isnan(hm)])
    # the two double-doubles differ by far less than an ulp of f64: measure in ulps of the mpmath value
    d = np.abs((h[fin] - hm[fin]) + (l[fin] - lm[fin])) / X.ulp_of(hm[fin], lm[fin], np.float64)
    assert d.max() < 2.0 ** -8, (op, d.max())


@pytest.mark.skipif(not X.HAVE_LONGDOUBLE, reason="no x86 extended precision here: the mpmath path is the reference itself")
@pytest.mark.parametrize("op", [o for o in X.UNARY if o not in ("sin", "cos", "tan", "cot", "sec", "csc")] + X.BINARY)
def test_longdouble_matches_mpmath_libm_ops(op):
    rng = np.random.default_rng(2)
    if op in ("acos", "asin"):
        x = rng.uniform(-1, 1, 500)
    elif op in ("log10", "log2", "sqrt", "log", "hypot"):
        x = np.exp(rng.uniform(-50, 50, 500))
    elif op in ("exp", "expm1", "cosh", "sinh"):
        x = rng.uniform(-700, 700, 500)
    else:
        x = rng.uniform(-1e3, 1e3, 500) * np.exp(rng.uniform(-20, 20, 500))
    if op in X.BINARY:
        y = np.exp(rng.uniform(-5, 5, 500)) * (rng.choice([-1, 1], 500) if op == "atan2" else 1)
        y[y == 1.0] = 2.0
        (h, l), (hm, lm) = X.exact_binary(op, x, y), X.exact_binary(op, x, y, use_mpmath=True)
    else:
        (h, l), (hm, lm) = X.exact_unary(op, x), X.exact_unary(op, x, use_mpmath=True)
    d = np.abs((h - hm) + (l - lm)) / X.ulp_of(hm, lm, np.float64)
    assert d.max() < 2.0 ** -8, (op, d.max())


def test_ulp_of_binade_edges_and_subnormals():
    f64, f32 = np.float64, np.float32
    assert X.ulp_of(np.array([1.0]), np.array([0.0]), f64)[0] == 2.0 ** -52
    # just below 1: hi rounds up to 1.0, lo negative -> the binade [0.5, 1)
    assert X.ulp_of(np.array([1.0]), np.array([-1e-20]), f64)[0] == 2.0 ** -53
    assert X.ulp_of(np.array([1.0]), np.array([1e-20]), f64)[0] == 2.0 ** -52
    assert X.ulp_of(np.array([-2.0]), np.array([1e-20]), f64)[0] == 2.0 ** -52
    assert X.ulp_of(np.array([np.nextafter(2.0, 0)]), np.array([0.0]), f64)[0] == 2.0 ** -52
    assert X.ulp_of(np.array([5e-324, 2.0 ** -1022, 0.0]), np.zeros(3), f64).tolist() == [2.0 ** -1074] * 3
    assert X.ulp_of(np.array([2.0 ** -1021]), np.zeros(1), f64)[0] == 2.0 ** -1073
    assert X.ulp_of(np.array([1.0, 2.0 ** -126, 2.0 ** -140, 0.0]), np.zeros(4), f32).tolist() == [2.0 ** -23, 2.0 ** -149, 2.0 ** -149, 2.0 ** -149]
    assert X.ulp_of(np.array([1.0]), np.array([-1e-20]), f32)[0] == 2.0 ** -24


def test_ulp_error_specials():
    f64, f32 = np.float64, np.float32
    one = np.array([1.0])
    z = np.zeros(1)
    assert X.ulp_error(np.array([np.nextafter(1.0, 2)]), one, z, f64)[0] == 1.0
    assert X.ulp_error(np.array([np.nextafter(1.0, 0)]), one, z, f64)[0] == 0.5        # 2^-53 below 1: half an ulp of [1, 2)
    assert X.ulp_error(np.array([1.0]), one, np.array([2.0 ** -54]), f64)[0] == 0.25
    assert X.ulp_error(np.array([np.nextafter(np.float32(1), np.float32(2))]), one, z, f32)[0] == 1.0
    # zeros: the sign must match; a nonzero result for an exact zero is counted in subnormal steps
    assert X.ulp_error(np.array([-0.0]), np.array([-0.0]), z, f64)[0] == 0
    assert X.ulp_error(np.array([0.0]), np.array([-0.0]), z, f64)[0] == np.inf
    assert X.ulp_error(np.array([-1.0]), one, z, f64)[0] == np.inf
    assert X.ulp_error(np.array([1e-323]), z, z, f64)[0] == 2.0
    assert X.ulp_error(np.array([2.0 ** -148]), z, z, f32)[0] == 2.0
    # NaN only against NaN
    assert X.ulp_error(np.array([np.nan]), np.array([np.nan]), z, f64)[0] == 0
    assert X.ulp_error(np.array([np.nan]), one, z, f64)[0] == np.inf
    assert X.ulp_error(one, np.array([np.nan]), z, f64)[0] == np.inf
    # infinity: only where the exact value overflows the format (or is infinite)
    big = np.array([1e39])
    assert X.ulp_error(np.array([np.inf]), big, z, f32)[0] == 0
    assert X.ulp_error(np.array([-np.inf]), big, z, f32)[0] == np.inf
    assert X.ulp_error(np.array([np.inf]), np.array([3e38]), z, f32)[0] == np.inf
    assert X.ulp_error(np.array([float(np.finfo(np.float32).max)]), big, z, f32)[0] == np.inf
    assert X.ulp_error(np.array([np.inf]), np.array([np.inf]), z, f64)[0] == 0
    assert X.ulp_error(np.array([np.inf]), np.array([1e308]), z, f64)[0] == np.inf


def test_round_to_f32_rounds_once():
    mid = 1.0 + 2.0 ** -24                     # half-way between 1 and the next float
    got = X.round_to(np.array([mid, mid, mid, 1.5]), np.array([1e-30, -1e-30, 0.0, 0.0]), np.float32)
    assert got.tolist() == [float(np.nextafter(np.float32(1), np.float32(2))), 1.0, 1.0, 1.5]


def test_exact_sums_and_gamma():
    from rust_dataframe_amd import _abi as A
    v = np.array([1e16, 1.0, -1e16, 3.0])
    s, mag, n = X.fsum_valid([A.HostArray.from_numpy(v, valid=[1, 1, 1, 0])])
    assert (s, mag, n) == (1.0, 2e16 + 1.0, 3)
    assert X.gamma(1) == pytest.approx(2.0 ** -53) and X.gamma(2 ** 20) > 2 ** 20 * 2.0 ** -53
    assert math.isfinite(X.gamma(10 ** 9))
