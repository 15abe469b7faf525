"""The exact reference of rdf_moments / rdf_comoments, the bounds a result is held to, and the inputs the tests share.

Every f64 is an integer times a power of two, so a column scales to Python integers: the power sums S1..S4 (and Sxy for a
pair) are exact integers, the central moments exact `Fraction`s, and so is the "absolute" third moment sum |d|^3 that bounds
the skewness.  Square roots are taken to 200 bits.  Nothing here rounds before the final comparison.

Bounds, with u = 2^-53 and B = gamma(2n) + 16u (exact_ref.gamma): the gamma term covers ANY order of the roughly 2n additions of
like-signed terms a one-pass algorithm makes per sum (n for the centring, n for the sum itself); the 16u covers the finish —
at most eight roundings of one u each (the divisions, the square root, the products of the statistic's formula), doubled.

    count                     exact
    mean                      |err| <= gamma(n) sum|x| / n + ulp(mean)
    variances and stddevs     relative error <= B
    skewness                  |err| <= B sqrt(n) sum|d|^3 / M2^1.5
    kurtosis                  |err| <= B (kurtosis + 3)
    covariances               |err| <= B sum|dx dy| / n        (_SAMP: / (n - 1))
    corr                      |err| <= B sum|dx dy| / sqrt(M2x M2y)

`tile_state` / `cotile_state` restate the kernel's tile step in numpy (centre on a double near the mean, sum d^k, shift to
the true mean, keep the mean as two doubles): the CPU tests build states with them and hold the library's merge to the bounds.
"""
import math
from fractions import Fraction

import numpy as np

from exact_ref import gamma

U = 2.0 ** -53
STATS = ["mean", "var_pop", "var_samp", "stddev_pop", "stddev_samp", "skewness", "kurtosis"]
COSTATS = ["covar_pop", "covar_samp", "corr"]
ILL = ["offset_1e9", "two_pow_52", "offset_1e15"]
BENIGN = ["normal", "lognormal", "uniform", "exponential"]
HARD = ["outlier_first", "two_clusters"]


def make_input(name, n, seed=0):
    """The named f64 inputs of the tests, n rows."""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    if name == "offset_1e9":
        return 1e9 + rng.standard_normal(n)
    if name == "two_pow_52":
        return 2.0 ** 52 + rng.integers(0, 1000, n).astype(np.float64)
    if name == "offset_1e15":
        return 1e15 + rng.integers(0, 8, n).astype(np.float64)
    if name == "normal":
        return rng.standard_normal(n)
    if name == "lognormal":
        return rng.lognormal(0.0, 1.0, n)
    if name == "uniform":
        return rng.uniform(-3.0, 5.0, n)
    if name == "exponential":
        return rng.exponential(2.0, n)
    if name == "outlier_first":
        x = rng.standard_normal(n)
        if n:
            x[0] = 1e15
        return x
    if name == "two_clusters":
        return np.where(rng.integers(0, 2, n) == 0, -1e12, 1e12) + rng.standard_normal(n)
    if name == "constant":
        return np.full(n, 0.1)
    raise KeyError(name)


# ---------------------------------------------------------------- exact arithmetic
def scaled_ints(x):
    """f64 vector (finite) -> (object array of Python ints k, e) with x[i] == k[i] * 2**e exactly."""
    x = np.asarray(x, dtype=np.float64)
    assert np.isfinite(x).all()
    m, ex = np.frexp(x)
    mi = np.ldexp(m, 53).astype(np.int64)          # exact: |m| < 1 has at most 53 fraction bits
    e = ex.astype(np.int64) - 53
    nz = mi != 0
    emin = int(e[nz].min()) if nz.any() else 0
    k = np.array([int(a) << int(b - emin) if a else 0 for a, b in zip(mi.tolist(), e.tolist())], dtype=object)
    return k, emin


def sqrt_fraction(f, bits=200):
    """sqrt of a non-negative Fraction to `bits` bits, as a Fraction."""
    if f == 0:
        return Fraction(0)
    shift = max(0, bits - (f.numerator.bit_length() - f.denominator.bit_length()) // 2)
    num = f.numerator << (2 * shift)
    return Fraction(math.isqrt(num * f.denominator), f.denominator << shift)


def ulp(v):
    return math.ulp(float(v)) if v != 0 else 2.0 ** -1074


class MomentsRef:
    """Exact count, mean, M2, M3, M4, sum|x| and sum|d|^3 of a f64 vector."""

    def __init__(self, x):
        x = np.asarray(x, dtype=np.float64)
        self.n = n = len(x)
        if n == 0:
            return
        k, e = scaled_ints(x)
        s = Fraction(2) ** e
        s1, s2, s3, s4 = int(k.sum()), int((k * k).sum()), int((k * k * k).sum()), int((k * k * k * k).sum())
        self.mean = Fraction(s1, n) * s
        self.sum_abs = int(np.abs(k).sum()) * s
        self.m2 = (s2 - Fraction(s1 * s1, n)) * s ** 2
        self.m3 = (s3 - Fraction(3 * s2 * s1, n) + Fraction(2 * s1 ** 3, n * n)) * s ** 3
        self.m4 = (s4 - Fraction(4 * s3 * s1, n) + Fraction(6 * s2 * s1 * s1, n * n) - Fraction(3 * s1 ** 4, n ** 3)) * s ** 4
        d = np.abs(k * n - s1)                       # n |d| in units of 2^e
        self.abs3 = Fraction(int((d * d * d).sum()), n ** 3) * s ** 3

    def stat(self, name):
        """The exact statistic as a Fraction (square roots to 200 bits), or None where the library answers "absent"."""
        n = self.n
        if n == 0 or (name.endswith("_samp") and n < 2):
            return None
        if name == "mean":
            return self.mean
        if name in ("var_pop", "stddev_pop", "var_samp", "stddev_samp"):
            v = self.m2 / (n if name.endswith("_pop") else n - 1)
            return sqrt_fraction(v) if name.startswith("stddev") else v
        if self.m2 == 0:
            return None
        if name == "skewness":
            return self.m3 * sqrt_fraction(Fraction(n) / self.m2 ** 3)
        if name == "kurtosis":
            return n * self.m4 / self.m2 ** 2 - 3
        raise KeyError(name)

    def bound(self, name):
        """The largest |error| the statistic may have (a float, rounded up by a hair)."""
        n = self.n
        b = gamma(2 * n) + 16 * U
        v = self.stat(name)
        if name == "mean":
            r = gamma(n) * float(self.sum_abs) / n + ulp(v)
        elif name == "skewness":
            r = b * float(self.abs3 * sqrt_fraction(Fraction(n) / self.m2 ** 3))
        elif name == "kurtosis":
            r = b * float(v + 3)
        else:
            r = b * float(v)
        return r * (1 + 2.0 ** -40)


class ComomentsRef:
    """Exact count, Cxy, M2x, M2y and sum|dx dy| of two f64 vectors of one length."""

    def __init__(self, x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        assert len(x) == len(y)
        self.n = n = len(x)
        self.x, self.y = MomentsRef(x), MomentsRef(y)
        if n == 0:
            return
        (kx, ex), (ky, ey) = scaled_ints(x), scaled_ints(y)
        s = Fraction(2) ** (ex + ey)
        sx, sy = int(kx.sum()), int(ky.sum())
        self.cxy = (int((kx * ky).sum()) - Fraction(sx * sy, n)) * s
        self.abs_xy = Fraction(int(np.abs((kx * n - sx) * (ky * n - sy)).sum()), n * n) * s

    def stat(self, name):
        n = self.n
        if n == 0 or (name == "covar_samp" and n < 2):
            return None
        if name == "covar_pop":
            return self.cxy / n
        if name == "covar_samp":
            return self.cxy / (n - 1)
        if name == "corr":
            if self.x.m2 == 0 or self.y.m2 == 0:
                return None
            return self.cxy / sqrt_fraction(self.x.m2 * self.y.m2)
        raise KeyError(name)

    def bound(self, name):
        n = self.n
        b = gamma(2 * n) + 16 * U
        if name == "covar_pop":
            r = b * float(self.abs_xy / n)
        elif name == "covar_samp":
            r = b * float(self.abs_xy / (n - 1))
        else:
            r = b * float(self.abs_xy / sqrt_fraction(self.x.m2 * self.y.m2))
        return r * (1 + 2.0 ** -40)


def error_in_bounds(got, ref, names):
    """got: name -> float | None.  -> name -> |got - exact| / bound (0 where both are absent or the value is exact); raises
    where one side is absent and the other is not."""
    out = {}
    for name in names:
        want = ref.stat(name)
        g = got[name]
        assert (g is None) == (want is None), f"{name}: got {g!r}, exact {want!r}"
        if want is None:
            out[name] = 0.0
            continue
        assert math.isfinite(g), f"{name}: got {g!r}, exact {float(want)!r}"
        err = abs(Fraction(g) - want)
        bound = ref.bound(name)
        out[name] = 0.0 if err == 0 else (float(err) / bound if bound > 0 else math.inf)
    return out


# ---------------------------------------------------------------- the kernel's tile step, restated
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def mean_add(hi, lo, t):
    s, e = two_sum(hi, t)
    e = e + lo
    h = s + e
    return h, e - (h - s)


def tile_state(x):
    """(count, mean, mean_lo, m2, m3, m4) of a small f64 vector the way one tile of the kernel forms it."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if n == 0:
        return (0, 0.0, 0.0, 0.0, 0.0, 0.0)
    c = x[0] if (x == x[0]).all() else np.float64(x.sum()) / np.float64(n)
    d = x - c
    d2 = d * d
    s1, s2, s3, s4 = (np.float64(v.sum()) for v in (d, d2, d2 * d, d2 * d2))
    nd = np.float64(n)
    e = s1 / nd
    e2 = e * e
    mean, lo = mean_add(np.float64(c), np.float64(0.0), e)
    m2 = s2 - nd * e2
    m3 = (s3 - (3.0 * e) * s2) + (2.0 * nd) * (e2 * e)
    m4 = ((s4 - (4.0 * e) * s3) + (6.0 * e2) * s2) - (3.0 * nd) * (e2 * e2)
    return (n, float(mean), float(lo), float(m2), float(m3), float(m4))


def cotile_state(x, y):
    """(count, mean_x, mean_x_lo, mean_y, mean_y_lo, m2x, m2y, cxy) of one tile of a pair."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(x)
    if n == 0:
        return (0,) + (0.0,) * 7
    nd = np.float64(n)
    cx = x[0] if (x == x[0]).all() else np.float64(x.sum()) / nd
    cy = y[0] if (y == y[0]).all() else np.float64(y.sum()) / nd
    dx, dy = x - cx, y - cy
    sx, sy, sxx, syy, sxy = (np.float64(v.sum()) for v in (dx, dy, dx * dx, dy * dy, dx * dy))
    ex, ey = sx / nd, sy / nd
    mx, mxl = mean_add(np.float64(cx), np.float64(0.0), ex)
    my, myl = mean_add(np.float64(cy), np.float64(0.0), ey)
    return (n, float(mx), float(mxl), float(my), float(myl), float(sxx - nd * (ex * ex)), float(syy - nd * (ey * ey)),
            float(sxy - nd * (ex * ey)))


def naive_variance(x):
    """The formula the kernel does NOT use: var_pop = (sum x^2 - (sum x)^2 / n) / n, all in f64."""
    x = np.asarray(x, dtype=np.float64)
    n = np.float64(len(x))
    s1, s2 = np.float64(x.sum()), np.float64((x * x).sum())
    return float((s2 - s1 * s1 / n) / n)
