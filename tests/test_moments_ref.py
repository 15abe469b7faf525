"""tests/moments_ref.py held against hand-computed cases and numpy on benign data, and the proof that the ill-conditioned
inputs discriminate: the textbook sum x, sum x^2 formula in f64 misses the variance bound on each of them."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import moments_ref as R


def test_hand_computed_moments():
    r = R.MomentsRef([1.0, 2.0, 3.0, 4.0, 10.0])
    # mean 4; d = -3 -2 -1 0 6: M2 = 50, M3 = -27 - 8 - 1 + 216 = 180, M4 = 81 + 16 + 1 + 1296 = 1394, sum|d|^3 = 252
    assert (r.n, r.mean, r.m2, r.m3, r.m4, r.abs3, r.sum_abs) == (5, 4, 50, 180, 1394, 252, 20)
    assert r.stat("var_pop") == 10 and r.stat("var_samp") == F(25, 2)
    assert abs(float(r.stat("stddev_pop")) - math.sqrt(10)) < 1e-15
    assert abs(float(r.stat("skewness")) - math.sqrt(5) * 180 / 50 ** 1.5) < 1e-15
    assert r.stat("kurtosis") == F(5 * 1394, 2500) - 3
    # values that are not integers, and a power-of-two scale well below 1
    r = R.MomentsRef([0.5, 0.25, 0.25])
    assert r.mean == F(1, 3) and r.m2 == F(1, 24) and r.stat("var_samp") == F(1, 48)


def test_hand_computed_comoments():
    r = R.ComomentsRef([1.0, 2.0, 3.0], [2.0, 4.0, 9.0])
    # dx = -1 0 1, dy = -3 -1 4: Cxy = 3 + 0 + 4 = 7, M2x = 2, M2y = 26, sum|dx dy| = 7
    assert (r.cxy, r.x.m2, r.y.m2, r.abs_xy) == (7, 2, 26, 7)
    assert r.stat("covar_pop") == F(7, 3) and r.stat("covar_samp") == F(7, 2)
    assert abs(float(r.stat("corr")) - 7 / math.sqrt(52)) < 1e-15
    r = R.ComomentsRef([1.0, -2.0, 0.5], [-1.0, 2.0, 0.0])       # a product that changes sign: sum|dx dy| > |Cxy|
    assert r.abs_xy >= abs(r.cxy)


def test_absent_statistics():
    e = R.MomentsRef([])
    assert all(e.stat(s) is None for s in R.STATS)
    one = R.MomentsRef([3.5])
    assert one.stat("mean") == F(7, 2) and one.stat("var_pop") == 0
    assert one.stat("var_samp") is None and one.stat("stddev_samp") is None and one.stat("skewness") is None and one.stat("kurtosis") is None
    const = R.MomentsRef(R.make_input("constant", 100))
    assert const.stat("var_samp") == 0 and const.stat("skewness") is None and const.stat("kurtosis") is None
    c = R.ComomentsRef([1.0, 1.0], [1.0, 2.0])
    assert c.stat("corr") is None and c.stat("covar_pop") == 0
    assert R.ComomentsRef([1.0], [2.0]).stat("covar_samp") is None


@pytest.mark.parametrize("name", R.BENIGN)
def test_against_numpy_on_benign_data(name):
    x = R.make_input(name, 5000)
    y = 3.0 * x + R.make_input("normal", 5000, seed=1)
    r, c = R.MomentsRef(x), R.ComomentsRef(x, y)
    assert abs(float(r.stat("mean")) - x.mean()) <= 1e-12 * abs(x).mean()
    assert abs(float(r.stat("var_pop")) - np.var(x)) <= 1e-12 * np.var(x)
    assert abs(float(r.stat("var_samp")) - np.var(x, ddof=1)) <= 1e-12 * np.var(x)
    assert abs(float(r.stat("stddev_samp")) - np.std(x, ddof=1)) <= 1e-12 * np.std(x)
    d = x - x.mean()
    assert abs(float(r.stat("skewness")) - math.sqrt(len(x)) * (d ** 3).sum() / (d ** 2).sum() ** 1.5) <= 1e-10
    assert abs(float(r.stat("kurtosis")) - (len(x) * (d ** 4).sum() / (d ** 2).sum() ** 2 - 3)) <= 1e-10
    assert abs(float(c.stat("corr")) - np.corrcoef(x, y)[0, 1]) <= 1e-12
    assert abs(float(c.stat("covar_samp")) - np.cov(x, y)[0, 1]) <= 1e-12 * abs(np.cov(x, y)[0, 1])
    # the reference's own answers are inside its own bounds, and the bounds are a few ulps wide, not percent
    got = {s: float(r.stat(s)) for s in R.STATS}
    assert max(R.error_in_bounds(got, r, R.STATS).values()) <= 1.0
    assert r.bound("var_pop") <= 2e-12 * float(r.stat("var_pop"))


def test_scaled_ints_are_exact():
    x = np.array([0.1, -3.75, 2.0 ** -1074, 1e300, 0.0, -2.0 ** 52 - 1])
    k, e = R.scaled_ints(x)
    assert all(F(float(v)) == F(int(ki)) * F(2) ** e for v, ki in zip(x, k))


@pytest.mark.parametrize("name", R.ILL)
def test_the_textbook_formula_misses_the_bound_on_the_ill_conditioned_inputs(name):
    """20 000 rows as in DESIGN.md 13: sum x^2 - (sum x)^2 / n loses the variance, the tile step keeps it."""
    x = R.make_input(name, 20000)
    r = R.MomentsRef(x)
    naive = R.naive_variance(x)
    assert abs(F(naive) - r.stat("var_pop")) > 100 * F(r.bound("var_pop"))
    # ... and a single tile of the kernel's step is inside it
    t = R.MomentsRef(x[:256])
    n, mean, lo, m2, m3, m4 = R.tile_state(x[:256])
    got = {"mean": mean + lo, "var_pop": m2 / n, "var_samp": m2 / (n - 1), "stddev_pop": math.sqrt(m2 / n), "stddev_samp": math.sqrt(m2 / (n - 1)),
           "skewness": math.sqrt(n) * m3 / (m2 * math.sqrt(m2)), "kurtosis": n * m4 / (m2 * m2) - 3}
    assert max(R.error_in_bounds(got, t, R.STATS).values()) <= 1.0
