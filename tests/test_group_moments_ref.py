"""tests/group_moments_ref.py without a GPU: the restated algorithm of rdf_groupby_moments (tiles, pieces, one tile step per
piece, merges level by level) is held to the per-group bounds B = gamma(2n) + 16u on the ill-conditioned, benign and hard
inputs of moments_ref at every group size around the wave and the tile, a constant group keeps M2 == 0.0 exactly, groups
that start around a tile boundary are right, the fast exact path agrees with MomentsRef, and the shortcut the kernel does
not take — per-group sum x, sum x^2 — is shown to break the bound on the ill-conditioned inputs."""
from fractions import Fraction as F

import numpy as np
import pytest

import moments_ref as M
import group_moments_ref as R

T = R.T
SIZES = [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]


def table(name, sizes, seed=0):
    """Groups of the given sizes one after the other (sorted positions), values from the named input."""
    seg = np.repeat(np.arange(len(sizes)), sizes)
    x = M.make_input(name, len(seg), seed)
    return seg, x


def check_groups(seg, ok, x, y=None):
    states = R.restated_states(seg, ok, x, y)
    worst = 0.0
    for g in range(int(seg[-1]) + 1):
        sel = (seg == g) & ok
        if y is None:
            ref = R.moments_ref_of(x[sel])
            e, name = R.errors_in_bounds(R.stats_of(states[g]), ref, R.STATS)
        else:
            ref = R.comoments_ref_of(x[sel], y[sel])
            e, name = R.errors_in_bounds(R.costats_of(states[g]), ref, R.COSTATS)
        assert states[g][0] == int(sel.sum())
        assert e <= 1.0, (g, int(sel.sum()), name, e)
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("name", M.ILL + M.BENIGN + M.HARD)
def test_every_group_size_is_inside_its_bound(name):
    seg, x = table(name, SIZES)
    ok = np.ones(len(seg), dtype=bool)
    print(name, "worst error / bound:", check_groups(seg, ok, x))
    # the same sizes in the opposite order put every boundary elsewhere in its tile; 10 % of the rows do not count
    seg, x = table(name, SIZES[::-1], seed=1)
    ok = np.random.default_rng(5).random(len(seg)) >= 0.1
    check_groups(seg, ok, x)


@pytest.mark.parametrize("name", ["offset_1e9", "normal", "two_clusters"])
def test_pairs_are_inside_their_bounds(name):
    seg, x = table(name, SIZES)
    y = 3.0 * x + M.make_input("normal", len(x), seed=2)
    check_groups(seg, np.ones(len(seg), dtype=bool), x, y)


@pytest.mark.parametrize("size", [1, 2, T - 1, T, T + 1, 3 * T + 5])
def test_a_constant_group_has_m2_exactly_zero(size):
    seg = np.repeat(np.arange(3), [5, size, 7])
    x = M.make_input("offset_1e9", len(seg))
    x[seg == 1] = 0.1
    st = R.restated_states(seg, np.ones(len(seg), dtype=bool), x)[1]
    assert st[0] == size and st[1] + st[2] == 0.1 and st[3:] == (0.0, 0.0, 0.0)
    s = R.stats_of(st)
    assert s["var_pop"] == 0.0 and s["skewness"] is None and s["kurtosis"] is None
    assert (s["var_samp"] is None) == (size == 1)


@pytest.mark.parametrize("start", [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1])
def test_groups_that_start_around_a_tile_boundary(start):
    seg = np.repeat(np.arange(4), [start, 2 * T, 1, 3])
    x = M.make_input("offset_1e15", len(seg), seed=start)
    check_groups(seg, np.ones(len(seg), dtype=bool), x)


def test_three_levels_of_small_integers_on_the_fast_exact_path():
    n = 2 * T * T + 77                       # 131149 rows -> 1026 -> 10 items: three levels
    assert len(R.levels_of(n)) == 3
    rng = np.random.default_rng(3)
    x = rng.integers(-511, 512, n).astype(np.float64)
    seg = np.zeros(n, dtype=np.int64)
    ok = np.ones(n, dtype=bool)
    check_groups(seg, ok, x)
    y = (rng.integers(-200, 200, n) + x // 2).astype(np.float64)
    check_groups(seg, ok, x, y)
    # the fast path is MomentsRef: the same Fractions
    a, b = R.SmallIntMomentsRef(x[:3000]), M.MomentsRef(x[:3000])
    assert (a.n, a.mean, a.m2, a.m3, a.m4, a.sum_abs, a.abs3) == (b.n, b.mean, b.m2, b.m3, b.m4, b.sum_abs, b.abs3)
    c, d = R.SmallIntComomentsRef(x[:3000], y[:3000]), M.ComomentsRef(x[:3000], y[:3000])
    assert (c.cxy, c.abs_xy, c.x.m2, c.y.m2) == (d.cxy, d.abs_xy, d.x.m2, d.y.m2)


def test_the_level_plan():
    assert R.levels_of(1) == [1] and R.levels_of(T) == [T] and R.levels_of(T + 1) == [T + 1, 4]
    assert R.levels_of(50_000_000) == [50_000_000, 390626, 3052, 24]


def test_group_order_counts_and_first_rows():
    keys = [(np.array([3, 1, 3, 2, 1, 3]), np.array([1, 1, 1, 0, 1, 1], dtype=bool))]
    x = (np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), np.array([1, 0, 1, 1, 1, 1], dtype=bool))
    rows, counts, vals, _ = R.group_moments_ref(keys, x)
    assert rows.tolist() == [1, 0, 3] and counts.tolist() == [1, 3, 1]            # keys 1, 3, NULL last
    assert [v.tolist() for v in vals] == [[5.0], [1.0, 3.0, 6.0], [4.0]]


@pytest.mark.parametrize("name", M.ILL)
def test_per_group_power_sums_miss_the_bound_on_the_ill_conditioned_inputs(name):
    """What the hash GROUP BY could deliver per group — sum x and sum x^2 in f64 — loses the variance of every group."""
    seg, x = table(name, [20000, 20000])
    for g in range(2):
        xs = x[seg == g]
        ref = M.MomentsRef(xs)
        assert abs(F(M.naive_variance(xs)) - ref.stat("var_pop")) > 100 * F(ref.bound("var_pop"))
