"""tests/window_frame_ref.py — the CPU restatement the GPU tests hold rdf_window_agg to — checked on its own: pandas' rolling /
expanding / transform on integer-valued data for the trailing and unbounded ROWS frames, hand-written vectors for what
pandas does not spell (FOLLOWING bounds, both bounds on one side, RANGE peer frames, empty frames, the NULL and NaN rules,
-0.0 < +0.0), and the vectorised path against the brute-force one."""
import math

import numpy as np
import pytest

import window_frame_ref as R
from window_frame_ref import UNBOUNDED_FOLLOWING as UF
from window_frame_ref import UNBOUNDED_PRECEDING as UP
from window_frame_ref import frame_ref as ref


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def L(pair):
    """(values, valid) -> a list with None for NULL."""
    return [v if ok else None for v, ok in zip(pair[0].tolist(), pair[1].tolist())]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_trailing_and_unbounded_rows_frames_against_pandas(seed):
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(seed)
    n = int(rng.integers(300, 1500))
    p = rng.integers(0, 7, n)
    o = rng.permutation(n)                                    # distinct: the order inside a partition is unambiguous
    x = rng.integers(-50, 50, n).astype(np.float64)
    valid = rng.random(n) > 0.2
    df = pd.DataFrame({"p": p, "o": o, "x": np.where(valid, x, np.nan)})
    s = df.sort_values(["p", "o"], kind="stable")
    part, order, vals = [(p, None)], [(o, None, False)], [(x, valid)]
    for w in (1, 2, 3, 10, 64, n + 5):
        frame = ("rows", -(w - 1), 0)
        got = ref(part, order, vals, [(f, 0, frame) for f in ("sum", "min", "max", "count", "avg")])
        roll = s.groupby("p")["x"].rolling(w, min_periods=1)
        for (g, ok), exp in zip(got, (roll.sum(), roll.min(), roll.max(), roll.count(), roll.mean())):
            e = exp.reset_index(level=0, drop=True).reindex(df.index).to_numpy()
            cnt = got[3][0]
            assert np.array_equal(ok, cnt > 0) or g.dtype == np.int64          # NULL exactly where no valid row is in the frame
            live = cnt > 0
            assert np.array_equal(np.asarray(g, dtype=np.float64)[live], e[live]), w
        assert np.array_equal(got[3][0], roll.count().reset_index(level=0, drop=True).reindex(df.index).to_numpy().astype(np.int64))
    exp_frames = ((("rows", UP, 0), s.groupby("p")["x"].expanding()),)
    for frame, e in exp_frames:
        got = ref(part, order, vals, [(f, 0, frame) for f in ("sum", "min", "max", "count", "avg")])
        cnt = got[3][0]
        for (g, ok), exp in zip(got, (e.sum(), e.min(), e.max(), e.count(), e.mean())):
            ev = exp.reset_index(level=0, drop=True).reindex(df.index).to_numpy()
            assert np.array_equal(np.asarray(g, dtype=np.float64)[cnt > 0], ev[cnt > 0])
    got = ref(part, order, vals, [("sum", 0, ("rows", UP, UF)), ("sum", 0, ("range", UP, UF)), ("count", 0, ("rows", UP, UF))])
    tot = df.groupby("p")["x"].transform("sum").to_numpy()
    c = df.groupby("p")["x"].transform("count").to_numpy()
    assert np.array_equal(got[2][0], c)
    assert np.array_equal(got[0][0][c > 0], tot[c > 0]) and np.array_equal(got[1][0], got[0][0])


def test_following_bounds_both_on_one_side_and_empty_frames():
    x = np.array([1, 2, 3, 4, 5, 10, 20], dtype=np.int64)
    p = np.array([0, 0, 0, 0, 0, 1, 1], dtype=np.int64)
    o = np.arange(7)
    run = lambda fn, frame: L(ref([(p, None)], [(o, None, False)], [(x, None)], [(fn, 0, frame)])[0])  # noqa: E731
    assert run("sum", ("rows", 0, 1)) == [3, 5, 7, 9, 5, 30, 20]
    assert run("sum", ("rows", -1, 1)) == [3, 6, 9, 12, 9, 30, 30]
    assert run("sum", ("rows", 1, 2)) == [5, 7, 9, 5, None, 20, None]                # the frame slides off the partition's end
    assert run("sum", ("rows", -2, -1)) == [None, 1, 3, 5, 7, None, 10]
    assert run("sum", ("rows", 2, 5)) == [12, 9, 5, None, None, None, None]
    assert run("count", ("rows", 2, 5)) == [3, 2, 1, 0, 0, 0, 0]                     # COUNT of an empty frame is 0, not NULL
    assert run("min", ("rows", 1, UF)) == [2, 3, 4, 5, None, 20, None]
    assert run("max", ("rows", UP, -1)) == [None, 1, 2, 3, 4, None, 10]
    assert run("max", ("rows", -1, 1)) == [2, 3, 4, 5, 5, 20, 20]
    assert run("avg", ("rows", -1, 0)) == [1.0, 1.5, 2.5, 3.5, 4.5, 10.0, 15.0]
    cnt = L(ref([(p, None)], [(o, None, False)], [], [("count", -1, ("rows", -1, 1))])[0])
    assert cnt == [2, 3, 3, 3, 2, 2, 2]
    desc = L(ref([(p, None)], [(o, None, True)], [(x, None)], [("sum", 0, ("rows", UP, 0))])[0])
    assert desc == [15, 14, 12, 9, 5, 30, 20]
    first = ref([(p, None)], [(o, None, True)], [], [("first_value", -1, ("rows", UP, UF)), ("last_value", -1, ("rows", 0, 1)),
                                                     ("first_value", -1, ("rows", 1, 1))])
    assert L(first[0]) == [4, 4, 4, 4, 4, 6, 6] and L(first[1]) == [0, 0, 1, 2, 3, 5, 5] and L(first[2]) == [None, 0, 1, 2, 3, None, 5]


def test_range_frames_follow_the_peers():
    o = np.array([1, 1, 2, 2, 2, 3], dtype=np.int64)
    x = np.array([1, 2, 4, 8, 16, 32], dtype=np.int64)
    run = lambda fn, frame: L(ref([], [(o, None, False)], [(x, None)], [(fn, 0, frame)])[0])  # noqa: E731
    assert run("sum", ("range", UP, 0)) == [3, 3, 31, 31, 31, 63]                    # SQL's default frame: [0, l]
    assert run("sum", ("rows", UP, 0)) == [1, 3, 7, 15, 31, 63]
    assert run("sum", ("range", 0, 0)) == [3, 3, 28, 28, 28, 32]
    assert run("max", ("range", 0, 0)) == [2, 2, 16, 16, 16, 32]
    assert run("sum", ("range", 0, UF)) == [63, 63, 60, 60, 60, 32]
    assert run("min", ("range", 0, UF)) == [1, 1, 4, 4, 4, 32]
    assert run("count", ("range", UP, UF)) == [6] * 6
    assert L(ref([], [], [(x, None)], [("sum", 0, ("range", 0, 0))])[0]) == [63] * 6   # no order keys: all rows are peers
    with pytest.raises(AssertionError):
        run("sum", ("range", -1, 0))


def test_null_and_nan_rules_and_the_zeros():
    inf, nan = math.inf, math.nan
    x = np.array([1.0, nan, 2.0, inf, 3.0, -inf, 4.0, 0.0, -0.0, 5.0])
    valid = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1, 0], dtype=bool)
    run = lambda fn, frame: ref([], [], [(x, valid)], [(fn, 0, frame)])[0]  # noqa: E731
    s, ok = run("sum", ("rows", -1, 0))
    assert ok.tolist() == [True] * 10                          # a NULL row next to a valid one; never two NULLs together
    assert math.isnan(s[1]) and math.isnan(s[2]) and s[3] == inf and s[4] == inf and s[5] == -inf and s[6] == -inf
    assert s[0] == 1.0 and s[7] == 4.0 and s[9] == 0.0 and bits(s[8:10]).tolist() == [0, 0]   # a frame after a NaN is finite; zero is +0.0
    s, ok = run("sum", ("rows", -2, 0))
    assert math.isnan(s[5]) and s[7] == -inf                   # both infinities in one frame
    s, ok = run("sum", ("rows", 0, 0))
    assert ok.tolist() == valid.tolist() and L((s, ok))[2] is None          # SUM over no valid row is NULL, not 0
    c, ok = run("count", ("rows", 0, 0))
    assert c.tolist() == valid.astype(int).tolist() and ok.all()
    m, ok = run("min", ("rows", -1, 0))
    assert m[1] == 1.0 and m[2] != m[2] and bits(m[2]) == bits(R.QNAN) and m[3] == inf      # NaN ignored, unless it is all there is
    assert bits(m[8]) == bits(-0.0) and bits(m[9]) == bits(-0.0)
    m, ok = run("max", ("rows", -1, 0))
    assert bits(m[8]) == bits(0.0) and bits(m[7]) == bits(4.0) and m[5] == 3.0 and m[6] == 4.0
    a, ok = run("avg", ("rows", -2, 0))
    assert a[9] == 0.0 and a[8] == 4.0 / 3.0 and ok.all()
    xi = np.array([np.iinfo(np.int64).max, 1, np.iinfo(np.int64).min, -1], dtype=np.int64)
    s, ok = ref([], [], [(xi, None)], [("sum", 0, ("rows", UP, 0))])[0]
    assert s.tolist() == [np.iinfo(np.int64).max, np.iinfo(np.int64).min, 0, -1]               # wraps
    m, ok = ref([], [], [(xi, np.array([1, 0, 1, 0], dtype=bool))], [("min", 0, ("rows", 0, 0)), ("max", 0, ("rows", 0, 0))])[0]
    assert L((m, ok)) == [np.iinfo(np.int64).max, None, np.iinfo(np.int64).min, None]          # the extremes are values, not NULLs


def test_the_slack_of_the_float_sum_bound():
    x = np.array([1e16, -1e16, 1.0, 1.0, 1.0])
    sl = R.sum_slack([], [], (x, None), ("rows", -2, 0))
    assert sl[0] == 8 * 2 * 2.0 ** -106 * np.nextafter(1e16, math.inf)
    assert 0 < sl[4] < 1e-13                                   # far below the error of 1 or more that a plain f64 prefix makes here


FRAMES = [("rows", UP, 0), ("rows", -3, 0), ("rows", -2, 2), ("rows", 0, UF), ("rows", 1, 4), ("rows", -5, -2), ("rows", UP, UF),
          ("range", UP, 0), ("range", 0, 0), ("range", 0, UF), ("rows", -70, 70), ("rows", 0, 0), ("rows", UP, -1), ("rows", 3, UF)]


@pytest.mark.parametrize("kind", ["int", "float"])
def test_the_vectorised_path_is_the_brute_force_one(kind):
    rng = np.random.default_rng(5)
    n = 700
    p = rng.integers(0, 9, n)
    o = rng.integers(0, 12, n)
    x = rng.integers(-1000, 1000, n)
    x = x.astype(np.int64) if kind == "int" else x.astype(np.float64)
    valid = rng.random(n) > 0.3
    assert R.exact_for_fast_path(x, valid)
    calls = [(fn, 0, fr) for fr in FRAMES for fn in ("sum", "min", "max", "count", "avg")]
    calls += [(fn, -1, fr) for fr in FRAMES for fn in ("count", "first_value", "last_value")]
    slow = ref([(p, None)], [(o, None, True)], [(x, valid)], calls)
    fast = R.frame_ref_fast([(p, None)], [(o, None, True)], [(x, valid)], calls)
    for c, (s, f) in zip(calls, zip(slow, fast)):
        assert s[0].dtype == f[0].dtype and np.array_equal(s[1], f[1]), c
        assert np.array_equal(s[0][s[1]], f[0][f[1]]), c
    if kind == "float":
        for fr in FRAMES[:4]:
            assert np.allclose(R.sum_slack([(p, None)], [(o, None, True)], (x, valid), fr),
                               R.sum_slack_fast([(p, None)], [(o, None, True)], (x, valid), fr), rtol=1e-12, atol=0)
    assert not R.exact_for_fast_path(np.array([0.5])) and not R.exact_for_fast_path(np.array([-0.0])) and not R.exact_for_fast_path(np.array([np.nan]))
