"""rdf_groupby_moments on the MI355X: variance, stddev, skewness, kurtosis, covar and corr per group, held to
tests/group_moments_ref.py.  Groups, their order, first rows and counts are compared bit for bit; every statistic of every
group is held to moments_ref's bound with n the GROUP's count, B = gamma(2n) + 16u, against the exact moments of the counted
values.  Every case runs over host and device memory, twice each, and the four results are identical bytes.  The shapes place
the group boundaries around the multiples of the level-0 tile T (A.GROUP_MOMENTS_TILE).  Each case prints its largest error
in units of its bound."""
import ctypes as C
import math

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
import moments_ref as M
import group_moments_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = A.GROUP_MOMENTS_TILE
MEMS = ["host", "device"]
NUMERIC = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64]
OFFSETS = [0, 1, 3, 7, 9, 13, 64]


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


# ---------------------------------------------------------------- inputs: a column is (numpy values, valid | None) or
# ([str | None, ...],) for Utf8

def is_text(col):
    return not isinstance(col[0], np.ndarray)


def chunks_of(col, lens, offsets, mem):
    out, at = [], 0
    for ln, off in zip(lens, offsets):
        if is_text(col):
            c = A.HostUtf8.from_pylist(col[0][at:at + ln], off % 13, off % 9)
            out.append(A.DeviceUtf8.from_host(c) if mem == "device" else c)
        else:
            valid = col[1] if len(col) > 1 else None
            c = A.HostArray.from_numpy(col[0][at:at + ln], None if valid is None else valid[at:at + ln], offset=off)
            if mem == "device":
                vt = torch.from_numpy(np.ascontiguousarray(c.values)).cuda()
                bt = torch.from_numpy(np.ascontiguousarray(c.validity)).cuda() if c.validity is not None else None
                c = A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, c.offset, c.length, c.dtype, c.null_count, keep=(vt, bt))
            out.append(c)
        at += ln
    return out


def run(api, keys, x, y, stats, mem="host", lens=None, offsets=None, **kw):
    cols = list(keys) + [c for c in (x, y) if c is not None]
    n = len(cols[0][0])
    lens = [n] if lens is None else lens
    offsets = [0] * len(lens) if offsets is None else offsets
    assert sum(lens) == n
    ch = [chunks_of(c, lens, offsets, mem) for c in cols]
    if mem == "device":
        torch.cuda.synchronize()
    k = len(keys)
    return api.groupby_moments(ch[:k], ch[k] if x is not None else None, ch[k + 1] if y is not None else None, stats=stats, states=x is not None, **kw)


def as_bytes(res):
    groups, rows, outs, counts, states = res
    return (groups, None if rows is None else rows.tobytes(), [(v.tobytes(), ok.tobytes()) for v, ok in outs],
            None if counts is None else counts.tobytes(), None if states is None else bytes(states))


def ref_col(col):
    if is_text(col):
        return ([None if r is None else r.encode() for r in col[0]],)
    return col


def four_runs(api, keys, x, y, stats, lens=None, offsets=None, what=""):
    """host, host, device, device: identical bytes.  -> the first result."""
    first = None
    for mem in MEMS:
        for rep in range(2):
            res = run(api, keys, x, y, stats, mem, lens, offsets)
            if first is None:
                first = res
            assert as_bytes(res) == as_bytes(first), (what, mem, rep, "the bytes differ")
    return first


def state_tuple(s):
    return tuple(getattr(s, f) for f, _ in s._fields_)


def check(api, keys, x, y=None, stats=None, lens=None, offsets=None, what=""):
    """Four identical runs held to the model.  -> (result, worst error / bound over finite groups)."""
    names = R.COSTATS if y is not None else R.STATS
    stats = names if stats is None else stats
    exp_rows, exp_counts, vals, _ = R.group_moments_ref([ref_col(k) for k in keys], x, y)
    groups, rows, outs, counts, states = res = four_runs(api, keys, x, y, stats, lens, offsets, what)
    assert groups == len(exp_rows), (what, groups, len(exp_rows))
    assert rows.dtype == np.uint32 and np.array_equal(rows, exp_rows), (what, "group rows")
    assert counts.dtype == np.int64 and np.array_equal(counts, exp_counts), (what, "counts")
    assert [s.count for s in states] == exp_counts.tolist(), (what, "state counts")
    worst, where = 0.0, None
    for g in range(groups):
        v = vals[g]
        got = {name: (float(outs[c][0][g]) if outs[c][1][g] else None) for c, name in enumerate(stats)}
        for c in range(len(stats)):
            assert outs[c][1][g] or outs[c][0][g] == 0.0, (what, g, "the value under a NULL is 0")
        finite = np.isfinite(v).all() if y is None else (np.isfinite(v[0]).all() and np.isfinite(v[1]).all())
        if exp_counts[g] == 0:
            assert all(t is None for t in got.values()), (what, g, got)
            assert bytes(states[g]) == bytes(C.sizeof(states[g])), (what, g, "the zero state")
        elif not finite:
            assert all(t is not None and math.isnan(t) for t in got.values()), (what, g, got)
        else:
            ref = R.moments_ref_of(v) if y is None else R.comoments_ref_of(*v)
            e, name = R.errors_in_bounds(got, ref, stats)
            assert e <= 1.0, (what, "group", g, "count", int(exp_counts[g]), name, e)
            if e > worst:
                worst, where = e, (g, name)
    print(f"{what}: groups {groups}, worst error / bound {worst:.3f} at {where}")
    return res, worst


def layout_keys(layout, n, rng):
    if layout == "one_group":
        return [(np.full(n, 7, dtype=np.int64),)]
    if layout == "own_group":
        return [(rng.permutation(np.arange(n, dtype=np.int64)) - n // 2,)]
    return []


# ---------------------------------------------------------------- shapes around the wave and the tile

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
@pytest.mark.parametrize("layout", ["one_group", "own_group", "no_keys"])
def test_row_counts_and_layouts(api, n, layout):
    rng = np.random.default_rng(n * 3 + len(layout))
    x = (M.make_input("offset_1e9", n, seed=n),)
    res, _ = check(api, layout_keys(layout, n, rng), x, what=(layout, n))
    assert res[0] == (n if layout == "own_group" else 1)
    y = (3.0 * x[0] + M.make_input("normal", n, seed=n + 1),)
    check(api, layout_keys(layout, n, rng), x, y, what=(layout, n, "pair"))


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_a_group_of_whole_tiles_between_one_row_groups(api, k, shift):
    """Single-row groups up to position k T + shift, then one group over 2 T rows, then single-row groups again."""
    start = k * T + shift
    sizes = [1] * start + [2 * T] + [1] * 5
    key = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    n = len(key)
    p = np.random.default_rng(start).permutation(n)
    x = M.make_input("two_pow_52", n, seed=start)
    res, _ = check(api, [(key[p],)], (x[p],), what=("whole tiles", k, shift))
    assert res[0] == len(sizes) and res[3][start] == 2 * T


@pytest.mark.parametrize("layout", ["one_group", "long_and_one_row"])
def test_three_levels_of_partials(api, layout):
    n = 2 * T * T + 77
    assert len(R.levels_of(n)) == 3
    rng = np.random.default_rng(11)
    x = rng.integers(-511, 512, n).astype(np.int16)
    y = (rng.integers(-200, 200, n) + x // 2).astype(np.int32)
    if layout == "one_group":
        key = np.zeros(n, dtype=np.int64)
    else:                                        # long groups of unequal length, each followed by a one-row group
        sizes, left = [], n
        while left > 95 * T:
            sizes += [int(rng.integers(5 * T, 90 * T)), 1]
            left -= sizes[-2] + 1
        sizes += [left - 1, 1]
        key = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    p = rng.permutation(n)
    res, _ = check(api, [(key[p],)], (x[p],), what=("three levels", layout))
    assert "2 x gm_fold_kernel" in lib.last_kernel()
    check(api, [(key[p],)], (x[p],), (y[p],), what=("three levels", layout, "pair"))


# ---------------------------------------------------------------- dtypes, NULLs, keys

def column_of(dt, n, rng):
    if np.dtype(dt).kind == "f":
        return (1e3 + rng.standard_normal(n)).astype(dt)
    info = np.iinfo(dt)
    if info.bits == 64:                          # beyond 2^53: `as f64` rounds, the model is held to the converted values
        return rng.integers(max(info.min, -2**62), 2**62, n, dtype=np.int64).astype(dt) if dt == np.int64 else \
            (rng.integers(0, 2**62, n, dtype=np.int64).astype(np.uint64) * np.uint64(3) + np.uint64(1))
    return rng.integers(info.min, int(info.max) + 1, n, dtype=np.int64).astype(dt)


@pytest.mark.parametrize("dt", NUMERIC, ids=lambda d: np.dtype(d).name)
def test_every_dtype_as_f64(api, dt):
    n = 2 * T + 9
    rng = np.random.default_rng(np.dtype(dt).num)
    key = (rng.integers(0, 5, n).astype(np.int32),)
    x = (column_of(dt, n, rng), rng.random(n) >= 0.1)
    if np.dtype(dt).itemsize == 8 and np.dtype(dt).kind in "iu":
        assert (np.abs(x[0].astype(np.float64)) > 2.0**53).any()
    check(api, [key], x, what=("dtype", np.dtype(dt).name))
    other = NUMERIC[(NUMERIC.index(dt) + 3) % len(NUMERIC)]          # pairs of differing dtypes
    y = (column_of(other, n, rng), rng.random(n) >= 0.1)
    check(api, [key], x, y, what=("dtype pair", np.dtype(dt).name, np.dtype(other).name))


def test_nulls_and_an_all_null_group(api):
    n = 3 * T + 5
    rng = np.random.default_rng(21)
    key = rng.integers(0, 6, n).astype(np.int64)
    xv, yv = M.make_input("offset_1e9", n), M.make_input("lognormal", n)
    xok, yok = rng.random(n) >= 0.1, rng.random(n) >= 0.1
    xok[key == 2] = False                                            # group 2: nothing counts
    (groups, rows, outs, counts, states), _ = check(api, [(key,)], (xv, xok), what="nulls")
    assert counts[2] == 0 and all(not ok[2] and v[2] == 0.0 for v, ok in outs) and bytes(states[2]) == bytes(48)
    (groups, rows, outs, counts, states), _ = check(api, [(key,)], (xv, xok), (yv, yok), what="nulls, pair")
    assert counts[2] == 0 and bytes(states[2]) == bytes(64) and not (xok == yok).all()
    assert counts.tolist() == [int((xok & yok & (key == g)).sum()) for g in range(6)]
    yok2 = yok.copy()
    yok2[key == 4] = ~xok[key == 4]                                  # every row of group 4 lacks one of the two
    (_, _, outs, counts, states), _ = check(api, [(key,)], (xv, xok), (yv, yok2), what="nulls, disjoint pair")
    assert counts[4] == 0 and bytes(states[4]) == bytes(64)


def test_null_keys_come_last(api):
    n = T + 40
    rng = np.random.default_rng(22)
    key = (rng.integers(-3, 3, n).astype(np.int16), rng.random(n) >= 0.2)
    x = (M.make_input("uniform", n),)
    (groups, rows, _, counts, _), _ = check(api, [key], x, what="null keys")
    assert groups == 7 and not key[1][rows[-1]] and key[1][rows[:-1]].all() and counts[-1] == int((~key[1]).sum())


@pytest.mark.parametrize("nkeys", [1, 2, 3, 4])
def test_mixed_keys(api, nkeys):
    n = 2 * T + 31
    rng = np.random.default_rng(30 + nkeys)
    floats = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.5])
    words = ["", "a", "ab", "b", "é", None]
    pool = [(floats[rng.integers(0, 6, n)], rng.random(n) >= 0.1),
            ([words[i] for i in rng.integers(0, 6, n)],),
            (rng.integers(-2, 2, n).astype(np.int8), rng.random(n) >= 0.1),
            (rng.integers(0, 3, n).astype(np.uint64), rng.random(n) >= 0.1)]
    x = (M.make_input("offset_1e15", n), rng.random(n) >= 0.05)
    (groups, *_), _ = check(api, pool[:nkeys], x, what=("mixed keys", nkeys))
    assert groups > 5
    check(api, pool[:nkeys][::-1], x, (M.make_input("normal", n),), what=("mixed keys reversed, pair", nkeys))


@pytest.mark.parametrize("name", M.ILL + M.HARD)
def test_ill_conditioned_inputs_inside_groups(api, name):
    sizes = [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]
    key = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    n = len(key)
    p = np.random.default_rng(len(name)).permutation(n)
    x = M.make_input(name, n)
    check(api, [(key[p],)], (x[p],), what=("ill", name))
    check(api, [(key[p],)], (x[p],), (2.0 * x[p] + M.make_input("normal", n, seed=3),), what=("ill pair", name))


# ---------------------------------------------------------------- absent and non-finite statistics

def test_constant_and_one_row_groups(api):
    sizes = [3 * T + 5, 1, T, 2]
    key = np.repeat(np.arange(4, dtype=np.int64), sizes)
    x = M.make_input("offset_1e9", len(key))
    x[key == 0] = 0.1                                                # a constant group over four tiles
    x[key == 3] = -7.25                                              # ... and one of two rows
    (_, _, outs, counts, states), _ = check(api, [(key,)], (x,), what="constant and one-row groups")
    o = dict(zip(R.STATS, outs))
    for g in (0, 3):
        assert states[g].m2 == 0.0 and states[g].m3 == 0.0 and states[g].m4 == 0.0
        assert o["var_pop"][0][g] == 0.0 and o["var_samp"][0][g] == 0.0 and o["stddev_samp"][0][g] == 0.0 and o["var_samp"][1][g]
        assert not o["skewness"][1][g] and not o["kurtosis"][1][g]
    assert o["mean"][0][0] == 0.1 and o["mean"][0][3] == -7.25
    assert o["var_pop"][1][1] and o["var_pop"][0][1] == 0.0 and o["stddev_pop"][0][1] == 0.0          # one row
    assert not o["var_samp"][1][1] and not o["stddev_samp"][1][1] and not o["skewness"][1][1] and not o["kurtosis"][1][1]
    assert o["skewness"][1][2] and o["kurtosis"][1][2]
    nulls = [int((~ok).sum()) for _, ok in outs]
    assert nulls == [0, 0, 1, 0, 1, 3, 3]
    y = M.make_input("normal", len(key))
    (_, _, outs, _, _), _ = check(api, [(key,)], (x,), (y,), what="constant x in a pair")
    o = dict(zip(R.COSTATS, outs))
    assert not o["corr"][1][0] and not o["corr"][1][1] and not o["corr"][1][3] and o["corr"][1][2]
    assert o["covar_pop"][0][0] == 0.0 and not o["covar_samp"][1][1] and o["covar_pop"][1][1]


def test_null_counts_are_reported(api):
    key = np.repeat(np.arange(5, dtype=np.int64), [1, 1, 4, 1, 3])
    x = np.arange(10, dtype=np.float64)
    for mem in MEMS:
        _, _, outs, _, _ = run(api, [(key,)], (x,), None, ["var_samp", "mean", "skewness"], mem, raw=True)
        assert [o.null_count for o in outs] == [3, 0, 3] and [o.length for o in outs] == [5, 5, 5]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_makes_its_group_nan_and_no_other(api, bad):
    sizes = [T + 3, 2 * T, 5]
    key = np.repeat(np.arange(3, dtype=np.int64), sizes)
    x = M.make_input("normal", len(key))
    x[T + 3 + T + 1] = bad                                           # inside group 1, in its second tile
    (_, _, outs, counts, _), _ = check(api, [(key,)], (x,), what=("non-finite", bad))
    assert all(ok[1] and math.isnan(v[1]) for v, ok in outs) and counts[1] == 2 * T
    assert all(ok[0] and ok[2] and math.isfinite(v[0]) and math.isfinite(v[2]) for v, ok in outs)
    check(api, [(key,)], (M.make_input("uniform", len(key)),), (x,), what=("non-finite y", bad))


def test_all_three_non_finite_values_in_one_group(api):
    key = np.repeat(np.arange(3, dtype=np.int64), [4, 6, 4])
    x = M.make_input("normal", len(key))
    x[4:7] = [np.nan, np.inf, -np.inf]
    (_, _, outs, _, _), _ = check(api, [(key,)], (x,), what="nan, +inf, -inf")
    assert all(ok.all() and math.isnan(v[1]) and math.isfinite(v[0]) and math.isfinite(v[2]) for v, ok in outs)


# ---------------------------------------------------------------- what must not change a byte, and what may

def test_seven_unequal_chunks_behind_offsets_give_the_bytes_of_one_chunk(api):
    n = 3 * T + 5
    rng = np.random.default_rng(40)
    lens = [1, 70, 0, T, 2 * T - 100, 33, 0]
    lens[-1] = n - sum(lens)
    keys = [(rng.integers(0, 9, n).astype(np.int32), rng.random(n) >= 0.1), ([["x", "yy", None][i] for i in rng.integers(0, 3, n)],)]
    x = (M.make_input("offset_1e9", n), rng.random(n) >= 0.1)
    y = (M.make_input("exponential", n).astype(np.float32), rng.random(n) >= 0.1)
    for yy in (None, y):
        one, _ = check(api, keys, x, yy, what=("one chunk", yy is not None))
        seven = four_runs(api, keys, x, yy, R.COSTATS if yy is not None else R.STATS, lens, OFFSETS, "seven chunks")
        assert as_bytes(seven) == as_bytes(one)


def test_a_shuffle_keeps_counts_and_stays_inside_the_bounds(api):
    n = 3 * T + 5
    rng = np.random.default_rng(41)
    key = rng.integers(0, 4, n).astype(np.int64)
    x, ok = M.make_input("offset_1e9", n), rng.random(n) >= 0.1
    (_, _, _, counts, _), _ = check(api, [(key,)], (x, ok), what="rows in order")
    p = rng.permutation(n)
    (_, _, _, counts2, _), _ = check(api, [(key[p],)], (x[p], ok[p]), what="rows shuffled")
    assert np.array_equal(counts, counts2)


def test_the_columns_are_the_host_statistics_of_the_states(api):
    """outs[c] == rdf_moments_stat / rdf_comoments_stat applied on the host to out_states, bit for bit: f64 division and
    square root round correctly on the device under the project's flags."""
    n = 3 * T + 5
    rng = np.random.default_rng(42)
    key = rng.integers(0, 40, n).astype(np.int64)
    key[:3] = [100, 101, 101]                                        # a one-row and a two-row group
    x = (M.make_input("lognormal", n), rng.random(n) >= 0.1)
    y = (M.make_input("offset_1e9", n),)
    for yy, names, stat in ((None, R.STATS, api.moments_stat), (y, R.COSTATS, api.comoments_stat)):
        (groups, _, outs, _, states), _ = check(api, [(key,)], x, yy, what=("host stat", yy is not None))
        differ = 0
        for c, name in enumerate(names):
            for g in range(groups):
                want = stat(states[g], name)
                assert (want is not None) == bool(outs[c][1][g]), (name, g)
                if want is not None and np.float64(want).tobytes() != outs[c][0][g].tobytes():
                    differ += 1
                    print("device", outs[c][0][g].hex(), "host", float(want).hex(), name, g)
        assert differ == 0


def test_two_shards_merged_group_by_group(api):
    n = 4 * T + 10
    rng = np.random.default_rng(43)
    key = rng.integers(0, 5, n).astype(np.int64)
    key[:5] = key[n // 2:n // 2 + 5] = np.arange(5)                  # every key in both shards
    x, y = M.make_input("offset_1e9", n), M.make_input("two_clusters", n)
    h = n // 2
    for pair in (False, True):
        a = run(api, [(key[:h],)], (x[:h],), (y[:h],) if pair else None, [], "device")
        b = run(api, [(key[h:],)], (x[h:],), (y[h:],) if pair else None, [], "host")
        assert a[0] == b[0] == 5
        worst = 0.0
        for g in range(5):
            merged = api.moments_merge(a[4][g], b[4][g])
            sel = key == g
            if pair:
                got = {s: api.comoments_stat(merged, s) for s in R.COSTATS}
                e, name = R.errors_in_bounds(got, M.ComomentsRef(x[sel], y[sel]), R.COSTATS)
            else:
                got = {s: api.moments_stat(merged, s) for s in R.STATS}
                e, name = R.errors_in_bounds(got, M.MomentsRef(x[sel]), R.STATS)
            assert merged.count == int(sel.sum()) and e <= 1.0, (pair, g, name, e)
            worst = max(worst, e)
        print("two shards, pair" if pair else "two shards", "worst error / bound", worst)


def test_group_rows_are_the_sorted_group_bys(api):
    n = 3 * T + 5
    rng = np.random.default_rng(44)
    keys = [(rng.integers(-4, 4, n).astype(np.int32), rng.random(n) >= 0.1), ([["p", "q", "", None][i] for i in rng.integers(0, 4, n)],)]
    x = (M.make_input("normal", n),)
    for mem in MEMS:
        ch = [chunks_of(k, [n], [0], mem) for k in keys]
        want_groups, want_rows, _ = api.groupby_sorted(ch, None, [])
        got = run(api, keys, x, None, ["var_samp"], mem)
        assert got[0] == want_groups and got[1].tobytes() == want_rows.tobytes()
        only = run(api, keys, None, None, [], mem)                   # the key tuples alone
        assert only[0] == want_groups and only[1].tobytes() == want_rows.tobytes() and only[3] is None and only[4] is None
        assert run(api, keys, None, None, [], mem, group_rows=False)[0] == want_groups       # the count-only call
        assert "gm_" not in lib.last_kernel() and "win_starts_kernel" in lib.last_kernel()


def test_counts_or_states_alone(api):
    key = (np.array([2, 1, 2, 1, 2], dtype=np.int64),)
    x = (np.array([1.0, 2.0, 3.0, 4.0, 5.0]), np.array([1, 1, 0, 1, 1], dtype=bool))
    for mem in MEMS:
        groups, rows, outs, counts, states = run(api, [key], x, None, [], mem, group_rows=False)
        assert groups == 2 and rows is None and outs == [] and counts.tolist() == [2, 2]
        assert [state_tuple(s) for s in states] == [(2, 3.0, 0.0, 2.0, 0.0, 2.0), (2, 3.0, 0.0, 8.0, 0.0, 32.0)]
        assert "gm_level0_kernel" in lib.last_kernel() and "gm_finish_kernel" in lib.last_kernel()


@pytest.mark.parametrize("mem", MEMS)
def test_short_capacities_report_the_groups_and_write_nothing(api, mem):
    n, G = 50, 10
    key = [chunks_of((np.arange(n, dtype=np.int64) % G,), [n], [0], mem)]
    x = chunks_of((np.arange(n, dtype=np.float64),), [n], [0], mem)
    device = mem == "device"

    def buffers(short):
        caps = [G - 1 if short == i else G for i in range(3)]
        outs = [api._window_out(A.F64, caps[0], device, True)]
        rows_out = api._window_out(A.U32, caps[1], device, False)
        counts_out = api._window_out(A.I64, caps[2], device, False)
        for o in (outs[0], rows_out, counts_out):
            if device:
                o.keep[0].fill_(0x4D4D4D4D4D4D4D4D)
            else:
                o.values.view(np.uint8)[:] = 0x4D
        return outs, rows_out, counts_out

    def untouched(o):
        raw = o.keep[0].cpu().numpy().view(np.uint8) if device else o.values.view(np.uint8)
        return bool((raw == 0x4D).all())

    for short in range(4):
        outs, rows_out, counts_out = buffers(short)
        with pytest.raises(A.RdfError) as ei:
            api.groupby_moments(key, x, stats=["var_samp"], states=True, outs=outs, rows_out=rows_out, counts_out=counts_out,
                                states_capacity=G - 1 if short == 3 else G, raw=True)
        assert ei.value.status == A.RDF_MEMORY_ERROR
        assert api.last_groups == G and outs[0].length == G and rows_out.length == G and counts_out.length == G
        assert untouched(outs[0]) and untouched(rows_out) and untouched(counts_out)
    outs, rows_out, counts_out = buffers(-1)                         # exactly G everywhere is enough
    groups, _, _, _, states = api.groupby_moments(key, x, stats=["var_samp"], states=True, outs=outs, rows_out=rows_out, counts_out=counts_out,
                                                  states_capacity=G, raw=True)
    assert groups == G and len(states) == G and all(s.count == 5 for s in states)
