"""rdf_groupby_sorted on the MI355X: count_distinct / sum_distinct / first / last per group, held to
tests/group_sorted_ref.py.  Counts, integer sums, group rows and row indices are compared bit for bit; a Float64 sum is
held to the bound of ANY summation order over the m distinct finite values of its group,
|got - exact| <= gamma(m - 1) * sum|v| (exact_ref.gamma; exact where m <= 1), and to IEEE exactly where it is not finite.
The head-list cases place the group boundaries around the multiples of the fold's tile T (A.GROUP_SORTED_TILE)."""
import math

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
import exact_ref
import group_sorted_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = A.GROUP_SORTED_TILE
MEMS = ["host", "device"]
ALL = ["count_distinct", "sum_distinct", "first", "last", ("first", 1), ("last", 1)]
NOSUM = ["count_distinct", "first", "last", ("first", 1), ("last", 1)]
NUMERIC = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64]


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


def rows_of(col):
    return len(col[0])


def chunks_of(col, lens, odd, mem):
    out, at = [], 0
    for i, ln in enumerate(lens):
        if is_text(col):
            c = A.HostUtf8.from_pylist(col[0][at:at + ln], (5 + 3 * i) % 13 if odd else 0, (7 * i) % 9 if odd else 0)
            out.append(A.DeviceUtf8.from_host(c) if mem == "device" else c)
        else:
            valid = col[1] if len(col) > 1 else None
            c = A.HostArray.from_numpy(col[0][at:at + ln], None if valid is None else valid[at:at + ln], offset=(3 + 2 * i) % 11 if odd else 0)
            if mem == "device":
                vt = torch.from_numpy(np.ascontiguousarray(c.values)).cuda()
                bt = torch.from_numpy(np.ascontiguousarray(c.validity)).cuda() if c.validity is not None else None
                c = A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, c.offset, c.length, c.dtype, c.null_count, keep=(vt, bt))
            out.append(c)
        at += ln
    return out


def run(api, keys, value, calls, mem="host", lens=None, odd=False, group_rows=True):
    cols = list(keys) + ([value] if value is not None else [])
    n = rows_of(cols[0])
    lens = [n] if lens is None else lens
    assert sum(lens) == n
    ch = [chunks_of(c, lens, odd, mem) for c in cols]
    if mem == "device":
        torch.cuda.synchronize()
    return api.groupby_sorted(ch[:len(keys)], ch[len(keys)] if value is not None else None, calls, group_rows=group_rows)


def ref_col(col):
    if is_text(col):
        return ([None if r is None else r.encode() for r in col[0]],)
    return col


def reference(keys, value, calls):
    return R.group_sorted_ref([ref_col(k) for k in keys], None if value is None else ref_col(value), calls, with_terms=True)


def same(got, exp, terms=None):
    """One call's result against the reference's: bit for bit, but a Float64 sum within the any-order bound."""
    if isinstance(exp, tuple):
        return got[0].dtype == np.uint32 and np.array_equal(got[1], exp[1]) and np.array_equal(got[0][exp[1]], exp[0][exp[1]])
    if got.dtype != exp.dtype or got.shape != exp.shape:
        return False
    if exp.dtype != np.float64:
        return np.array_equal(got, exp)
    for g, e, m, sabs in zip(got.tolist(), exp.tolist(), terms["m"].tolist(), terms["sum_abs"].tolist()):
        if not math.isfinite(e):
            if not (math.isnan(g) if math.isnan(e) else g == e):
                return False
        elif not abs(g - e) <= (exact_ref.gamma(m - 1) * sabs if m > 1 else 0.0) or (g == 0 and math.copysign(1, g) < 0):
            return False
    return True


def check(api, keys, value, calls=ALL, lens=None, odd=False, mems=MEMS, what=""):
    exp_rows, exp, terms = reference(keys, value, calls)
    for mem in mems:
        groups, rows, got = run(api, keys, value, calls, mem, lens, odd)
        assert groups == len(exp_rows), (what, mem, groups, len(exp_rows))
        assert rows.dtype == np.uint32 and np.array_equal(rows, exp_rows), (what, mem, "group rows")
        for c, (g, e) in enumerate(zip(got, exp)):
            assert same(g, e, terms), (what, mem, calls[c])
    return exp_rows, exp


def expand(rng, keys_per_head, vals_per_head, null_heads):
    """Rows from a head list: every head 1 .. 3 times, the rows shuffled.  -> (key column, value column)"""
    reps = rng.integers(1, 4, len(keys_per_head))
    k = np.repeat(np.asarray(keys_per_head, dtype=np.int64), reps)
    v = np.repeat(np.asarray(vals_per_head, dtype=np.int64), reps)
    ok = ~np.repeat(np.asarray(null_heads, dtype=bool), reps)
    p = rng.permutation(len(k))
    return (k[p],), (v[p], ok[p])


# ---------------------------------------------------------------- the head list around the fold's tile

@pytest.mark.parametrize("D", [1, T - 1, T, T + 1, 3 * T + 5])
@pytest.mark.parametrize("layout", ["one_group", "own_group", "no_keys"])
def test_head_list_shapes(api, D, layout):
    rng = np.random.default_rng(D * 7 + len(layout))
    vals = rng.permutation(np.arange(-D, 2 * D, dtype=np.int64))[:D] * 1_000_003
    nulls = np.zeros(D, dtype=bool)
    if layout == "own_group":
        keys = rng.permutation(np.arange(D, dtype=np.int64)) - D // 2
        nulls[rng.integers(0, D)] = True                      # one group has nothing but NULL values
    else:
        keys = np.zeros(D, dtype=np.int64)
        if D > 1:
            nulls[D - 1] = True                               # the group's NULL run is its last head
    key, value = expand(rng, keys, vals, nulls)
    exp_rows, _ = check(api, [] if layout == "no_keys" else [key], value, what=(layout, D))
    assert len(exp_rows) == (D if layout == "own_group" else 1)


def test_a_group_that_spans_whole_tiles_between_single_head_groups(api):
    # heads: 40 groups of one, then ONE group from the middle of tile 0 over tiles 1 and 2 into tile 3, then 3 groups of one
    rng = np.random.default_rng(5)
    D, before, after = 3 * T + 5, 40, 3
    big = D - before - after
    keys = np.concatenate([np.arange(before), np.full(big, before), before + 1 + np.arange(after)]).astype(np.int64)
    vals = rng.permutation(np.arange(4 * D, dtype=np.int64))[:D] - D
    nulls = np.zeros(D, dtype=bool)
    nulls[before + big - 1] = True
    key, value = expand(rng, keys, vals, nulls)
    exp_rows, exp = check(api, [key], value, what="spanning group")
    assert len(exp_rows) == before + 1 + after and exp[0][before] == big - 1
    fvalue = (value[0].astype(np.float64) * 0.1, value[1])    # the same heads with a Float64 sum carried across the tiles
    check(api, [key], fvalue, what="spanning group, Float64")


def test_three_levels_of_partials(api):
    # 2^17 rows, each its own pair: 512 tiles, then 1024 partial items in 4 tiles, then 8 items; groups of 1 .. 3000 heads
    rng = np.random.default_rng(6)
    n = 1 << 17
    sizes = rng.integers(1, 3000, 200)
    keys = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)[:n]
    keys = np.concatenate([keys, np.arange(n - len(keys), dtype=np.int64) + 1000])
    vals = rng.permutation(n).astype(np.int64) - n // 3
    ok = rng.random(n) > 0.01
    p = rng.permutation(n)
    check(api, [(keys[p],)], (vals[p], ok[p]), mems=["device"], what="three levels")


# ---------------------------------------------------------------- value dtypes

@pytest.mark.parametrize("dtype", NUMERIC, ids=lambda d: np.dtype(d).name)
def test_every_numeric_value_dtype(api, dtype):
    rng = np.random.default_rng(np.dtype(dtype).num)
    n = 3001
    key = (rng.integers(-20, 20, n).astype(np.int64), rng.random(n) > 0.05)
    if np.dtype(dtype).kind == "f":
        pool = np.concatenate([rng.standard_normal(60) * 1e3, [0.0, -0.0, math.nan, -math.nan, math.inf, 1e30, -1e30]]).astype(dtype)
        vals = pool[rng.integers(0, len(pool), n)]
        vals[key[0] == 3] = np.abs(vals[key[0] == 3])         # (a group without -inf next to +inf)
    else:
        info = np.iinfo(dtype)
        pool = np.concatenate([rng.integers(info.min, info.max, 60, dtype=dtype, endpoint=True), np.array([info.min, info.max, 0], dtype=dtype)])
        vals = pool[rng.integers(0, len(pool), n)]
    value = (vals, rng.random(n) > 0.2)
    value[1][key[0] == 7] = False                             # an all-NULL group
    check(api, [key], value, lens=[1000, 0, 2001], odd=True, what=np.dtype(dtype).name)


def test_utf8_values_and_the_refusal_of_their_sum(api):
    rng = np.random.default_rng(11)
    n = 2000
    long_a, long_b = "x" * 640 + "a", "x" * 640 + "b"         # 600 bytes or more: compared by a whole wave
    pool = ["", "a", "a\0", "ab", "b", "zebra", long_a, long_b, "x" * 640, None, None]
    vals = [pool[i] for i in rng.integers(0, len(pool), n)]
    key = (rng.integers(0, 30, n).astype(np.int64),)
    for g in np.flatnonzero(key[0] == 4):
        vals[g] = None                                        # an all-NULL group
    for g in np.flatnonzero(key[0] == 5):
        vals[g] = ""                                          # the empty string is a value
    check(api, [key], (vals,), calls=NOSUM, lens=[700, 1300], odd=True, what="utf8")
    for mem in MEMS:
        with pytest.raises(A.RdfError) as ei:
            run(api, [key], (vals,), ["sum_distinct"], mem)
        assert ei.value.status == A.RDF_INVALID_ARGUMENT


def test_first_and_last_of_a_column_without_validity_need_no_bitmap(api):
    key = (np.array([2, 1, 2, 1, 2], dtype=np.int64),)
    k = chunks_of(key, [5], False, "host")
    v = chunks_of((np.array([5, 6, 7, 8, 9], dtype=np.int32),), [5], False, "host")
    outs = [A.HostArray.empty_out(A.U32, 5, False) for _ in range(2)]
    groups, rows, outs = api.groupby_sorted([k], v, [("first", 1), ("last", 1)], outs=outs, raw=True)
    assert groups == 2 and outs[0].values[:2].tolist() == [1, 0] and outs[1].values[:2].tolist() == [3, 4]
    assert outs[0].null_count == 0 and outs[1].null_count == 0


# ---------------------------------------------------------------- keys

def mixed_keys(rng, n):
    k0 = (rng.integers(-3, 3, n).astype(np.int32), rng.random(n) > 0.1)
    words = ["", "a", "ab", "b", "y" * 700, None]
    k1 = ([words[i] for i in rng.integers(0, len(words), n)],)
    fpool = np.array([-0.0, 0.0, math.nan, -math.nan, math.inf, -math.inf, 1.5])
    k2 = (fpool[rng.integers(0, len(fpool), n)], rng.random(n) > 0.1)
    return [k0, k1, k2]


def test_mixed_keys_with_nulls_in_each(api):
    rng = np.random.default_rng(21)
    n = 2500
    keys = mixed_keys(rng, n)
    value = (rng.integers(0, 9, n).astype(np.int64), rng.random(n) > 0.3)
    check(api, keys, value, lens=[1200, 1300], odd=True, what="int32 + utf8 + float64")
    k3 = (rng.integers(0, 2, n).astype(np.uint8),)
    check(api, keys + [k3], value, what="four keys")


def test_a_float64_key_holding_zeros_nans_and_infinity(api):
    key = (np.array([-0.0, 0.0, math.nan, -math.nan, math.inf, 0.0, math.nan, 2.0]),)
    value = (np.array([1, 2, 3, 4, 5, 1, 3, 9], dtype=np.int64),)
    exp_rows, exp = check(api, [key], value, what="float key")
    assert exp_rows.tolist() == [0, 7, 4, 2] and exp[0].tolist() == [2, 1, 1, 2] and exp[1].tolist() == [3, 9, 5, 7]


def test_group_rows_gather_back_to_the_keys(api):
    rng = np.random.default_rng(22)
    n = 1500
    k0 = (rng.integers(-50, 50, n).astype(np.int64), rng.random(n) > 0.1)
    k1 = ([["", "p", "q", None][i] for i in rng.integers(0, 4, n)],)
    groups, rows, _ = run(api, [k0, k1], None, [])
    idx = A.HostArray.from_numpy(rows)
    got0 = api.take(chunks_of(k0, [n], False, "host"), idx).to_pylist()
    got1 = api.utf8_take(chunks_of(k1, [n], False, "host"), idx, as_arrow="pylist")
    tuples = list(zip(got0, got1))
    want = sorted({(None if not o else int(v), s) for v, o, s in zip(k0[0], k0[1], k1[0])},
                  key=lambda t: (t[0] is None, t[0] or 0, t[1] is None, t[1] or ""))
    assert groups == len(want) and tuples == want


# ---------------------------------------------------------------- Float64 sums

def test_float_sums_stay_within_the_bound_of_any_order(api):
    rng = np.random.default_rng(31)
    n = 6000
    vals = np.ldexp(rng.standard_normal(n), rng.integers(-20, 20, n))          # 40 binades
    key = rng.integers(0, 12, n).astype(np.int64)
    vals[:3], key[:3] = [1e16, -1e16, 1.0], 100                                  # exact answer 1.0, bound 2e16 * gamma(2)
    vals[3:6], key[3:6] = [1e16, -1e16, 1.0], 0                                  # ... and among 500 others
    dup = rng.integers(0, n, n // 2)
    vals, key = np.concatenate([vals, vals[dup]]), np.concatenate([key, key[dup]])
    check(api, [(key,)], (vals,), calls=["sum_distinct", "count_distinct"], what="40 binades")
    check(api, [], (vals,), calls=["sum_distinct"], what="40 binades, one group")


def test_non_finite_sums_follow_ieee(api):
    inf, nan = math.inf, math.nan
    key = (np.array([0, 0, 1, 1, 2, 2, 3, 3, 3, 4, 4], dtype=np.int64),)
    value = (np.array([inf, 1.0, inf, -inf, -inf, -inf, nan, 1.0, inf, -0.0, 0.0]),)
    for mem in MEMS:
        _, _, (s, c) = run(api, [key], value, ["sum_distinct", "count_distinct"], mem)
        assert s[0] == inf and math.isnan(s[1]) and s[2] == -inf and math.isnan(s[3])
        assert s[4] == 0.0 and not np.signbit(s[4])                              # -0.0 / +0.0 count once, as +0.0
        assert c.tolist() == [2, 2, 1, 3, 1]


# ---------------------------------------------------------------- invariance: bytes equal

def raw_bytes(res):
    groups, rows, outs = res
    parts = [rows.tobytes()]
    for o in outs:
        parts += [o[0].tobytes(), o[1].tobytes()] if isinstance(o, tuple) else [o.tobytes()]
    return groups, parts


def test_chunking_memory_kind_and_repetition_change_no_byte(api):
    rng = np.random.default_rng(41)
    n = 5000
    key = (rng.integers(0, 40, n).astype(np.int64), rng.random(n) > 0.05)
    value = (np.ldexp(rng.standard_normal(n), rng.integers(-30, 30, n)).round(3), rng.random(n) > 0.1)
    value[0][rng.integers(0, n, n // 3)] = value[0][rng.integers(0, n, n // 3)]
    base = raw_bytes(run(api, [key], value, ALL, "host"))
    seven = [700, 1, 0, 1999, 300, 1500, 500]
    assert raw_bytes(run(api, [key], value, ALL, "host")) == base                        # twice
    assert raw_bytes(run(api, [key], value, ALL, "host", lens=seven, odd=True)) == base  # 7 uneven chunks, one empty
    assert raw_bytes(run(api, [key], value, ALL, "device")) == base                      # device memory
    assert raw_bytes(run(api, [key], value, ALL, "device", lens=seven)) == base


def test_row_order_changes_no_byte(api):
    rng = np.random.default_rng(42)
    n = 5000
    key = (rng.integers(0, 40, n).astype(np.int64), rng.random(n) > 0.05)
    value = (np.ldexp(rng.standard_normal(n), rng.integers(-30, 30, n)).round(3), rng.random(n) > 0.1)
    g0, rows0, outs0 = run(api, [key], value, ALL, "device")
    p = rng.permutation(n)                                    # shuffled row i is original row p[i]
    g1, rows1, outs1 = run(api, [(key[0][p], key[1][p])], (value[0][p], value[1][p]), ALL, "device")
    assert g0 == g1
    assert outs0[0].tobytes() == outs1[0].tobytes() and outs0[1].tobytes() == outs1[1].tobytes()
    # first / last name rows by index, so they move with the shuffle: mapped back through it, the row a call names lies in
    # the same group as the row the unshuffled call names ...
    for a, b in zip(outs0[2:], outs1[2:]):
        assert np.array_equal(a[1], b[1])
        ra, rb = a[0][a[1]].astype(np.int64), p[b[0][b[1]].astype(np.int64)]
        assert np.array_equal(key[1][ra], key[1][rb]) and np.array_equal(key[0][ra][key[1][ra]], key[0][rb][key[1][rb]])
    # ... and it is the smallest / largest index of the shuffled rows, as the reference over the shuffled rows says
    exp_rows, exp, _ = reference([(key[0][p], key[1][p])], (value[0][p], value[1][p]), ALL)
    for c in range(2, 6):
        assert same(outs1[c], exp[c])
    assert np.array_equal(rows1, exp_rows)


# ---------------------------------------------------------------- against the library's other routes

def test_count_distinct_of_a_whole_column_equals_uniques(api):
    rng = np.random.default_rng(51)
    n = 20000
    cols = {"i64": (rng.integers(-3000, 3000, n).astype(np.int64), rng.random(n) > 0.1),
            "f64": (np.concatenate([rng.integers(-2000, 2000, n - 4) * 0.25, [0.0, -0.0, math.nan, -math.nan]]), rng.random(n) > 0.1)}
    words = [None] + ["w%d" % i for i in range(700)] + [""]
    text = ([words[i] for i in rng.integers(0, len(words), n)],)
    try:
        for route in (0, 1):
            lib.set_option("uniques_route", route)
            for name, col in cols.items():
                want = api.uniques(chunks_of(col, [n], False, "host"), count_only=True)
                _, _, (got,) = run(api, [], col, ["count_distinct"])
                assert got.tolist() == [want], (name, route)
            want = api.utf8_uniques(chunks_of(text, [n], False, "host")).length
            _, _, (got,) = run(api, [], text, ["count_distinct"])
            assert got.tolist() == [want], ("utf8", route)
    finally:
        lib.set_option("uniques_route", 0)


def test_count_distinct_equals_two_hash_groupbys_composed(api):
    rng = np.random.default_rng(52)
    n = 30000
    key = rng.integers(0, 300, n).astype(np.int64)
    val = rng.integers(0, 50, n).astype(np.int64)
    K, V = [A.HostArray.from_numpy(key)], [A.HostArray.from_numpy(val)]
    pk, _, _ = api.groupby_agg([K, V], None, "count", 300 * 50 + 8)               # the distinct (key, value) pairs
    pair_keys = pk[0].to_numpy().copy()
    ok, _, oc = api.groupby_agg([[A.HostArray.from_numpy(pair_keys)]], None, "count", 308)
    want = dict(zip(ok[0].to_numpy().tolist(), oc.to_numpy().tolist()))
    groups, rows, (got,) = run(api, [(key,)], (val,), ["count_distinct"])
    assert groups == len(want)
    assert got.tolist() == [want[int(k)] for k in key[rows]]


# ---------------------------------------------------------------- sizing

def test_short_capacities_report_the_groups_and_write_nothing(api):
    key = [A.HostArray.from_numpy(np.array([3, 1, 3, 2, 1, 9], dtype=np.int64))]
    val = [A.HostArray.from_numpy(np.array([5, 5, 6, 7, 5, 1], dtype=np.int64))]
    for short in range(3):
        outs = [A.HostArray.empty_out(A.I64, 8, False), A.HostArray.empty_out(A.U32, 8, True)]
        rows_out = A.HostArray.empty_out(A.U32, 8, False)
        arrs = outs + [rows_out]
        for a in arrs:
            a.values[:] = 77
        outs[1].validity[:] = 77
        arrs[short].length = 3                                                    # an output's capacity is its length; 4 groups
        with pytest.raises(A.RdfError) as ei:
            api.groupby_sorted([key], val, ["count_distinct", ("last", 1)], outs=outs, rows_out=rows_out, raw=True)
        assert ei.value.status == A.RDF_MEMORY_ERROR
        assert api.last_groups == 4 and [a.length for a in arrs] == [4, 4, 4]
        assert all((a.values == 77).all() for a in arrs) and (outs[1].validity == 77).all()
    groups, rows, res = api.groupby_sorted([key], None, [], group_rows=False)      # the count-only call
    assert groups == 4 and rows is None and res == []
    groups, rows, res = api.groupby_sorted([key], None, [])                        # the distinct tuples
    assert groups == 4 and rows.tolist() == [1, 3, 0, 5] and res == []
    groups, rows, res = api.groupby_sorted([key], val, ["sum_distinct"], group_rows=False)
    assert groups == 4 and rows is None and res[0].tolist() == [5, 7, 11, 1]
