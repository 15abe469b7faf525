"""rdf_groupby_percentile on the MI355X, held to tests/percentile_ref.py bit for bit: CONT results as the bits of their
Float64, DISC results as row indices, validity, counts and group rows.  Every call the select route can serve (no grouping
keys, a numeric value) runs on the sorted route AND on the select route, and the two outputs are compared byte for byte.
Group counts are placed around the pick kernel's block (A.PERCENTILE_PICK_BLOCK), row counts around the select route's tile
and finish threshold (A.PCT_SELECT_TILE, A.PCT_SELECT_FINISH)."""
import math

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
import percentile_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B = A.PERCENTILE_PICK_BLOCK
TILE, FINISH, BITS = A.PCT_SELECT_TILE, A.PCT_SELECT_FINISH, A.PCT_SELECT_BITS
MEMS = ["host", "device"]
NUMERIC = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64]
MIXED = ["median", ("cont", 0.0), ("cont", 1.0), ("cont", 0.9), ("disc", 0.0), ("disc", 0.5), ("disc", 1.0), ("disc", 0.31)]
DISCS = [("disc", 0.0), ("disc", 0.5), ("disc", 1.0), ("disc", 0.31)]


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    yield a
    lib.set_option("percentile_route", 0)


# ---------------------------------------------------------------- inputs: a column is (numpy values, valid | None) or
# ([str | None, ...],) for Utf8

def is_text(col):
    return not isinstance(col[0], np.ndarray)


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


def run(api, keys, value, calls, mem="host", lens=None, odd=False, route=0, counts=True):
    """-> (groups, group rows, [(value bits / rows, valid)], counts, the kernels that ran)"""
    cols = list(keys) + ([value] if value is not None else [])
    n = len(cols[0][0])
    lens = [n] if lens is None else lens
    assert sum(lens) == n
    ch = [chunks_of(c, lens, odd, mem) for c in cols]
    if mem == "device":
        torch.cuda.synchronize()
    lib.set_option("percentile_route", route)
    try:
        groups, rows, outs, cnt = api.groupby_percentile(ch[:len(keys)], ch[len(keys)] if value is not None else None, calls, counts=counts)
    finally:
        lib.set_option("percentile_route", 0)
    outs = [(v.view(np.uint64) if v.dtype == np.float64 else v, ok) for v, ok in outs]
    return groups, rows, outs, cnt, lib.last_kernel()


def ref_col(col):
    if is_text(col):
        return ([None if r is None else r.encode() for r in col[0]],)
    return col


def raw_bytes(res):
    groups, rows, outs, cnt, _ = res
    parts = [rows.tobytes(), cnt.tobytes()]
    for v, ok in outs:
        parts += [v.tobytes(), ok.tobytes()]
    return groups, parts


def select_eligible(keys, value):
    return not keys and value is not None and not is_text(value)


def check(api, keys, value, calls=MIXED, lens=None, odd=False, mems=MEMS, what=""):
    """Every memory kind, and every route the call can take, against the model; the routes against each other."""
    exp_rows, exp, exp_counts = R.percentile_ref([ref_col(k) for k in keys], ref_col(value), calls)
    routes = [1, 2] if select_eligible(keys, value) else [1]
    seen = []
    for mem in mems:
        for route in routes:
            res = run(api, keys, value, calls, mem, lens, odd, route)
            groups, rows, got, cnt, kernels = res
            tag = (what, mem, route)
            assert kernels.startswith("select:" if route == 2 else "sorted:"), (tag, kernels)
            assert groups == len(exp_rows), (tag, groups, len(exp_rows))
            assert rows.dtype == np.uint32 and np.array_equal(rows, exp_rows), (tag, "group rows")
            assert cnt.dtype == np.int64 and np.array_equal(cnt, exp_counts), (tag, "counts")
            for c, ((gv, gok), (ev, eok)) in enumerate(zip(got, exp)):
                assert gv.dtype == ev.dtype and np.array_equal(gok, eok), (tag, calls[c], "validity")
                assert np.array_equal(gv, ev), (tag, calls[c], [hex(int(x)) for x in gv[:4]], [hex(int(x)) for x in ev[:4]])
            seen.append(raw_bytes(res))
    assert all(s == seen[0] for s in seen), (what, "routes and memory kinds differ")
    return exp_rows, exp, exp_counts


def float_pool(dtype, rng, k=40):
    return np.concatenate([rng.standard_normal(k) * 1e3, [0.0, -0.0, math.nan, -math.nan, math.inf, -math.inf, 1e30, -1e30]]).astype(dtype)


# ---------------------------------------------------------------- the sorted route: dtypes

@pytest.mark.parametrize("validity", [True, False], ids=["nullable", "dense"])
@pytest.mark.parametrize("dtype", NUMERIC, ids=lambda d: np.dtype(d).name)
def test_every_numeric_value_dtype_per_group(api, dtype, validity):
    rng = np.random.default_rng(np.dtype(dtype).num + 100 * validity)
    n = 2003
    key = (rng.integers(-15, 15, n).astype(np.int64), rng.random(n) > 0.05)
    if np.dtype(dtype).kind == "f":
        pool = float_pool(dtype, rng)
    else:
        info = np.iinfo(dtype)
        pool = np.concatenate([rng.integers(info.min, info.max, 40, dtype=dtype, endpoint=True), np.array([info.min, info.max, 0], dtype=dtype)])
    vals = pool[rng.integers(0, len(pool), n)]
    if validity:
        ok = rng.random(n) > 0.2
        ok[key[0] == 7] = False                               # an all-NULL group
        value = (vals, ok)
    else:
        value = (vals,)
    _, _, counts = check(api, [key], value, lens=[1000, 0, 1003], odd=True, what=np.dtype(dtype).name)
    assert (counts == 0).any() == validity


@pytest.mark.parametrize("validity", [True, False], ids=["nullable", "dense"])
def test_utf8_values_take_disc_and_refuse_cont(api, validity):
    rng = np.random.default_rng(11 + validity)
    n = 1500
    long_a, long_b = "x" * 640 + "a", "x" * 640 + "b"
    pool = ["", "a", "a\0", "ab", "b", "zebra", "é", long_a, long_b, "x" * 640] + ([None, None] if validity else [])
    vals = [pool[i] for i in rng.integers(0, len(pool), n)]
    key = (rng.integers(0, 25, n).astype(np.int64),)
    if validity:
        for g in np.flatnonzero(key[0] == 4):
            vals[g] = None
    check(api, [key], (vals,), calls=DISCS, lens=[700, 800], odd=True, what="utf8 per group")
    check(api, [], (vals,), calls=DISCS, what="utf8 whole column")
    for mem in MEMS:
        with pytest.raises(A.RdfError) as ei:
            run(api, [key], (vals,), ["median"], mem)
        assert ei.value.status == A.RDF_INVALID_ARGUMENT


# ---------------------------------------------------------------- the sorted route: groups

def test_groups_of_one_and_two_rows_null_groups_and_a_null_key(api):
    key = (np.array([5, 3, 5, 9, 9, 1, 0, 0, 4], dtype=np.int32), np.array([1, 1, 1, 1, 1, 1, 0, 0, 1], dtype=bool))
    value = (np.array([2.0, 7.0, 4.0, 1.0, 1.0, 6.0, 8.0, 3.0, 5.0]), np.array([1, 1, 1, 0, 0, 0, 1, 1, 1], dtype=bool))
    rows, exp, counts = check(api, [key], value, what="small groups")
    assert rows.tolist() == [5, 1, 8, 0, 3, 6] and counts.tolist() == [0, 1, 1, 2, 0, 2]      # keys 1, 3, 4, 5, 9, NULL
    assert [R.from_bits(int(b)) for b in exp[0][0][[1, 3, 5]]] == [7.0, 3.0, 5.5]


def test_utf8_keys_and_four_keys(api):
    rng = np.random.default_rng(21)
    n = 1800
    k0 = (rng.integers(-3, 3, n).astype(np.int32), rng.random(n) > 0.1)
    words = ["", "a", "ab", "b", "y" * 700, None]
    k1 = ([words[i] for i in rng.integers(0, len(words), n)],)
    fpool = np.array([-0.0, 0.0, math.nan, -math.nan, math.inf, -math.inf, 1.5])
    k2 = (fpool[rng.integers(0, len(fpool), n)], rng.random(n) > 0.1)
    k3 = (rng.integers(0, 2, n).astype(np.uint8),)
    value = (rng.integers(-9, 9, n).astype(np.int64), rng.random(n) > 0.3)
    check(api, [k1], value, lens=[800, 1000], odd=True, what="utf8 key")
    check(api, [k0, k1, k2, k3], value, what="four keys")


@pytest.mark.parametrize("G", [1, B - 1, B, B + 1, 2 * B - 1, 2 * B + 1])
@pytest.mark.parametrize("ncalls", [1, 8])
def test_group_counts_around_the_pick_block(api, G, ncalls):
    # one thread per (group, call): G * ncalls threads, the last block full, short by one or over by one
    rng = np.random.default_rng(G * 10 + ncalls)
    sizes = rng.integers(1, 6, G)
    key = np.repeat(np.arange(G, dtype=np.int64) * 3 - G, sizes)
    n = len(key)
    p = rng.permutation(n)
    value = ((rng.standard_normal(n) * 100).round(1), rng.random(n) > 0.15)
    check(api, [(key[p],)], value, calls=MIXED[:ncalls], mems=["device"], what=("groups", G, ncalls))


def test_one_group_of_every_row_and_every_row_its_own_group(api):
    rng = np.random.default_rng(23)
    n = 3 * B + 7
    value = (rng.integers(-1000, 1000, n).astype(np.int32), rng.random(n) > 0.1)
    check(api, [(np.zeros(n, dtype=np.int64),)], value, what="one group")
    check(api, [], value, what="no keys")
    rows, _, counts = check(api, [(rng.permutation(n).astype(np.int64),)], value, what="own groups")
    assert len(rows) == n and set(counts.tolist()) == {0, 1}


def test_eight_calls_at_the_ends_of_p(api):
    rng = np.random.default_rng(24)
    n = 1000
    key = (rng.integers(0, 9, n).astype(np.int16),)
    value = (rng.standard_normal(n), rng.random(n) > 0.1)
    calls = [("cont", 0.0), ("cont", 1.0), ("disc", 0.0), ("disc", 1.0), ("cont", 1e-300), ("cont", float(np.nextafter(1.0, 0.0))),
             ("disc", 1e-300), ("disc", float(np.nextafter(1.0, 0.0)))]
    check(api, [key], value, calls=calls, what="ends of p")
    check(api, [], value, calls=calls, what="ends of p, whole column")


# ---------------------------------------------------------------- the select route

def whole(api, vals, valid=None, calls=MIXED, what="", **kw):
    return check(api, [], (vals,) if valid is None else (vals, valid), calls=calls, what=what, **kw)


@pytest.mark.parametrize("n", [1, 2, FINISH - 1, FINISH, FINISH + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_row_counts_around_the_tile_and_the_finish(api, n):
    rng = np.random.default_rng(n)
    whole(api, rng.standard_normal(n), what=("dense", n))
    whole(api, rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64), rng.random(n) > 0.1, what=("int64, nullable", n))


def test_live_rows_around_the_finish_among_many_nulls(api):
    rng = np.random.default_rng(31)
    n = 4 * TILE + 3
    for m in (0, 1, FINISH - 1, FINISH, FINISH + 1):
        ok = np.zeros(n, dtype=bool)
        ok[rng.permutation(n)[:m]] = True
        _, _, counts = whole(api, rng.integers(0, 1 << 30, n).astype(np.uint32), ok, mems=["device"], what=("live rows", m))
        assert counts.tolist() == [m]


def test_all_equal_and_two_valued_columns(api):
    rng = np.random.default_rng(32)
    n = 5 * TILE + 11
    for dtype in (np.int64, np.float64, np.int8):
        _, _, _ = whole(api, np.full(n, 42, dtype=dtype), what=("all equal", np.dtype(dtype).name))
        two = np.where(rng.random(n) < 0.3, 7, -7).astype(dtype)
        whole(api, two, rng.random(n) > 0.1, what=("two values", np.dtype(dtype).name))
    res = run(api, [], (np.full(n, 42, dtype=np.int64),), ["median"], route=2)
    assert res[4].startswith("select: %d x pct_sel_hist_kernel" % (64 // BITS)), res[4]      # a bucket of every row: every digit, no more


def test_keys_that_differ_in_one_digit_only(api):
    rng = np.random.default_rng(33)
    n = 2 * TILE + 77
    low = (0x1234567800000000 + rng.integers(0, 1 << BITS, n)).astype(np.int64)              # only the lowest digit differs
    whole(api, low, what="lowest digit")
    res = run(api, [], (low,), ["median", ("disc", 0.9)], route=2)
    assert res[4].startswith("select: %d x pct_sel_hist_kernel" % (64 // BITS)) and "finish" not in res[4], res[4]
    top = (rng.integers(0, 1 << BITS, n).astype(np.uint64) << np.uint64(64 - BITS)) | np.uint64(0x55AA55)      # only the top digit differs
    whole(api, top, what="top digit")
    res = run(api, [], (top,), ["median"], route=2)
    assert res[4].startswith("select: 1 x pct_sel_hist_kernel") and "finish" in res[4], res[4]      # one digit leaves a handful of rows


def test_ranks_in_one_bucket_and_in_sixteen(api):
    rng = np.random.default_rng(34)
    n = 6 * TILE + 1
    spread = [("cont", (2 * i + 1) / 16.0 + 1e-3) for i in range(8)]                          # lo / hi of eight calls: sixteen ranks
    vals = rng.permutation(n).astype(np.uint32) * np.uint32(170_000)                          # spread over the top digit
    whole(api, vals, calls=spread, what="sixteen buckets")
    near = [("cont", 0.5 + i * 1e-6) for i in range(4)] + [("disc", 0.5 + i * 1e-6) for i in range(4)]
    whole(api, rng.standard_normal(n).astype(np.float32), calls=near, what="one bucket")
    res = run(api, [], (vals,), spread, route=2)
    assert "finish" in res[4] or res[4].startswith("select: 4 x"), res[4]


@pytest.mark.parametrize("dtype", NUMERIC, ids=lambda d: np.dtype(d).name)
def test_every_dtype_on_both_routes(api, dtype):
    rng = np.random.default_rng(np.dtype(dtype).num + 40)
    n = TILE + FINISH + 13
    if np.dtype(dtype).kind == "f":
        vals = float_pool(dtype, rng, 3000)[rng.integers(0, 3008, n)]
    else:
        info = np.iinfo(dtype)
        vals = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
        vals[:2] = [info.min, info.max]
    whole(api, vals, rng.random(n) > 0.1, lens=[TILE - 1, 0, FINISH + 14], odd=True, what=np.dtype(dtype).name)
    res = run(api, [], (vals,), ["median"], route=2)
    assert 1 <= int(res[4].split()[1]) <= np.dtype(dtype).itemsize * 8 // BITS, res[4]        # never more passes than the key has digits
    if np.dtype(dtype).itemsize == 1:
        assert res[4].startswith("select: 1 x pct_sel_hist_kernel") and "finish" not in res[4], res[4]     # one histogram answers it


def test_int64_extremes_and_nan_as_the_maximum(api):
    i = np.iinfo(np.int64)
    vals = np.array([i.max, i.min, i.max - 1, i.min + 1, 0, -1, 1, i.max, i.min] * 300, dtype=np.int64)
    whole(api, vals, what="int64 extremes")
    f = np.array([1.0, math.nan, -math.inf, math.inf, -0.0, 0.0, -math.nan, 5e-324, -5e-324] * 300)
    _, exp, _ = whole(api, f, what="NaN is the maximum")
    assert int(exp[2][0][0]) == R.NAN_BITS                                                     # ("cont", 1.0)
    whole(api, np.array([math.nan, math.nan, -math.nan]), what="only NaN")


def test_the_select_route_refuses_what_it_cannot_serve(api):
    key = (np.arange(5, dtype=np.int64),)
    for keys, value, calls in (([key], (np.arange(5.0),), ["median"]), ([], (["a", "b", None, "c", "d"],), [("disc", 0.5)])):
        with pytest.raises(A.RdfError) as ei:
            run(api, keys, value, calls, route=2)
        assert ei.value.status == A.RDF_INVALID_ARGUMENT
    assert run(api, [key], (np.arange(5.0),), ["median"], route=0)[4].startswith("sorted:")
    assert run(api, [], (["a", "b", None, "c", "d"],), [("disc", 0.5)], route=0)[4].startswith("sorted:")


def test_the_auto_rule_takes_select_wherever_it_can(api):
    # the select route measured faster for every dtype, size and distribution, so auto takes it when it can
    n = TILE + 5
    for dtype in NUMERIC:
        res = run(api, [], (np.arange(n).astype(dtype),), ["median"], route=0)
        assert res[4].startswith("select:"), (np.dtype(dtype).name, res[4])
    assert run(api, [(np.zeros(n, dtype=np.int64),)], (np.arange(n, dtype=np.int32),), ["median"], route=0)[4].startswith("sorted:")


# ---------------------------------------------------------------- invariance: bytes equal

def test_chunking_memory_kind_and_repetition_change_no_byte(api):
    rng = np.random.default_rng(41)
    n = 5000
    key = (rng.integers(0, 40, n).astype(np.int64), rng.random(n) > 0.05)
    value = (np.ldexp(rng.standard_normal(n), rng.integers(-30, 30, n)).round(3), rng.random(n) > 0.1)
    seven = [700, 1, 0, 1999, 300, 1500, 500]
    for keys, routes in (([key], [1]), ([], [1, 2])):
        base = raw_bytes(run(api, keys, value, MIXED, "host", route=routes[0]))
        for route in routes:
            assert raw_bytes(run(api, keys, value, MIXED, "host", route=route)) == base                         # twice
            assert raw_bytes(run(api, keys, value, MIXED, "host", lens=seven, odd=True, route=route)) == base   # 7 uneven chunks, one empty
            assert raw_bytes(run(api, keys, value, MIXED, "device", route=route)) == base
            assert raw_bytes(run(api, keys, value, MIXED, "device", lens=seven, odd=True, route=route)) == base


def test_row_order_changes_no_cont_byte_and_no_disc_value(api):
    rng = np.random.default_rng(42)
    n = 5000
    key = (rng.integers(0, 40, n).astype(np.int64), rng.random(n) > 0.05)
    value = (np.ldexp(rng.standard_normal(n), rng.integers(-30, 30, n)).round(3), rng.random(n) > 0.1)
    value[0][rng.integers(0, n, n // 3)] = value[0][rng.integers(0, n, n // 3)]
    p = rng.permutation(n)
    for keys, skeys, routes in (([key], [(key[0][p], key[1][p])], [1]), ([], [], [1, 2])):
        for route in routes:
            g0, _, o0, c0, _ = run(api, keys, value, MIXED, "device", route=route)
            g1, _, o1, c1, _ = run(api, skeys, (value[0][p], value[1][p]), MIXED, "device", route=route)
            assert g0 == g1 and np.array_equal(c0, c1)
            for (kind, *_), (a, aok), (b, bok) in zip(R.normalise_calls(MIXED), o0, o1):
                assert np.array_equal(aok, bok)
                if kind == "cont":
                    assert a.tobytes() == b.tobytes()
                else:
                    assert np.array_equal(value[0][a[aok]] + 0.0, value[0][p][b[bok]] + 0.0)      # (+ 0.0: the zeros are peers)


# ---------------------------------------------------------------- sizing

def test_short_capacities_report_the_groups_and_write_nothing(api):
    key = [A.HostArray.from_numpy(np.array([3, 1, 3, 2, 1, 9], dtype=np.int64))]
    val = [A.HostArray.from_numpy(np.array([5.0, 5.0, 6.0, 7.0, 5.0, 1.0]))]
    for short in range(4):
        outs = [A.HostArray.empty_out(A.F64, 8, True), A.HostArray.empty_out(A.U32, 8, True)]
        rows_out, counts_out = A.HostArray.empty_out(A.U32, 8, False), A.HostArray.empty_out(A.I64, 8, False)
        arrs = outs + [rows_out, counts_out]
        for a in arrs:
            a.values[:] = 77
        arrs[short].length = 3                                                    # an output's capacity is its length; 4 groups
        with pytest.raises(A.RdfError) as ei:
            api.groupby_percentile([key], val, ["median", ("disc", 1.0)], outs=outs, rows_out=rows_out, counts_out=counts_out, raw=True)
        assert ei.value.status == A.RDF_MEMORY_ERROR
        assert api.last_groups == 4 and [a.length for a in arrs] == [4, 4, 4, 4]
        assert all((a.values == 77).all() for a in arrs)
    groups, rows, res, cnt = api.groupby_percentile([key], None, [], group_rows=False)      # the count-only call
    assert groups == 4 and rows is None and res == [] and cnt is None
    groups, rows, res, cnt = api.groupby_percentile([key], None, [])                        # the distinct tuples
    assert groups == 4 and rows.tolist() == [1, 3, 0, 5]
    groups, rows, res, cnt = api.groupby_percentile([key], val, [], group_rows=False, counts=True)
    assert groups == 4 and cnt.tolist() == [2, 1, 2, 1]
    groups, rows, res, cnt = api.groupby_percentile([key], val, ["median"], group_rows=False)
    assert res[0][0].tolist() == [5.0, 7.0, 5.5, 1.0] and res[0][1].all()
