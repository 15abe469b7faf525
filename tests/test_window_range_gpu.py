"""rdf_window_range_agg on the MI355X: sum / min / max / count / avg / first_value / last_value over RANGE frames whose offsets are
in the order key's units.  Every case runs in host and in device memory and is held to tests/window_range_ref.py (a direct
predicate over the partition's keys per frame end; its cumulative-sum path for the large cases, where the data is integer-valued
and every cumulative sum exact):
  - Int64 results, counts, row indices and validity bitmaps bit for bit; COUNT(-1), FIRST_VALUE and LAST_VALUE pin the frame's two
    ends exactly;
  - Float64 MIN / MAX bit for bit on the uint64 view;
  - Float64 SUM within  ulp(F) + 8 (m + 1) 2^-106 T  of F = math.fsum(frame) (DESIGN 11's bound: the scans are rdf_window_agg's) —
    and bit for bit where the data is integer-valued;
  - AVG == the same request's SUM / COUNT, one IEEE division.
T = WINDOW_RANGE_TILE positions per block of the bounds pass, L = WINDOW_RANGE_LDS_KEYS keys of a tile's window staged in LDS.
"""
import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
import window_range_ref as R
import test_window_agg_gpu as W
from test_window_agg_gpu import MEMS, N, bits
from window_range_ref import FOLLOWING as FOLL
from window_range_ref import PRECEDING as PREC
from window_range_ref import UNBOUNDED_FOLLOWING as UF
from window_range_ref import UNBOUNDED_PRECEDING as UP

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T, L = A.WINDOW_RANGE_TILE, A.WINDOW_RANGE_LDS_KEYS
LDS_KERNEL, GLOBAL_KERNEL = "wrange_bounds_lds_kernel", "wrange_bounds_global_kernel"
I64_MIN, I64_MAX = R.I64_MIN, R.I64_MAX


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


def run(api, partition, order, values, calls, mem, lens=None, odd=False, raw=False, outs=None):
    cols = partition + [order] + values
    n = W.rows_of(cols[0])
    lens = [n] if lens is None else lens
    assert sum(lens) == n
    chunks = [W.host_chunks(k, lens, odd) for k in cols]
    if mem == "device":
        chunks = [[W.to_device(c) for c in col] for col in chunks]
        torch.cuda.synchronize()
    np_ = len(partition)
    return api.window_range_agg(chunks[:np_], [(chunks[np_], order["desc"])], chunks[np_ + 1:], calls, mem=mem, raw=raw, outs=outs)


def ref_args(partition, order, values):
    return [W.ref_key(k, False) for k in partition], W.ref_key(order, True), [(v["values"], v["valid"]) for v in values]


def check(api, partition, order, values, calls, lens=None, odd=False, fast=False, exact=False, mems=MEMS, what=""):
    """The calls in requests of up to 8, in host and in device memory, against the model.  exact: Float64 sums bit for bit."""
    p, o, v = ref_args(partition, order, values)
    exp = (R.range_ref_fast if fast else R.range_ref)(p, o, v, calls)
    slack = []
    for name, vi, fr in calls:
        is_f = vi >= 0 and values[vi]["values"].dtype == np.float64
        slack.append(R.sum_slack(p, o, v[vi], fr) if name == "sum" and is_f and not exact else None)
    got = {}
    for mem in mems:
        got[mem] = []
        for at in range(0, len(calls), 8):
            got[mem] += run(api, partition, order, values, calls[at:at + 8], mem, lens, odd)
        W.compare(got[mem], exp, calls, slack, (what, mem))
    return exp, got


def partitions(rng, sizes):
    ids = np.repeat(np.arange(len(sizes)), sizes)
    return ids[rng.permutation(len(ids))]


def pins(frames):
    """COUNT(*), FIRST_VALUE and LAST_VALUE of a frame give b - a + 1, a and b."""
    return [(name, -1, fr) for fr in frames for name in ("count", "first_value", "last_value")]


# ---------------------------------------------------------------- the rule, on 16 rows

def rule_frames(offsets):
    """Every allowed (start kind, end kind) pair over the offsets, offset 0 spelled as an offset (0 PRECEDING) and as CURRENT ROW."""
    starts = [UP] + [(PREC, s) for s in offsets] + [0] + [(FOLL, s) for s in offsets]
    ends = [(PREC, s) for s in offsets] + [0] + [(FOLL, s) for s in offsets] + [UF]
    kind = lambda b: 0 if b == UP else 4 if b == UF else 2 if b == 0 else b[0]
    out = []
    for s in starts:
        for e in ends:
            if kind(s) > kind(e):
                continue
            if kind(s) == kind(e) == PREC and s[1] < e[1]:
                continue
            if kind(s) == kind(e) == FOLL and s[1] > e[1]:
                continue
            out.append((s, e))
    return out


RULE_PART = np.array([0] * 7 + [1] * 9, dtype=np.int64)
RULE_KEY = np.array([5, 5, 6, 9, 9, 12, 0, 1, 2, 2, 6, 7, 8, 13, 20, 20], dtype=np.int64)
RULE_KVALID = np.array([True] * 6 + [False] + [True] * 9)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("kdtype", [np.int64, np.int32, np.float64])
def test_every_pair_of_bound_kinds_on_sixteen_rows(api, desc, kdtype):
    rng = np.random.default_rng(1)
    perm = rng.permutation(16)
    key = N(RULE_KEY.astype(kdtype)[perm], RULE_KVALID[perm], desc)
    part = N(RULE_PART[perm])
    off = (lambda s: float(s)) if kdtype == np.float64 else (lambda s: s)
    frames = rule_frames([off(0), off(1), off(3)])
    assert len(frames) == 43
    exp, _ = check(api, [part], key, [], pins(frames), what="rule")
    # the model itself: empty frames at the first row of the first partition and at the last row of the last
    order = R.range_bounds([(part["values"],)], (key["values"], key["valid"], desc), (UP, UF))[0]
    counts = {fr: exp[3 * i][0] for i, fr in enumerate(frames)}
    assert counts[((PREC, off(3)), (PREC, off(1)))][order[0]] == 0 and counts[((FOLL, off(1)), (FOLL, off(3)))][order[-1]] == 0
    assert not RULE_KVALID[perm][order[6]] and counts[((FOLL, off(1)), (FOLL, off(3)))][order[6]] == 1      # a NULL key: its own peer group


def test_sums_and_extremes_on_the_sixteen_rows(api):
    rng = np.random.default_rng(2)
    x = N(rng.integers(-9, 9, size=16).astype(np.int64), rng.random(16) > 0.2)
    y = N(rng.integers(-9, 9, size=16).astype(np.float64), rng.random(16) > 0.2)
    for desc in (False, True):
        key = N(RULE_KEY, RULE_KVALID, desc)
        calls = []
        for fr in ((-1, 0), (0, 3), (-3, 3), ((PREC, 3), (PREC, 1)), (1, 3)):
            calls += [(f, v, fr) for v in (0, 1) for f in ("sum", "count", "avg")] + [("count", -1, fr), ("last_value", -1, fr)]
        for fr in ((UP, 1), (UP, (PREC, 1)), (-3, UF), (1, UF), (UP, UF), (UP, 0), (0, UF)):
            calls += [(f, v, fr) for v in (0, 1) for f in ("min", "max")] + [("sum", 0, fr), ("count", 0, fr), ("avg", 0, fr), ("first_value", -1, fr)]
        check(api, [N(RULE_PART)], key, [x, y], calls, exact=True, what=("sixteen", desc))


# ---------------------------------------------------------------- 3 T + 5 rows: every partition size around a tile

def tile_case(sizes, seed):
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    assert n == 3 * T + 5
    part = N(partitions(rng, sizes).astype(np.int64))
    keyv = rng.integers(0, 41, size=n).astype(np.int64)                      # a small range: peers everywhere
    kvalid = rng.random(n) > 0.1
    x = N(rng.integers(-1000, 1000, size=n).astype(np.int64), rng.random(n) > 0.1)
    y = N(rng.integers(-1000, 1000, size=n).astype(np.float64), rng.random(n) > 0.1)
    return part, keyv, kvalid, x, y


def tile_calls(offsets):
    calls = []
    for s in offsets:
        s2 = min(2 * s, I64_MAX)
        calls += [("sum", 0, (-s, 0)), ("sum", 1, (-s, 0)), ("count", 1, (-s, 0)), ("avg", 1, (-s, 0)), ("count", -1, (-s, s)), ("first_value", -1, (-s, s)),
                  ("last_value", -1, (-s, s)), ("sum", 1, (-s, s))]
        calls += [("min", 0, (UP, s)), ("max", 1, (-s, UF)), ("count", -1, ((FOLL, s), (FOLL, s2))), ("first_value", -1, ((PREC, s2), (PREC, s))),
                  ("sum", 0, (0, s)), ("count", 0, (0, s)), ("avg", 0, (0, s)), ("last_value", -1, (0, s))]
    return calls


# the cycle 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 T + 3 is longer than 3 T + 5 rows: two tables of 3 T + 5 rows hold all of it
TILE_SIZES = {"small": [1, 2, 63, 64, 65, T - 1, T, 3 * T + 5 - (2 * T + 194)], "large": [T + 1, 2 * T + 3, 1]}
OFFSETS = [0, 1, 7, 20, 2 ** 62]


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("which", ["small", "large"])
def test_partitions_around_the_tile_size(api, which, desc):
    part, keyv, kvalid, x, y = tile_case(TILE_SIZES[which], 3)
    check(api, [part], N(keyv, kvalid, desc), [x, y], tile_calls(OFFSETS), fast=True, exact=True, what=(which, desc))


# ---------------------------------------------------------------- Float64 keys

def test_float_keys_with_nan_infinities_zeros_and_subnormals(api):
    sub = float(np.nextafter(0.0, 1.0))
    base = [np.nan, np.nan, np.inf, np.inf, -np.inf, 0.0, -0.0, 0.0, sub, -sub, 2 * sub, 0.1, 0.2, 0.3, 0.30000000000000004, 0.5, 0.6, 1.0, 1.5, -0.5, -0.4, 1e300,
            -1e300, 1e-300, 5e299, 0.7, 0.7]
    rng = np.random.default_rng(4)
    keyv = np.array(base + base)[rng.permutation(2 * len(base))]
    kvalid = rng.random(len(keyv)) > 0.1
    part = N((np.arange(len(keyv)) % 2).astype(np.int64))
    x = N(rng.integers(-9, 9, size=len(keyv)).astype(np.int64), rng.random(len(keyv)) > 0.1)
    for desc in (False, True):
        calls = []
        for s in (0.0, 0.1, 0.2, 0.5, 1e300, sub):
            calls += pins([(-s, 0.0), (0.0, s), (-s, s), ((PREC, 2 * s), (PREC, s)), ((FOLL, s), (FOLL, 2 * s))])
            calls += [("sum", 0, (-s, s)), ("max", 0, (UP, s)), ("min", 0, (-s, UF))]
        check(api, [part], N(keyv, kvalid, desc), [x], calls, what=("float keys", desc))
    # the rounding example of the header: whether 0.1 lies in 0.3's frame is decided by 0.1 >= fl(0.3 - 0.2)
    k = N(np.array([0.1, 0.3]))
    for mem in MEMS:
        got = run(api, [], k, [], [("count", -1, (-0.2, 0.0)), ("count", -1, (0.0, 0.2))], mem)
        assert got[0][0].tolist() == [1, 2] and got[1][0].tolist() == [2, 1]


# ---------------------------------------------------------------- the ends of the integer range

@pytest.mark.parametrize("desc", [False, True])
def test_extreme_integer_keys_do_not_wrap(api, desc):
    for kdtype, lo, hi in ((np.int64, I64_MIN, I64_MAX), (np.int32, -2 ** 31, 2 ** 31 - 1)):
        keyv = np.array([lo, lo + 1, -1, 0, 1, hi - 1, hi, lo, hi, 0], dtype=kdtype)
        x = N(np.arange(10, dtype=np.int64))
        calls = []
        for s in (1, I64_MAX):
            calls += pins([(-s, 0), (0, s), (-s, s), ((PREC, s), (PREC, 1)), ((FOLL, 1), (FOLL, s))]) + [("sum", 0, (-s, s)), ("max", 0, (UP, s)), ("min", 0, (-s, UF))]
        exp, _ = check(api, [], N(keyv, None, desc), [x], calls, what=("extremes", kdtype.__name__, desc))
        if kdtype == np.int64 and not desc:
            assert exp[0][0].tolist() == [2, 3, 1, 3, 3, 1, 3, 2, 3, 3]             # 1 PRECEDING .. CURRENT ROW, by hand
            i = calls.index(("count", -1, (-I64_MAX, 0)))
            assert exp[i][0].tolist() == [2, 3, 4, 4, 4, 5, 6, 2, 6, 4]               # MIN - (2^63 - 1) does not wrap to +1


# ---------------------------------------------------------------- routes

def test_a_frame_wider_than_the_window_takes_the_global_search(api):
    n = 4 * L + 7
    rng = np.random.default_rng(5)
    keyv = rng.permutation(n).astype(np.int64)                              # one partition of dense unique keys
    x = N(rng.integers(-100, 100, size=n).astype(np.int64))
    wide, narrow = L + 5, 3
    calls = [("count", -1, (-wide, wide)), ("first_value", -1, (-wide, wide)), ("last_value", -1, (-wide, wide)), ("sum", 0, (-wide, wide))]
    check(api, [], N(keyv), [x], calls, fast=True, exact=True, mems=["device"], what="wide")
    assert GLOBAL_KERNEL in lib.last_kernel() and LDS_KERNEL not in lib.last_kernel(), lib.last_kernel()
    calls = [("count", -1, (-narrow, narrow)), ("sum", 0, (-narrow, narrow))]
    check(api, [], N(keyv), [x], calls, fast=True, exact=True, mems=["device"], what="narrow")
    assert LDS_KERNEL in lib.last_kernel() and GLOBAL_KERNEL not in lib.last_kernel(), lib.last_kernel()


def test_one_call_can_take_both_routes(api):
    rng = np.random.default_rng(12)
    long_rows = 2 * L + 100
    sizes = [long_rows] + [50] * ((4 * L + 7 - long_rows) // 50) + [(4 * L + 7 - long_rows) % 50]
    n = sum(sizes)
    ids = partitions(rng, sizes)
    keyv = np.zeros(n, dtype=np.int64)
    for i, m in enumerate(sizes):
        keyv[ids == i] = rng.permutation(m)                                  # dense: a frame of L + 5 key units is L + 5 rows wide
    x = N(rng.integers(-100, 100, size=n).astype(np.int64), rng.random(n) > 0.1)
    wide = L + 5
    calls = pins([(-wide, 0), (-3, wide)]) + [("sum", 0, (-wide, wide)), ("min", 0, (UP, wide))]
    for desc in (False, True):
        check(api, [N(ids.astype(np.int64))], N(keyv, None, desc), [x], calls, fast=True, exact=True, mems=["device"], what=("mixed", desc))
        assert GLOBAL_KERNEL in lib.last_kernel() and LDS_KERNEL in lib.last_kernel(), lib.last_kernel()   # the long partition's tiles, and the short ones'


def test_both_routes_give_the_same_bytes(api):
    part, keyv, kvalid, x, y = tile_case(TILE_SIZES["small"], 6)
    calls = tile_calls([1, 7])[:8] + tile_calls([20, 2 ** 62])[8:16]
    outs = {}
    try:
        for route, kernel, other in ((1, LDS_KERNEL, GLOBAL_KERNEL), (2, GLOBAL_KERNEL, LDS_KERNEL), (0, LDS_KERNEL, GLOBAL_KERNEL)):
            lib.set_option("window_range_route", route)
            for desc in (False, True):
                for at in (0, 8):
                    got = run(api, [part], N(keyv, kvalid, desc), [x, y], calls[at:at + 8], "device")
                    assert kernel in lib.last_kernel() and other not in lib.last_kernel(), (route, lib.last_kernel())
                    outs[(route, desc, at)] = got
    finally:
        lib.set_option("window_range_route", 0)
    for desc in (False, True):
        for at in (0, 8):
            for route in (2, 0):
                for (gv, gok), (wv, wok) in zip(outs[(route, desc, at)], outs[(1, desc, at)]):
                    assert np.array_equal(gok, wok) and gv.tobytes() == wv.tobytes(), (route, desc, at)
    exp = R.range_ref_fast(*ref_args([part], N(keyv, kvalid, False), [x, y]), calls)
    W.compare(outs[(2, False, 0)] + outs[(2, False, 8)], exp, calls, [None] * len(calls), "global route")


# ---------------------------------------------------------------- agreement with rdf_window_agg

@pytest.mark.parametrize("desc", [False, True])
def test_dense_unique_keys_answer_as_rows_frames_do(api, desc):
    rng = np.random.default_rng(7)
    sizes = [1, 2, 65, T + 1, 700]
    n = sum(sizes)
    ids = partitions(rng, sizes)
    keyv = np.zeros(n, dtype=np.int64)
    for i, m in enumerate(sizes):
        keyv[ids == i] = rng.permutation(m)                                  # 0 .. m - 1 in every partition
    part, key = N(ids.astype(np.int64)), N(keyv, None, desc)
    x = N(rng.normal(size=n) * 10.0 ** rng.integers(-3, 9, size=n), rng.random(n) > 0.1)
    z = N(rng.integers(-10 ** 12, 10 ** 12, size=n).astype(np.int64), rng.random(n) > 0.1)
    two_sided = [(-2, 1), (-40, -3), (5, 90), (0, 7), (-T, 0)]
    one_sided = [(UP, 3), (-3, UF), (UP, UF), (UP, -2), (4, UF)]
    calls = [(f, v, fr) for fr in two_sided for v in (0, 1) for f in ("sum", "count", "avg")] + [(f, -1, fr) for fr in two_sided for f in ("count", "first_value", "last_value")]
    calls += [(f, v, fr) for fr in one_sided for v in (0, 1) for f in W.FIVE] + [("last_value", -1, fr) for fr in one_sided]
    for mem in MEMS:
        for at in range(0, len(calls), 8):
            got = run(api, [part], key, [x, z], calls[at:at + 8], mem)
            rows = W.run(api, [part], [key], [x, z], [(f, v, ("rows", s, e)) for f, v, (s, e) in calls[at:at + 8]], mem)
            for c, ((gv, gok), (wv, wok)) in zip(calls[at:at + 8], zip(got, rows)):
                assert gv.dtype == wv.dtype and np.array_equal(gok, wok) and gv[gok].tobytes() == wv[wok].tobytes(), (c, mem)


# ---------------------------------------------------------------- Float64 sums on general data

def test_float_sums_stay_inside_the_bound_of_the_scans(api):
    x = N(np.array([1e16, -1e16, 1.0, 1.0, 1.0]))
    k = N(np.arange(5, dtype=np.int64))
    frames = [(-1, 1), (-2, 0), (0, 2), (UP, 0), (-1, UF), (2, 3)]
    check(api, [], k, [x], [(f, 0, fr) for fr in frames for f in ("sum", "count", "avg")], what="cancellation")
    rng = np.random.default_rng(8)
    n = 500
    vals = rng.normal(size=n) * 10.0 ** rng.integers(-8, 12, size=n)
    vals[rng.random(n) < 0.02] = np.nan
    vals[rng.random(n) < 0.02] = np.inf
    vals[rng.random(n) < 0.01] = -np.inf
    y = N(vals, rng.random(n) > 0.1)
    part = N(partitions(rng, [n - 150, 149, 1]).astype(np.int64))
    key = N(rng.integers(0, 200, size=n).astype(np.int32), rng.random(n) > 0.05)
    frames = [(-3, 0), (-10, 10), (0, 25), (UP, 2), (-2, UF), (5, 9)]
    check(api, [part], key, [y], [(f, 0, fr) for fr in frames for f in ("sum", "count", "avg")], what="magnitudes")


# ---------------------------------------------------------------- plumbing

def test_three_chunks_at_odd_offsets(api):
    part, keyv, kvalid, x, y = tile_case(TILE_SIZES["small"], 9)
    n = 3 * T + 5
    calls = tile_calls([7])
    for desc in (False, True):
        check(api, [part], N(keyv, kvalid, desc), [x, y], calls, lens=[n - 1030, 1, 1029], odd=True, fast=True, exact=True, what=("chunks", desc))


def test_rolling_seven_days_and_microsecond_windows(api):
    rng = np.random.default_rng(10)
    n = 400
    account = W.T([b"acct-%d" % i for i in rng.integers(0, 6, size=n)])
    day = N((19000 + rng.integers(0, 90, size=n)).astype(np.int32))          # Date32 storage: days since the epoch
    amount = N(rng.integers(1, 500, size=n).astype(np.int64), rng.random(n) > 0.05)
    pcodes = np.array([int(r[5:]) for r in account["rows"]], dtype=np.int64)
    calls = [("sum", 0, (-7, 0)), ("count", 0, (-7, 0)), ("avg", 0, (-7, 0)), ("first_value", -1, (-7, 0)), ("max", 0, (UP, 0)), ("sum", 0, (-6, 0)), ("count", -1, (1, 7))]
    exp = R.range_ref([(pcodes,)], (day["values"], None, False), [(amount["values"], amount["valid"])], calls)
    for mem in MEMS:
        got = run(api, [account], day, [amount], calls, mem)
        W.compare(got, exp, calls, [None] * len(calls), ("7 days", mem))
    ts = N(1_700_000_000_000_000 + rng.integers(0, 5000, size=n).astype(np.int64))       # Timestamp(us) storage
    calls = pins([(-500, 500), (-500, 0), ((FOLL, 1), (FOLL, 500))])
    for desc in (False, True):
        check(api, [], N(ts["values"], None, desc), [], calls, what=("500 us", desc))


def test_eight_calls_with_eight_distinct_frames_from_one_sort(api):
    rng = np.random.default_rng(11)
    n = 300
    part = N(rng.integers(0, 4, size=n).astype(np.int64))
    key = N(rng.integers(-30, 30, size=n).astype(np.int64), rng.random(n) > 0.1)
    x = N(rng.integers(-50, 50, size=n).astype(np.float64), rng.random(n) > 0.1)
    calls = [("sum", 0, (-1, 0)), ("sum", 0, (-2, 3)), ("count", -1, (4, 9)), ("avg", 0, (-9, -4)), ("first_value", -1, (0, 5)), ("last_value", -1, (-5, 0)),
             ("min", 0, (UP, 6)), ("max", 0, (-7, UF))]
    p, o, v = ref_args([part], key, [x])
    exp = R.range_ref(p, o, v, calls + [("sum", 0, (-9, -4)), ("count", 0, (-9, -4))])
    for mem in MEMS:
        got = run(api, [part], key, [x], calls, mem)                          # ONE request: 11 distinct offset bounds
        assert "wrange_keys_kernel" in lib.last_kernel()
        for c, (gv, gok), (wv, wok) in zip(calls, got, exp):
            assert np.array_equal(gok, wok), (c, mem)
            if c[0] == "avg":
                assert np.array_equal(bits(gv[gok]), bits(exp[8][0][gok] / exp[9][0][gok].astype(np.float64))), (c, mem)
            else:
                assert gv[gok].tobytes() == wv[wok].tobytes(), (c, mem)


def test_zero_rows_short_capacities_and_no_partition_keys(api):
    for mem in MEMS:
        empty = N(np.zeros(0, dtype=np.int64))
        got = run(api, [], empty, [N(np.zeros(0))], [("sum", 0, (-1, 1)), ("count", -1, (-1, 1))], mem)
        assert got[0][0].shape == (0,) and got[1][0].shape == (0,)
        key = N(np.array([3, 1, 2, 2, 9], dtype=np.int64))
        x = N(np.array([1, 2, 3, 4, 5], dtype=np.int64))
        got = run(api, [], key, [x], [("sum", 0, (-1, 0)), ("count", -1, (0, 1)), ("last_value", -1, (1, 7))], mem)       # no partition keys
        assert got[0][0].tolist() == [8, 2, 9, 9, 5] and got[1][0].tolist() == [1, 3, 3, 3, 1]
        assert got[2][1].tolist() == [True, True, True, True, False] and got[2][0][:4].tolist() == [4, 0, 4, 4]
        outs = [A.Api._window_out(A.I64, 4, mem == "device", True), A.Api._window_out(A.I64, 5, mem == "device", False)]
        with pytest.raises(A.RdfError) as ei:
            run(api, [], key, [x], [("sum", 0, (-1, 0)), ("count", -1, (0, 1))], mem, outs=outs, raw=True)
        assert ei.value.status == A.RDF_MEMORY_ERROR
        assert [o.length for o in outs] == [5, 5]                              # ... with the lengths set to the rows
