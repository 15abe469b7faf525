"""rdf_window_agg on the MI355X: sum / min / max / count / avg / first_value / last_value over ROWS and RANGE frames.
Every case runs in host and in device memory and is held to tests/window_frame_ref.py (brute force per frame; its vectorised
path for the large cases, where the data is integer-valued and every cumulative sum exact):
  - Int64 results, counts, row indices and validity bitmaps bit for bit;
  - Float64 MIN / MAX bit for bit on the uint64 view;
  - Float64 SUM within  ulp(F) + 8 (m + 1) 2^-106 T  of F = math.fsum(frame), m = the partition's rows up to the frame's end,
    T = the sum of |x| over them (two double-double prefixes at 3.1 m u^2 T each, their subtraction at 3.1 u^2 2T, one rounding
    of the result and one of F; u = 2^-53) — and bit for bit where the data is integer-valued;
  - AVG == the same request's SUM / COUNT, one IEEE division.
"""
import math

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
import exact_ref
import window_frame_ref as R
import window_ref
from window_frame_ref import UNBOUNDED_FOLLOWING as UF
from window_frame_ref import UNBOUNDED_PRECEDING as UP

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MEMS = ["host", "device"]
FIVE = ("sum", "min", "max", "count", "avg")


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


# ---------------------------------------------------------------- inputs (built as tests/test_window_gpu.py builds them)

def N(values, valid=None, desc=False):
    return {"kind": "num", "values": np.asarray(values), "valid": None if valid is None else np.asarray(valid, dtype=bool), "desc": desc}


def T(rows, desc=False):
    return {"kind": "utf8", "rows": rows, "desc": desc}


def utf8(rows, row_offset=0, data_offset=0):
    enc = [b"j" * (i % 3 + 1) for i in range(row_offset)] + [b"" if r is None else r for r in rows]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in enc]) if enc else []
    data = np.frombuffer(b"\xee" * data_offset + b"".join(enc) + b"\0" * 8, dtype=np.uint8).copy()
    nulls = sum(r is None for r in rows)
    valid = A.pack_bits(np.array([True] * row_offset + [r is not None for r in rows], dtype=bool)) if nulls else None
    return A.HostUtf8(offs.astype(np.int32), data, valid, row_offset, len(rows), data_offset, nulls)


def rows_of(key):
    return len(key["values"]) if key["kind"] == "num" else len(key["rows"])


def host_chunks(key, lens, odd):
    out, at = [], 0
    for i, ln in enumerate(lens):
        if key["kind"] == "num":
            v = None if key["valid"] is None else key["valid"][at:at + ln]
            out.append(A.HostArray.from_numpy(key["values"][at:at + ln], v, offset=(3 + 2 * i) % 11 if odd else 0))
        else:
            out.append(utf8(key["rows"][at:at + ln], (5 + 3 * i) % 13 if odd else 0, (7 * i) % 9 if odd else 0))
        at += ln
    return out


def to_device(x):
    if isinstance(x, A.HostUtf8):
        return A.DeviceUtf8.from_host(x)
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def ref_key(key, with_desc):
    vals, valid = (key["values"], key["valid"]) if key["kind"] == "num" else (key["rows"], None)
    return (vals, valid, key["desc"]) if with_desc else (vals, valid)


def ref_args(partition, order, values):
    return [ref_key(k, False) for k in partition], [ref_key(k, True) for k in order], [(v["values"], v["valid"]) for v in values]


def run(api, partition, order, values, calls, mem, lens=None, odd=False, nrows=0, raw=False):
    cols = partition + order + values
    n = rows_of(cols[0]) if cols else nrows
    lens = [n] if lens is None else lens
    assert sum(lens) == n
    chunks = [host_chunks(k, lens, odd) for k in cols]
    if mem == "device":
        chunks = [[to_device(c) for c in col] for col in chunks]
        torch.cuda.synchronize()
    np_, no_ = len(partition), len(order)
    pk = chunks[:np_]
    ok = [(col, k["desc"]) for col, k in zip(chunks[np_:np_ + no_], order)]
    return api.window_agg(pk, ok, chunks[np_ + no_:], calls, mem=mem, nrows=nrows, raw=raw)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def compare(got, exp, calls, slack, what):
    """got / exp: [(values, valid)] per call; slack[c]: the second term of the Float64 SUM bound per row, or None = bit for bit."""
    by_key = {(name, v, fr): i for i, (name, v, fr) in enumerate(calls)}
    for c, ((name, v, fr), (gv, gok), (ev, eok)) in enumerate(zip(calls, got, exp)):
        tag = (what, name, v, fr)
        assert gv.dtype == ev.dtype and gv.shape == ev.shape, tag
        assert np.array_equal(gok, eok), tag
        g, e = gv[eok], ev[eok]
        if ev.dtype != np.float64:
            assert np.array_equal(g, e), tag
        elif name in ("min", "max") or (name == "sum" and slack[c] is None):
            assert np.array_equal(bits(g), bits(e)), tag
        elif name == "sum":
            fin = np.isfinite(e)
            assert np.array_equal(bits(g[~fin]), bits(e[~fin])), tag          # NaN is the quiet NaN, infinities keep their sign
            err = np.abs(g[fin] - e[fin])
            bound = exact_ref.ulp_of(e[fin], np.zeros(fin.sum()), np.float64) + slack[c][eok][fin]
            worst = float((err / bound).max()) if fin.any() else 0.0
            print(f"{tag}: worst |got - F| / bound = {worst:.3g}")
            assert (err <= bound).all(), (tag, worst)
            assert not (np.signbit(g[fin]) & (g[fin] == 0)).any(), tag          # a zero sum is +0.0
        else:   # avg: one IEEE division of the same request's SUM by its COUNT
            s, k = got[by_key[("sum", v, fr)]], got[by_key[("count", v, fr)]]
            with np.errstate(invalid="ignore"):
                want = s[0][eok].astype(np.float64) / k[0][eok].astype(np.float64)
            assert np.array_equal(bits(g), bits(want)), tag


def check(api, partition, order, values, calls, lens=None, odd=False, nrows=0, fast=False, exact=False, mems=MEMS, what=""):
    """The calls in requests of up to 8, in host and in device memory, against the reference.  exact: sums bit for bit."""
    p, o, v = ref_args(partition, order, values)
    fn = R.frame_ref_fast if fast else R.frame_ref
    exp = fn(p, o, v, calls, nrows=nrows or None)
    slack = []
    for name, vi, fr in calls:
        is_f = vi >= 0 and values[vi]["values"].dtype == np.float64
        slack.append((R.sum_slack_fast if fast else R.sum_slack)(p, o, v[vi], fr, nrows=nrows or None) if name == "sum" and is_f and not exact else None)
    for mem in mems:
        got = []
        for at in range(0, len(calls), 8):
            got += run(api, partition, order, values, calls[at:at + 8], mem, lens, odd, nrows)
        compare(got, exp, calls, slack, (what, mem))
    return exp


def with_sum_count(calls):
    """Every avg call needs the sum and the count of its column and frame in the same request of 8: groups of five stay whole."""
    out = []
    for fr, v in calls:
        out += [(f, v, fr) for f in FIVE]
        out += [("count", -1, fr), ("first_value", -1, fr), ("last_value", -1, fr)]
    return out


def frames_of_width(w):
    """Every ROWS shape with both bounds finite and an unclipped length of w."""
    return [("rows", -(w - 1), 0), ("rows", 0, w - 1), ("rows", -(w // 2), w - 1 - w // 2), ("rows", -(w + 1), -2), ("rows", 2, w + 1)]


OPEN_FRAMES = [("rows", UP, 0), ("rows", 0, UF), ("rows", UP, UF), ("rows", UP, -1), ("rows", 1, UF), ("rows", UP, 3), ("rows", -3, UF),
               ("rows", UP, -4), ("rows", 4, UF), ("range", UP, 0), ("range", 0, 0), ("range", 0, UF), ("range", UP, UF)]


def partitions(rng, sizes, shuffle=True):
    ids = np.repeat(np.arange(len(sizes)), sizes)
    return ids[rng.permutation(len(ids))] if shuffle else ids


# ---------------------------------------------------------------- small cases, brute force

def test_the_header_s_frames_on_a_small_table(api):
    p = N(np.array([0, 0, 0, 0, 0, 1, 1], dtype=np.int64))
    o = N(np.arange(7, dtype=np.int32))
    x = N(np.array([1, 2, 3, 4, 5, 10, 20], dtype=np.int64))
    for mem in MEMS:
        got = run(api, [p], [o], [x], [("sum", 0, ("rows", 0, 1)), ("sum", 0, ("rows", 1, 2)), ("count", 0, ("rows", 2, 5)),
                                       ("min", 0, ("rows", 1, UF)), ("max", 0, ("rows", UP, -1)), ("avg", 0, ("rows", -1, 0)),
                                       ("last_value", -1, ("rows", 0, 1)), ("sum", 0, ("range", UP, 0))], mem)
        L = lambda pair: [v if k else None for v, k in zip(pair[0].tolist(), pair[1].tolist())]  # noqa: E731
        assert L(got[0]) == [3, 5, 7, 9, 5, 30, 20]
        assert L(got[1]) == [5, 7, 9, 5, None, 20, None]
        assert L(got[2]) == [3, 2, 1, 0, 0, 0, 0]
        assert L(got[3]) == [2, 3, 4, 5, None, 20, None]
        assert L(got[4]) == [None, 1, 2, 3, 4, None, 10]
        assert L(got[5]) == [1.0, 1.5, 2.5, 3.5, 4.5, 10.0, 15.0]
        assert L(got[6]) == [1, 2, 3, 4, 4, 6, 6]
        assert L(got[7]) == [1, 3, 6, 10, 15, 10, 30]


@pytest.mark.parametrize("w", [1, 2, 3, 64, 65])
def test_every_frame_shape_on_general_doubles_and_int64(api, w):
    rng = np.random.default_rng(100 + w)
    sizes = [1, 2, 3, 63, 64, 65, 66, 129, 130, 7, 500, 1, 700]
    ids = partitions(rng, sizes)
    n = len(ids)
    p, o = N(ids.astype(np.int32)), N(rng.integers(0, 40, n).astype(np.int16), desc=bool(w % 2))
    xf = N(rng.normal(size=n) * 10.0 ** rng.integers(-3, 6, n), rng.random(n) > 0.15)
    xi = N(rng.integers(-2**62, 2**62, n), rng.random(n) > 0.15)
    frames = frames_of_width(w) + (OPEN_FRAMES if w == 3 else [])
    check(api, [p], [o], [xf, xi], with_sum_count([(fr, 0) for fr in frames]), what=f"Float64, w={w}")
    calls = [(f, 1, fr) for fr in frames for f in ("sum", "min", "max", "count")]
    check(api, [p], [o], [xf, xi], calls, what=f"Int64, w={w}")


def test_frames_wider_than_every_partition_and_offsets_beyond_2_pow_32(api):
    rng = np.random.default_rng(7)
    n = 2000
    p, o = N(rng.integers(0, 5, n).astype(np.int64)), N(rng.permutation(n).astype(np.int32))
    x = N(np.round(rng.normal(size=n) * 100), rng.random(n) > 0.1)
    frames = frames_of_width(n + 5)[:3] + [("rows", -2**40, 2**50), ("rows", -2**62, 0), ("rows", 2**33, 2**34), ("rows", -2**40, -2**35)]
    exp = check(api, [p], [o], [x], with_sum_count([(fr, 0) for fr in frames]), exact=True, what="w > n")
    assert not exp[5 * 8][1].any() and (exp[5 * 8 + 3][0] == 0).all()      # 2^33 FOLLOWING .. : every frame is empty


def test_the_cancellation_case_a_plain_f64_prefix_fails(api):
    """Partition 0 is the issue's: 1e16, -1e16, then values near 1.  Partition 1 keeps the running sum at 1e16 while the values near
    1 pass (1e16, values near 1, -1e16): there a plain f64 prefix returns 0, 2 or 4 for a frame of three ones."""
    rng = np.random.default_rng(3)
    tail = 1.0 + rng.random(5000) * 1e-3
    x = np.concatenate([[1e16, -1e16], tail, [1e16], tail, [-1e16], rng.normal(size=3000)])
    ids = np.concatenate([np.zeros(2 + len(tail), dtype=np.int64), np.ones(2 + len(tail), dtype=np.int64), np.full(3000, 2, dtype=np.int64)])
    o = np.arange(len(x))
    frame = ("rows", -2, 0)
    calls = [("sum", 0, frame), ("count", 0, frame), ("avg", 0, frame), ("sum", 0, ("rows", UP, 0)), ("sum", 0, ("rows", -1, 1))]
    exp = check(api, [N(ids)], [N(o)], [N(x)], calls, what="1e16, -1e16, then values near 1")
    # the same frames from a plain f64 running sum miss the bound by far: the test would catch a kernel that did that
    first = 2 + len(tail)                                                    # partition 1 starts here
    cs = np.concatenate([[0.0], np.cumsum(x[first:first + 1 + len(tail)])])
    k = np.arange(3, len(tail) + 1)                                          # frames of three values near 1
    plain = cs[k + 1] - cs[k - 2]
    F = exp[0][0][first + k]
    assert (np.abs(F - 3.0) < 0.01).all() and (np.abs(plain - F) > 0.5).all()
    slack = R.sum_slack([(ids, None)], [(o, None, False)], (x, None), frame)[first + k]
    assert (np.abs(plain - F) > 1e6 * (exact_ref.ulp_of(F, np.zeros(len(F)), np.float64) + slack)).all()


def specials(rng, n):
    x = np.round(rng.normal(size=n) * 3)
    pick = rng.random(n)
    x[pick < 0.04] = np.nan
    x[(pick >= 0.04) & (pick < 0.06)] = np.array([0xFFF8000000000123], dtype=np.uint64).view(np.float64)[0]
    x[(pick >= 0.06) & (pick < 0.10)] = np.inf
    x[(pick >= 0.10) & (pick < 0.14)] = -np.inf
    x[(pick >= 0.14) & (pick < 0.22)] = -0.0
    x[(pick >= 0.22) & (pick < 0.30)] = 0.0
    return x


def test_infinities_nans_zeros_all_null_frames_and_empty_frames(api):
    rng = np.random.default_rng(17)
    n = 6000
    x = specials(rng, n)
    valid = rng.random(n) > 0.25
    valid[1000:1100] = False                                                 # runs of NULLs: all-NULL frames
    p, o = N(rng.integers(0, 12, n).astype(np.int32)), N(rng.permutation(n).astype(np.int64))
    frames = [("rows", -2, 0), ("rows", -1, 1), ("rows", 2, 5), ("rows", UP, 0), ("rows", 0, UF), ("rows", UP, UF), ("rows", 0, 0), ("range", 0, 0)]
    exp = check(api, [p], [o], [N(x, valid)], with_sum_count([(fr, 0) for fr in frames]), exact=True, what="specials")
    s, ok = exp[0]                                                           # SUM over ROWS 2 PRECEDING
    assert np.isnan(s[ok]).any() and np.isinf(s[ok]).any() and np.isfinite(s[ok]).any() and (~ok).any()
    # one partition in row order: frames that hold the NaN are NaN, the frames AFTER it are finite again
    y = np.array([1.0, 2.0, np.nan, 4.0, 5.0, 6.0, np.inf, 8.0, 9.0, 10.0, -np.inf, np.inf, 1.0, 1.0, 1.0])
    for mem in MEMS:
        (s, ok), (m, mok) = run(api, [], [], [N(y)], [("sum", 0, ("rows", -1, 0)), ("max", 0, ("rows", -1, 0))], mem)
        assert ok.all() and mok.all()
        assert s[:2].tolist() == [1.0, 3.0] and np.isnan(s[2:4]).all() and s[4:6].tolist() == [9.0, 11.0]
        assert s[6:8].tolist() == [np.inf, np.inf] and s[8:10].tolist() == [17.0, 19.0] and s[10] == -np.inf and np.isnan(s[11])
        assert s[12] == np.inf and s[13:].tolist() == [2.0, 2.0]
        assert m[2] == 2.0 and m[3] == 4.0 and m[11] == np.inf
    # 2 FOLLOWING .. 5 FOLLOWING at a partition's end: the last two rows of every partition have an empty frame
    c = exp[2 * 8 + 5]                                                       # COUNT(*) of that frame
    assert (c[0] == 0).sum() >= 2 * 12 - 2 and c[1].all()
    assert not exp[2 * 8 + 6][1][c[0] == 0].any()                            # FIRST_VALUE is NULL there
    # Int64 extremes are values, not NULLs
    xi = np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min, 5, np.iinfo(np.int64).max, np.iinfo(np.int64).min], dtype=np.int64)
    vi = np.array([1, 1, 0, 1, 1], dtype=bool)
    check(api, [], [], [N(xi, vi)], [(f, 0, fr) for fr in (("rows", 0, 0), ("rows", -1, 0), ("rows", UP, UF)) for f in ("min", "max", "sum", "count")],
          what="Int64 extremes")


# ---------------------------------------------------------------- large cases, the vectorised reference

SEG = 4096


@pytest.mark.parametrize("w", [1, 2, 3, 64, 65, 4096, 10**6])
def test_partitions_around_the_scan_segments_and_one_across_several(api, w):
    """Partition starts inside a segment and on segment boundaries, partitions shorter than, equal to and longer than w, one of
    20 000 rows across several segments.  Integer-valued doubles and Int64: every result bit for bit."""
    rng = np.random.default_rng(200 + w % 1000)
    sizes = [SEG, SEG - 1, 1, SEG + 1, 2 * SEG, 3, 64, 65, 63, SEG - 132, 20_000 + 5, 2, 2 * SEG - 2, 100, SEG, 7]
    for shuffle in (False, True):                                            # sorted input: the starts are exactly where `sizes` says
        ids = partitions(rng, sizes, shuffle)
        n = len(ids)
        p, o = N(ids.astype(np.int64)), N((np.arange(n) if not shuffle else rng.permutation(n)).astype(np.int32))
        xf = N(rng.integers(-1000, 1000, n).astype(np.float64), rng.random(n) > 0.2)
        xi = N(rng.integers(-2**40, 2**40, n), rng.random(n) > 0.2)
        frames = frames_of_width(w) + (OPEN_FRAMES if w == 64 else [])
        check(api, [p], [o], [xf, xi], with_sum_count([(fr, 0) for fr in frames]), fast=True, exact=True, what=f"Float64 w={w} shuffle={shuffle}")
        check(api, [p], [o], [xf, xi], [(f, 1, fr) for fr in frames for f in ("sum", "min", "max", "count")], fast=True, what=f"Int64 w={w}")


def test_2e6_rows(api):
    rng = np.random.default_rng(301)
    n = 2_000_000
    p = N(rng.integers(0, 300, n).astype(np.int32))
    o = N(rng.integers(0, 5000, n).astype(np.int64), desc=True)
    x = N(rng.integers(-100, 100, n).astype(np.float64), rng.random(n) > 0.1)
    frames = [("rows", -9, 0), ("rows", -100, 100), ("range", UP, 0), ("rows", 0, UF)]
    check(api, [p], [o], [x], with_sum_count([(fr, 0) for fr in frames]), fast=True, exact=True, what="2e6 rows")


# ---------------------------------------------------------------- keys, chunkings, requests

def city_rows(rng, n, null_frac=0.0):
    words = [b"Aberdeen", b"Bath", b"Bat", b"Bath\0", b"", b"\0", b"Birmingham", b"Bristol", b"York", b"Z\xc3\xbcrich", b"\xff"]
    return [None if rng.random() < null_frac else words[int(rng.integers(0, len(words)))] for _ in range(n)]


def test_utf8_partition_and_order_keys_no_keys_and_odd_chunkings(api):
    rng = np.random.default_rng(41)
    n = 7001
    t1, t2 = T(city_rows(rng, n, 0.05)), T(city_rows(rng, n, 0.05), desc=True)
    k = N(rng.integers(0, 4, n).astype(np.uint16), rng.random(n) > 0.1)
    x = N(np.round(rng.normal(size=n) * 50), rng.random(n) > 0.1)
    y = N(rng.integers(-10**6, 10**6, n))
    # (column 1 is Int64 with sums far below 2^53: its AVG, through the Float64 path, equals its Int64 SUM / COUNT exactly)
    calls = with_sum_count([(("rows", -3, 2), 0), (("range", UP, 0), 0), (("rows", UP, UF), 1), (("rows", -70, 0), 1)])
    check(api, [t1], [k], [x, y], calls, exact=True, what="Utf8 partition key")
    check(api, [k], [t2], [x, y], calls, exact=True, what="Utf8 order key, descending")
    uneven = [1, 900, 13, 2500, 64, 3000, 523]
    assert sum(uneven) == n
    for lens, odd, what in ((uneven, False, "7 uneven chunks"), ([0, 0, 4000, 0, 3001, 0], False, "empty chunks"),
                            ([n], True, "one chunk behind an offset"), (uneven, True, "7 chunks, offsets, validity at odd bits")):
        check(api, [t1, k], [t2], [x, y], calls, lens=lens, odd=odd, exact=True, what=what)
    # no keys at all: one partition in row order, every row a peer; the value chunks give the rows
    check(api, [], [], [x, y], calls, lens=uneven, odd=True, exact=True, what="no keys")
    check(api, [], [], [x, y], calls, nrows=n, exact=True, what="no keys, nrows repeated")
    # no keys and no values: nrows_if_no_keys gives the rows
    exp = R.frame_ref([], [], [], [("count", -1, ("rows", -2, 1)), ("first_value", -1, ("rows", 1, 1))], nrows=50)
    for mem in MEMS:
        got = api.window_agg([], [], [], [("count", -1, ("rows", -2, 1)), ("first_value", -1, ("rows", 1, 1))], mem=mem, nrows=50)
        compare(got, exp, [("count", -1, ("rows", -2, 1)), ("first_value", -1, ("rows", 1, 1))], [None, None], "no keys, no values")
    z = N(np.zeros(0))
    for mem in MEMS:
        got = run(api, [N(np.zeros(0, dtype=np.int64))], [], [z], [("sum", 0, ("rows", UP, 0)), ("count", -1, ("rows", UP, 0))], mem, lens=[0, 0])
        assert [g[0].shape for g in got] == [(0,), (0,)]


def test_eight_calls_four_value_columns_eight_frames_equal_the_single_calls(api):
    rng = np.random.default_rng(51)
    n = 30_000
    p, o = N(rng.integers(0, 9, n).astype(np.int8)), N(rng.integers(0, 2000, n).astype(np.int32))
    vals = [N(rng.normal(size=n) * 1e3, rng.random(n) > 0.1), N(rng.integers(-2**50, 2**50, n), rng.random(n) > 0.1),
            N(specials(rng, n)), N(rng.integers(-5, 5, n))]
    calls = [("sum", 0, ("rows", -5, 0)), ("avg", 1, ("rows", -4096, 4095)), ("min", 2, ("rows", -64, 0)), ("max", 3, ("range", 0, 0)),
             ("count", 2, ("rows", 1, UF)), ("sum", 1, ("range", UP, 0)), ("last_value", -1, ("rows", 2, 5)), ("max", 0, ("rows", UP, -1))]
    assert len({c[2] for c in calls}) == 8 and {c[1] for c in calls} >= {0, 1, 2, 3}
    for mem in MEMS:
        together = run(api, [p], [o], vals, calls, mem, raw=True)
        t_np = [A.Api.window_agg_to_numpy(x) for x in together]
        for c, call in enumerate(calls):
            alone = run(api, [p], [o], vals, [call], mem, raw=True)[0]
            assert alone.null_count == together[c].null_count, (mem, call)
            av, aok = A.Api.window_agg_to_numpy(alone)
            assert np.array_equal(aok, t_np[c][1]) and av.dtype == t_np[c][0].dtype, (mem, call)
            assert av[aok].tobytes() == t_np[c][0][aok].tobytes(), (mem, call)      # identical, bit for bit
            assert alone.null_count == int((~aok).sum())
    pr, orr, vr = ref_args([p], [o], vals)
    exp = R.frame_ref(pr, orr, vr, [calls[2], calls[3], calls[4], calls[6]])
    compare([t_np[2], t_np[3], t_np[4], t_np[6]], exp, [calls[2], calls[3], calls[4], calls[6]], [None] * 4, "together vs reference")


def test_first_and_last_value_through_take_and_utf8_take(api):
    rng = np.random.default_rng(61)
    n = 4000
    p, o = N(rng.integers(0, 30, n).astype(np.int32)), N(rng.integers(0, 1000, n).astype(np.int64))
    vals, vvalid = rng.normal(size=n), rng.random(n) > 0.1
    words = city_rows(rng, n, 0.1)
    fcol, tcol = A.HostArray.from_numpy(vals, vvalid), utf8(words)
    flist = [float(v) if k else None for v, k in zip(vals, vvalid)]
    calls = [("first_value", -1, ("rows", -2, -1)), ("last_value", -1, ("rows", 0, UF)), ("first_value", -1, ("range", 0, 0))]
    pr, orr, _ = ref_args([p], [o], [])
    exp = R.frame_ref(pr, orr, [], calls)
    for mem in MEMS:
        outs = run(api, [p], [o], [], calls, mem, raw=True)
        for out, (idx, ok) in zip(outs, exp):
            assert out.null_count == int((~ok).sum())
            if mem == "host":
                got_f = api.take([fcol], out).to_pylist()
                got_t = api.utf8_take([tcol], out)
            else:
                t = torch.zeros(n + 64, dtype=torch.float64, device="cuda")
                v = torch.zeros((n + 63) // 64 * 8 + 8, dtype=torch.uint8, device="cuda")
                dout = A.DeviceArray(t.data_ptr(), v.data_ptr(), 0, n, A.F64, 0, keep=(t, v))
                api.take([to_device(fcol)], out, dout)
                torch.cuda.synchronize()
                hv = A.unpack_bits(v.cpu().numpy(), 0, n)
                got_f = [float(x) if k else None for x, k in zip(t[:n].cpu().numpy(), hv)]
                got_t = api.utf8_take([to_device(tcol)], out).to_host()
            assert got_f == window_ref.gather(flist, idx, ok), mem                  # a NULL value is a value here: not skipped
            o_, raw_ = got_t.offsets[got_t.offset:got_t.offset + n + 1].astype(np.int64) + got_t.data_offset, got_t.data.tobytes()
            got_rows = [raw_[o_[i]:o_[i + 1]] if k else None for i, k in enumerate(got_t.valid_mask())]
            assert got_rows == window_ref.gather(words, idx, ok), mem


def test_rdf_window_on_the_same_keys_is_unchanged_by_the_shared_front(api):
    rng = np.random.default_rng(71)
    n = 50_000
    p = N(rng.integers(0, 40, n).astype(np.int64), rng.random(n) > 0.05)
    o = N(np.round(rng.normal(size=n), 1), rng.random(n) > 0.05, desc=True)
    x = N(rng.integers(-9, 9, n).astype(np.float64))
    calls = ["row_number", "rank", "dense_rank", "percent_rank", "cume_dist", ("ntile", 7), ("lag", 1), ("lead", 2)]
    exp = window_ref.window_ref([ref_key(p, False)], [ref_key(o, True)], calls)
    for mem in MEMS:
        run(api, [p], [o], [x], [("sum", 0, ("rows", -3, 0)), ("min", 0, ("rows", -3, 3))], mem)
        chunks = [host_chunks(k, [n], False) for k in (p, o)]
        if mem == "device":
            chunks = [[to_device(c) for c in col] for col in chunks]
        got = api.window([chunks[0]], [(chunks[1], True)], calls, mem=mem)
        assert "wagg" not in lib.last_kernel() and lib.last_kernel().endswith("win_flags_kernel + win_starts_kernel + win_emit_kernel")
        for g, e in zip(got, exp):
            if isinstance(e, tuple):
                assert np.array_equal(g[1], e[1]) and np.array_equal(g[0][e[1]], e[0][e[1]])
            elif e.dtype == np.float64:
                assert np.array_equal(bits(g), bits(e))
            else:
                assert np.array_equal(g, e)
