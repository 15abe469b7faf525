"""rdf_groupby_agg on the MI355X, every planner path held to tests/groupby_ref.py (never to the oracle): gb2_stream_kernel in each
replica layout, the line-aligned scatter + aggregate path in its record and table forms, the capacity plan, the heavy-hitter
split, the single table in HBM, the first-generation combining path, and the hand-overs between them.

Every case runs in host and in device memory, asserts by lib.last_kernel() WHICH path answered before it compares, and puts
the options it changes back.  Two value families per case (groupby_ref): integer-valued data with distinct magnitudes per row
within a group (every sum exact in any order: bit for bit) and general doubles (the any-order bound); for MIN / MAX the special
floats, with groups that hold only NaN, only zeros of both signs and only NULLs.  Keys include the ends of their type, the key
whose hash is the LDS free marker and a NULL key; chunks are ragged (an empty one, element offsets, validity at odd bits).
Output capacities are min(max_groups, rows) + 2, the least the header allows.

Smallest shape that reached each path (kernel name, and the engine's RDF_DEBUG lines for what the name does not say):
  stream, 32 / 16 / 8 / 4 / 2 / 1 sub-tables      1 row (max_groups 55 ... 2048; the debug line names the layout)
  scatter, 16- / 12- / 4-byte records, both tables  1 row under gb_partition = 4 (the debug line names the table form); 2049 rows is
                                                    the first with two blocks, 40 001 the first that carries between super-tiles
  planner cuts                                      5000 rows at max_groups 2048 | 2049 and 1 305 600 | 1 305 601
  12-byte records of 8-byte keys, window and miss   40 001 rows, 3000 groups
  capacity plan                                     40 001 rows, 3000 groups, gb_skew_plan = 2, gb_hot = 0
  region overflow (flag 16) -> first generation / HBM table      40 001 rows, half in one key
  LDS table full (flag 32) -> HBM table             405 000 rows.  GREW from 9000: 9000 one-row keys of one partition overflow that
                                                    partition's scatter regions first (flag 16); 46 of them per block do not
  heavy-hitter split                                1 100 000 rows (65 536 samples at one row in 16, plus the sampled NULL keys)
  the split gives up                                through flag 16 — 400 unsampled rows of one key in one super-tile.  A hot class with
                                                    many distinct keys cannot do it: only the up to 100 hot KEYS enter the hot table
  key columns                                       5000 rows (range-packed 2 / 3 / 4 columns, dictionary-coded, full-range nullable);
                                                    the 64-bit refusal needs 66 000 rows (17 bits a column even dictionary-coded)
Measured on an MI355X: the file's 91 cases 25.4 s, test_heavy_hitter_split 5.3 s, test_lds_table_full_hands_over 2.4 s, every
other case under 0.6 s.

What these tests found.  (1) gb2_finish_kernel and key_unpack_kernel took `__ballot(in)` under `lane == 0`, so null_count of
out_values (MIN / MAX) and of every unpacked key output counted lane 0 only: wrong on every path.  (2) max_groups: with the NULL
key or the marker key among d distinct keys, max_groups = d - 1 came back as d groups (seen on the forced scatter path; by the
code the stream path, the HBM table, the capacity plan, the split, the first-generation path and the streamed loop did the same:
each checked only the groups its tables held).  Both are fixed; the oracle had the same slack and did not order the two zeros.
"""
import contextlib
import re

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
import groupby_ref as G
import hash_models as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MEMS = ["host", "device"]
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
FREE = H.G2_FREE_KEY
K_G2_MAX_GROUPS = 256 * 5100          # kG2MaxGroups
DEFAULTS = {"gb_partition": 3, "gb_skew_plan": 1, "gb_hot": 1, "gb_compact": 1, "gb_bucket": 0}

STREAM, TABLE, FIRST_GEN = "gb2_stream_kernel", "gb2_table_rows_kernel", "gb_aggregate_kernel"
SCATTER = "gb2_scatter_kernel+gb2_aggregate_kernel"


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


@contextlib.contextmanager
def options(**kw):
    try:
        for k, v in kw.items():
            lib.set_option(k, v)
        yield
    finally:
        for k in kw:
            lib.set_option(k, DEFAULTS[k])


# ---------------------------------------------------------------- calls
def to_device(x):
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def to_host(out):
    if isinstance(out, A.HostArray):
        return out
    t, v = out.keep
    vals = t.cpu().numpy().view(A.NP_OF[out.dtype])[:max(out.length, 1)].copy()
    return A.HostArray(vals, v.cpu().numpy() if v is not None else None, 0, out.length, out.dtype, out.null_count)


def call(api, cols, vals, agg, max_groups, mem):
    """-> (keys, values, counts) as host arrays."""
    device = mem == "device"
    rows = sum(c.length for c in cols[0])
    cap = min(max_groups, rows) + 2
    vdt = None if vals is None or agg == "count" else vals[0].dtype
    outs = ([A.Api._window_out(col[0].dtype, cap, device, True) for col in cols], A.Api._window_out(G.out_dtype(agg, vdt), cap, device, True),
            A.Api._window_out(A.I64, cap, device, False))
    if device:
        cols = [[to_device(c) for c in col] for col in cols]
        vals = None if vals is None else [to_device(c) for c in vals]
    ok, ov, oc = api.groupby_agg(cols, vals, agg, max_groups, outs=outs)
    return [to_host(k) for k in ok], to_host(ov), to_host(oc)


def names(kernel):
    """A kernel name, or a predicate over it."""
    return kernel if callable(kernel) else (lambda name: name == kernel)


def check(api, cols, vals, agg, max_groups, kernel, what, exact=False):
    model = G.groupby(cols, vals, agg, max_groups)
    for mem in MEMS:
        w = f"{what}, {agg}, max_groups {max_groups}, {mem}"
        if isinstance(model, G.Failure):
            G.expect_failure(lambda: call(api, cols, vals, agg, max_groups, mem), model, w)
            continue
        got = G.groups_of(*call(api, cols, vals, agg, max_groups, mem))
        assert names(kernel)(lib.last_kernel()), f"{w}: answered by {lib.last_kernel()!r}"
        G.check_groupby(got, model, agg, w, max_groups=max_groups, floats_exact=exact)
    return model


# ---------------------------------------------------------------- inputs
def distinct_keys(rng, dt, count, specials=()):
    """`count` distinct keys of the dtype, `specials` among them, the others drawn over the whole range of the type."""
    info = np.iinfo(A.NP_OF[dt])
    have = list(dict.fromkeys(int(s) for s in specials if info.min <= s <= info.max))[:count]
    count = min(count, info.max - info.min + 1)
    seen = set(have)
    while len(have) < count:
        for x in rng.integers(info.min, info.max, 2 * (count - len(have)) + 8, dtype=A.NP_OF[dt], endpoint=True).tolist():
            if x not in seen and len(have) < count and x != FREE:
                seen.add(x)
                have.append(x)
    return have


def spread(rng, dt, n, pool, weights=None):
    """n rows over the pool (None = the NULL key): every entry at least once where n allows it.  -> (keys, valid | None, group id)."""
    d = len(pool)
    idx = rng.permutation(np.concatenate([np.arange(d), rng.choice(d, n - d, p=weights)]) if n >= d else rng.permutation(d)[:n])
    table = np.array([0 if p is None else p for p in pool], dtype=A.NP_OF[dt])
    null = np.array([p is None for p in pool], dtype=bool)
    valid = ~null[idx]
    return table[idx], (valid if null.any() else None), idx


def specials_of(dt):
    info = np.iinfo(A.NP_OF[dt])
    out = [info.min, info.max]
    if dt in (A.I64, A.U64):
        out += [FREE, 1 << 63 if dt == A.U64 else 0]
    return out


def value_runs(rng, gid, aggs=G.AGGS):
    """-> [(agg, values | None as (data, valid), exact)]: the two value families of every aggregate, COUNT once."""
    n = len(gid)
    nulls = rng.uniform(size=n) >= 0.1
    labels = np.unique(gid)
    plant = [int(labels[i * (len(labels) - 1) // 3]) if len(labels) >= 4 else -1 - i for i in (1, 2, 3)]
    runs = []
    for agg in aggs:
        if agg == "count":
            runs.append((agg, None, True))
        elif agg == "sum":
            runs.append((agg, (G.exact_values(rng, gid, np.float64), nulls), True))
            runs.append((agg, (G.general_values(rng, n), nulls), False))
        else:
            runs.append((agg, (G.exact_values(rng, gid, np.int64), nulls), True))
            runs.append((agg, G.plant_groups(G.special_values(rng, n), nulls, gid, *plant), True))
    return runs


def run_all(api, rng, cols, gid, max_groups, kernel, what, aggs=G.AGGS, cuts=None):
    for agg, v, exact in value_runs(rng, gid, aggs):
        vals = None if v is None else G.ragged(v[0], v[1], rng, cuts)
        k = kernel(agg, vals) if getattr(kernel, "per_agg", False) else kernel
        check(api, cols, vals, agg, max_groups, k, f"{what} ({'no values' if v is None else v[0].dtype})", exact)


def per_agg(fn):
    fn.per_agg = True
    return fn


def promise(api, rng, dt, n, d, kernel, what, agg="count", weights=None):
    """The max_groups promise: d distinct keys with max_groups = d succeed, max_groups = d - 1 is RDF_MEMORY_ERROR — with the NULL
    key and the key whose hash is the free marker among the d (the two groups no table ever holds) and without them."""
    for with_specials in (True, False):
        pool = distinct_keys(rng, dt, d - 1 if with_specials else d, specials_of(dt) if with_specials else ())
        pool = pool + [None] if with_specials else pool
        assert len(pool) == d and (not with_specials or dt not in (A.I64, A.U64) or FREE in pool)
        kv, valid, gid = spread(rng, dt, n, pool, weights)
        cols = [G.ragged(kv, valid, rng)]
        vals = None if agg == "count" else G.ragged(G.exact_values(rng, gid, np.float64), None, rng)
        w = f"{what}, promise {'with' if with_specials else 'without'} the set-aside keys"
        model = check(api, cols, vals, agg, d, kernel, w, exact=True)
        assert len(model) == d
        check(api, cols, vals, agg, d - 1, kernel, w)


# ---------------------------------------------------------------- gb2_stream_kernel
@pytest.mark.parametrize("kdt", [A.I8, A.U64])
@pytest.mark.parametrize("max_groups", [55, 56, 119, 120, 244, 245, 497, 498, 995, 996, 2048])
def test_stream_path_every_replica_layout(api, max_groups, kdt, monkeypatch, capfd):
    """max_groups on either side of every step of `prime_slots[r + 1] >= 2 * max_groups + 2` (32, 16, 8, 4, 2 and 1 sub-tables), with
    as many distinct keys as max_groups, the rows and the key type allow, the NULL key and (UInt64) the marker key among them."""
    rng = np.random.default_rng(1000 * max_groups + kdt)
    replicas = {55: 32, 56: 16, 119: 16, 120: 8, 244: 8, 245: 4, 497: 4, 498: 2, 995: 2, 996: 1, 2048: 1}[max_groups]
    monkeypatch.setenv("RDF_DEBUG", "1")
    capfd.readouterr()
    for n in (1, 1023, 1025, 5000):
        d = min(max_groups, n, 257 if kdt == A.I8 else n)
        pool = distinct_keys(rng, kdt, d - 1 if d > 1 else 1, specials_of(kdt)) + ([None] if d > 1 else [])
        kv, valid, gid = spread(rng, kdt, n, pool)
        run_all(api, rng, [G.ragged(kv, valid, rng)], gid, max_groups, STREAM, f"stream, {n} rows, {d} keys of {kdt}")
    layouts = re.findall(r"gb2 stream path: (\d+) sub-tables", capfd.readouterr().err)      # the engine's debug line names the layout
    assert len(layouts) == 4 * 7 * len(MEMS) and set(layouts) == {str(replicas)}, (replicas, set(layouts), len(layouts))
    if kdt == A.U64:
        promise(api, rng, kdt, 5000, max_groups, STREAM, "stream")


# ---------------------------------------------------------------- planner cuts
@pytest.mark.parametrize("max_groups,partition,kernel", [(2048, 3, STREAM), (2049, 3, SCATTER), (K_G2_MAX_GROUPS, 3, SCATTER), (K_G2_MAX_GROUPS + 1, 3, TABLE),
                                                         (2048, 0, TABLE), (2049, 0, TABLE), (K_G2_MAX_GROUPS, 0, TABLE)])
def test_planner_cuts(api, max_groups, partition, kernel):
    """5000 rows on either side of kG2StreamGroups (2048) and of kG2MaxGroups (1 305 600); gb_partition = 0 is the HBM table at
    every size.  The outputs hold min(max_groups, rows) + 2 groups."""
    rng = np.random.default_rng(max_groups + partition)
    n = 5000
    d = min(max_groups, 3000)
    pool = distinct_keys(rng, A.I64, d - 1, specials_of(A.I64)) + [None]
    kv, valid, gid = spread(rng, A.I64, n, pool)
    with options(gb_partition=partition):
        run_all(api, rng, [G.ragged(kv, valid, rng)], gid, max_groups, kernel, f"cut at {max_groups}, gb_partition {partition}")


# ---------------------------------------------------------------- the scatter path, forced
@pytest.mark.parametrize("bucket", [0, 1, 4])
@pytest.mark.parametrize("compact", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2047, 2049, 40_001])
def test_scatter_path_records_and_tables(api, n, compact, bucket, monkeypatch, capfd):
    """1, 1, 2 and 20 scatter blocks (the larger sizes carry between super-tiles) x 16-, 12- and 4-byte records x the aggregate
    pass's two table forms, on keys packed into [0, ngroups) (Int32 / UInt16: the compact records of narrow types, their type's
    ends and a NULL key included) and on keys drawn over all 64 bits.  gb_bucket = 1 on random keys — one key per probe where
    keys do collide — and gb_bucket = 4 on packed keys are the combinations nothing else reaches."""
    rng = np.random.default_rng(10 * n + 3 * compact + bucket)
    d = min(n, 1500)
    narrow = A.I32 if (n + compact) % 2 else A.U16

    @per_agg
    def narrow_kernel(agg, vals):
        twelve = compact == 2 or (compact == 1 and (vals is None or agg == "count"))
        return SCATTER + (" (12-byte records)" if twelve else "")

    monkeypatch.setenv("RDF_DEBUG", "1")
    capfd.readouterr()
    with options(gb_partition=4, gb_compact=compact, gb_bucket=bucket):
        info = np.iinfo(A.NP_OF[narrow])
        pool = list(dict.fromkeys(list(range(d - 3)) + [info.min, info.max])) + [None] if d > 3 else [5]
        kv, valid, gid = spread(rng, narrow, n, pool)
        run_all(api, rng, [G.ragged(kv, valid, rng)], gid, d, narrow_kernel, f"scatter, packed keys of {narrow}, {n} rows, gb_compact {compact}, gb_bucket {bucket}")
        pool = distinct_keys(rng, A.I64, d - 1, specials_of(A.I64)) + [None] if d > 1 else [FREE]
        kv, valid, gid = spread(rng, A.I64, n, pool)
        # (one row: one key, whose span of 0 fits any window — compact records where the option allows them)
        wide_kernel = SCATTER if n > 1 else narrow_kernel
        run_all(api, rng, [G.ragged(kv, valid, rng)], gid, d, wide_kernel, f"scatter, 64-bit keys, {n} rows, gb_compact {compact}, gb_bucket {bucket}")
    tables = re.findall(r"gb2 aggregate pass: ([a-z ]+)", capfd.readouterr().err)             # the engine's debug line names the table form
    assert len(tables) >= 2 * 7 * len(MEMS)
    if bucket:
        assert set(tables) == {"one key per probe" if bucket == 1 else "buckets of four"}, set(tables)


def test_scatter_path_keeps_the_max_groups_promise(api):
    rng = np.random.default_rng(77)
    with options(gb_partition=4):
        promise(api, rng, A.I64, 5000, 3000, SCATTER, "scatter")
        promise(api, rng, A.I64, 5000, 3000, SCATTER, "scatter", agg="sum")
    with options(gb_partition=4, gb_compact=2):
        promise(api, rng, A.I32, 5000, 3000, SCATTER + " (12-byte records)", "scatter, 12-byte records", agg="sum")
    with options(gb_partition=0):
        promise(api, rng, A.I64, 5000, 3000, TABLE, "HBM table")
        promise(api, rng, A.I64, 5000, 3000, TABLE, "HBM table", agg="min")


def call_sum(api, keys, vals, max_groups, mem):
    """rdf_groupby_sum -> (keys, sums, counts) as host arrays."""
    device = mem == "device"
    cap = min(max_groups, sum(c.length for c in keys)) + 2
    sdt = A.F64 if vals is not None and vals[0].dtype in G.FLOATS else A.I64
    outs = (A.Api._window_out(keys[0].dtype, cap, device, True), A.Api._window_out(sdt, cap, device, False), A.Api._window_out(A.I64, cap, device, False))
    if device:
        keys = [to_device(c) for c in keys]
        vals = None if vals is None else [to_device(c) for c in vals]
    ok, ov, oc = api.groupby_sum(keys, vals, max_groups, outs=outs)
    return [to_host(ok)], to_host(ov), to_host(oc)


@pytest.mark.parametrize("partition,kernel", [(3, SCATTER), (1, FIRST_GEN)])
def test_groupby_sum_keeps_the_max_groups_promise(api, partition, kernel):
    """rdf_groupby_sum: through rdf_groupby_agg by default, on the first-generation path under gb_partition = 1.  3000 distinct keys
    in 5000 rows, the NULL key and the marker key among them or not."""
    rng = np.random.default_rng(21 + partition)
    n, d = 5000, 3000
    with options(gb_partition=partition):
        for with_specials in (True, False):
            pool = distinct_keys(rng, A.I64, d - 1, specials_of(A.I64)) + [None] if with_specials else distinct_keys(rng, A.I64, d)
            kv, valid, gid = spread(rng, A.I64, n, pool)
            keys = G.ragged(kv, valid, rng)
            for vals in (G.ragged(G.exact_values(rng, gid, np.float64), rng.uniform(size=n) >= 0.1, rng), G.ragged(G.exact_values(rng, gid, np.int32), None, rng), None):
                agg = "sum" if vals is not None else "count"
                model = G.groupby(keys, vals, agg)
                assert len(model) == d
                for mem in MEMS:
                    w = f"groupby_sum, gb_partition {partition}, {'with' if with_specials else 'without'} the set-aside keys, {mem}"
                    got = G.groups_of(*call_sum(api, keys, vals, d, mem))
                    assert lib.last_kernel().startswith(kernel), f"{w}: answered by {lib.last_kernel()!r}"
                    G.check_groupby(got, model, agg, w, max_groups=d, floats_exact=True)
                    G.expect_failure(lambda: call_sum(api, keys, vals, d - 1, mem), G.groupby(keys, vals, agg, d - 1), w)


# ---------------------------------------------------------------- every value dtype
@pytest.mark.parametrize("partition,kernel", [(3, STREAM), (4, SCATTER), (0, TABLE)])
def test_every_value_dtype(api, partition, kernel):
    """Integer values over the whole range of their type (sign- and zero-extension, sums that wrap, UInt64 extremes above 2^63
    through the UInt64 output) and Float32 / Float64 with the special floats (sums by kind, Float32 widened exactly), 5000 rows."""
    rng = np.random.default_rng(40 + partition)
    n, d = 5000, 1500
    pool = distinct_keys(rng, A.I64, d - 1, specials_of(A.I64)) + [None]
    kv, valid, gid = spread(rng, A.I64, n, pool)
    cols = [G.ragged(kv, valid, rng)]
    with options(gb_partition=partition):
        for vdt in (A.I8, A.I16, A.I32, A.I64, A.U8, A.U16, A.U32, A.U64, A.F32, A.F64):
            npdt = A.NP_OF[vdt]
            v = G.special_values(rng, n, npdt) if vdt in G.FLOATS else rng.integers(np.iinfo(npdt).min, np.iinfo(npdt).max, n, dtype=npdt, endpoint=True)
            vals = G.ragged(v, rng.uniform(size=n) >= 0.1, rng)
            for agg in ("sum", "min", "max"):
                check(api, cols, vals, agg, d, kernel, f"values of {vdt}, gb_partition {partition}")


# ---------------------------------------------------------------- 12-byte records of 8-byte keys: the 2^39 window
@pytest.mark.parametrize("case", ["middle", "bottom of i64", "top of i64", "bottom of u64", "top of u64", "outlier"])
def test_compact_records_key_window(api, case):
    """40 001 rows, 3000 groups, gb_compact = 2: a window in the middle of the key range, clamped at either end of i64 and of u64
    (the end itself is a key), and one key outside the window at a row the probe does not sample (rows 0, 16, 32, ... of a tile
    are sampled) — the scatter notices, and the call answers from 16-byte records."""
    rng = np.random.default_rng(len(case))
    n, d = 40_001, 3000
    base = np.arange(d - 1, dtype=np.int64)
    dt = A.U64 if "u64" in case else A.I64
    keys = {"middle": base * 3 + (1 << 40) - 4000, "bottom of i64": I64_MIN + base * 5, "top of i64": I64_MAX - base * 5,
            "bottom of u64": base.astype(np.uint64) * np.uint64(7), "top of u64": np.uint64(2 ** 64 - 1) - base.astype(np.uint64) * np.uint64(7),
            "outlier": base * 11 - 77}[case]
    pool = [int(k) for k in keys.tolist()] + [None]
    kv, valid, gid = spread(rng, dt, n, pool)
    if case == "outlier":
        kv[1], valid[1], gid[1] = 1 << 45, True, d            # row 1 of the first tile is not sampled
        pool.append(1 << 45)
    cols = [[A.HostArray.from_numpy(kv, valid=valid, offset=3, rng=rng)]] if case == "outlier" else [G.ragged(kv, valid, rng)]
    cuts = [n] if case == "outlier" else None
    with options(gb_partition=4, gb_compact=2):
        run_all(api, rng, cols, gid, len(pool), SCATTER + ("" if case == "outlier" else " (12-byte records)"), f"key window: {case}", cuts=cuts)


# ---------------------------------------------------------------- the capacity plan
@pytest.mark.parametrize("keys", ["a third in one key", "even"])
def test_capacity_plan(api, keys):
    """gb_skew_plan = 2, gb_hot = 0 at 40 001 rows and 3000 groups: one key holding a third of the rows (its partition is cut into
    one aggregate item per scatter block, whose groups meet in the global table) and even keys."""
    rng = np.random.default_rng(len(keys))
    n, d = 40_001, 3000
    pool = distinct_keys(rng, A.I64, d - 1, specials_of(A.I64)) + [None]
    weights = None
    if keys != "even":
        weights = np.full(d, (2 / 3) / (d - 1))
        weights[7] = 1 / 3
    kv, valid, gid = spread(rng, A.I64, n, pool, weights)
    with options(gb_partition=4, gb_skew_plan=2, gb_hot=0):
        run_all(api, rng, [G.ragged(kv, valid, rng)], gid, d, SCATTER + " (capacity plan)", f"capacity plan, {keys}")
        promise(api, rng, A.I64, n, d, SCATTER + " (capacity plan)", f"capacity plan, {keys}", weights=weights)


# ---------------------------------------------------------------- hand-over: a scatter region overflows
def _debug_flags(err):
    return [int(x, 16) for x in re.findall(r"gb2 partition path: .* flags=0x([0-9a-f]+)", err)]


@pytest.mark.parametrize("partition", [3, 4])
def test_region_overflow_hands_over(api, partition, monkeypatch, capfd):
    """40 001 rows, half of them in one key, max_groups = 3000 distinct keys: a block's 2048 rows put about 1024 records into a
    region of 56.  Default options: sum and count answer from the first-generation combining path, min and max from the HBM
    table; with gb_partition = 4 the HBM table always.  The engine's debug line shows that the scatter path gave up on flag 16."""
    rng = np.random.default_rng(5 + partition)
    n, d = 40_001, 3000
    pool = distinct_keys(rng, A.I64, d - 1, specials_of(A.I64)) + [None]
    weights = np.full(d, 0.5 / (d - 1))
    weights[11] = 0.5
    kv, valid, gid = spread(rng, A.I64, n, pool, weights)
    monkeypatch.setenv("RDF_DEBUG", "1")

    @per_agg
    def kernel(agg, vals):
        first_gen = partition == 3 and agg in ("sum", "count")
        return (lambda name: name.startswith(FIRST_GEN)) if first_gen else TABLE

    with options(gb_partition=partition):
        capfd.readouterr()
        run_all(api, rng, [G.ragged(kv, valid, rng)], gid, d, kernel, f"region overflow, gb_partition {partition}")
        flags = _debug_flags(capfd.readouterr().err)
        assert flags and all(f & 16 for f in flags), flags
        promise(api, rng, A.I64, n, d, kernel("sum", None), f"region overflow, gb_partition {partition}", agg="sum", weights=weights)


# ---------------------------------------------------------------- hand-over: a partition's LDS table fills up
def test_lds_table_full_hands_over(api, monkeypatch, capfd):
    """9000 distinct keys whose hash shares its top 8 bits (hash_models.g2_keys_in_partition: the inverse of g2_hash), one row each:
    more than the 7919 slots (7892 in buckets of four) of their partition's LDS table.  At 9000 rows they overflow the partition's
    scatter REGIONS first (a block's 2048 rows meet 56 records: flag 16, the other hand-over).  The smallest input that fills the
    table instead spreads them: one of them every 45 rows among 405 000 rows (46 per block and region), the other rows over 2000
    keys of the other 255 partitions.  The debug line shows flag 32 alone, and the HBM table answers."""
    rng = np.random.default_rng(9)
    crowd = [k - (1 << 64) if k >> 63 else k for k in H.g2_keys_in_partition(0x5C, 9000, seed=3)]
    others = [k for k in distinct_keys(rng, A.I64, 2300, specials_of(A.I64)) if H.g2_partition(k) != 0x5C][:2000]
    n = 9000 * 45
    kv = np.array(others, dtype=np.int64)[rng.integers(0, len(others), n)]
    kv[:len(others)] = others
    kv[44::45] = crowd
    valid = np.ones(n, dtype=bool)
    valid[1::5000] = False
    gid = np.unique(np.where(valid, kv, 1), return_inverse=True)[1]
    cols = [[A.HostArray.from_numpy(kv, valid=valid, offset=5, rng=rng)]]
    d = len(G.groupby(cols, None, "count"))
    assert 10_900 < d <= 9000 + len(others) + 1
    monkeypatch.setenv("RDF_DEBUG", "1")
    for bucket in (4, 1):
        with options(gb_partition=4, gb_bucket=bucket):
            capfd.readouterr()
            run_all(api, rng, cols, gid, d, TABLE, f"LDS table full, gb_bucket {bucket}", aggs=("sum", "count") if bucket == 4 else ("min", "max"), cuts=[n])
            flags = _debug_flags(capfd.readouterr().err)
            assert flags and all(f & 0x30 == 0x20 for f in flags), [hex(f) for f in flags]
    # the promise, with the NULL key and the marker key among the d (above) and without them
    plain = np.where(valid & (kv != FREE), kv, others[10])
    cols_plain = [[A.HostArray.from_numpy(plain, offset=5, rng=rng)]]
    d_plain = len(G.groupby(cols_plain, None, "count"))
    assert d_plain == d - 2
    with options(gb_partition=4):
        capfd.readouterr()
        check(api, cols, None, "count", d - 1, TABLE, "LDS table full, promise with the set-aside keys")
        check(api, cols_plain, None, "count", d_plain, TABLE, "LDS table full, promise without the set-aside keys")
        check(api, cols_plain, None, "count", d_plain - 1, TABLE, "LDS table full, promise without the set-aside keys")
        flags = _debug_flags(capfd.readouterr().err)
        assert flags and all(f & 0x30 == 0x20 for f in flags), [hex(f) for f in flags]


# ---------------------------------------------------------------- the heavy-hitter split
def test_heavy_hitter_split(api, monkeypatch, capfd):
    """The split wants 65 536 probe samples and the probe takes one row in 16 of every tile: 1 048 576 rows at the least, more
    by the sampled rows whose key is NULL — 1 100 000 here.  Zipf-like keys: one key holds a third of the rows, the next nine
    0.3 / rank^1.2 each, the rest spreads over 30 000 keys.

    The hot pass takes only the rows whose KEY is one of the up to 100 sampled heavy hitters (g2_prepare looks the hashed key up in
    the hot keys' table), so no number of distinct keys in a hot class can fill its LDS table.  What makes the split give up is a
    region of the other rows overflowing: 400 rows of one key the probe never samples, inside one super-tile.  The call is re-run
    without the split; the debug line says so and the kernel name no longer names the heavy hitters."""
    rng = np.random.default_rng(404)
    n, cold = 1_100_000, 30_000
    pool = distinct_keys(rng, A.I64, cold + 6) + specials_of(A.I64) + [None]          # (the ten heavy keys are plain ones)
    d = len(pool)
    assert len(set(pool)) == d
    shares = np.array([1 / 3] + [0.3 / r ** 1.2 for r in range(2, 11)])
    weights = np.concatenate([shares, np.full(d - 10, (1 - shares.sum()) / (d - 10))])
    kv, valid, gid = spread(rng, A.I64, n, pool, weights)
    cols = [G.ragged(kv, valid, rng)]
    hot_name = lambda name: name.startswith("gb2_stream_kernel (heavy hitters) + " + SCATTER)     # noqa: E731
    with options(gb_partition=4, gb_skew_plan=2):
        run_all(api, rng, cols, gid, d, hot_name, "heavy hitters", aggs=("sum", "count"))
        v, ok = G.plant_groups(G.special_values(rng, n), rng.uniform(size=n) >= 0.1, gid, 0, 3, 12)      # the heaviest key all NaN
        check(api, cols, G.ragged(v, ok, rng), "min", d, hot_name, "heavy hitters (special floats)")
        check(api, cols, None, "count", d - 1, hot_name, "heavy hitters, promise with the set-aside keys")
        plain = np.where(valid & (kv != FREE), kv, pool[20])                 # no NULL key, no marker key
        cols_plain = [G.ragged(plain, None, rng)]
        assert len(G.groupby(cols_plain, None, "count")) == d - 2
        check(api, cols_plain, None, "count", d - 2, hot_name, "heavy hitters, promise without the set-aside keys")
        check(api, cols_plain, None, "count", d - 3, hot_name, "heavy hitters, promise without the set-aside keys")
        # the split gives up
        unsampled = [i for i in range(5 * 2048, 6 * 2048) if i % 16 != ((i // 1024) * 7) & 15][:400]     # (gb2_skew_probe_kernel: row 16 * lane + (7 * tile & 15) of a tile)
        kv2, valid2 = kv.copy(), valid.copy()
        kv2[unsampled], valid2[unsampled] = 123_456_789, True
        gid2 = np.unique(np.where(valid2, kv2, 1), return_inverse=True)[1]
        cols2 = [G.ragged(kv2, valid2, rng)]
        monkeypatch.setenv("RDF_DEBUG", "1")
        capfd.readouterr()
        vals2 = G.ragged(G.exact_values(rng, gid2, np.float64), rng.uniform(size=n) >= 0.1, rng)
        check(api, cols2, vals2, "sum", d + 1, lambda name: "heavy hitters" not in name, "heavy hitters, the split gives up", exact=True)
        err = capfd.readouterr().err
        assert "the heavy-hitter split gave up" in err, err[-2000:]


# ---------------------------------------------------------------- several key columns
def _tuple_columns(rng, n, specs):
    """specs = [(dtype, pool of values, NULL fraction)] -> (chunk lists, group id per row)."""
    cols, parts = [], []
    cuts = [n // 3, 0, n - n // 3]
    for dt, pool, nulls in specs:
        idx = rng.integers(0, len(pool), n)
        kv = np.array(pool, dtype=A.NP_OF[dt])[idx]
        valid = rng.uniform(size=n) >= nulls if nulls else None
        if nulls >= 1:
            valid = np.zeros(n, dtype=bool)
        cols.append(G.ragged(kv, valid, rng, cuts))
        parts.append(np.where(valid, idx, -1) if valid is not None else idx)
    gid = np.unique(np.stack(parts), axis=1, return_inverse=True)[1].reshape(-1)
    return cols, gid


@pytest.mark.parametrize("case", ["2 packed", "3 packed", "4 packed", "dictionary", "full range nullable", "all NULL column"])
def test_several_key_columns(api, case, monkeypatch, capfd):
    """5000 rows.  Range-packed tuples of 2, 3 and 4 columns of mixed widths with NULLs in every column (the column's smallest
    value, whose field code sits next to the NULL code, is always a key); dictionary-coded columns whose ranges together pass 64
    bits; a nullable column over the full 64-bit range (dictionary only); an all-NULL column.  max_groups is the number of
    distinct tuples, and one less is RDF_MEMORY_ERROR."""
    rng = np.random.default_rng(len(case) * 7)
    n = 5000
    packed = [(A.I64, [-10 ** 15 + 3 * i for i in range(6)], 0.1), (A.I8, [-128, -127, 0, 127], 0.1), (A.U32, [4_000_000_000 + i for i in range(5)], 0.15), (A.I16, [100, -32768], 0.2)]
    specs = {"2 packed": packed[:2], "3 packed": packed[:3], "4 packed": packed,
             "dictionary": [(A.I64, distinct_keys(rng, A.I64, 40, [I64_MIN, I64_MAX]), 0.03), (A.U64, distinct_keys(rng, A.U64, 25, [0, 2 ** 64 - 1]), 0.0),
                            (A.I32, distinct_keys(rng, A.I32, 9), 0.05)],
             "full range nullable": [(A.I64, [I64_MIN, I64_MAX, 0, FREE, -1], 0.1), (A.U8, [0, 255, 7], 0.1)],
             "all NULL column": [(A.I32, [1, 2, 3], 1.0), (A.I64, [I64_MIN, FREE, 5], 0.1)]}[case]
    cols, gid = _tuple_columns(rng, n, specs)
    d = len(G.groupby(cols, None, "count"))
    kernel = STREAM if d <= 2048 else (lambda name: name.startswith(SCATTER))      # (COUNT over the packed 64-bit key takes 4-byte records)
    monkeypatch.setenv("RDF_DEBUG", "1")
    capfd.readouterr()
    run_all(api, rng, cols, gid, d, kernel, f"key columns: {case}", cuts=[n // 3, 0, n - n // 3])
    coding = set(re.findall(r"groupby key column (\d): ([a-z-]+)", capfd.readouterr().err))   # the engine's debug line names each column's coding
    coded = {k for k, how in coding if how == "dictionary-coded"}
    # (full range nullable: no spare code for NULL; all NULL column: 1 bit next to a nullable column spanning 64 bits is 65)
    assert {k for k, _ in coding} == {str(k) for k in range(len(cols))} and len(coding) == len(cols), coding
    assert coded == ({"dictionary": coded, "full range nullable": {"0"}, "all NULL column": {"1"}}.get(case, set())) and (case != "dictionary" or coded), coding
    check(api, cols, None, "count", d - 1, lambda name: True, f"key columns: {case}, promise")
    with options(gb_partition=0):
        run_all(api, rng, cols, gid, d, TABLE, f"key columns: {case}, HBM table", aggs=("sum", "count"), cuts=[n // 3, 0, n - n // 3])
        check(api, cols, None, "count", d - 1, lambda name: True, f"key columns: {case}, HBM table, promise")


def test_a_null_does_not_merge_with_a_value(api):
    """(NULL, 5) against (v, 5) for v at both ends of the column's range and in it: NULL's field code is no value's."""
    cols = [[A.HostArray.from_numpy(np.array([0, 3, 9, 0, 3, 9, 0], dtype=np.int16), valid=np.array([1, 1, 1, 0, 0, 1, 1], dtype=bool), offset=1)],
            [A.HostArray.from_numpy(np.array([5, 5, 5, 5, 5, 5, 6], dtype=np.uint8), valid=np.array([1, 1, 1, 1, 0, 1, 0], dtype=bool), offset=2)]]
    vals = [A.HostArray.from_numpy(np.array([1, 2, 4, 8, 16, 32, 64], dtype=np.int64))]
    model = check(api, cols, vals, "sum", 6, STREAM, "NULL next to a value")
    assert {k: v[0] for k, v in model.items()} == {(0, 5): 1, (3, 5): 2, (9, 5): 36, (None, 5): 8, (None, None): 16, (0, None): 64}


def test_tuples_beyond_64_bits_are_an_invalid_argument(api):
    """Four columns of 66 000 distinct sparse values each: 17 bits apiece even dictionary-coded."""
    rng = np.random.default_rng(8)
    wide = [[A.HostArray.from_numpy(rng.integers(-2 ** 62, 2 ** 62, 66_000).astype(np.int64))] for _ in range(4)]
    for mem in MEMS:
        with pytest.raises(A.RdfError) as ei:
            call(api, wide, None, "count", 100_000, mem)
        assert ei.value.status == A.RDF_INVALID_ARGUMENT
