"""rdf_groupby_multi on the MI355X, both routes held to tests/groupby_ref.py (never to the oracle, never to rdf_groupby_agg).

For every call c of a case the model is groupby_ref.groupby(keys, values[c], agg_c) and the comparison groupby_ref.check_groupby:
keys, counts, integer values and float MIN / MAX bits exact, float sums inside the any-order bound, bit for bit on the
integer-valued family (exact_values).  A COUNT over a value column counts that column's non-NULL values (the header's
out_counts rule; the model's counts of the same column).  All outputs of a call share ONE set of key columns, so comparing every
call against those keys is the statement that row g of every output names the same group; out_group_rows is held to the
model's group sizes.  Text keys are modelled by their first-occurrence rank as an Int64 key.

Every case runs under route 1 (gbm_stream_kernel: asserted by name while max_groups is within the capacity; beyond it the route
hands over to the table when a block table fills up) and route 2 (gbm_table_kernel), in device memory, the small ones in host
memory too.  Sizes: a sub-tile is 512 rows and a tile 1024, so rows 0, 1, 63, 64, 65, 1023, 1024, 1025 and 3 x 1024 + 7 sit on
and around every boundary of the loaders (1, 2 and 4 rows a thread) and give more than one block from 2049 rows on; the
capacity boundary is reached with "groupby_multi_slots" = 64.  The colliding Utf8 rows of tests/hash_fixtures.py are keys here;
its colliding tuples hold Float32 / Float64 columns, which no GROUP BY key may be, so they have no case.
"""
import contextlib

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
import groupby_ref as G
import hash_fixtures as HF
import hash_models as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FREE = H.G2_FREE_KEY
STREAM, TABLE = "gbm_stream_kernel", "gbm_table_kernel"
ROUTES = {0: "gbm_", 1: STREAM, 2: TABLE}
NP = A.NP_OF


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


@pytest.fixture(autouse=True)
def _default_options():
    yield
    lib.set_option("groupby_multi_route", 0)
    lib.set_option("groupby_multi_slots", 0)


@contextlib.contextmanager
def options(route=0, slots=0):
    try:
        lib.set_option("groupby_multi_route", route)
        lib.set_option("groupby_multi_slots", slots)
        yield
    finally:
        lib.set_option("groupby_multi_route", 0)
        lib.set_option("groupby_multi_slots", 0)


# ---------------------------------------------------------------- calls
def to_device(x):
    if isinstance(x, A.HostUtf8):
        return A.DeviceUtf8.from_host(x)
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def to_host(out):
    if out is None or isinstance(out, (A.HostArray, A.HostUtf8)):
        return out
    if isinstance(out, A.DeviceUtf8):
        return out.to_host()
    t, v = out.keep
    vals = t.cpu().numpy().view(NP[out.dtype])[:max(out.length, 1)].copy()
    return A.HostArray(vals, v.cpu().numpy() if v is not None else None, 0, out.length, out.dtype, out.null_count)


def call(api, key_cols, values, calls, max_groups, mem):
    if mem == "device":
        key_cols = [[to_device(c) for c in col] for col in key_cols]
        values = [[to_device(c) for c in col] for col in values]
    keys, outs, counts, rows = api.groupby_multi(key_cols, values, calls, max_groups)
    return [to_host(k) for k in keys], [to_host(o) for o in outs], [to_host(o) for o in counts], to_host(rows)


class CodeKeys:
    """A Utf8 key output seen as the Int64 codes the model groups by."""

    def __init__(self, out, code_of):
        self.rows = [None if s is None else code_of[s] for s in out.to_pylist()]
        self.length, self.dtype, self.null_count = out.length, A.I64, out.null_count

    def to_pylist(self):
        return self.rows


def text_codes(rows):
    """rows (str | None) -> ({str: first-occurrence rank}, the Int64 model column as (data, valid))."""
    code_of = {}
    for r in rows:
        if r is not None and r not in code_of:
            code_of[r] = len(code_of)
    data = np.array([0 if r is None else code_of[r] for r in rows], dtype=np.int64)
    valid = np.array([r is not None for r in rows], dtype=bool)
    return code_of, data, (None if valid.all() else valid)


class Case:
    """key_cols / values as chunk lists of host arrays; model_keys: the integer chunk lists the model groups by (a Utf8 key as its
    codes, cut like the key); code_of[k]: the dictionary of a Utf8 key column, None for a numeric one; exact[v]: value column v is of
    the integer-valued family."""

    def __init__(self, what, key_cols, values, calls, model_keys=None, code_of=None, exact=None):
        self.what, self.key_cols, self.values, self.calls = what, key_cols, values, calls
        self.model_keys = model_keys if model_keys is not None else key_cols
        self.code_of = code_of if code_of is not None else [None] * len(key_cols)
        self.exact = exact if exact is not None else [False] * len(values)
        self._models = None

    def models(self):
        """The reference, computed once per case and shared by every route and memory kind."""
        if self._models is None:
            ms = []
            for agg, v in self.calls:
                if agg == "count" and v >= 0:   # non-NULL values of the column: the counts of any other aggregate over it
                    m = G.groupby(self.model_keys, self.values[v], "sum")
                    c = G.Groups({k: (G.ANY, cnt, None) for k, (_, cnt, _) in m.items()})
                    c.key_dtypes, c.value_dtype = m.key_dtypes, None
                    m = c
                else:
                    m = G.groupby(self.model_keys, None if v < 0 else self.values[v], agg)
                ms.append(m)
            self._models = (ms, G.groupby(self.model_keys, None, "count"))
        return self._models

    def ngroups(self):
        return len(self.models()[1])


def check(api, case, max_groups, routes=(1, 2), mems=("device",), slots=0, expect_stream=None):
    models, sizes = case.models()
    results = []
    for route in routes:
        for mem in mems:
            w = f"{case.what}, route {route}, max_groups {max_groups}, {mem}"
            with options(route, slots):
                keys, outs, counts, rows = call(api, case.key_cols, case.values, case.calls, max_groups, mem)
                kernel = lib.last_kernel()
            want = ROUTES[route] if expect_stream is None or route == 2 else (STREAM if expect_stream else TABLE)
            if len(sizes):
                assert want in kernel, f"{w}: answered by {kernel!r}"
            mkeys = [k if code is None else CodeKeys(k, code) for k, code in zip(keys, case.code_of)]
            for c, ((agg, v), model) in enumerate(zip(case.calls, models)):
                got = G.groups_of(mkeys, outs[c], counts[c])
                G.check_groupby(got, model, agg, f"{w}, call {c} ({agg} of {v})", floats_exact=agg == "sum" and v >= 0 and case.exact[v])
            got = G.groups_of(mkeys, rows, rows)
            assert {k: c for k, (_, c) in got.items()} == {k: c for k, (_, c, _) in sizes.items()}, f"{w}: out_group_rows"
            results.append((keys, outs, counts, rows))
    return results


# ---------------------------------------------------------------- inputs
def distinct_keys(rng, dt, count, specials=()):
    info = np.iinfo(NP[dt])
    have = list(dict.fromkeys(int(s) for s in specials if info.min <= s <= info.max))[:count]
    count = min(count, info.max - info.min + 1)
    seen = set(have)
    while len(have) < count:
        for x in rng.integers(info.min, info.max, 2 * (count - len(have)) + 8, dtype=NP[dt], endpoint=True).tolist():
            if x not in seen and len(have) < count and x != FREE:
                seen.add(x)
                have.append(x)
    return have


def chunks(data, valid, rng, ragged=True):
    if ragged:
        return G.ragged(data, valid, rng)
    return [A.HostArray.from_numpy(data, valid=valid)]


def int_values(rng, n, dt, nullable=True):
    info = np.iinfo(NP[dt])
    v = rng.integers(info.min, info.max, n, dtype=NP[dt], endpoint=True)
    return v, (rng.uniform(size=n) < 0.8 if nullable else None)


MIXED_DTYPES = [A.I8, A.U8, A.I32, A.U64, A.F32, A.F64]
# I8 sum/min, U8 max, I32 sum, U64 min/max (UInt64 outputs), F32 sum (general), F64 min; a count of rows and one of a column
MIXED_CALLS = [("sum", 0), ("max", 1), ("sum", 2), ("min", 3), ("max", 3), ("sum", 4), ("min", 5), ("count", -1)]


def mixed_values(rng, n, gid):
    cols, exact = [], []
    for dt in MIXED_DTYPES:
        if dt == A.F32:
            v, valid = G.general_values(rng, n).astype(np.float32), rng.uniform(size=n) < 0.8
        elif dt == A.F64:
            v, valid = G.plant_groups(G.special_values(rng, n), rng.uniform(size=n) < 0.8, gid, 0, 1, 2)
        else:
            v, valid = int_values(rng, n, dt)
        cols.append((v, valid))
        exact.append(False)
    return cols, exact


def one_key_case(rng, n, groups, calls=None, specials=(FREE, -2 ** 63, 2 ** 63 - 1), null_key=True, what="", ragged=True, kdt=A.I64):
    """One integer key with `groups` distinct values (specials among them) + the NULL key, the mixed value columns."""
    pool = distinct_keys(rng, kdt, groups, specials)
    gid = rng.integers(0, len(pool) + (1 if null_key else 0), n) if n else np.zeros(0, dtype=np.int64)
    if 0 < len(pool) + (1 if null_key else 0) <= n:
        gid[:len(pool) + (1 if null_key else 0)] = np.arange(len(pool) + (1 if null_key else 0))   # every group exists
    kvalid = gid < len(pool)
    kdata = np.array(pool + [0], dtype=NP[kdt])[gid] if n else np.zeros(0, dtype=NP[kdt])
    cols, exact = mixed_values(rng, n, gid)
    calls = MIXED_CALLS if calls is None else calls
    return Case(what or f"{n} rows, {groups} keys", [chunks(kdata, None if kvalid.all() else kvalid, rng, ragged)],
                [chunks(v, valid, rng, ragged) for v, valid in cols], calls, exact=exact), gid


# ---------------------------------------------------------------- sizes, chunks, dtypes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 7])
def test_rows_around_the_tile(api, n):
    """Eight calls over six value dtypes in ragged chunks (an empty chunk, element offsets, validity at odd bits), the NULL key
    and the key whose hash is the free marker among the keys, at every row count on and around a tile."""
    rng = np.random.default_rng(100 + n)
    case, _ = one_key_case(rng, n, 19)
    check(api, case, 64, mems=("device", "host") if n in (0, 1, 65, 1025) else ("device",), expect_stream=True)


@pytest.mark.parametrize("ncalls", [1, 2, 5, 8])
def test_number_of_calls(api, ncalls):
    """1, 2, 5 and 8 calls: every loader width (4, 2 and 1 rows a thread) and every LDS layout width; without the special keys."""
    rng = np.random.default_rng(200 + ncalls)
    calls = {1: [("min", 3)], 2: [("sum", 4), ("count", -1)], 5: [("sum", 0), ("min", 0), ("max", 0), ("count", 0), ("sum", 5)], 8: MIXED_CALLS}[ncalls]
    case, _ = one_key_case(rng, 2049, 300, calls=calls, specials=(), null_key=False, kdt=A.I32)
    # (fewer value columns than the case carries would change the loader: hand over only those the calls name)
    used = sorted({v for _, v in calls if v >= 0})
    case.values = [case.values[v] for v in used]
    case.exact = [case.exact[v] for v in used]
    case.calls = [(a, used.index(v) if v >= 0 else -1) for a, v in calls]
    check(api, case, 300, expect_stream=True)


def test_exact_float_sums_and_two_calls_on_one_column(api):
    """The integer-valued family: sums bit for bit in any order; SUM, MIN, MAX, COUNT and a second SUM on ONE column, next to
    general doubles under the any-order bound."""
    rng = np.random.default_rng(3)
    n, groups = 3 * 1024 + 7, 41
    gid = rng.integers(0, groups, n)
    keys = np.array(distinct_keys(rng, A.I64, groups, (FREE,)), dtype=np.int64)[gid]
    ev, gv = G.exact_values(rng, gid, np.float64), G.general_values(rng, n)
    evalid = rng.uniform(size=n) < 0.9
    case = Case("exact sums", [chunks(keys, None, rng)], [chunks(ev, evalid, rng), chunks(gv, None, rng)],
                [("sum", 0), ("min", 0), ("max", 0), ("count", 0), ("sum", 0), ("sum", 1), ("count", -1)], exact=[True, False])
    check(api, case, groups, mems=("device", "host"), expect_stream=True)


def test_groups_of_nulls_nans_and_zeros(api):
    """A group whose every value is NULL (sum 0, MIN / MAX NULL, count 0, the row present), one of NaN only, one of +-0.0 only, in
    Float64 and Float32; infinities and denormals scattered through the rest."""
    rng = np.random.default_rng(4)
    n, groups = 1025, 9
    gid = rng.integers(0, groups, n)
    gid[:groups] = np.arange(groups)
    keys = np.array(distinct_keys(rng, A.I64, groups), dtype=np.int64)[gid]
    cols = []
    for npdt in (np.float64, np.float32):
        v, valid = G.plant_groups(G.special_values(rng, n, npdt), rng.uniform(size=n) < 0.8, gid, 3, 4, 5)
        cols.append(chunks(v, valid, rng))
    iv, ivalid = int_values(rng, n, A.I64)
    ivalid[gid == 5] = False
    cols.append(chunks(iv, ivalid, rng))
    calls = [("min", 0), ("max", 0), ("min", 1), ("max", 1), ("sum", 2), ("min", 2), ("max", 2), ("count", 2)]
    case = Case("planted groups", [chunks(keys, None, rng)], cols, calls)
    res = check(api, case, groups, expect_stream=True)
    keys_out, outs, counts, _ = res[0]
    g = keys_out[0].to_pylist().index(int(keys[np.flatnonzero(gid == 5)[0]]))
    assert outs[4].to_pylist()[g] == 0 and outs[5].to_pylist()[g] is None and outs[6].to_pylist()[g] is None and counts[4].to_pylist()[g] == 0


def test_special_float_sums(api):
    """NaN, infinities of one and both signs and signed zeros in float SUMS (the model: group_ref.float_sum)."""
    rng = np.random.default_rng(5)
    n, groups = 1023, 6
    gid = rng.integers(0, groups, n)
    keys = gid.astype(np.int64) * 1000003
    v = G.special_values(rng, n)
    case = Case("special sums", [chunks(keys, None, rng)], [chunks(v, None, rng)], [("sum", 0), ("count", 0)])
    check(api, case, groups, expect_stream=True)


# ---------------------------------------------------------------- keys
@pytest.mark.parametrize("nkeys", [2, 3, 4])
def test_several_key_columns(api, nkeys):
    """2, 3 and 4 key columns of mixed integer dtypes, a NULL in each: range-packed into one key by the shared packer."""
    rng = np.random.default_rng(600 + nkeys)
    n = 1025
    dts = [A.I32, A.U8, A.I64, A.I16][:nkeys]
    key_cols = []
    for dt in dts:
        pool = np.array(distinct_keys(rng, dt, 4, ()), dtype=NP[dt])
        if dt == A.I64:
            pool = (pool >> 20)            # (keeps the tuple inside 64 bits without dictionary coding)
        idx = rng.integers(0, 5, n)
        key_cols.append(chunks(pool[np.minimum(idx, 3)], idx < 4, rng))
    iv, ivalid = int_values(rng, n, A.I32)
    fv = G.general_values(rng, n)
    case = Case(f"{nkeys} keys", key_cols, [chunks(iv, ivalid, rng), chunks(fv, None, rng)],
                [("sum", 0), ("min", 0), ("max", 1), ("sum", 1), ("count", -1)])
    check(api, case, 5 ** nkeys, expect_stream=None)


def text_case(rng, rows, with_int_key, what):
    n = len(rows)
    code_of, cdata, cvalid = text_codes(rows)
    cut = [n // 3, 0, n - n // 3]
    bounds = np.cumsum([0] + cut)
    tcol = [A.HostUtf8.from_pylist(rows[a:b], row_offset=1 + i, data_offset=2 * i) for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]
    mcol = [A.HostArray.from_numpy(cdata[a:b], valid=None if cvalid is None else cvalid[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    key_cols, model_keys, codes = [tcol], [mcol], [code_of]
    if with_int_key:
        ik = rng.integers(-3, 3, n).astype(np.int32)
        icol = G.ragged(ik, rng.uniform(size=n) < 0.9, rng, cuts=cut)
        key_cols.append(icol); model_keys.append(icol); codes.append(None)
    iv, ivalid = int_values(rng, n, A.I64)
    fv = G.general_values(rng, n)
    vals = [G.ragged(iv, ivalid, rng, cuts=cut), G.ragged(fv, None, rng, cuts=cut)]
    return Case(what, key_cols, vals, [("sum", 0), ("min", 0), ("max", 1), ("sum", 1), ("count", -1)], model_keys=model_keys, code_of=codes)


@pytest.mark.parametrize("with_int_key", [False, True])
def test_text_keys(api, with_int_key):
    """A Utf8 key alone and next to an Int32 key: NULL rows, the empty string, sliced chunks, and rows that share one hash in the
    dictionary encoder (tests/hash_fixtures.py) as distinct groups."""
    rng = np.random.default_rng(7 + with_int_key)
    fx = HF.utf8_fixtures()
    words = ["", "a", "b", "ab", "Zürich", "x" * 40] + [s.decode("ascii") for name in ("adjacent", "lengths_15_16", "free_word", "group_32") for s in fx[name]]
    assert len(set(words)) == len(words)
    n = 1025
    idx = rng.integers(0, len(words) + 1, n)
    idx[:len(words) + 1] = np.arange(len(words) + 1)
    rows = [None if i == len(words) else words[i] for i in idx.tolist()]
    case = text_case(rng, rows, with_int_key, "text key" + (" + Int32 key" if with_int_key else ""))
    # (with a Utf8 key the two set-aside groups do not count against max_groups: the promise is the non-NULL tuples)
    check(api, case, case.ngroups(), mems=("device", "host"), expect_stream=True)


def test_without_the_special_keys(api):
    rng = np.random.default_rng(8)
    case, _ = one_key_case(rng, 1024, 50, specials=(), null_key=False)
    check(api, case, 50, expect_stream=True)


def test_narrow_key_dtypes(api):
    for kdt in (A.I8, A.U16, A.U32, A.U64):
        rng = np.random.default_rng(900 + kdt)
        case, _ = one_key_case(rng, 65, 11, calls=[("sum", 2), ("max", 3), ("count", -1)], specials=(FREE, 0), kdt=kdt, what=f"key dtype {kdt}")
        check(api, case, 12, expect_stream=True)


# ---------------------------------------------------------------- capacity, max_groups
def groups_case(rng, groups, n=None, what=""):
    """Exactly `groups` groups (the NULL key and the free-marker key among them), integer values: everything exact."""
    n = 2 * groups + 5 if n is None else n
    pool = distinct_keys(rng, A.I64, groups - 1, (FREE,))
    gid = rng.integers(0, groups, n)
    gid[:groups] = np.arange(groups)
    kdata = np.array(pool + [0], dtype=np.int64)[gid]
    iv, ivalid = int_values(rng, n, A.I64)
    ev = G.exact_values(rng, gid, np.float64)
    return Case(what or f"{groups} groups", [chunks(kdata, gid < groups - 1, rng)], [chunks(iv, ivalid, rng), chunks(ev, None, rng)],
                [("sum", 0), ("min", 0), ("max", 0), ("sum", 1), ("count", -1)], exact=[False, True])


def test_capacity_boundary(api):
    """"groupby_multi_slots" = 64: capacity 32.  capacity - 1 and capacity groups on both routes; capacity + 1 groups under a
    promise of capacity is RDF_MEMORY_ERROR on route 1 with nothing written; under auto with a larger promise it succeeds through
    the table route."""
    rng = np.random.default_rng(10)
    cap = 32
    for g in (cap - 1, cap):
        check(api, groups_case(rng, g), g, slots=64, expect_stream=True)
        with options(0, 64):
            c = groups_case(rng, g)
            call(api, c.key_cols, c.values, c.calls, g, "device")
            assert STREAM in lib.last_kernel()
    over = groups_case(rng, cap + 1)
    for route in (1, 2):
        with options(route, 64):
            G.expect_failure(lambda: call(api, over.key_cols, over.values, over.calls, cap, "device"), G.Failure(A.RDF_MEMORY_ERROR, "capacity + 1 groups"), f"route {route}")
    check(api, over, cap + 1, routes=(0,), slots=64, expect_stream=None)
    with options(0, 64):
        call(api, over.key_cols, over.values, over.calls, cap + 1, "device")
        assert TABLE in lib.last_kernel() and STREAM not in lib.last_kernel()
    # route 1 forced beyond its capacity: a block table that fills up hands the call to the table route
    many = groups_case(rng, 200)
    check(api, many, 200, routes=(1,), slots=64, expect_stream=False)



def test_nothing_is_written_on_memory_error(api):
    """max_groups + 1 groups: RDF_MEMORY_ERROR and every caller buffer as it was (host memory: the buffers are ours to look at)."""
    rng = np.random.default_rng(11)
    case = groups_case(rng, 8)
    a = lib.api()
    outs = {}
    orig = A.Api._window_out

    def marked(dtype, n, device, with_validity):
        o = orig(dtype, n, device, with_validity)
        o.values[:] = 0x5A if o.values.dtype.itemsize == 1 else 23130
        outs[id(o)] = (o, o.values.copy())
        return o
    A.Api._window_out = staticmethod(marked)
    try:
        for route in (1, 2):
            with options(route, 0):
                G.expect_failure(lambda: a.groupby_multi(case.key_cols, case.values, case.calls, 7), G.Failure(A.RDF_MEMORY_ERROR, "8 groups, max_groups 7"), f"route {route}")
    finally:
        A.Api._window_out = staticmethod(orig)
    assert outs and all((o.values == before).all() for o, before in outs.values())


@pytest.mark.parametrize("groups", [7, 40])
def test_exactly_max_groups(api, groups):
    """Exactly max_groups groups (NULL and the marker key counted) succeed, max_groups - 1 promised fails, on both routes."""
    rng = np.random.default_rng(12 + groups)
    case = groups_case(rng, groups)
    check(api, case, groups, expect_stream=True)
    for route in (1, 2):
        with options(route, 0):
            G.expect_failure(lambda: call(api, case.key_cols, case.values, case.calls, groups - 1, "device"), G.Failure(A.RDF_MEMORY_ERROR, "one group too many"), f"route {route}")


def test_planned_capacity_is_the_route_boundary(api):
    """Without overrides the planner takes the LDS route up to rdf_groupby_multi_capacity(ncalls) promised groups and the table
    beyond."""
    rng = np.random.default_rng(13)
    case = groups_case(rng, 50)
    cap = api.groupby_multi_capacity(len(case.calls))
    for promise, want in ((cap, STREAM), (cap + 1, TABLE)):
        call(api, case.key_cols, case.values, case.calls, promise, "device")
        assert want in lib.last_kernel(), (promise, lib.last_kernel())


def test_more_groups_than_a_block_table(api):
    """3000 groups over 6000 rows with 5 calls (capacity 567): the table route by plan, and route 1 handing over."""
    rng = np.random.default_rng(14)
    case = groups_case(rng, 3000, n=6000)
    check(api, case, 3000, routes=(0, 1, 2), expect_stream=False)


# ---------------------------------------------------------------- contention, determinism
def test_one_hot_key(api):
    """One key holding every row: all 512 lanes of a block add into one slot, on both routes; Int64 sums wrap."""
    rng = np.random.default_rng(15)
    n = 3 * 1024 + 7
    keys = np.full(n, 42, dtype=np.int64)
    iv, ivalid = int_values(rng, n, A.I64)
    ev = G.exact_values(rng, np.zeros(n, dtype=np.int64), np.float64)
    case = Case("hot key", [chunks(keys, None, rng)], [chunks(iv, ivalid, rng), chunks(ev, None, rng)],
                [("sum", 0), ("min", 0), ("max", 0), ("sum", 1), ("count", 0), ("count", -1)], exact=[False, True])
    check(api, case, 1, expect_stream=True)


def test_same_input_twice_gives_the_same_integer_bytes(api):
    rng = np.random.default_rng(16)
    case, _ = one_key_case(rng, 3 * 1024 + 7, 300, calls=[("sum", 0), ("min", 2), ("max", 3), ("sum", 2), ("count", 1), ("count", -1)])
    for route in (1, 2):
        runs = []
        for _ in range(2):
            with options(route, 0):
                keys, outs, counts, rows = call(api, case.key_cols, case.values, case.calls, 400, "device")
            order = np.argsort(np.where(keys[0].valid_mask(), keys[0].to_numpy(), 0).astype(np.int64) * 2 + keys[0].valid_mask(), kind="stable")
            runs.append([np.asarray(x.to_numpy())[order].tobytes() for x in [keys[0]] + outs + counts + [rows]]
                        + [np.asarray(o.valid_mask())[order].tobytes() for o in outs])
        assert runs[0] == runs[1], f"route {route}"
