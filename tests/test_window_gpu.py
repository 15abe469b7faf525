"""rdf_window on the MI355X: row_number / rank / dense_rank / percent_rank / cume_dist / ntile / lag / lead over partitions.
Every case runs in host and in device memory, with all eight functions in one call and one at a time, and is held to
tests/window_ref.py: integers and row indices bit for bit, percent_rank / cume_dist bit for bit too (== on the uint64
views: each is one IEEE division of exact integers, no tolerance is granted)."""
import importlib.util
import os

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
import window_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMS = ["host", "device"]
ALL = ["row_number", "rank", "dense_rank", "percent_rank", "cume_dist", ("ntile", 5), ("lag", 1), ("lead", 2)]


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


# ---------------------------------------------------------------- inputs

def N(values, valid=None, desc=False):
    """A numeric key: values, valid (bool, None = no bitmap), descending."""
    return {"kind": "num", "values": np.asarray(values), "valid": None if valid is None else np.asarray(valid, dtype=bool), "desc": desc}


def T(rows, desc=False, codes=None):
    """A Utf8 key: rows of bytes (None = NULL).  codes: numbers that order and compare like the rows (the reference then
    skips its Python loop over a million byte strings)."""
    return {"kind": "utf8", "rows": rows, "desc": desc, "codes": codes}


def utf8(rows, row_offset=0, data_offset=0):
    enc = [b"j" * (i % 3 + 1) for i in range(row_offset)] + [b"" if r is None else r for r in rows]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in enc]) if enc else []
    data = np.frombuffer(b"\xee" * data_offset + b"".join(enc) + b"\0" * 8, dtype=np.uint8).copy()
    nulls = sum(r is None for r in rows)
    valid = A.pack_bits(np.array([True] * row_offset + [r is not None for r in rows], dtype=bool)) if nulls else None
    return A.HostUtf8(offs.astype(np.int32), data, valid, row_offset, len(rows), data_offset, nulls)


def utf8_from_words(words, codes):
    """One chunk whose row i is words[codes[i]], built without a Python loop over the rows."""
    wl = np.array([len(w) for w in words], dtype=np.int64)
    ws = np.concatenate([[0], np.cumsum(wl)])[:-1]
    blob = np.frombuffer(b"".join(words), dtype=np.uint8)
    lens = wl[codes]
    offs = np.concatenate([[0], np.cumsum(lens)])
    src = np.repeat(ws[codes] - offs[:-1], lens) + np.arange(offs[-1], dtype=np.int64)
    data = np.concatenate([blob[src], np.zeros(8, dtype=np.uint8)])
    return A.HostUtf8(offs.astype(np.int32), data, None, 0, len(codes), 0, 0)


def rows_of(key):
    if key["kind"] == "num":
        return len(key["values"])
    return key["rows"].length if isinstance(key["rows"], A.HostUtf8) else len(key["rows"])


def host_chunks(key, lens, odd):
    out, at = [], 0
    for i, ln in enumerate(lens):
        if key["kind"] == "num":
            v = None if key["valid"] is None else key["valid"][at:at + ln]
            out.append(A.HostArray.from_numpy(key["values"][at:at + ln], v, offset=(3 + 2 * i) % 11 if odd else 0))
        elif isinstance(key["rows"], A.HostUtf8):
            assert len(lens) == 1
            out.append(key["rows"])
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
    if key["kind"] == "num":
        vals, valid = key["values"], key["valid"]
    elif key.get("codes") is not None:
        vals, valid = np.asarray(key["codes"]), None
    else:
        vals, valid = key["rows"], None
    return (vals, valid, key["desc"]) if with_desc else (vals, valid)


def reference(partition, order, calls, nrows=None):
    return window_ref.window_ref([ref_key(k, False) for k in partition], [ref_key(k, True) for k in order], calls, nrows=nrows)


def same(got, exp):
    if isinstance(exp, tuple):
        return (got[0].dtype == np.uint32 and np.array_equal(got[1], exp[1])
                and np.array_equal(got[0][exp[1]], np.asarray(exp[0])[exp[1]]))
    exp = np.asarray(exp)
    if got.dtype != exp.dtype or got.shape != exp.shape:
        return False
    if exp.dtype == np.float64:
        return np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    return np.array_equal(got, exp)


def run(api, partition, order, calls, mem, lens=None, odd=False, nrows=0, raw=False):
    keys = partition + order
    n = rows_of(keys[0]) if keys else nrows
    lens = [n] if lens is None else lens
    assert sum(lens) == n
    chunks = [host_chunks(k, lens, odd) for k in keys]
    if mem == "device":
        chunks = [[to_device(c) for c in col] for col in chunks]
        torch.cuda.synchronize()
    pk = chunks[:len(partition)]
    ok = [(col, k["desc"]) for col, k in zip(chunks[len(partition):], order)]
    return api.window(pk, ok, calls, mem=mem, nrows=nrows, raw=raw)


def check(api, partition, order, calls=ALL, lens=None, odd=False, nrows=0, exp=None, what=""):
    """All calls in one rdf_window and each on its own, in host and in device memory, against the reference."""
    exp = reference(partition, order, calls, nrows) if exp is None else exp
    for mem in MEMS:
        got = run(api, partition, order, calls, mem, lens, odd, nrows)
        for c, (g, e) in enumerate(zip(got, exp)):
            assert same(g, e), (what, mem, "together", calls[c])
        for c in range(len(calls)):
            g = run(api, partition, order, [calls[c]], mem, lens, odd, nrows)[0]
            assert same(g, exp[c]), (what, mem, "alone", calls[c])
    return exp


def golden_module():
    spec = importlib.util.spec_from_file_location("make_window_golden", os.path.join(ROOT, "tests", "golden", "make_window_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------- the header's example, the frozen fixture

def test_the_worked_example(api):
    p = N(np.array([1, 1, 1, 2, 2, 1], dtype=np.int64))
    o = N(np.array([10, 20, 10, 5, 0, 20], dtype=np.int64), [1, 1, 1, 1, 0, 1])
    calls = ["row_number", "rank", "dense_rank", "percent_rank", "cume_dist", ("ntile", 3), ("lag", 1), ("lead", 1)]
    for mem in MEMS:
        rn, rk, dr, pr, cd, nt, lag, lead = run(api, [p], [o], calls, mem)
        assert rn.tolist() == [1, 3, 2, 1, 2, 4]
        assert rk.tolist() == [1, 3, 1, 1, 2, 3]
        assert dr.tolist() == [1, 2, 1, 1, 2, 2]
        assert pr.tolist() == [0.0, 2 / 3, 0.0, 0.0, 1.0, 2 / 3]
        assert cd.tolist() == [0.5, 1.0, 0.5, 0.5, 1.0, 1.0]
        assert nt.tolist() == [1, 2, 1, 1, 2, 3]
        assert window_ref.gather(list(range(6)), *lag) == [None, 2, 0, None, 3, 1]
        assert window_ref.gather(list(range(6)), *lead) == [2, 5, 1, 4, None, None]
    check(api, [p], [o], calls)


def test_the_golden_fixture(api):
    m = golden_module()
    cases = m.load(os.path.join(ROOT, "tests", "golden", "window_v1.npz"))
    assert sorted(cases) == ["float_partition", "mixed_numeric", "text_order", "text_partition"]
    for name, case in cases.items():
        conv = lambda k: N(k["values"], k["valid"], k["desc"]) if k["kind"] == "num" else T(k["rows"], k["desc"])  # noqa: E731
        n = rows_of(conv((case["partition"] + case["order"])[0]))
        check(api, [conv(k) for k in case["partition"]], [conv(k) for k in case["order"]], case["calls"], exp=case["expected"], what=name)
        check(api, [conv(k) for k in case["partition"]], [conv(k) for k in case["order"]], case["calls"], exp=case["expected"],
              lens=[n // 3, 0, n - n // 3], odd=True, what=name + " in chunks")


# ---------------------------------------------------------------- which keys there are

def test_no_partition_keys_no_order_keys_neither_zero_rows_one_row(api):
    rng = np.random.default_rng(11)
    n = 5000
    p, o = N(rng.integers(0, 7, n).astype(np.int32)), N(rng.integers(0, 50, n).astype(np.int64))
    check(api, [], [o], what="no partition keys")
    e = check(api, [p], [], what="no order keys")
    assert (e[2] == 1).all() and (e[4] == 1.0).all()                     # every row of a partition is a peer of every other
    e = check(api, [], [], nrows=n, what="no keys at all")
    assert np.array_equal(e[0], np.arange(1, n + 1)) and (e[1] == 1).all()
    for mem in MEMS:                                                       # nrows_if_no_keys may repeat the keys' rows
        assert same(run(api, [p], [o], ["rank"], mem, nrows=n)[0], reference([p], [o], ["rank"])[0])
    z = N(np.zeros(0, dtype=np.int64))
    for part, order, nrows in (([z], [z], 0), ([], [z], 0), ([], [], 0)):
        for mem in MEMS:
            got = run(api, part, order, ALL, mem, nrows=nrows)
            assert [g[0].shape if isinstance(g, tuple) else g.shape for g in got] == [(0,)] * 8
            for c in ALL:
                g = run(api, part, order, [c], mem, nrows=nrows)[0]
                assert (g[0].shape if isinstance(g, tuple) else g.shape) == (0,)
    for mem in MEMS:                                                       # zero rows in several empty chunks
        assert run(api, [z], [], ["row_number"], mem, lens=[0, 0, 0])[0].shape == (0,)
    one = N(np.array([42], dtype=np.int16))
    e = check(api, [one], [N(np.array([1.5]))], what="one row")
    assert [x.tolist() for x in e[:6]] == [[1], [1], [1], [0.0], [1.0], [1]] and not e[6][1].any() and not e[7][1].any()
    check(api, [], [], nrows=1, what="one row, no keys")


DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64]


@pytest.mark.parametrize("npart,nord", [(1, 1), (1, 2), (2, 1), (2, 2), (4, 1), (4, 2)])
def test_every_dtype_as_partition_and_order_key(api, npart, nord):
    """Every dtype rdf_sort_to_indices takes, in every key position over the rounds, ascending and descending mixed."""
    rng = np.random.default_rng(100 * npart + nord)
    n = 6000
    for rot in range(len(DTYPES)):
        keys = []
        for k in range(npart + nord):
            dt = DTYPES[(rot + k) % len(DTYPES)]
            card = 3 if k < npart else 9
            if np.dtype(dt).kind == "f":
                v = (rng.integers(0, card, n) - card // 2).astype(dt) / dt(2)
            elif np.dtype(dt).kind == "i":
                v = (rng.integers(0, card, n) - card // 2).astype(dt) * dt(np.iinfo(dt).max // card)      # both signs, wide apart
            else:
                v = rng.integers(0, card, n).astype(dt) * dt(np.iinfo(dt).max // card)
            keys.append(N(v, rng.random(n) > 0.05 if (rot + k) % 3 == 0 else None, desc=bool((rot + k) % 2)))
        check(api, keys[:npart], keys[npart:], what=f"rotation {rot}")


def test_a_dtype_the_sort_refuses_is_refused_with_the_same_status(api):
    b = A.HostArray.from_numpy(np.array([1, 0, 1], dtype=bool), dtype=A.BOOL)
    with pytest.raises(A.RdfError) as es:
        api.sort_to_indices([[b]], [False])
    with pytest.raises(A.RdfError) as ew:
        api.window([[b]], [], ["row_number"])
    with pytest.raises(A.RdfError) as eo:
        api.window([], [[b]], ["row_number"])
    assert es.value.status == ew.value.status == eo.value.status == A.RDF_INVALID_ARGUMENT


# ---------------------------------------------------------------- text keys

def city_rows(rng, n, null_frac=0.0):
    prefix = bytes(rng.integers(97, 123, 1024, dtype=np.uint8))
    words = [b"Aberdeen", b"Bath", b"Bat", b"Bath\0", b"Bath\0\0", b"", b"\0", b"Birmingham", b"Bristol", b"Bristol Temple Meads",
             b"York", b"Z\xc3\xbcrich", b"\xff", prefix, prefix + b"a", prefix + b"b", prefix[:1000], prefix[:-1] + b"\0"]
    return [None if rng.random() < null_frac else words[int(rng.integers(0, len(words)))] for _ in range(n)]


def test_utf8_partition_key_utf8_order_key_and_mixed(api):
    rng = np.random.default_rng(21)
    n = 3000
    t1, t2 = city_rows(rng, n, 0.05), city_rows(rng, n, 0.05)
    x = N(np.round(rng.normal(size=n) * 2), rng.random(n) > 0.1)
    k = N(rng.integers(0, 4, n).astype(np.uint16))
    check(api, [T(t1)], [x], what="Utf8 partition key")
    check(api, [k], [T(t2, desc=True)], what="Utf8 order key, descending")
    check(api, [T(t1)], [T(t2)], what="Utf8 both")
    check(api, [k, T(t1)], [N(x["values"], x["valid"], True), T(t2)], what="Utf8 + numeric mixed")
    check(api, [T(t1), T(t2)], [], what="two Utf8 partition keys, no order")
    check(api, [], [T(t1), T(t2, desc=True)], lens=[0, 1, 999, 0, 2000], odd=True, what="Utf8 order keys in odd chunks")


# ---------------------------------------------------------------- NULLs, float specials

def test_nulls_in_partition_and_order_keys(api):
    rng = np.random.default_rng(31)
    n = 4000
    pv, ov = rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 20, n).astype(np.int64)
    for frac in (0.1, 1.0):
        pn, on = rng.random(n) >= frac, rng.random(n) >= frac
        e = check(api, [N(pv, pn)], [N(ov)], what=f"{frac} NULL partition keys")
        if frac == 1.0:
            assert e[0].max() == n                                      # NULL is one key value: one partition of all rows
        for desc in (False, True):
            e = check(api, [N(pv)], [N(ov, on, desc)], what=f"{frac} NULL order keys")
            if frac == 1.0:
                assert (e[2] == 1).all()                                # NULLs are peers of each other
        check(api, [N(pv, pn), T(city_rows(rng, n, frac))], [N(ov, on), T(city_rows(rng, n, frac), desc=True)], what=f"{frac} NULLs everywhere")
    # NULLs last in both directions: the NULL rows of a partition carry the highest ranks
    on = rng.random(n) >= 0.3
    for desc in (False, True):
        rk = run(api, [], [N(ov, on, desc)], ["rank"], "device")[0]
        assert rk[~on].min() == on.sum() + 1 and rk[on].max() <= on.sum()


def float_specials(rng, n, dtype):
    v = np.round(rng.normal(size=n) * 2).astype(dtype)
    u = np.uint64 if dtype == np.float64 else np.uint32
    if dtype == np.float64:
        nans = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFF8000000000000,
                         0xFFF0000000000001, 0xFFFFFFFFFFFFFFFF, 0xFFF8000000000123], dtype=u).view(dtype)
    else:
        nans = np.array([0x7FC00000, 0x7FC00001, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFF800001, 0xFFFFFFFF, 0xFFC00123], dtype=u).view(dtype)
    pick = rng.random(n)
    v[pick < 0.08] = nans[rng.integers(0, len(nans), int((pick < 0.08).sum()))]
    v[(pick >= 0.08) & (pick < 0.16)] = -0.0
    v[(pick >= 0.16) & (pick < 0.24)] = 0.0
    v[(pick >= 0.24) & (pick < 0.27)] = np.inf
    v[(pick >= 0.27) & (pick < 0.30)] = -np.inf
    return v


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_float_specials_are_peers_and_the_sort_is_unchanged(api, dtype):
    rng = np.random.default_rng(41)
    n = 5000
    x = float_specials(rng, n, dtype)
    bits = x.view(np.uint64 if dtype == np.float64 else np.uint32)
    assert len(np.unique(bits[np.isnan(x)])) == 8 and (np.signbit(x) & (x == 0)).any()
    for desc in (False, True):
        e = check(api, [], [N(x, desc=desc)], what=f"order key, desc={desc}")
        rn, rk = e[0], e[1]
        zeros, nans = np.nonzero(x == 0)[0], np.nonzero(np.isnan(x))[0]
        assert len(np.unique(rk[zeros])) == 1 and (np.diff(rn[zeros]) == 1).all()        # -0.0 / +0.0: peers, in row order
        assert len(np.unique(rk[nans])) == 1 and (np.diff(rn[nans]) == 1).all()          # every NaN: one peer group, in row order
        if desc:
            assert rk[nans][0] == 1 and rk[np.nonzero(x == np.inf)[0]][0] == len(nans) + 1
        else:
            assert rk[nans][0] == n - len(nans) + 1 and rn[np.nonzero(x == np.inf)[0]].max() == n - len(nans)   # after +inf
    e = check(api, [N(x)], [N(np.arange(n, dtype=np.int32) % 7)], what="partition key")
    assert e[0][np.isnan(x)].max() == np.isnan(x).sum() and e[0][x == 0].max() == (x == 0).sum()            # one partition each
    # the plain sort keeps its IEEE total order: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, stable
    for desc in (False, True):
        want = window_ref.total_order_argsort(x, desc)
        got = api.sort_to_indices([[A.HostArray.from_numpy(x)]], [desc])
        assert np.array_equal(np.asarray(got.values[:n]).astype(np.int64), want)
        lex = api.lexsort_to_indices([([A.HostArray.from_numpy(x)], desc)])
        assert np.array_equal(np.asarray(lex.values[:n]).astype(np.int64), want)


# ---------------------------------------------------------------- chunking

def test_chunking_offsets_and_odd_validity(api):
    rng = np.random.default_rng(51)
    n = 7001
    p = N(rng.integers(0, 9, n).astype(np.int64), rng.random(n) > 0.1)
    o = N(np.round(rng.normal(size=n), 1), rng.random(n) > 0.1, desc=True)
    t = T(city_rows(rng, n, 0.1))
    exp = reference([p, t], [o], ALL)
    uneven = [1, 900, 13, 2500, 64, 3000, 523]
    assert sum(uneven) == n and len(uneven) == 7
    for lens, odd, what in (([n], False, "one chunk"), (uneven, False, "7 uneven chunks"), ([0, 0, 4000, 0, 3001, 0], False, "empty chunks"),
                            ([n], True, "one chunk behind an offset"), (uneven, True, "7 chunks, offsets, validity at odd bits")):
        check(api, [p, t], [o], lens=lens, odd=odd, exp=exp, what=what)


# ---------------------------------------------------------------- shapes

def test_one_partition_of_a_million_rows_and_every_row_its_own(api):
    rng = np.random.default_rng(61)
    n = 1_000_000
    o = N(rng.integers(0, 1000, n).astype(np.int32))
    e = check(api, [N(np.zeros(n, dtype=np.int8))], [o], what="one partition")
    assert e[0].max() == n
    e = check(api, [N(rng.permutation(n).astype(np.int64))], [o], what="every row its own partition")
    assert (e[0] == 1).all() and (e[4] == 1.0).all() and not e[6][1].any()
    e = check(api, [], [N(np.full(n, 7.5))], what="every row a peer of every other")
    assert np.array_equal(e[0], np.arange(1, n + 1)) and (e[1] == 1).all() and (e[4] == 1.0).all()
    e = check(api, [], [N(rng.permutation(n).astype(np.uint32), desc=True)], what="all distinct")
    assert np.array_equal(np.sort(e[1]), np.arange(1, n + 1)) and np.array_equal(e[1], e[2])


def test_partitions_around_the_tile_sizes_and_one_giant_among_tiny(api):
    rng = np.random.default_rng(71)
    sizes = [255, 256, 257, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 1, 1, 2, 8191, 8192, 8193]
    ids = np.repeat(np.arange(len(sizes)), sizes)
    perm = rng.permutation(len(ids))
    o = N(rng.integers(0, 40, len(ids)).astype(np.int16))
    e = check(api, [N(ids[perm].astype(np.int32))], [o], what="partitions of tile size - 1, tile size, tile size + 1")
    assert sorted(np.bincount(ids[perm], weights=(e[0] == 1)).astype(int).tolist()) == [1] * len(sizes)
    # the same sizes as consecutive runs of the sort order when the rows are already sorted (boundaries exactly at tile edges)
    check(api, [N(ids.astype(np.int32))], [o], what="sorted input")
    tiny = 200_000
    ids = np.concatenate([np.arange(tiny), np.full(600_000, tiny // 2), np.arange(tiny)])
    ids = ids[rng.permutation(len(ids))]
    e = check(api, [N(ids.astype(np.int64))], [N(rng.integers(0, 5, len(ids)).astype(np.uint8))], what="one giant among tiny")
    assert e[0].max() == 600_002


# ---------------------------------------------------------------- ntile, lag / lead and the gather

def test_ntile_buckets(api):
    rng = np.random.default_rng(81)
    n = 1000
    o = N(rng.permutation(n).astype(np.int32))
    calls = [("ntile", b) for b in (1, 2, 3, 7, 64, 999, n, n + 1)]
    e = check(api, [], [o], calls, what="ntile over one partition")
    assert (e[0] == 1).all() and np.array_equal(np.sort(e[6]), np.arange(1, n + 1)) and np.array_equal(e[6], e[7])
    assert np.bincount(e[3])[1:].tolist() == [143] * 6 + [142]          # 1000 = 6 * 143 + 142: the first r buckets hold q + 1
    p = N(rng.integers(0, 37, 5000).astype(np.int32))
    check(api, [p], [N(rng.integers(0, 9, 5000).astype(np.int64))], [("ntile", b) for b in (1, 4, 100, 135, 136, 2**40, 2**62)], what="ntile, b around the partition sizes")


def test_lag_lead_offsets_and_the_gather_of_a_float64_and_a_utf8_column(api):
    rng = np.random.default_rng(91)
    n = 4000
    p = N(rng.integers(0, 30, n).astype(np.int32))
    o = N(rng.integers(0, 1000, n).astype(np.int64))
    calls = [(f, k) for k in (0, 1, 7, 200, 10**6, 2**40) for f in ("lag", "lead")]
    for half in (calls[:8], calls[8:]):
        e = check(api, [p], [o], half, what="offsets 0, 1, 7, >= partition size")
    assert not e[-1][1].any() and not e[-2][1].any()
    idx0, ok0 = reference([p], [o], [("lag", 0)])[0]
    assert ok0.all() and np.array_equal(idx0, np.arange(n))               # offset 0 is the row itself
    # SQL's lag(value) / lead(value): the index array goes into rdf_take / rdf_utf8_take, NULL index -> NULL row
    vals = rng.normal(size=n)
    vvalid = rng.random(n) > 0.1
    words = city_rows(rng, n, 0.1)
    fcol, tcol = A.HostArray.from_numpy(vals, vvalid), utf8(words)
    flist = [float(v) if ok else None for v, ok in zip(vals, vvalid)]
    for mem in MEMS:
        outs = run(api, [p], [o], [("lag", 1), ("lead", 7)], mem, raw=True)
        for out, (fn, off) in zip(outs, (("lag", 1), ("lead", 7))):
            idx, ok = reference([p], [o], [(fn, off)])[0]
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
            assert got_f == window_ref.gather(flist, idx, ok), (mem, fn, "Float64")
            o_, raw_ = got_t.offsets[got_t.offset:got_t.offset + n + 1].astype(np.int64) + got_t.data_offset, got_t.data.tobytes()
            got_rows = [raw_[o_[i]:o_[i + 1]] if k else None for i, k in enumerate(got_t.valid_mask())]
            assert got_rows == window_ref.gather(words, idx, ok), (mem, fn, "Utf8")


# ---------------------------------------------------------------- sizes

def test_1e7_rows_in_1e4_partitions_in_full(api):
    rng = np.random.default_rng(101)
    n = 10_000_000
    p = N(rng.integers(0, 10_000, n).astype(np.int64))
    o = N(np.round(rng.normal(size=n), 2), desc=True)
    calls = ["row_number", "rank", "dense_rank", "percent_rank", "cume_dist", ("ntile", 100), ("lag", 1), ("lead", 3)]
    exp = reference([p], [o], calls)
    check(api, [p], [o], calls, exp=exp, what="1e7 rows")
    # a Utf8 partition key of 1000 words over 2e6 rows (the reference takes the words' codes: same order, same equality)
    m = 2_000_000
    words = sorted({bytes(rng.integers(97, 123, int(rng.integers(1, 20)), dtype=np.uint8)) for _ in range(1100)})[:1000]
    codes = rng.integers(0, len(words), m)
    t = T(utf8_from_words(words, codes), codes=codes)
    assert rows_of(t) == m
    check(api, [t], [N(rng.integers(0, 100, m).astype(np.int32))], what="2e6 rows, Utf8 partition key")


def _dev_i64(n, col, lo, hi):
    t = torch.empty(n + 64, dtype=torch.int64, device="cuda")
    lib.fill_uniform_i64(t.data_ptr(), n, 42, col, 0, lo, hi)
    return t


def _out(dtype, n, es=8, validity=False):
    pad = (n + 63) // 64 * 64 + 64
    v = torch.zeros(pad * es, dtype=torch.uint8, device="cuda")
    b = torch.zeros(pad // 8, dtype=torch.uint8, device="cuda") if validity else None
    return A.DeviceArray(v.data_ptr(), b.data_ptr() if validity else None, 0, n, dtype, 0, keep=(v, b))


def test_1e8_rows_generated_on_the_device_by_properties_from_other_entry_points(api):
    """1e8 rows, ~1e5 partitions, keys from rdf_fill_uniform_i64.  Nothing of this size goes through the CPU: per partition
    max(row_number) (rdf_groupby_agg MAX) equals the partition's rows (rdf_groupby_agg COUNT), sum(row_number) equals the
    sum of n(n+1)/2 over those counts, rank <= row_number and dense_rank <= rank everywhere (rdf_pipeline comparisons ->
    count), and cume_dist of the rows with row_number == n — picked by rdf_filter through the NULLs of a lead(1) — is exactly
    1.0 (the last row's last peer is itself)."""
    n = 100_000_000
    ng = 100_000
    pk, ok_ = _dev_i64(n, 1, 0, ng), _dev_i64(n, 2, -1000, 1000)
    lib.synchronize()
    P = A.DeviceArray(pk.data_ptr(), None, 0, n, A.I64, 0, keep=pk)
    O = A.DeviceArray(ok_.data_ptr(), None, 0, n, A.I64, 0, keep=ok_)
    outs = [_out(A.I64, n), _out(A.I64, n), _out(A.I64, n), _out(A.F64, n)]
    api.window([[P]], [[O]], ["row_number", "rank", "dense_rank", "cume_dist"], outs=outs, raw=True)
    assert [o.length for o in outs] == [n] * 4
    RN, RK, DR, CD = outs
    gouts = lambda: ([_out(A.I64, ng + 2)], _out(A.I64, ng + 2), _out(A.I64, ng + 2))  # noqa: E731
    mk, mv, mc = api.groupby_agg([[P]], [RN], "max", ng, gouts())
    ck, cv, cc = api.groupby_agg([[P]], None, "count", ng, gouts())
    g = mk[0].length
    assert g == ck[0].length and 99_000 < g <= ng
    tonp = lambda a, dt=np.int64: a.keep[0].cpu().numpy().view(dt)[:a.length].copy()  # noqa: E731
    keys_m, maxrn, keys_c, cnt = tonp(mk[0]), tonp(mv), tonp(ck[0]), tonp(cc)
    om, oc = np.argsort(keys_m), np.argsort(keys_c)
    assert np.array_equal(keys_m[om], keys_c[oc]) and np.array_equal(maxrn[om], cnt[oc])      # max(row_number) == rows, per partition
    assert cnt.sum() == n
    e = A.Expr()
    c0, c1 = e.col(0), e.col(1)
    tot = api.pipeline(e, [[RN]], [c0])[0]
    assert tot.count == n and tot.min == 1 and tot.max == cnt.max()
    assert tot.sum == int((cnt * (cnt + 1) // 2).sum())                                       # sum(row_number) == sum of n(n+1)/2
    assert api.pipeline(e, [[RK], [RN]], [c0], e.op("le", c0, c1))[0].count == n              # rank <= row_number
    assert api.pipeline(e, [[DR], [RK]], [c0], e.op("le", c0, c1))[0].count == n              # dense_rank <= rank
    assert api.pipeline(e, [[DR]], [c0])[0].min == 1
    cd = api.pipeline(e, [[CD]], [c0])[0]
    assert cd.max == 1.0 and cd.min > 0.0
    # The rows with row_number == n are the rows without a successor: lead(1) is NULL exactly there, one per partition.  Its
    # bitmap, inverted, is the filter mask that selects their cume_dist (must be exactly 1.0) and their row_number (must be
    # the partitions' row counts).
    ld = _out(A.U32, n, 4, validity=True)
    api.window([[P]], [[O]], [("lead", 1)], outs=[ld], raw=True)
    assert ld.null_count == g                                                                  # one row without a successor per partition
    nullmask = ~ld.keep[1][:(n + 7) // 8]                                                      # bit set = NULL lead = the partition's last row
    M = A.DeviceArray(nullmask.data_ptr(), None, 0, n, A.BOOL, 0, keep=nullmask)
    sel = _out(A.F64, g + 64)
    torch.cuda.synchronize()
    api.filter([CD], [M], [sel])
    assert sel.length == g
    v = sel.keep[0].cpu().numpy().view(np.float64)[:g]
    assert (v.view(np.uint64) == np.float64(1.0).view(np.uint64)).all()                        # exactly 1.0
    rsel = _out(A.I64, g + 64)
    api.filter([RN], [M], [rsel])
    assert np.array_equal(np.sort(rsel.keep[0].cpu().numpy().view(np.int64)[:g]), np.sort(cnt))   # ... and those rows are the ones with row_number == n
    del pk, ok_, outs, ld
    torch.cuda.empty_cache()
