"""rdf_groupby_collect and rdf_list_explode on the MI355X, bit for bit against tests/collect_ref.py, in host and device
memory.  The item lists are placed around the multiples of the tile T (A.COLLECT_TILE): item counts, group boundaries and
NULL runs.  The LDS window of explode and the segment of launch_scan are read from the source, so that the cases that cross
them keep crossing them."""
import os
import re

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
import collect_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = A.COLLECT_TILE
MEMS = ["host", "device"]
KINDS = ["list", "set"]
NUMERIC = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust_dataframe_amd", "csrc")


def source_constant(file, name):
    text = open(os.path.join(CSRC, file)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


WINDOW = source_constant("rdf_collect.h", "kExplodeWindow")
SCAN_SEG = source_constant("rdf_kernels.hip", "kScanThreads") * source_constant("rdf_kernels.hip", "kScanPer")


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


def to_device(c):
    vt = torch.from_numpy(np.ascontiguousarray(c.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(c.validity)).cuda() if c.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, c.offset, c.length, c.dtype, c.null_count, keep=(vt, bt))


def chunks_of(col, lens, odd, mem):
    out, at = [], 0
    for i, ln in enumerate(lens):
        if is_text(col):
            c = A.HostUtf8.from_pylist(col[0][at:at + ln], (5 + 3 * i) % 13 if odd else 0, (7 * i) % 9 if odd else 0)
            out.append(A.DeviceUtf8.from_host(c) if mem == "device" else c)
        else:
            valid = col[1] if len(col) > 1 else None
            c = A.HostArray.from_numpy(col[0][at:at + ln], None if valid is None else valid[at:at + ln], offset=(3 + 2 * i) % 11 if odd else 0)
            out.append(to_device(c) if mem == "device" else c)
        at += ln
    return out


def run(api, keys, value, kind, mem="host", lens=None, odd=False, **kw):
    n = len(value[0])
    lens = [n] if lens is None else lens
    assert sum(lens) == n
    ch = [chunks_of(c, lens, odd, mem) for c in list(keys) + [value]]
    if mem == "device":
        torch.cuda.synchronize()
    return api.groupby_collect(ch[:len(keys)], ch[len(keys)], kind, **kw)


def ref_col(col):
    if is_text(col):
        return ([None if r is None else r.encode() for r in col[0]],)
    return col


def reference(keys, value, kind):
    return R.collect_ref([ref_col(k) for k in keys], ref_col(value), kind)


def same_bytes(got, exp):
    """(groups, group_rows, offsets, child_rows, values | None) against the model's four arrays: dtypes and bytes."""
    if got[0] != len(exp[0]):
        return False
    for g, e in zip(got[1:], exp):
        if (g is None) != (e is None):
            return False
        if e is not None and (g.dtype != e.dtype or g.shape != e.shape or g.tobytes() != e.tobytes()):
            return False
    return True


def check(api, keys, value, kinds=KINDS, lens=None, odd=False, mems=MEMS, what=""):
    exps = {}
    for kind in kinds:
        exps[kind] = reference(keys, value, kind)
        for mem in mems:
            got = run(api, keys, value, kind, mem, lens, odd)
            assert same_bytes(got, exps[kind]), (what, kind, mem)
    return exps


def nulls_of(rng, n, fraction=0.2):
    ok = rng.uniform(size=n) >= fraction
    return ok


# ---------------------------------------------------------------- the item list around the tile

@pytest.mark.parametrize("n", [T - 1, T, T + 1, 3 * T + 5])
@pytest.mark.parametrize("layout", ["one_group", "own_group", "no_keys"])
def test_item_counts(api, n, layout):
    rng = np.random.default_rng(n * 5 + len(layout))
    vals = rng.permutation(np.arange(-n, n, dtype=np.int64))[:n] * 1_000_003      # distinct: the heads of SET are n too
    keys = rng.permutation(np.arange(n, dtype=np.int64)) - n // 2 if layout == "own_group" else np.zeros(n, dtype=np.int64)
    ok = nulls_of(rng, n)
    klist = [] if layout == "no_keys" else [(keys,)]
    exps = check(api, klist, (vals, ok), kinds=["list"], what=(layout, n))
    assert len(exps["list"][0]) == (n if layout == "own_group" else 1)
    one = np.ones(n, dtype=bool)
    if layout != "own_group":
        one[rng.integers(0, n)] = False                   # a second NULL would share the first one's head
    check(api, klist, (vals, ok if layout == "own_group" else one), kinds=["set"], what=(layout, n, "set"))


def sized_groups(rng, sizes, shuffle=True):
    """An Int64 key column whose group g (in key order) has sizes[g] rows, the rows shuffled."""
    k = np.repeat(np.arange(len(sizes), dtype=np.int64) * 3 - 7, sizes)
    return k[rng.permutation(len(k))] if shuffle else k


def test_group_boundaries_around_the_tile_multiples(api):
    rng = np.random.default_rng(11)
    cuts = [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T - 1, 3 * T, 3 * T + 1, 3 * T + 5]
    sizes = np.diff([0] + cuts)
    k = sized_groups(rng, sizes)
    n = len(k)
    vals = rng.permutation(n).astype(np.int64)            # distinct: SET's head list has the same boundaries
    exps = check(api, [(k,)], (vals,), what="no nulls")
    assert exps["list"][1].tolist() == [0] + cuts
    check(api, [(k,)], (vals, nulls_of(rng, n)), kinds=["list"], what="nulls")


def test_one_group_spanning_three_tiles_between_small_ones(api):
    rng = np.random.default_rng(12)
    k = sized_groups(rng, [5, 3 * T, 7])
    n = len(k)
    check(api, [(k,)], (rng.permutation(n).astype(np.int32), nulls_of(rng, n)), kinds=["list"])
    check(api, [(k,)], (rng.permutation(n).astype(np.int32),), kinds=["set"])
    check(api, [(k,)], (rng.integers(0, 50, n).astype(np.int32), nulls_of(rng, n)))   # duplicates: fewer heads than rows


def test_empty_lists_first_middle_last_and_adjacent(api):
    rng = np.random.default_rng(13)
    sizes = [3, 4, 2 * T + 9, 2, 5, 6, T, 1, 2]          # groups 0, 2, 4, 5, 8 hold only NULL values; group 2 covers whole tiles
    k = sized_groups(rng, sizes)
    n = len(k)
    vals = rng.integers(0, 9, n).astype(np.int64)
    ok = ~np.isin(k, np.array([0, 2, 4, 5, 8]) * 3 - 7)
    kok = ~((k == 6 * 3 - 7) & (rng.uniform(size=n) < 0.1))   # and the NULL key group, last: some rows of group 6
    exps = check(api, [(k, kok)], (vals, ok), what="empty lists")
    lens = np.diff(exps["list"][1])
    assert (lens[[0, 2, 4, 5, 8]] == 0).all() and lens[1] > 0 and len(lens) == 10
    all_null = np.zeros(n, dtype=bool)
    exps = check(api, [(k,)], (vals, all_null), what="every value NULL")
    assert exps["set"][1].tolist() == [0] * 10 and len(exps["set"][2]) == 0


def test_a_tile_of_null_heads(api):
    n = 3 * T + 5
    rng = np.random.default_rng(14)
    k = np.arange(n, dtype=np.int32)                      # every row its own group: the heads are the rows
    ok = ~((k >= T) & (k < 2 * T))
    p = rng.permutation(n)
    check(api, [(k[p],)], (rng.integers(0, 5, n).astype(np.int16), ok[p]))


def test_no_validity_and_an_all_valid_bitmap_give_the_same_bytes(api):
    rng = np.random.default_rng(15)
    n = 2 * T + 77
    k = rng.integers(0, 40, n).astype(np.int64)
    v = rng.integers(0, 30, n).astype(np.float64)
    for kind in KINDS:
        for mem in MEMS:
            fast = run(api, [(k,)], (v,), kind, mem)
            slow = run(api, [(k,)], (v, np.ones(n, dtype=bool)), kind, mem)
            exp = reference([(k,)], (v,), kind)
            assert same_bytes(fast, exp) and same_bytes(slow, exp), (kind, mem)


# ---------------------------------------------------------------- SET: duplicates, floats, text

def test_set_duplicates_within_and_across_tiles(api):
    rng = np.random.default_rng(16)
    n = 4 * T + 3
    k = rng.integers(0, 3, n).astype(np.int8)
    v = rng.integers(0, 2 * T, n).astype(np.uint32)       # about 2T distinct values per group: heads span tiles
    exps = check(api, [(k,)], (v, nulls_of(rng, n, 0.1)), kinds=["set"])
    assert T < len(exps["set"][2]) < n


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_set_float_zeros_and_nans_are_canonical(api, dt):
    bits = np.uint32 if dt == np.float32 else np.uint64
    nan_a = np.array([0x7FC00001 if dt == np.float32 else 0x7FF8000000000001], dtype=bits).view(dt)[0]
    nan_b = np.array([0xFFC00000 if dt == np.float32 else 0xFFF8000000000000], dtype=bits).view(dt)[0]
    v = np.array([1.5, nan_a, -0.0, 0.0, nan_b, -0.0, np.inf, 1.5, -np.inf, nan_a], dtype=dt)
    k = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1], dtype=np.int32)
    exps = check(api, [(k,)], (v,))
    rows, offs, child, vals = exps["set"]
    assert offs.tolist() == [0, 3, 8] and child.tolist() == [2, 0, 1, 8, 5, 7, 6, 9]   # the smallest row of every value
    qnan = 0x7FC00000 if dt == np.float32 else 0x7FF8000000000000
    assert vals.view(bits)[[0, 2, 4, 7]].tolist() == [0, qnan, 0, qnan]                # -inf is element 3


def test_set_of_text_with_the_empty_string_and_embedded_zeros(api):
    words = ["", "a", "a\0", "a\0b", "b", "\0", None, "ab", "", "a", None, "a\0"]
    rng = np.random.default_rng(17)
    n = 600
    v = [words[i] for i in rng.integers(0, len(words), n)]
    k = rng.integers(0, 4, n).astype(np.int64)
    exps = check(api, [(k,)], (v,), what="text")
    assert exps["set"][3] is None and np.diff(exps["set"][1]).tolist() == [7, 7, 7, 7]


# ---------------------------------------------------------------- dtypes, several keys, no keys, layouts

@pytest.mark.parametrize("dt", NUMERIC + ["utf8"], ids=lambda d: d if isinstance(d, str) else np.dtype(d).name)
def test_every_value_dtype(api, dt):
    rng = np.random.default_rng(18)
    n = 300
    k = rng.integers(0, 7, n).astype(np.int32)
    raw = rng.integers(0, 20, n)
    if dt == "utf8":
        value = ([None if r == 3 else "w%d" % r for r in raw],)
    else:
        value = ((raw - (10 if np.dtype(dt).kind != "u" else 0)).astype(dt), raw != 3)
    check(api, [(k,)], value, what=dt)


def test_two_and_four_keys_mixing_text_and_numbers(api):
    rng = np.random.default_rng(19)
    n = T + 50
    a = ([None if r == 0 else "k%d" % r for r in rng.integers(0, 4, n)],)
    b = (rng.integers(-2, 2, n).astype(np.int16), rng.uniform(size=n) > 0.1)
    c = (np.where(rng.integers(0, 2, n) == 0, np.float32(-0.0), np.float32(0.0)),)   # one value under the canonical compare
    d = ([""] * n,)
    v = (rng.integers(0, 6, n).astype(np.int64), nulls_of(rng, n))
    check(api, [a, b], v, what="two keys")
    check(api, [b, a, c, d], v, what="four keys")
    check(api, [a, b], ([None if r == 1 else "v%d" % r for r in rng.integers(0, 5, n)],), what="text value")


def test_no_keys_is_one_group(api):
    rng = np.random.default_rng(20)
    n = 2 * T + 1
    v = (rng.integers(0, 100, n).astype(np.int32), nulls_of(rng, n))
    exps = check(api, [], v)
    assert len(exps["list"][0]) == 1 and exps["list"][0][0] == 0
    check(api, [], (v[0],), what="no validity")
    check(api, [], (["t%d" % r for r in rng.integers(0, 9, n)],), what="text")


def test_chunking_memory_kind_and_repetition_change_no_byte(api):
    rng = np.random.default_rng(21)
    n = 3 * T + 5
    k = (rng.integers(0, 9, n).astype(np.int64), rng.uniform(size=n) > 0.05)
    v = (rng.integers(0, 40, n).astype(np.float64), nulls_of(rng, n))
    lens = [1, 700, 3, 1024, 333, 900, n - 2961]
    for kind in KINDS:
        exp = reference([k], v, kind)
        for mem in MEMS:
            assert same_bytes(run(api, [k], v, kind, mem), exp)
            assert same_bytes(run(api, [k], v, kind, mem, lens=lens, odd=True), exp)
            assert same_bytes(run(api, [k], v, kind, mem, lens=lens, odd=True), exp)


def test_set_does_not_depend_on_the_row_order(api):
    rng = np.random.default_rng(22)
    n = 2 * T + 9
    k = rng.integers(0, 5, n).astype(np.int32)
    v = rng.integers(0, 60, n).astype(np.float32)
    v[rng.integers(0, n, 40)] = np.float32(-0.0)
    ok = nulls_of(rng, n)
    base = run(api, [(k,)], (v, ok), "set", "device")
    p = rng.permutation(n)
    shuf = run(api, [(k[p],)], (v[p], ok[p]), "set", "device")
    assert base[0] == shuf[0] and base[2].tobytes() == shuf[2].tobytes() and base[4].tobytes() == shuf[4].tobytes()
    assert np.array_equal(v[p][shuf[3]].view(np.uint32) & 0x7FFFFFFF, v[base[3]].view(np.uint32) & 0x7FFFFFFF)
    first = {}
    for new, old in enumerate(p):                         # child rows map back: the smallest NEW row of the same (key, value)
        first.setdefault((int(k[old]), float(v[old]) + 0.0, bool(ok[old])), new)
    assert all(first[(int(k[p][r]), float(v[p][r]) + 0.0, True)] == r for r in shuf[3])


# ---------------------------------------------------------------- sizing

@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("kind", KINDS)
def test_sizing(api, kind, mem):
    rng = np.random.default_rng(23)
    n = T + 9
    k = (rng.integers(0, 6, n).astype(np.int64),)
    v = (rng.integers(0, 12, n).astype(np.int64), nulls_of(rng, n))
    exp = reference([k], v, kind)
    G, E = len(exp[0]), len(exp[2])
    run(api, [k], v, kind, mem, outs=(None, None, None, None))     # the count-only call
    assert (api.last_groups, api.last_elements) == (G, E)
    device = mem == "device"

    def outs(caps):
        return tuple(api._window_out(dt, cap, device, False) for dt, cap in zip((A.U32, A.I32, A.U32, A.I64), caps))

    exact = outs((G, G + 1, E, E))
    got = run(api, [k], v, kind, mem, outs=exact)
    assert same_bytes(got, exp)
    for short in range(4):
        caps = [G, G + 1, E, E]
        caps[short] -= 1
        o = outs(caps)
        before = [x.keep[0].cpu().numpy().copy() if device else x.values.copy() for x in o]
        with pytest.raises(A.RdfError) as ei:
            run(api, [k], v, kind, mem, outs=o)
        assert ei.value.status == A.RDF_MEMORY_ERROR
        assert (api.last_groups, api.last_elements) == (G, E)
        after = [x.keep[0].cpu().numpy() if device else x.values for x in o]
        assert all(np.array_equal(b, a) for b, a in zip(before, after)) and all((b == 0).all() for b in before)


def test_more_tiles_than_one_scan_segment(api):
    """The tile counts are scanned by launch_scan in segments of SCAN_SEG entries: SCAN_SEG tiles + 1 row need two."""
    n = SCAN_SEG * T + 1
    rng = np.random.default_rng(24)
    k = (rng.integers(0, 3, n).astype(np.int32),)
    v = (rng.integers(0, 1 << 30, n).astype(np.int32), nulls_of(rng, n, 0.3))
    exp = reference([k], v, "list")
    got = run(api, [k], v, "list", "host")
    assert same_bytes(got, exp)


# ---------------------------------------------------------------- explode

def make_list(offsets, valid=None, row_offset=0, mem="host"):
    """A List<Int64> over explicit value_offsets (rows + 1 entries after `row_offset` leading junk rows) whose child
    holds its own index times 3."""
    offsets = np.asarray(offsets, dtype=np.int32)
    n = len(offsets) - 1
    offs = np.concatenate([np.full(row_offset, 1, dtype=np.int32), offsets])
    vals = A.HostArray.from_numpy(np.arange(max(int(offsets.max()), 1), dtype=np.int64) * 3)
    bits = None
    if valid is not None:
        bits = A.pack_bits(np.concatenate([np.ones(row_offset, dtype=bool), np.asarray(valid, dtype=bool)]))
    if mem == "host":
        return A.HostList(offs, vals, bits, row_offset, n)
    ot = torch.from_numpy(offs).cuda()
    bt = torch.from_numpy(bits).cuda() if bits is not None else None
    dv = to_device(vals)
    return A.DeviceList(ot.data_ptr(), n, dv, bt.data_ptr() if bt is not None else None, row_offset, keep=(ot, bt, dv))


def check_explode(api, offsets, valid=None, row_offset=0, what=""):
    for outer in (False, True):
        ep, ec, epos, ev = R.explode_ref(offsets, valid, outer)
        for mem in MEMS:
            lst = make_list(offsets, valid, row_offset, mem)
            if mem == "device":
                torch.cuda.synchronize()
            parent, (child, cvalid), (pos, pvalid) = api.list_explode(lst, outer=outer, pos=True)
            tag = (what, outer, mem)
            assert api.last_rows == len(ep), tag
            assert parent.dtype == np.uint32 and child.dtype == np.uint32 and pos.dtype == np.int32, tag
            assert np.array_equal(parent, ep), tag
            assert np.array_equal(cvalid, ev) and np.array_equal(pvalid, ev), tag
            assert np.array_equal(child, ec) and np.array_equal(pos, epos), tag      # NULL slots hold 0 on both sides
            parent2, (child2, _), none = api.list_explode(lst, outer=outer)
            assert none is None and np.array_equal(parent2, ep) and np.array_equal(child2, ec), tag


def offsets_of(lens, start=0):
    return np.concatenate([[start], start + np.cumsum(lens)]).astype(np.int64)


def test_explode_lists_of_one(api):
    check_explode(api, offsets_of(np.ones(2 * T + 3, dtype=np.int64)))


def test_explode_one_long_list_between_empty_ones(api):
    check_explode(api, offsets_of([0, 0, 3 * T + 1, 0, 0, 0]))
    check_explode(api, offsets_of([0, 0, 3 * T + 1, 0, 0, 0]), valid=[True, False, True, False, True, True])


def test_explode_a_run_of_empty_rows_beyond_the_lds_window(api):
    gap = 4 * WINDOW
    assert gap + 2 > SCAN_SEG                             # (the row counts cross a scan segment too)
    lens = np.zeros(gap + 2, dtype=np.int64)
    lens[0], lens[-1] = 5, 7
    valid = np.ones(gap + 2, dtype=bool)
    valid[1:gap + 1:3] = False                            # empty and NULL rows mixed
    check_explode(api, offsets_of(lens), valid, what="gap")
    lens[1:gap + 1:2] = 1                                 # and with one-element rows in between: more than one tile of them
    check_explode(api, offsets_of(lens), what="sparse")


def test_explode_skips_null_lists_whose_offsets_span_elements(api):
    rng = np.random.default_rng(31)
    lens = rng.integers(0, 6, 700)
    valid = rng.uniform(size=700) > 0.3
    assert (lens[~valid] > 0).any()
    check_explode(api, offsets_of(lens), valid)


def test_explode_offsets_not_starting_at_zero_and_a_sliced_array(api):
    rng = np.random.default_rng(32)
    lens = rng.integers(0, 9, 333)
    valid = rng.uniform(size=333) > 0.2
    check_explode(api, offsets_of(lens, start=41), valid, what="start 41")
    check_explode(api, offsets_of(lens, start=41), valid, row_offset=13, what="sliced")
    check_explode(api, offsets_of(lens), None, row_offset=5, what="sliced, no validity")


def test_explode_outer_rows_first_last_and_adjacent(api):
    lens = [0, 0, 2, 0, 3, 3, 0, 0, 0, 1, 0]
    valid = [False, True, True, True, False, True, True, False, False, True, False]
    check_explode(api, offsets_of(lens), valid)
    ep, ec, epos, ev = R.explode_ref(offsets_of(lens), valid, True)
    assert ep.tolist() == [0, 1, 2, 2, 3, 4, 5, 5, 5, 6, 7, 8, 9, 10] and ev.sum() == 6


def test_explode_zero_rows_and_only_empty_lists(api):
    check_explode(api, [0])
    check_explode(api, [7])
    check_explode(api, offsets_of(np.zeros(T + 3, dtype=np.int64), start=4))
    check_explode(api, offsets_of(np.ones(50, dtype=np.int64)), valid=np.zeros(50, dtype=bool))


@pytest.mark.parametrize("mem", MEMS)
def test_explode_sizing(api, mem):
    lens = [2, 0, 3, 1]
    lst = make_list(offsets_of(lens), None, 0, mem)
    device = mem == "device"
    for outer, rows in ((False, 6), (True, 7)):
        api.list_explode(lst, outer=outer, outs=(None, None, None))
        assert api.last_rows == rows
        o = tuple(api._window_out(dt, rows - 1, device, True) for dt in (A.U32, A.U32, A.I32))
        with pytest.raises(A.RdfError) as ei:
            api.list_explode(lst, outer=outer, outs=o)
        assert ei.value.status == A.RDF_MEMORY_ERROR and api.last_rows == rows
        for x in o:
            vals = x.keep[0].cpu().numpy() if device else x.values
            assert (vals == 0).all()
        o = tuple(api._window_out(dt, rows, device, True) for dt in (A.U32, A.U32, A.I32))
        parent, (child, valid), (pos, _) = api.list_explode(lst, outer=outer, outs=o)
        ep, ec, epos, ev = R.explode_ref(offsets_of(lens), None, outer)
        assert np.array_equal(parent, ep) and np.array_equal(child, ec) and np.array_equal(pos, epos) and np.array_equal(valid, ev)


# ---------------------------------------------------------------- round trips

def test_explode_of_collect_list_is_the_sorted_frame_without_nulls(api):
    rng = np.random.default_rng(41)
    n = 2 * T + 31
    k = rng.integers(0, 50, n).astype(np.int64)
    v = rng.integers(0, 1000, n).astype(np.int64)
    ok = nulls_of(rng, n)
    kc, vc = [A.HostArray.from_numpy(k)], [A.HostArray.from_numpy(v, ok)]
    groups, rows, offs, child, vals = api.groupby_collect([kc], vc, "list")
    lst = A.HostList(offs.copy(), A.HostArray.from_numpy(vals), None, 0, groups)
    parent, (idx, valid), _ = api.list_explode(lst)
    order = api.lexsort_to_indices([kc]).to_numpy()      # stable: every group in row order
    keep = ok[order]
    assert valid.all() and np.array_equal(vals[idx], v[order][keep])
    assert np.array_equal(k[rows][parent], k[order][keep])          # the group of every element is its key's
    assert np.array_equal(parent, np.repeat(np.arange(groups, dtype=np.uint32), np.diff(offs)))


def test_collect_set_lengths_are_count_distinct(api):
    rng = np.random.default_rng(42)
    n = 2 * T + 31
    k = [A.HostArray.from_numpy(rng.integers(0, 70, n).astype(np.int32), rng.uniform(size=n) > 0.05)]
    v = [A.HostArray.from_numpy(rng.integers(0, 25, n).astype(np.float64) - 0.0, nulls_of(rng, n))]
    groups, rows, offs, child, vals = api.groupby_collect([k], v, "set")
    g2, rows2, (counts,) = api.groupby_sorted([k], v, ["count_distinct"])
    assert groups == g2 and np.array_equal(rows, rows2) and np.array_equal(np.diff(offs).astype(np.int64), counts)
