"""The "hash equal, keys different" branches on the MI355X, run on keys that really collide (tests/hash_fixtures.py, built with
the exact models of tests/hash_models.py and held to the header's own hash by tests/test_hash_models.py):

  Utf8     rdf_utf8_uniques / rdf_utf8_dictionary_encode hash every row, verify it against its hash's representative and, on a
           mismatch, redo the call on the exact route.  Every collision case must equal the reference, give the same bytes on
           both routes and on a repeated call, and END ON THE EXACT ROUTE when left to choose (rdf_last_kernel); its control
           — one byte of every collider but the first changed, so that nothing collides — must stay on the hash route.  GROUP BY
           and join on text keys go through the same encoder.
  tuples   rdf_equijoin_indices_multi hashes 2..4 key columns and verifies every candidate: tuples X != Y with one hash on both
           sides, X on one side and Y on the other only (every candidate rejected: an outer join's NULL partner), and a non-NULL
           tuple whose hash is 0, the hash the NULL rows are given.
  order    the pair order rdf_mi355x.h promises (probe rows ascending, partners ascending, then FULL's unmatched build rows)
           as exact index arrays, for every join table and key dtype, and float keys compared as bits.

References: tests/text_keys_ref.py (numeric keys as their bytes, so equality is bitwise) and the oracle, which states the same
order.  Everything is exact.  Measured on the CPU with time.perf_counter: constructing every colliding fixture takes 0.2 s, the
Utf8 columns and tuple sides around them 1.0 s, the inputs of the order tests 0.6 s."""
import functools
import random
from collections import Counter

import numpy as np
import pytest

import hash_fixtures as F
import hash_models as H
import text_keys_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
from test_text_keys_gpu import (MEMS, ROUTES, _default_options, api, expected_groups, num_col, place, run_encode,  # noqa: F401
                                run_groupby, run_join, text_col, text_rows)

pytestmark = pytest.mark.gpu

HOWS = ["left", "right", "inner", "full"]


# ---------------------------------------------------------------- Utf8 columns around the colliders

def background(n, seed, distinct=None):
    """n rows over short distinct-ish values with ~5 % NULLs; none of them is as long as a collider."""
    rng = random.Random(seed)
    distinct = distinct or max(3, n // 3)
    return [None if rng.random() < 0.05 else b"bg-%d" % rng.randrange(distinct) for _ in range(n)]


def change_one_byte(row, at=0):
    return row[:at] + bytes([row[at] ^ 1]) + row[at + 1:]


def control_of(rows, colliders):
    """The same column with one byte of every collider but the first changed: nothing collides any more."""
    swap = {c: change_one_byte(c, k % len(c)) for k, c in enumerate(colliders) if k > 0}
    out = [swap.get(r, r) for r in rows]
    hashes = [H.utf8_hash(r) for r in set(out) - {None}]
    assert len(set(hashes)) == len(hashes)                     # (by the model the header was held to)
    return out


UTF8_CUTS = (337, 700)
UTF8_OFFSETS = [(0, 0), (3, 13), (7, 5)]      # junk rows (validity bit offsets 3 and 7) and junk bytes in front of chunks 1 and 2


@functools.lru_cache(maxsize=None)
def utf8_case(name):
    """-> (rows, control rows, cuts): ~1000 rows (3000 for the group of 32) cut into 3 chunks."""
    rows_of = F.utf8_fixtures()[name]
    a, b = rows_of[0], rows_of[1]
    n, cuts = 1000, UTF8_CUTS
    rows = background(n, sum(name.encode()))
    if name == "adjacent":
        spots = {20: a, 500: a, 501: b}
    elif name == "far_apart":
        spots = {350: a, 690: b}                               # one chunk, more than a block of 256 rows apart
    elif name == "two_chunks":
        spots = {100: a, 101: a, 800: b, 999: b}
    elif name == "rep_is_the_other":
        spots = {5: b, 50: b, 400: b, 720: b, n - 1: a}        # a occurs once and last: its hash's representative is row 5
    elif name == "behind_nulls":
        spots = {i: None for i in range(0, 12)}
        spots.update({i: None for i in range(640, 700)})
        spots.update({12: b, 700: b, 300: a})                  # b stands only behind NULL rows (the column's and a chunk's first)
    elif name == "group_32":
        n, cuts = 3000, (1000, 2100)
        rows = background(n, 77)
        rng = random.Random(78)
        spots = {}
        for r in rows_of:
            for _ in range(rng.randint(1, 20)):
                spots[rng.randrange(n)] = r
        for k, r in enumerate(rows_of):                        # (every one of the 32 at least once, whatever was overwritten)
            spots[40 * k + 7] = r
    else:                                                      # the odd shapes: both strings several times, in every chunk
        spots = {7: a, 8: b, 333: a, 336: b, 338: b, 600: a, 900: a, 999: b}
    for i, v in spots.items():
        rows[i] = v
    assert set(rows_of) <= set(rows)
    return rows, control_of(rows, rows_of), cuts


def utf8_chunks(rows, cuts):
    return text_col(rows, cuts, UTF8_OFFSETS)


def lists_of(rows, cuts):
    bounds = [0] + list(cuts) + [len(rows)]
    return [rows[a:b] for a, b in zip(bounds[:-1], bounds[1:])]


UTF8_CASES = list(F.UTF8_NAMES)


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("name", UTF8_CASES)
def test_encode_of_colliding_rows(api, name, mem):
    rows, control, cuts = utf8_case(name)
    exp_codes, exp_dict = R.factorize(lists_of(rows, cuts))
    chunks = utf8_chunks(rows, cuts)
    for route in ROUTES:
        codes, dic = run_encode(api, chunks, mem, route)       # (twice, the two answers compared byte for byte)
        k = lib.last_kernel()
        assert "lexsort" in k and "cs_dict_heads_kernel" in k, (route, k)     # route 0 too: the kernel saw the collision
        assert dic == exp_dict, route
        assert codes == exp_codes, route
    exp_codes, exp_dict = R.factorize(lists_of(control, cuts))
    codes, dic = run_encode(api, utf8_chunks(control, cuts), mem, 0)
    k = lib.last_kernel()
    assert "lexsort" not in k and "cs_dict_rep_kernel" in k, k                # ... and nothing else caused the hand-over
    assert dic == exp_dict and codes == exp_codes


def uniques_twice(api, chunks, mem, route):
    lib.set_option("uniques_route", route)
    placed = place(chunks, mem)
    a = sorted(text_rows(api.utf8_uniques(placed)), key=lambda v: (v is None, v))     # (the order of the values is unspecified)
    b = sorted(text_rows(api.utf8_uniques(placed)), key=lambda v: (v is None, v))
    assert a == b
    return a


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("name", UTF8_CASES)
def test_uniques_of_colliding_rows(api, name, mem):
    rows, control, cuts = utf8_case(name)
    chunks = utf8_chunks(rows, cuts)
    want = set(rows) - {None}
    got = {}
    for route in ROUTES:
        got[route] = uniques_twice(api, chunks, mem, route)
        k = lib.last_kernel()
        assert "cs_utf8_runs_kernel" in k and "cs_utf8_verify_kernel" not in k, (route, k)
        assert None not in got[route] and len(got[route]) == len(want) and set(got[route]) == want, route
    assert got[0] == got[1]
    want = set(control) - {None}
    vals = uniques_twice(api, utf8_chunks(control, cuts), mem, 0)
    k = lib.last_kernel()
    assert "cs_utf8_verify_kernel" in k and "cs_utf8_runs_kernel" not in k, k
    assert None not in vals and len(vals) == len(want) and set(vals) == want


# ---------------------------------------------------------------- GROUP BY and join on text keys that collide

def sprinkle(rows, values, seed, times):
    rng = random.Random(seed)
    for v in values:
        for _ in range(rng.randint(*times)):
            rows[rng.randrange(len(rows))] = v
    return rows


@functools.lru_cache(maxsize=None)
def groupby_collider_data():
    fx = F.utf8_fixtures()
    colliders = [r for name in ("adjacent", "tail_7_bytes", "lengths_15_16", "long_512", "long_1040_round_2", "free_word") for r in fx[name]]
    colliders += fx["group_32"][:12]
    n = 900
    text = sprinkle(background(n, 5, 40), colliders, 6, (1, 6))
    for i, c in enumerate(colliders):
        text[20 * i + 3] = c
    rng = random.Random(7)
    ints = [None if rng.random() < 0.05 else rng.randrange(3) for _ in range(n)]
    vals = [None if rng.random() < 0.1 else rng.randrange(-40, 50) for _ in range(n)]
    return text, ints, vals


GB_CUTS = (300, 301, 640)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
def test_groupby_on_a_text_key_with_colliders(api, mem, route):
    text, _, vals = groupby_collider_data()
    keys = [text_col(text, GB_CUTS, [(0, 0), (3, 2), (7, 9), (1, 0)])]
    for agg in ("sum", "count"):
        got = run_groupby(api, keys, num_col(vals, np.int64, GB_CUTS), agg, 128, mem, route)
        assert got == expected_groups([text], vals, agg), agg


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
def test_groupby_on_text_and_int64_keys_with_colliders(api, mem, route):
    text, ints, vals = groupby_collider_data()
    got = run_groupby(api, [text_col(text, GB_CUTS), num_col(ints, np.int64, GB_CUTS)], num_col(vals, np.int64, GB_CUTS), "sum", 400, mem, route)
    assert got == expected_groups([text, ints], vals, "sum")
    got = run_groupby(api, [num_col(ints, np.int64, GB_CUTS), text_col(text, GB_CUTS)], num_col(vals, np.int64, GB_CUTS), "max", 400, mem, route)
    assert got == expected_groups([ints, text], vals, "max")


@functools.lru_cache(maxsize=None)
def join_collider_data():
    """Colliders on both sides: some pairs whole on both sides, of some string A on the left only and B on the right only."""
    fx = F.utf8_fixtures()
    both = [r for name in ("adjacent", "lengths_15_16", "long_512_words_62_63", "free_word") for r in fx[name]] + fx["group_32"][8:16]
    split = ("two_chunks", "tail_7_bytes", "long_1040_round_2")
    left_only = [fx[name][0] for name in split] + fx["group_32"][:8]
    right_only = [fx[name][1] for name in split] + fx["group_32"][16:24]
    left = sprinkle(background(700, 11, 150), both + left_only, 12, (1, 4))
    right = sprinkle(background(500, 13, 150), both + right_only, 14, (1, 4))
    for i, c in enumerate(both + left_only):
        left[25 * i + 1] = c
    for i, c in enumerate(both + right_only):
        right[17 * i + 2] = c
    assert not (set(left_only) & set(right)) and not (set(right_only) & set(left))
    rng = random.Random(15)
    lnum = [None if rng.random() < 0.04 else rng.randrange(2) for _ in left]
    rnum = [None if rng.random() < 0.04 else rng.randrange(2) for _ in right]
    return left, right, lnum, rnum


def check_text_join(pairs, left_lists, right_lists, how):
    assert Counter(pairs) == R.equijoin(left_lists, right_lists, how)
    R.assert_ordered(pairs, left_lists, right_lists, how)
    # a collider that stands on one side only has no partner, whatever shares its hash on the other side
    only_left = set(left_lists[0]) - set(right_lists[0]) - {None}
    lone = [i for i, v in enumerate(left_lists[0]) if v in only_left and all(c[i] is not None for c in left_lists)]
    assert len(lone) > 20
    count = Counter(pairs)
    assert not any(l in set(lone) and r is not None for l, r in pairs)
    if how in ("left", "full"):
        assert all(count[(i, None)] == 1 for i in lone)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("how", HOWS)
def test_join_on_a_text_pair_with_colliders(api, how, mem, route):
    left, right, _, _ = join_collider_data()
    pairs = run_join(api, [text_col(left, (250, 251))], [text_col(right, (77,), [(3, 4), (0, 0)])], how, mem, route)
    check_text_join(pairs, [left], [right], how)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("how", HOWS)
def test_join_on_text_and_int64_pairs_with_colliders(api, how, mem, route):
    left, right, lnum, rnum = join_collider_data()
    pairs = run_join(api, [text_col(left, (250, 251)), num_col(lnum, np.int64, (250, 251))],
                     [text_col(right, (77,)), num_col(rnum, np.int64, (77,))], how, mem, route)
    check_text_join(pairs, [left, lnum], [right, rnum], how)


# ---------------------------------------------------------------- numeric keys: columns, byte keys, exact order

U8 = "u8"
NP_OF = {H.I64: np.int64, H.I32: np.int32, H.F64: np.float64, H.F32: np.float32, U8: np.uint8}
BITS_OF = {H.F64: np.uint64, H.F32: np.uint32}


def np_column(values, dtype):
    """values: integers (for a float column: its BITS), None = NULL."""
    plain = [0 if v is None else v for v in values]
    if dtype in BITS_OF:
        return np.array(plain, dtype=BITS_OF[dtype]).view(NP_OF[dtype])
    return np.array(plain, dtype=NP_OF[dtype])


def num_chunks(values, dtype, cuts, offsets=None, force_validity=False):
    arr = np_column(values, dtype)
    valid = np.array([v is not None for v in values], dtype=bool)
    bounds = [0] + list(cuts) + [len(values)]
    out = []
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        v = valid[a:b] if force_validity or not valid[a:b].all() else None
        out.append(A.HostArray.from_numpy(arr[a:b], valid=v, offset=offsets[i] if offsets else 0))
    return out


def byte_keys(values, dtype):
    """The column as the reference sees it: every key its bytes in memory, so equal means bitwise equal."""
    arr = np_column(values, dtype)
    return [None if v is None else arr[i].tobytes() for i, v in enumerate(values)]


def pairs_of(ol, orr):
    left, right = ol.to_pylist(), orr.to_pylist()
    assert len(left) == len(right) == ol.length == orr.length
    assert ol.null_count == sum(v is None for v in left) and orr.null_count == sum(v is None for v in right)
    return list(zip(left, right))


def check_numeric_join(pairs, ora_pairs, lkeys, rkeys, how):
    assert Counter(pairs) == R.equijoin(lkeys, rkeys, how)
    R.assert_ordered(pairs, lkeys, rkeys, how)                 # exact index arrays and validity; FULL's tail as a set
    n = R.full_probe_rows(lkeys, rkeys) if how == "full" else len(pairs)
    assert pairs[:n] == ora_pairs[:n] and sorted(pairs[n:], key=lambda p: p[1]) == ora_pairs[n:]   # the oracle states the same order


# ---------------------------------------------------------------- colliding tuples through rdf_equijoin_indices_multi

SCENARIOS = ["both_sides", "split", "hash_0", "hash_0_validity_buffers", "hash_0_null_rows"]
TUPLE_CUTS = {9: (4,), 300: (100, 101), 5000: (1500, 3000)}
TUPLE_OFFSETS = {9: (0, 3), 300: (0, 3, 5), 5000: (0, 3, 5)}


@functools.lru_cache(maxsize=None)
def tuple_case(nk, n, scenario):
    """-> (dtypes, left columns, right columns, force validity buffers); columns are lists of values (floats as bits)."""
    dt, x, y, z = F.tuple_fixtures()[nk]
    rng = random.Random(1000 * nk + n)
    pool = [tuple(H.random_value(rng, d) for d in dt) for _ in range(max(2, n // 3))]
    # rows the special tuples take: inside one 64-row wave and on both sides of a 256-thread block's end
    spots = list(range(6)) if n == 9 else list(range(250, 262)) + [n // 2, n - 1]
    if scenario == "both_sides":
        lsp = {p: (x, y)[i % 2] for i, p in enumerate(spots)}                      # X Y X Y ...
        rsp = {p: (y, x, x, y, y)[i % 5] for i, p in enumerate(spots)}             # Y X X Y Y ...
    elif scenario == "split":
        lsp = {p: x for p in spots}                                               # X on the left only, Y on the right only
        rsp = {p: y for p in spots}
    else:
        lsp = {p: (z, x, z, y)[i % 4] for i, p in enumerate(spots)}
        rsp = {p: (y, z, z, x)[i % 4] for i, p in enumerate(spots)}
    nulls = scenario in ("both_sides", "split", "hash_0_null_rows")

    def side(rows_n, special):
        rows = [pool[rng.randrange(len(pool))] for _ in range(rows_n)]
        for p, t in special.items():
            rows[p] = t
        cols = [[r[k] for r in rows] for k in range(nk)]
        if nulls:
            free = [i for i in range(rows_n) if i not in special]
            for i in rng.sample(free, max(1, rows_n // 20)):
                cols[rng.randrange(nk)][i] = None
        return cols

    return dt, side(n, lsp), side(n, rsp), scenario == "hash_0_validity_buffers"


@functools.lru_cache(maxsize=None)
def tuple_inputs(nk, n, scenario):
    dt, lcols, rcols, force = tuple_case(nk, n, scenario)
    cuts, offs = TUPLE_CUTS[n], TUPLE_OFFSETS[n]
    lch = [num_chunks(c, d, cuts, offs, force) for c, d in zip(lcols, dt)]
    rch = [num_chunks(c, d, cuts[:1], offs[:2], force) for c, d in zip(rcols, dt)]   # the right side cut differently
    return lch, rch, [byte_keys(c, d) for c, d in zip(lcols, dt)], [byte_keys(c, d) for c, d in zip(rcols, dt)]


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("n", [9, 300, 5000])
@pytest.mark.parametrize("nk", [2, 3, 4])
def test_join_of_colliding_tuples(api, ora, nk, n, scenario, how):
    lch, rch, lkeys, rkeys = tuple_inputs(nk, n, scenario)
    pairs = pairs_of(*api.equijoin_indices_multi(lch, rch, how))
    again = pairs_of(*api.equijoin_indices_multi(lch, rch, how))
    assert Counter(pairs) == Counter(again)
    check_numeric_join(pairs, pairs_of(*ora.equijoin_indices_multi(lch, rch, how)), lkeys, rkeys, how)
    if scenario == "split":
        # every candidate of a special row is a stranger with its hash: an outer join emits the row once, with a NULL partner,
        # and FULL appends the build side's strangers as unmatched
        dt, lcols, rcols, _ = tuple_case(nk, n, scenario)
        x, y = F.tuple_fixtures()[nk][1:3]
        lx = [i for i in range(n) if tuple(c[i] for c in lcols) == x]
        ry = [j for j in range(n) if tuple(c[j] for c in rcols) == y]
        assert len(lx) >= 6 and len(ry) >= 6
        count = Counter(pairs)
        assert not any(l in lx and r is not None for l, r in pairs) and not any(r in ry and l is not None for l, r in pairs)
        if how in ("left", "full"):
            assert all(count[(i, None)] == 1 for i in lx)
        if how in ("right", "full"):
            assert all(count[(None, j)] == 1 for j in ry)


# ---------------------------------------------------------------- the order contract, one key column

ORDER_SHAPES = [(4095, 4097), (4096, 4096), (4097, 4095), (9000, 8999), (300, 0), (0, 300)]
ORDER_DTYPES = [H.I64, H.I32, U8, H.F64, H.F32]


@functools.lru_cache(maxsize=None)
def order_inputs(dtype, shape):
    """Duplicate-heavy keys (about 5 rows per key), ~5 % NULLs on both sides, 3 chunks with offsets per side."""
    rng = random.Random(sum(shape) + len(dtype) + ord(dtype[0]))
    card = max(2, max(shape) // 5)
    if dtype == U8:
        card = 250

    def key(j):
        if dtype in BITS_OF:
            return H.raw_bits((j - card // 2) * 0.25, dtype)
        return j if dtype == U8 else j - card // 2

    def side(n):
        vals = [None if rng.random() < 0.05 else key(rng.randrange(card)) for _ in range(n)]
        cuts = (n // 3, n // 3 + 1) if n else ()
        return vals, num_chunks(vals, dtype, cuts, (3, 0, 5) if n else (2,)), byte_keys(vals, dtype)

    return side(shape[0]), side(shape[1])


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("shape", ORDER_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", ORDER_DTYPES)
def test_pair_order_of_a_single_key_join(api, ora, dtype, shape, how):
    (_, lch, lkeys), (_, rch, rkeys) = order_inputs(dtype, shape)
    ora_pairs = pairs_of(*ora.equijoin_indices(lch, rch, how))
    for table in (2, 0):
        lib.set_option("join_table", table)
        try:
            pairs = pairs_of(*api.equijoin_indices(lch, rch, how))
        finally:
            lib.set_option("join_table", 2)
        try:
            check_numeric_join(pairs, ora_pairs, [lkeys], [rkeys], how)
        except AssertionError as e:
            raise AssertionError(f"join_table {table}: {e}") from e


@pytest.mark.parametrize("how", HOWS)
def test_the_retired_join_table_value_means_the_default(api, how):
    """join_table = 1 named the table whose slots were claimed by compare-and-swap: the value is still accepted and the call takes
    the default route — the same index arrays and validity as under 2 (FULL's tail of unmatched build rows is written through an
    atomic cursor, so it is the same rows in any order: the contract above)."""
    (_, lch, lkeys), (_, rch, rkeys) = order_inputs(H.I64, (4097, 4095))
    got = {}
    for table in (2, 1):
        lib.set_option("join_table", table)
        try:
            got[table] = pairs_of(*api.equijoin_indices(lch, rch, how))
        finally:
            lib.set_option("join_table", 2)
    n = R.full_probe_rows([lkeys], [rkeys]) if how == "full" else len(got[2])
    assert len(got[1]) == len(got[2]) and got[1][:n] == got[2][:n]
    assert sorted(got[1][n:], key=lambda p: p[1]) == sorted(got[2][n:], key=lambda p: p[1])


# ---------------------------------------------------------------- float keys are bits

def float_specials(dtype):
    """+-0.0, NaNs of two payloads and both signs, +-inf, a denormal, and two ordinary values — as bits."""
    if dtype == H.F64:
        return [0x0000000000000000, 0x8000000000000000, 0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0xFFF8000000000001,
                0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, H.raw_bits(1.5, H.F64), H.raw_bits(-1.5, H.F64)]
    return [0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0xFFC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000001,
            H.raw_bits(1.5, H.F32), H.raw_bits(-1.5, H.F32)]


@functools.lru_cache(maxsize=None)
def float_inputs(dtype):
    rng = random.Random(len(dtype) * 31)
    sp = float_specials(dtype)
    left = [None if rng.random() < 0.05 else rng.choice(sp) for _ in range(330)]
    right = [None if rng.random() < 0.05 else rng.choice(sp[:-1]) for _ in range(270)]      # (-1.5 on the left only)
    right = [v for v in right if v != sp[5]]                                                # (one NaN on the left only)
    return left, right


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("dtype", [H.F64, H.F32])
def test_float_keys_join_on_their_bits(api, ora, dtype, how):
    left, right = float_inputs(dtype)
    lch, rch = num_chunks(left, dtype, (100, 200), (0, 3, 5)), num_chunks(right, dtype, (64,), (1, 0))
    lkeys, rkeys = [byte_keys(left, dtype)], [byte_keys(right, dtype)]
    # the rule, spelled out: -0.0 does not join +0.0, a NaN joins the NaN with its own bits only
    exp = R.equijoin(lkeys, rkeys, "inner")
    sp = float_specials(dtype)
    zero_rows = [i for i, v in enumerate(left) if v == sp[1]]
    assert zero_rows and all(right[j] == sp[1] for i in zero_rows for (a, j) in exp if a == i)
    ora_pairs = pairs_of(*ora.equijoin_indices(lch, rch, how))
    for table in (2, 0):
        lib.set_option("join_table", table)
        try:
            pairs = pairs_of(*api.equijoin_indices(lch, rch, how))
        finally:
            lib.set_option("join_table", 2)
        check_numeric_join(pairs, ora_pairs, lkeys, rkeys, how)
    # ... and as one column of a two-column key
    ints = [i % 2 for i in range(len(left))], [j % 2 for j in range(len(right))]
    l2 = [lch, num_chunks(ints[0], H.I32, (100, 200), (0, 3, 5))]
    r2 = [rch, num_chunks(ints[1], H.I32, (64,), (1, 0))]
    pairs = pairs_of(*api.equijoin_indices_multi(l2, r2, how))
    check_numeric_join(pairs, pairs_of(*ora.equijoin_indices_multi(l2, r2, how)), lkeys + [byte_keys(ints[0], H.I32)],
                       rkeys + [byte_keys(ints[1], H.I32)], how)
