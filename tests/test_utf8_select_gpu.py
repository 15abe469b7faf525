"""rdf_utf8_coalesce / rdf_utf8_case_when on the MI355X: byte-exact against tests/select_ref.py (utf8_coalesce, utf8_case_when),
over host and over device memory, every output behind guard bytes (the buffers, the sizing call and the checks are those of
tests/test_utf8_build_gpu.py: the two calls run on its machinery).

Shapes: row lengths 0, 1, 15, 16, 17 and 2200 bytes (around one 16-byte piece of the copy pass, and a row that spans copy tiles);
literals of 0, 1 and 1024 bytes; parts whose value offsets do not start at 0 and whose rows sit behind a row offset; every row
NULL; the sizing call and a capacity one byte short; a chunk of one row and an empty chunk; coalesce(col, 'unknown') as the key of
rdf_groupby_agg_keys over tests/golden/uk_cities_with_headers.csv with some cities nulled.  Text is compared byte for byte; the one
bound is worked out at the group sums of the last test."""
import csv
import os

import numpy as np
import pytest

import select_ref as R
import test_utf8_build_gpu as B
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMS = ["host", "device"]
ROW_BYTES = [0, 1, 15, 16, 17, 2200]
LENS = [257, 1, 0, 64, 1000]                       # a chunk of one row, an empty chunk, more than one size tile (256 rows)
LITERALS = [b"", b"?", bytes(range(32, 96)) * 16]  # 0, 1 and 1024 bytes


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


def rows_of_bytes(rng, n, null_frac):
    """n ASCII rows of the lengths of ROW_BYTES (2200 rarely), None with probability null_frac"""
    out = []
    for _ in range(n):
        if rng.random() < null_frac:
            out.append(None)
            continue
        k = ROW_BYTES[rng.integers(0, 5)] if rng.random() > 0.02 else 2200
        out.append("".join(chr(c) for c in rng.integers(97, 123, k)))
    return out


def column(rng, null_frac, row_offset, data_offset, lens=LENS):
    return [A.HostUtf8.from_pylist(rows_of_bytes(rng, n, null_frac), row_offset=row_offset, data_offset=data_offset) for n in lens]


def as_bytes(rows):
    return [None if r is None else r.encode() for r in rows]


def conditions(rng, lens, k):
    """(numpy (values, valid | None) per chunk, the Boolean chunks behind a bit offset)"""
    raw = [(rng.random(n) < 0.4, (rng.random(n) > 0.25) if k % 2 == 0 else None) for n in lens]
    return raw, [A.HostArray.from_numpy(v, m, offset=[0, 3, 9, 1, 64][i % 5]) for i, (v, m) in enumerate(raw)]


def to_device(x):
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def run(api, mem, parts, conds=None, shift=0):
    """parts: host chunk lists, bytes literals, None (case_when: the values, then `otherwise`); conds: [(raw, chunks)] -> the checked result"""
    cols = [p for p in parts if isinstance(p, list)]
    lens = [c.length for c in cols[0]]
    placed = [B.place(p, mem) if isinstance(p, list) else p for p in parts]
    cplaced = None if conds is None else [[to_device(c) for c in ch] if mem == "device" else ch for _, ch in conds]
    call, _, nullable = api.utf8_select_call(placed, cplaced)
    res = B.run_call(call, lens, nullable, mem, shift)
    exp = []
    for c, n in enumerate(lens):
        model = [as_bytes(p[c].to_pylist()) if isinstance(p, list) else p for p in parts]
        if conds is None:
            exp.append(R.utf8_coalesce(model) if n else [])
        else:
            exp.append(R.utf8_case_when([raw[c] for raw, _ in conds], model[:-1], model[-1]) if n else [])
    can = lambda p, c: p is None or (isinstance(p, list) and p[c].validity is not None)  # noqa: E731
    assert nullable == [(all if conds is None else any)(can(p, c) for p in parts) for c in range(len(lens))]
    B.check(res, exp, nullable, f"{'coalesce' if conds is None else 'case_when'} {mem}")
    return res, exp


@pytest.mark.parametrize("mem", MEMS)
def test_coalesce_over_chunks_offsets_nulls_and_literals(api, mem):
    rng = np.random.default_rng(3)
    a, b, c = column(rng, 0.4, 3, 1), column(rng, 0.4, 0, 7), column(rng, 0.4, 5, 0)
    dense = column(rng, 0.0, 1, 2)
    for lit in LITERALS:
        run(api, mem, [a, lit])                      # fill_null: never NULL, the literal copied into every row that takes it
        run(api, mem, [a, b, lit, c])                # c is never reached
        run(api, mem, [lit, a])                      # a literal first: a is never read
    for parts in ([a], [a, b], [a, b, c], [a, None, b], [None, a, None], [a, dense, b], [a, b, c, a, b, c, a, LITERALS[1]]):
        run(api, mem, parts, shift=1 if len(parts) == 2 else 0)


@pytest.mark.parametrize("mem", MEMS)
def test_every_row_null_and_rows_that_span_copy_tiles(api, mem):
    rng = np.random.default_rng(4)
    nulls = [A.HostUtf8.from_pylist([None] * n, row_offset=2) for n in LENS]
    res, _ = run(api, mem, [nulls, nulls])
    assert all(len(data) == 0 for _, data, _, _ in res)
    run(api, mem, [nulls, None])
    run(api, mem, [nulls, b"x" * 17])
    long_rows = [A.HostUtf8.from_pylist(["".join(chr(c) for c in rng.integers(97, 123, 2200)) if i % 3 else None for i in range(n)], data_offset=5) for n in (40, 1, 7)]
    short = [A.HostUtf8.from_pylist([None if i % 2 else "s" * (i % 18) for i in range(n)]) for n in (40, 1, 7)]
    run(api, mem, [long_rows, short])
    run(api, mem, [short, long_rows, LITERALS[2]])


@pytest.mark.parametrize("mem", MEMS)
def test_case_when_conditions_with_validity_literals_and_no_otherwise(api, mem):
    rng = np.random.default_rng(5)
    a, b, c = column(rng, 0.3, 1, 3), column(rng, 0.3, 4, 0), column(rng, 0.0, 0, 1)
    c0, c1, c2 = (conditions(rng, LENS, k) for k in range(3))
    never = ([(np.zeros(n, dtype=bool), None) for n in LENS], [A.HostArray.from_numpy(np.zeros(n, dtype=bool)) for n in LENS])
    always = ([(np.ones(n, dtype=bool), None) for n in LENS], [A.HostArray.from_numpy(np.ones(n, dtype=bool), offset=7) for n in LENS])
    run(api, mem, [a, b], [c0])                                        # if_else
    run(api, mem, [b"low", b"mid", c], [c0, c1])                       # bucket labels, never NULL
    run(api, mem, [a, LITERALS[2], b, None], [c0, c1, c2])             # no otherwise: NULL
    run(api, mem, [a, b, c], [never, never])                           # all false: otherwise
    run(api, mem, [a, b, None], [never, never])                        # all false, no otherwise: every row NULL
    run(api, mem, [b, a, LITERALS[0]], [always, always])               # overlapping: the first wins
    run(api, mem, [None, a, b"else"], [c0, always])                    # a chosen NULL literal
    eight = [conditions(rng, LENS, k) for k in range(8)]
    run(api, mem, [a, b"1", b, b"22", c, b"", a, b, None], eight)      # eight branches


@pytest.mark.parametrize("mem", MEMS)
def test_a_capacity_one_byte_short_is_refused_with_the_lengths_set(api, mem):
    rng = np.random.default_rng(6)
    a = column(rng, 0.3, 1, 1, [100, 0, 31])
    cond = conditions(rng, [100, 0, 31], 0)
    for parts, conds in (([a, b"unknown"], None), ([a, b"other", None], [cond, cond])):
        placed = [B.place(p, mem) if isinstance(p, list) else p for p in parts]
        cplaced = None if conds is None else [[to_device(c) for c in ch] if mem == "device" else ch for _, ch in conds]
        call, _, nullable = api.utf8_select_call(placed, cplaced)
        rows = [c.length for c in a]
        _, exp = run(api, mem, parts, conds)
        want = [sum(len(e) for e in ex if e is not None) for ex in exp]
        for short in (0, 2):
            caps = list(want)
            caps[short] -= 1
            co, cd, keep = B.buffers(rows, nullable, mem, caps)
            assert call(co, cd) == A.RDF_MEMORY_ERROR
            assert [cd[i].length for i in range(3)] == want and [co[i].length for i in range(3)] == [r + 1 for r in rows]
            for ob, vb, db in keep:
                for b in (ob, vb, db):
                    assert b is None or ((b.read()[0] == 0xAA).all() and b.read()[1]), "a refused call wrote"


@pytest.mark.parametrize("mem", MEMS)
def test_coalesce_with_a_literal_is_a_group_by_key_over_the_cities(api, mem):
    with open(os.path.join(ROOT, "tests", "golden", "uk_cities_with_headers.csv"), newline="") as f:
        table = list(csv.DictReader(f))
    rng = np.random.default_rng(8)
    cities = [None if rng.random() < 0.3 else row["city"].split(",")[-2].strip() for row in table]      # the county / country part; some nulled
    lats = np.array([float(row["lat"]) for row in table])
    cuts = [0, 20, 20, len(table)]
    col = [A.HostUtf8.from_pylist(cities[a:b], row_offset=2) for a, b in zip(cuts[:-1], cuts[1:])]
    vals = [A.HostArray.from_numpy(lats[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    placed = B.place(col, mem)
    key = api.utf8_coalesce([placed, "unknown"])
    model = [s.decode() for s in R.utf8_coalesce([as_bytes(cities), b"unknown"])]
    got_rows = [s for k in key for s in (k.to_host() if isinstance(k, A.DeviceUtf8) else k).to_pylist()]
    key = [k.to_host() if isinstance(k, A.DeviceUtf8) else k for k in key]
    assert got_rows == model and "unknown" in model and all(k.validity is None for k in key)       # a literal last: never NULL, no bitmap
    key = B.place(key, mem)
    if mem == "device":
        dvals = [A.DeviceArray(t.data_ptr(), None, 0, v.length, A.F64, 0, keep=(t, None)) for v in vals for t in [torch.from_numpy(v.values).cuda()]]
    else:
        dvals = vals
    groups = list(dict.fromkeys(model))
    keys, sums, counts = api.groupby_agg_keys([key], dvals, "sum", len(groups))
    k = keys[0].to_host() if isinstance(keys[0], A.DeviceUtf8) else keys[0]

    def nums(o, dt):
        return (o.to_numpy() if isinstance(o, A.HostArray) else o.keep[0].cpu().numpy().view(dt))[:o.length].tolist()

    got = dict(zip(k.to_pylist(), nums(counts, np.int64)))
    want = {g: model.count(g) for g in groups}
    assert got == want
    got_sums = dict(zip(k.to_pylist(), nums(sums, np.float64)))
    # the groups equal the model's; their sums are at most 36 latitudes below 61, so below 2200 (one ulp there: 4.5e-13), and any
    # order of adding them differs by less than 36 ulps = 1.7e-11
    for g in groups:
        assert abs(got_sums[g] - sum(v for v, m in zip(lats, model) if m == g)) <= 1.7e-11
