"""The inputs of tests/test_group_pipeline_gpu.py, drawn here so that tests/test_group_ref.py (no GPU) can draw the same ones
and assert what the cases rely on: that an exact-family input really is exact, that a threshold case really has the replica
count it names, that the long case really gives every block three tiles.

Two input families:
  * EXACT.  Every measure is a small dyadic rational: price in quarters below 2^17, disc and tax in 64ths, qty an integer.
    price * (1 - disc) is then k (64 - d) / 2^8 with a numerator below 2^25, the charge k (64 - d) (64 + t) / 2^14 with one
    below 2^32, and every sum over up to 10^6 rows stays below 2^53 / 2^14: each product and each partial sum in ANY order is
    exactly representable, so every engine must return the five Q1 sums bit for bit.  `q1_exact_model` computes them in
    integer arithmetic.
  * GENERAL.  standard_normal scaled by ldexp over +-30 binades, a third of the rows the negation of another row (so groups
    cancel).  Held to group_ref's any-order bound.
"""
import numpy as np

from rust_dataframe_amd import _abi as A

import group_ref as GR
from test_group_pipeline import Q1_CUTOFF, q1_program

Q1_NAMES = ("qty", "price", "disc", "tax", "flag", "status", "ship")
CHUNKED = [1024, 0, 1, 1023, 257, 2178]            # a tail tile before a full one, an empty chunk between
UNIT_ROWS = [1, 2, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2049]      # a wave-load, a wave's share, a tile
EVEN_OFFSETS = [2, 62, 64, 66]                     # keep the 2-row vector loads; validity windows start on both sides of a word
ODD_OFFSET = 13                                    # misaligned for the vector loads: the interpreter answers
TILE = 1024

TAG = {A.F64: "d", A.I64: "l", A.U64: "u", A.F32: "f", A.I32: "i", A.U32: "j", A.BOOL: "b", A.I8: "a", A.U8: "h", A.I16: "s", A.U16: "t"}


# ---------------------------------------------------------------- the catalog of rdf_gspec.hip, restated
def q1_sig(G):
    dp = f"({A.OP_MUL} c4d ({A.OP_SUB} k2d c5d))"
    return (f"G{G};P:({A.OP_LE} c0i k0d);K:({A.OP_ADD} ({A.OP_MUL} {{{A.I32} c1a}} k1i) {{{A.I32} c2a}});"
            f"V:c3d;c4d;{dp};({A.OP_MUL} {dp} ({A.OP_ADD} k2d c6d));c5d;")


def key_sig(key_dt, val_dts, G=8):
    return f"G{G};P:-;K:c0{TAG[key_dt]};V:" + "".join(f"c{i + 1}{TAG[dt]};" for i, dt in enumerate(val_dts))


KEY_FAMILY = [(k, vs) for k in (A.I8, A.I32, A.I64) for vs in ((A.F64,), (A.I64,), (A.F64, A.F64))]
CATALOG = [q1_sig(6), q1_sig(8)] + [key_sig(k, vs) for k, vs in KEY_FAMILY]       # the registration list: 11 kernels


# ---------------------------------------------------------------- what the host plans (rdf_program_plan.h), restated
def group_words(ngroups, nvalues):
    return (ngroups + 1) * (2 * nvalues + 1)


TMP_SLOT_BYTES = 4 * 256 * 8 + 256 * 4


def group_replicas(gwords, ntmp=0):
    """LDS copies of the interpreter's table: a power of two <= 32 that fits 32 KB (64 KB with the TMP spill area)."""
    reps = 32
    while reps > 1 and (reps * gwords * 8 > 32768 or ntmp * TMP_SLOT_BYTES + reps * gwords * 8 > 65536):
        reps >>= 1
    return reps


# (ngroups, nvalues, replicas): both sides of every halving at 2 values (5 words a slot), none of whose programs needs a TMP slot
REPLICA_CASES = [(24, 2, 32), (25, 2, 16), (50, 2, 16), (51, 2, 8), (101, 2, 8), (102, 2, 4), (203, 2, 4), (204, 2, 2), (408, 2, 2),
                 (409, 2, 1)]
SLOT_LIMIT_CASES = [(1023, 1), (127, 8), (511, 2)]     # (ngroups + 1) * nvalues == 1024
TABLE_ROWS = 20_000


def long_rows(cus):
    """With one block a CU the grid is `cus`; 3 cus + 2 tiles, the last one of 300 rows."""
    return (3 * cus + 1) * TILE + 300


def tiles_of(lens):
    return sum((n + TILE - 1) // TILE for n in lens)


def tiles_per_block(lens, grid):
    """gspec_kernel's plain walk: block p takes tiles p, p + grid, p + 2 grid, ..."""
    nt = tiles_of(lens)
    grid = min(grid, nt)
    return [len(range(p, nt, grid)) for p in range(grid)]


def long_key_lens(cus):
    """Three chunks; the first ends 500 rows into tile cus + 7, block 7's second."""
    n = long_rows(cus)
    a, b = (cus + 7) * TILE + 500, (cus + 3) * TILE + 11
    return [a, b, n - a - b]


def third_tile_row(cus, block=9, row=513):
    """A row of block `block`'s third tile in a one-chunk long case."""
    return (2 * cus + block) * TILE + row


# ---------------------------------------------------------------- arrays
def _mask(rng, n, nf):
    if nf is None or (np.isscalar(nf) and nf <= 0):
        return None
    if np.isscalar(nf):
        return rng.uniform(size=n) >= nf
    return np.asarray(nf, dtype=bool)


def chunks_of(rng, values, lens, dtype, valid=None, off=0):
    """One column cut into chunks of `lens`; valid: bool vector over all rows or None."""
    out, r = [], 0
    for n in lens:
        out.append(A.HostArray.from_numpy(values[r:r + n], valid=None if valid is None else valid[r:r + n], offset=off, dtype=dtype, rng=rng))
        r += n
    return out


def general_f64(rng, n):
    x = rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-30, 31, n))
    k = n // 3
    if k:
        x[n - k:] = -x[rng.permutation(n - k)[:k]]         # cancellation
    return x


# ---------------------------------------------------------------- Q1
def q1_exact_columns(rng, lens, ngroups=6, nulls=0.0, off=0, drop_all=False):
    """cols in q1_program's order.  nulls: one fraction for every column, or {name: fraction | bool vector of valid rows}."""
    n = sum(lens)
    gid = rng.integers(0, ngroups, n)
    raw = {"qty": (rng.integers(1, 51, n).astype(np.float64), A.F64),
           "price": (rng.integers(4 * 900, 2 ** 19, n) / 4.0, A.F64),
           "disc": (rng.integers(0, 8, n) / 64.0, A.F64),
           "tax": (rng.integers(0, 6, n) / 64.0, A.F64),
           "flag": ((gid // 2).astype(np.int8), A.I8),
           "status": ((gid % 2).astype(np.int8), A.I8),
           "ship": ((np.full(n, Q1_CUTOFF + 1) if drop_all else rng.integers(8036, 10562, n)).astype(np.int32), A.I32)}
    cols = []
    for name in Q1_NAMES:
        v, dt = raw[name]
        nf = nulls.get(name) if isinstance(nulls, dict) else nulls
        cols.append(chunks_of(rng, v, lens, dt, _mask(rng, n, nf), off))
    return cols


def q1_general_columns(rng, lens, nulls=0.0, off=0):
    cols = q1_exact_columns(rng, lens, 6, nulls, off)
    n = sum(lens)
    for i in range(4):      # the four measures: general family, same validity
        valid = np.concatenate([c.valid_mask() for c in cols[i]]) if any(c.validity is not None for c in cols[i]) else None
        cols[i] = chunks_of(rng, general_f64(rng, n), lens, A.F64, valid, off)
    return cols


def q1_exact_model(cols, ngroups) -> GR.Model:
    """The Q1 answer of an exact-family input in integer arithmetic: numerators over 1, 4, 2^8, 2^14 and 64."""
    c = dict(zip(Q1_NAMES, GR.columns_of(cols)))
    n = len(c["qty"][0])
    ok = {k: np.ones(n, dtype=bool) if m is None else m for k, (_, m) in c.items()}
    q = c["qty"][0].astype(np.int64)
    k4 = (c["price"][0] * 4).astype(np.int64)
    d = (c["disc"][0] * 64).astype(np.int64)
    t = (c["tax"][0] * 64).astype(np.int64)
    for name, num, den in (("qty", q, 1), ("price", k4, 4), ("disc", d, 64), ("tax", t, 64)):
        assert np.array_equal(num / den, c[name][0]), f"{name}: not of the exact family"
    keep = ok["ship"] & (c["ship"][0] <= Q1_CUTOFF)
    gvalid = ok["flag"] & ok["status"]
    gid = c["flag"][0].astype(np.int64) * 2 + c["status"][0]
    assert not (keep & gvalid & ((gid < 0) | (gid >= ngroups))).any()
    slot = np.where(gvalid, gid, ngroups)
    vals = [(q, 0, ok["qty"]), (k4, 2, ok["price"]), (k4 * (64 - d), 8, ok["price"] & ok["disc"]),
            (k4 * (64 - d) * (64 + t), 14, ok["price"] & ok["disc"] & ok["tax"]), (d, 6, ok["disc"])]
    S_ = ngroups + 1
    rows = [int((keep & (slot == g)).sum()) for g in range(S_)]
    sums, counts = [], []
    for num, shift, vok in vals:
        assert int(num.sum()) < 2 ** 53, "a partial sum could leave the exactly representable range"
        sel = [keep & vok & (slot == g) for g in range(S_)]
        sums.append([float(np.ldexp(float(int(num[s].sum())), -shift)) for s in sel])
        counts.append([int(s.sum()) for s in sel])
    return GR.Model(ngroups, [A.F64] * 5, sums, counts, rows, [[None] * S_ for _ in vals])


def q1_wide_program():
    """The Q1 group id (two key columns) behind Q1's predicate with EIGHT value expressions, all exact on the exact family."""
    e, pred, gid, vals = q1_program()
    qty, price, tax = vals[0], vals[1], 3               # q1_program's column nodes are its first seven, in column order
    vals = vals + [tax, e.op("multiply", qty, price), e.op("multiply", price, tax)]
    return e, pred, gid, vals


# ---------------------------------------------------------------- key column as the group id
def key_values(rng, dt, n, family):
    if dt in (A.F64, A.F32):
        if family == "exact":       # 64ths below 2^14 (f32: quarters below 2^10, exact in 24 bits); sums of 10^6 rows stay exact in f64
            return (rng.integers(-2 ** 20, 2 ** 20, n) / 64.0).astype(np.float64) if dt == A.F64 else (rng.integers(-2 ** 12, 2 ** 12, n) / 4.0).astype(np.float32)
        return general_f64(rng, n).astype(A.NP_OF[dt])
    if dt == A.BOOL:
        return rng.integers(0, 2, n).astype(bool)
    info = np.iinfo(A.NP_OF[dt])
    v = rng.integers(info.min, info.max, n, dtype=A.NP_OF[dt], endpoint=True)
    if n >= 2:
        v[0], v[1] = info.min, info.max
    return v


def key_columns(rng, key_dt, val_dts, lens, ngroups, nulls=0.0, off=0, family="exact", keys=None):
    """[key, v0, v1, ...]; nulls: a fraction for every column or {column index: fraction | valid vector}."""
    n = sum(lens)
    if keys is None:
        keys = rng.integers(0, ngroups, n)
    cols = []
    for i, dt in enumerate((key_dt,) + tuple(val_dts)):
        v = (keys.astype(bool) if dt == A.BOOL else keys.astype(A.NP_OF[dt])) if i == 0 else key_values(rng, dt, n, family)
        nf = nulls.get(i) if isinstance(nulls, dict) else nulls
        cols.append(chunks_of(rng, v, lens, dt, _mask(rng, n, nf), off))
    return cols


def key_program(nvals, pred_col=None):
    """group id = column 0, values = columns 1 .. nvals; pred_col: keep rows where that (Int32) column is not 0."""
    e = A.Expr()
    k = e.col(0)
    vals = [e.col(i + 1) for i in range(nvals)]
    pred = e.op("ne", e.col(pred_col), e.scalar(0, A.I32)) if pred_col is not None else -1
    return e, pred, k, vals


def plant(col, row, value=None, valid=None):
    """Overwrite one row of a chunked column in place (its value, or its validity bit)."""
    for ch in col:
        if row < ch.length:
            if value is not None:
                ch.values[ch.offset + row] = value
            if valid is not None:
                bit = ch.offset + row
                if valid:
                    ch.validity[bit >> 3] |= np.uint8(1 << (bit & 7))
                else:
                    ch.validity[bit >> 3] &= np.uint8(~(1 << (bit & 7)) & 0xFF)
                ch.null_count = -1
            return
        row -= ch.length
    raise IndexError(row)


# ---------------------------------------------------------------- the cases
from dataclasses import dataclass, field      # noqa: E402
from typing import Optional                   # noqa: E402

INTERP = "eval_kernel<GROUP>"


@dataclass
class Case:
    """One call.  kernel: the catalog signature that must run in 'spec' mode, INTERP where the host must decline the
    specialised kernel, None where the case does not name one.  exact: of the exact family, float sums bit for bit.
    q1_groups: a Q1 input of the exact family, whose reference is q1_exact_model.  replicas: of the interpreter's table."""
    name: str
    expr: object
    cols: list
    vals: list
    gid: int
    ngroups: int
    pred: int = -1
    kernel: Optional[str] = None
    exact: bool = False
    q1_groups: Optional[int] = None
    replicas: Optional[int] = None
    frame: bool = False
    jit: bool = False
    options: dict = field(default_factory=dict)

    def model(self):
        if self.q1_groups is not None:
            return q1_exact_model(self.cols, self.q1_groups)
        return GR.run_chunks(self.expr, self.cols, self.vals, self.gid, self.ngroups, self.pred)

    def rows(self):
        return sum(ch.length for ch in self.cols[0])


def q1_case(name, seed, lens, ngroups=6, nulls=0.0, off=0, kernel="auto", general=False, **kw):
    rng = np.random.default_rng(seed)
    e, pred, gid, vals = q1_program()
    cols = q1_general_columns(rng, lens, nulls, off) if general else q1_exact_columns(rng, lens, ngroups, nulls, off, kw.pop("drop_all", False))
    if kernel == "auto":
        kernel = q1_sig(6 if ngroups <= 6 else 8) if off % 2 == 0 else INTERP
    return Case(name, e, cols, vals, gid, ngroups, pred, kernel, exact=not general, q1_groups=None if general else ngroups, **kw)


def key_case(name, seed, key_dt, val_dts, lens, ngroups, nulls=0.0, off=0, family="exact", kernel="auto", keys=None, **kw):
    rng = np.random.default_rng(seed)
    e, pred, k, vals = key_program(len(val_dts))
    cols = key_columns(rng, key_dt, val_dts, lens, ngroups, nulls, off, family, keys)
    if kernel == "auto":
        in_catalog = (key_dt, tuple(val_dts)) in KEY_FAMILY and ngroups <= 8 and off % 2 == 0
        kernel = key_sig(key_dt, val_dts) if in_catalog else (INTERP if ngroups > 8 or off % 2 else None)
    return Case(name, e, cols, vals, k, ngroups, pred, kernel, exact=family == "exact", **kw)


RAGGED = [700, 0, 1500, 333]


def catalog_cases():
    """Every catalog kernel by name over one ragged layout with 10 % NULLs in keys and values."""
    out = []
    for ng in (7, 8):
        out.append((f"q1-G8-ng{ng}", lambda ng=ng: q1_case(f"q1 ngroups {ng}", 100 + ng, RAGGED, ng, 0.1)))
    out.append(("q1-G6", lambda: q1_case("q1 ngroups 6", 106, RAGGED, 6, 0.1)))
    for key_dt, val_dts in KEY_FAMILY:
        for ng in (7, 8, 1):      # 1: the unused accumulators stay out of the result
            name = f"key{TAG[key_dt]}-{''.join(TAG[d] for d in val_dts)}-ng{ng}"
            out.append((name, lambda key_dt=key_dt, val_dts=val_dts, ng=ng, name=name:
                        key_case(name, 200 + key_dt * 31 + len(val_dts) * 7 + val_dts[0] + ng, key_dt, val_dts, RAGGED, ng, 0.1)))
    return out


def unit_cases():
    """One chunk of n rows around every unit of the kernel, on Q1 (G6) and the two-value key kernel."""
    out = []
    for n in UNIT_ROWS:
        out.append((f"q1-{n}", lambda n=n: q1_case(f"q1 {n} rows", 300 + n, [n])))
        out.append((f"key2-{n}", lambda n=n: key_case(f"key2 {n} rows", 400 + n, A.I32, (A.F64, A.F64), [n], 5)))
    return out


def layout_cases():
    out = [("q1-chunked", lambda: q1_case("q1 chunked", 500, CHUNKED, nulls=0.1, frame=True)),
           ("key2-chunked", lambda: key_case("key2 chunked", 501, A.I8, (A.F64, A.F64), CHUNKED, 8, 0.1, frame=True)),
           ("q1-general-chunked", lambda: q1_case("q1 general family", 502, CHUNKED, nulls=0.1, general=True))]
    for off in EVEN_OFFSETS + [ODD_OFFSET]:
        out.append((f"q1-off{off}", lambda off=off: q1_case(f"q1 offset {off}", 510 + off, [1500, 700], nulls=0.1, off=off)))
        out.append((f"key2-off{off}", lambda off=off: key_case(f"key2 offset {off}", 520 + off, A.I64, (A.F64, A.F64), [1500, 700], 7, 0.1, off=off)))
    return out


def _all_valid(n):
    return np.ones(n, dtype=bool)


def long_cases(cus):
    """The persistent loop: one block a CU, every block three or four tiles.  Exact family throughout."""
    n = long_rows(cus)
    one = {"gspec_blocks_per_cu": 1}

    def planted():
        valid = _all_valid(n)
        c = q1_case("long q1, one NULL id and one NULL value in a third tile", 604, [n], nulls={"flag": valid, "price": valid}, options=one)
        plant(c.cols[Q1_NAMES.index("flag")], third_tile_row(cus, 9, 513), valid=False)
        plant(c.cols[Q1_NAMES.index("price")], third_tile_row(cus, 9, 514), valid=False)
        plant(c.cols[Q1_NAMES.index("ship")], third_tile_row(cus, 9, 513), value=Q1_CUTOFF)       # both rows pass the filter
        plant(c.cols[Q1_NAMES.index("ship")], third_tile_row(cus, 9, 514), value=Q1_CUTOFF)
        return c
    return [("q1-dense", lambda: q1_case("long q1, no NULLs", 600, [n], options=one, frame=True)),
            ("q1-nulls", lambda: q1_case("long q1, 10 % NULLs", 601, [n], nulls=0.1, options=one)),
            ("key2-chunks", lambda: key_case("long key2, three chunks", 602, A.I32, (A.F64, A.F64), long_key_lens(cus), 8, 0.05, options=one)),
            ("q1-rot", lambda: q1_case("long q1, rotated walk", 600, [n], options={**one, "spec_tile_rot": 1})),
            ("q1-swz", lambda: q1_case("long q1, swizzled walk", 600, [n], options={**one, "spec_xcd_swz": 1})),
            ("q1-rot-swz", lambda: q1_case("long q1, rotated and swizzled", 600, [n], options={**one, "spec_tile_rot": 1, "spec_xcd_swz": 1})),
            ("q1-planted", planted)]


def sparse_cases():
    """NULL ids and NULL values take LDS atomics beside the register accumulators."""
    n = sum(CHUNKED)
    rng = np.random.default_rng(700)
    both = rng.uniform(size=n) >= 0.1
    keys = rng.integers(0, 6, n)
    return [("null-ids", lambda: q1_case("NULL ids only", 701, CHUNKED, nulls={"flag": 0.1, "status": 0.05})),
            ("null-values", lambda: q1_case("NULL values only", 702, CHUNKED, nulls={"price": 0.1, "tax": 0.1, "qty": 0.02})),
            ("null-both", lambda: q1_case("NULL id and NULL value on one row", 703, CHUNKED, nulls={"flag": both, "price": both})),
            ("null-group", lambda: key_case("a group whose every value is NULL", 704, A.I32, (A.F64, A.F64), CHUNKED, 6,
                                            nulls={1: keys != 3, 2: 0.1}, keys=keys)),
            ("null-column", lambda: key_case("a value column without a valid row", 705, A.I64, (A.F64, A.F64), CHUNKED, 6,
                                             nulls={2: np.zeros(n, dtype=bool)})),
            ("none-pass", lambda: q1_case("all rows filtered out", 706, CHUNKED, nulls=0.1, drop_all=True)),
            ("null-predicate", lambda: q1_case("a predicate that is NULL on some rows", 707, CHUNKED, nulls={"ship": 0.2}))]


RANGE_KEYS = (A.I8, A.I16, A.I32, A.I64, A.U8)
RANGE_LENS = [1024, 300]                               # the last row of the tail tile is row 1323
RANGE_POSITIONS = {"first": 0, "tail-end": 1323, "null-value": 517}


def range_case(key_dt, where, bad_id, ngroups=5, cus=None, dropped=False):
    """One id outside [0, ngroups) planted at `where`; dropped: column 2 (Int32) is 0 at that row and a predicate reads it."""
    lens = RANGE_LENS if cus is None else [long_rows(cus)]
    n = sum(lens)
    row = RANGE_POSITIONS[where] if cus is None else third_tile_row(cus, 5, 77)
    rng = np.random.default_rng(800 + key_dt)
    e, pred, k, vals = key_program(1, pred_col=2 if dropped else None)
    vvalid = _all_valid(n)
    if where == "null-value":
        vvalid[row] = False
    cols = key_columns(rng, key_dt, (A.F64,), lens, min(ngroups, 100), {1: vvalid})
    okcol = np.ones(n, dtype=np.int32)
    okcol[row] = 0
    if dropped:
        cols.append(chunks_of(rng, okcol, lens, A.I32))
    plant(cols[0], row, value=bad_id)
    in_catalog = (key_dt, (A.F64,)) in KEY_FAMILY and ngroups <= 8 and not dropped
    return Case(f"key {TAG[key_dt]} id {bad_id} at {where if cus is None else 'third tile'}" + (" dropped" if dropped else ""), e, cols, vals, k,
                ngroups, pred, key_sig(key_dt, (A.F64,)) if in_catalog else (INTERP if ngroups > 8 else None), exact=True,
                options={"gspec_blocks_per_cu": 1} if cus is not None else {})


Q1_RANGE_ROWS = (0, 1323, 700)


def q1_range_case(row, dropped=False):
    """The computed Q1 id: a fourth flag code (id 6) with ngroups 6 at `row`; dropped: the ship date filters that row out."""
    c = q1_case(f"q1 id 6 of 6 at row {row}" + (" dropped" if dropped else ""), 850, RANGE_LENS, 6, nulls=0.05)
    for name, value in (("flag", 3), ("status", 0), ("ship", Q1_CUTOFF + 1 if dropped else Q1_CUTOFF)):
        plant(c.cols[Q1_NAMES.index(name)], row, value=value, valid=True)
    c.q1_groups = None          # the integer restatement takes ids in range for granted: the model decides
    return c


def table_cases():
    """The interpreter's LDS table at every replica count and at the slot limit: an f64 of the general family and an i64 at
    its extremes (wrapping sums); v + i for further values."""
    def build(ng, nv, reps, skew=False):
        rng = np.random.default_rng(900 + ng + nv)
        n = TABLE_ROWS
        keys = np.concatenate([np.arange(ng), rng.integers(0, ng, n - ng)])       # every group populated
        if skew:
            keys[ng:][rng.uniform(size=n - ng) < 0.9] = 7                          # most rows in one group
        keys = keys[rng.permutation(n)]
        kdt = A.I16 if ng > 127 else A.I8
        cols = key_columns(rng, kdt, (A.F64, A.I64), [n], ng, {0: 0.03, 1: 0.05, 2: 0.05}, family="general", keys=keys)
        e = A.Expr()
        k, f, i = e.col(0), e.col(1), e.col(2)
        vals = ([f, i] + [e.op("add", f, e.scalar(float(j))) if j % 2 else e.op("add", i, e.scalar(j, A.I64)) for j in range(2, nv)])[:nv]
        if nv == 1:
            vals = [i]
        return Case(f"table ngroups {ng} nvalues {nv}", e, cols, vals, k, ng, -1, INTERP, replicas=reps)
    out = [(f"reps{reps}-ng{ng}", lambda ng=ng, nv=nv, reps=reps: build(ng, nv, reps)) for ng, nv, reps in REPLICA_CASES]
    out += [(f"limit-ng{ng}-nv{nv}", lambda ng=ng, nv=nv: build(ng, nv, 1, skew=ng == 511)) for ng, nv in SLOT_LIMIT_CASES]
    return out


def jit_cases():
    """The template through the run-time compiler: G2, G4, G8; 1- and 2-byte columns; a computed key; eight values."""
    def bool_key():
        c = key_case("BOOL key at G2", 1001, A.BOOL, (A.F64,), CHUNKED, 2, 0.1, kernel=INTERP, jit=True)
        return c

    def u8_u16():
        rng = np.random.default_rng(1002)
        cols = key_columns(rng, A.U8, (A.U16,), CHUNKED, 4, 0.1)
        e = A.Expr()
        k, v = e.col(0), e.cast(e.col(1), A.I64)
        return Case("U8 key, U16 value cast to I64 at G4", e, cols, [v], k, 4, -1, f"G4;P:-;K:c0h;V:{{{A.I64} c1t}};", exact=True, jit=True)

    def computed_i16():
        rng = np.random.default_rng(1003)
        n = sum(CHUNKED)
        a = chunks_of(rng, rng.integers(0, 3, n).astype(np.int8), CHUNKED, A.I8, _mask(rng, n, 0.05))
        b = chunks_of(rng, rng.integers(0, 2, n).astype(np.int8), CHUNKED, A.I8, _mask(rng, n, 0.05))
        v = chunks_of(rng, key_values(rng, A.F32, n, "general"), CHUNKED, A.F32, _mask(rng, n, 0.1))
        e = A.Expr()
        gid = e.op("add", e.op("multiply", e.cast(e.col(0), A.I16), e.scalar(3, A.I16)), e.cast(e.col(1), A.I16))
        sig = f"G8;P:-;K:({A.OP_ADD} ({A.OP_MUL} {{{A.I16} c0a}} k0s) {{{A.I16} c1a}});V:c2f;"
        return Case("I16 key a * 3 + b from two I8 columns, F32 value at G8", e, [a, b, v], [e.col(2)], gid, 8, -1, sig, jit=True)

    def q1_wide():
        rng = np.random.default_rng(1004)
        e, pred, gid, vals = q1_wide_program()
        cols = q1_exact_columns(rng, CHUNKED, 8, 0.1)
        sig = q1_sig(8) + f"c6d;({A.OP_MUL} c3d c4d);({A.OP_MUL} c4d c6d);"
        return Case("two key columns, eight values at G8", e, cols, vals, gid, 8, pred, sig, exact=True, jit=True)
    return [("bool-G2", bool_key), ("u8-u16-G4", u8_u16), ("i16-computed-G8", computed_i16), ("q1-wide-G8", q1_wide)]


VALUE_DTYPES = (A.I8, A.I16, A.I32, A.I64, A.U8, A.U16, A.U32, A.U64)


def value_cases():
    lens = [3000, 1, 777]
    n = sum(lens)

    def compare():
        rng = np.random.default_rng(1101)
        cols = key_columns(rng, A.I32, (A.F64,), lens, 5, 0.1, family="general")
        e = A.Expr()
        return Case("a comparison as a value", e, cols, [e.op("gt", e.col(1), e.scalar(0.0)), e.col(1)], e.col(0), 5, -1, None)

    def nonfinite():
        rng = np.random.default_rng(1102)
        keys = rng.integers(0, 5, n)
        cols = key_columns(rng, A.I32, (A.F64,), lens, 5, {0: 0.02}, family="general", keys=keys)
        col = cols[1]
        for g, specials in enumerate(([np.nan, np.inf], [np.inf, np.inf], [-np.inf], [np.inf, -np.inf])):      # group 4 stays finite
            where = np.flatnonzero(keys == g)
            for j, x in enumerate(specials):
                plant(col, int(where[len(where) // 2 + j]), value=x)
        e = A.Expr()
        return Case("NaN and infinities in a group", e, cols, [e.col(1)], e.col(0), 5, -1, key_sig(A.I32, (A.F64,)))
    out = [(f"int-{TAG[dt]}", lambda dt=dt: key_case(f"{TAG[dt]} values at their extremes", 1110 + dt, A.I32, (dt,), lens, 5, 0.1))
           for dt in VALUE_DTYPES]
    out.append(("f32", lambda: key_case("F32 values, widened exactly", 1120, A.I32, (A.F32,), lens, 5, 0.1, family="general")))
    out += [("compare", compare), ("nonfinite", nonfinite)]
    return out


GENERATORS = {"catalog": catalog_cases, "unit": unit_cases, "layout": layout_cases, "sparse": sparse_cases, "table": table_cases,
              "jit": jit_cases, "value": value_cases}
