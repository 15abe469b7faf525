"""The executable model of rdf_null_test / rdf_coalesce / rdf_case_when / rdf_extremum / rdf_nanvl and of the Utf8 forms of
coalesce / case_when: Spark 3's semantics in numpy over (values, valid) pairs and Python lists of `bytes | None`.

A part is a pair (values, valid) of equal length — values a numpy array of the call's dtype, valid a bool array — or a
literal: a Python scalar, or None for the NULL literal.  Results are pairs too; NULL rows hold 0.  Values are moved as they
are, never recomputed: a NaN keeps its payload and -0.0 its sign.

    ordering   integers in their own signedness; floats with -0.0 == 0.0, NaN == NaN and NaN above every number
    extremum   a left-to-right fold with a STRICT comparison: of equal parts the leftmost one's bits are returned
    nanvl      a unless it is NaN, then b; NULL with a, and with b where a is NaN
    case_when  the first branch whose condition is valid AND true; none: `otherwise`, which absent is NULL

tests/test_select_ref.py holds this file to pyarrow where the two agree and to Spark's documented answers."""
import numpy as np

IS_NULL, IS_NOT_NULL, IS_NAN = range(3)
DTYPES = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32,
          "u64": np.uint64, "f32": np.float32, "f64": np.float64}
FLOATS = ("f32", "f64")


def bits_of(v):
    """The unsigned integers holding the values' bytes."""
    v = np.ascontiguousarray(v)
    return v.view(f"u{v.dtype.itemsize}")


def part(p, n, dtype):
    """(values, valid) of a part over n rows."""
    if isinstance(p, tuple):
        v, m = p
        v = np.asarray(v)
        assert v.dtype == np.dtype(dtype) and len(v) == n, (v.dtype, dtype, len(v), n)
        return v, (np.ones(n, dtype=bool) if m is None else np.asarray(m, dtype=bool))
    if p is None:
        return np.zeros(n, dtype=dtype), np.zeros(n, dtype=bool)
    return np.full(n, p, dtype=dtype), np.ones(n, dtype=bool)


def rows_of(parts):
    return next(len(p[0]) for p in parts if isinstance(p, tuple))


def finish(v, m):
    v = v.copy()
    v[~m] = 0
    return v, m


# ---------------------------------------------------------------- masks
def null_test(op, values, valid):
    """-> bool array (never NULL).  valid None: no row is NULL.  isnan(NULL) is false."""
    n = len(values)
    m = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    if op == IS_NULL:
        return ~m
    if op == IS_NOT_NULL:
        return m.copy()
    return m & np.isnan(values)


# ---------------------------------------------------------------- coalesce / case_when
def coalesce(parts, dtype):
    n = rows_of(parts)
    out, have = np.zeros(n, dtype=dtype), np.zeros(n, dtype=bool)
    for p in parts:
        v, m = part(p, n, dtype)
        take = m & ~have
        out[take] = v[take]
        have |= m
    return finish(out, have)


def case_when(conds, values, otherwise, dtype):
    """conds: [(bool values, valid | None)]; values: parts; otherwise: a part (None: NULL, as an absent one)."""
    n = len(conds[0][0])
    out, ok, decided = np.zeros(n, dtype=dtype), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for (c, cm), p in zip(conds, values):
        holds = np.asarray(c, dtype=bool) & (np.ones(n, dtype=bool) if cm is None else np.asarray(cm, dtype=bool))
        v, m = part(p, n, dtype)
        take = holds & ~decided
        out[take] = v[take]
        ok[take] = m[take]
        decided |= holds
    v, m = part(otherwise, n, dtype)
    out[~decided] = v[~decided]
    ok[~decided] = m[~decided]
    return finish(out, ok)


# ---------------------------------------------------------------- Spark's ordering
def gt(a, b):
    """a > b elementwise; NaN is above every number and equal to NaN; -0.0 == 0.0."""
    if a.dtype.kind != "f":
        return a > b
    na, nb = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        return np.where(na, ~nb, np.where(nb, False, a > b))


def extremum(greatest, parts, dtype):
    n = rows_of(parts)
    acc, have = np.zeros(n, dtype=dtype), np.zeros(n, dtype=bool)
    for p in parts:
        v, m = part(p, n, dtype)
        better = gt(v, acc) if greatest else gt(acc, v)
        take = m & (~have | better)
        acc[take] = v[take]
        have |= m
    return finish(acc, have)


def nanvl(a, b, dtype):
    n = rows_of([a, b])
    (av, am), (bv, bm) = part(a, n, dtype), part(b, n, dtype)
    nan = np.isnan(av)
    out = np.where(nan, bv, av)
    return finish(out, am & (~nan | bm))


# ---------------------------------------------------------------- Utf8: lists of bytes | None; a literal is bytes or None
def utf8_part(p, n):
    return list(p) if isinstance(p, list) else [p] * n


def utf8_coalesce(parts):
    n = next(len(p) for p in parts if isinstance(p, list))
    cols = [utf8_part(p, n) for p in parts]
    return [next((c[i] for c in cols if c[i] is not None), None) for i in range(n)]


def utf8_case_when(conds, values, otherwise):
    n = len(conds[0][0])
    cols, other = [utf8_part(p, n) for p in values], utf8_part(otherwise, n)
    out = []
    for i in range(n):
        k = next((k for k, (c, cm) in enumerate(conds) if c[i] and (cm is None or cm[i])), None)
        out.append(other[i] if k is None else cols[k][i])
    return out


# ---------------------------------------------------------------- values that matter
def edge_values(name):
    """The extremes of a dtype: for floats also +-0, +-inf, the subnormal ends and NaNs with different payloads and signs."""
    dt = np.dtype(DTYPES[name])
    if dt.kind != "f":
        info = np.iinfo(dt)
        span = [info.min, info.min + 1, -1, 0, 1, info.max - 1, info.max] if dt.kind == "i" else [0, 1, info.max // 2, info.max // 2 + 1, info.max - 1, info.max]
        return np.array(span, dtype=dt)
    fi = np.finfo(dt)
    u = f"u{dt.itemsize}"
    nan_bits = {4: [0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], 8: [0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF]}[dt.itemsize]
    plain = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, fi.max, fi.min, fi.tiny, -fi.tiny, fi.smallest_subnormal, 123.0, 1.5], dtype=dt)
    return np.concatenate([plain, np.array(nan_bits, dtype=u).view(dt)])


def random_values(name, n, rng):
    """A third edge values, a third a narrow range (ties happen), a third the type's full range of bit patterns."""
    dt = np.dtype(DTYPES[name])
    edges = edge_values(name)
    narrow = rng.integers(0, 4, n).astype(dt) if dt.kind == "u" else rng.integers(-2, 3, n).astype(dt)
    wide = rng.integers(0, 2**(8 * dt.itemsize), n, dtype=np.uint64, endpoint=False) if dt.itemsize < 8 else rng.integers(0, 2**64, n, dtype=np.uint64, endpoint=False)
    wide = wide.astype(f"u{dt.itemsize}").view(dt)
    pick = rng.integers(0, 3, n)
    return np.where(pick == 0, edges[rng.integers(0, len(edges), n)], np.where(pick == 1, narrow, wide)).astype(dt)


# ---------------------------------------------------------------- the table of tests/cpp/test_select_host.cpp
def write_host_table(path, rows_per_dtype=10_000, seed=11):
    """One line per row, every number in hex, a part as `valid bits`:
         X dtype nparts part*   coalesce greatest least      (each result as `valid bits`)
         W dtype nbranches holds part*(nbranches + 1)   result      (bit k of holds: condition k is valid and true; the last part is `otherwise`)
         N dtype a b   result                                        (Float32 / Float64)
    Per dtype rows_per_dtype random rows of 1..8 parts with random NULLs, and every pair and triple of the edge values.
    -> the number of lines."""
    rng = np.random.default_rng(seed)
    lines = []

    def cell(v, m, i):
        return f"{int(m[i]):x} {int(bits_of(v)[i]):x}"

    for name, npdt in DTYPES.items():
        dt = np.dtype(npdt)
        edges = edge_values(name)
        e = len(edges)
        batches = []                                                        # (nparts, [(values, valid)])
        per = rows_per_dtype // 8 + 1
        for nparts in range(1, 9):
            batches.append([(random_values(name, per, rng), rng.uniform(size=per) > 0.35) for _ in range(nparts)])
        a, b = np.repeat(edges, e), np.tile(edges, e)                       # every ordered pair, then every ordered triple
        batches.append([(a, np.ones(e * e, dtype=bool)), (b, np.ones(e * e, dtype=bool))])
        a3, b3, c3 = np.repeat(edges, e * e), np.tile(np.repeat(edges, e), e), np.tile(edges, e * e)
        batches.append([(a3, np.ones(e**3, dtype=bool)), (b3, rng.uniform(size=e**3) > 0.2), (c3, np.ones(e**3, dtype=bool))])
        for parts in batches:
            n = len(parts[0][0])
            co, gr, le = coalesce(parts, dt), extremum(True, parts, dt), extremum(False, parts, dt)
            for i in range(n):
                lines.append(f"X {name} {len(parts):x} " + " ".join(cell(v, m, i) for v, m in parts) + f" {cell(*co, i)} {cell(*gr, i)} {cell(*le, i)}")
        for nb in range(1, 9):
            n = per
            conds = [(rng.uniform(size=n) > 0.6, rng.uniform(size=n) > 0.2) for _ in range(nb)]
            parts = [(random_values(name, n, rng), rng.uniform(size=n) > 0.3) for _ in range(nb + 1)]
            res = case_when(conds, parts[:-1], parts[-1], dt)
            holds = sum((c & m).astype(np.int64) << k for k, (c, m) in enumerate(conds))
            for i in range(n):
                lines.append(f"W {name} {nb:x} {int(holds[i]):x} " + " ".join(cell(v, m, i) for v, m in parts) + f" {cell(*res, i)}")
        if name in FLOATS:
            n = rows_per_dtype
            av, bv = np.concatenate([random_values(name, n, rng), np.repeat(edges, e)]), np.concatenate([random_values(name, n, rng), np.tile(edges, e)])
            am, bm = rng.uniform(size=len(av)) > 0.2, rng.uniform(size=len(av)) > 0.2
            res = nanvl((av, am), (bv, bm), dt)
            for i in range(len(av)):
                lines.append(f"N {name} {cell(av, am, i)} {cell(bv, bm, i)} {cell(*res, i)}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)
