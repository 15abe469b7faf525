"""The layouts the streamed batch loop is held to its model at (stream_ref.py), shared by the CPU test that pins the model to the
oracle and the GPU test that holds the library to the model.

One layout for every sink: 23 266 rows in 13 batches whose lengths sit on both sides of a byte, a 64-row word, a 1024-row piece
and two pieces, with an empty batch, a 6000-row batch that is cut into six pieces, an all-NULL batch and a 9000-row batch;
every batch at an offset of its own (0-9), so that the bit phase `(offset + row0) & 7` of the pieces differs from batch to
batch; NULL fractions 0 and 0.1.  Slabs of 16 KiB, 64 KiB and 200 KiB cut it into some twenty, five and two slabs for 16-byte
rows; a call whose input is too small for two slabs of that size gets a third of its bytes instead (`slabs_for`)."""
import numpy as np

from rust_dataframe_amd import _abi as A

LENS = [1023, 1024, 1025, 0, 1, 7, 9, 63, 65, 2049, 6000, 3000, 9000]
ALL_NULL_BATCH = 11
OFFSETS = [3, 0, 7, 1, 9, 2, 8, 5, 4, 6, 1, 3, 5]
SLABS = (16 << 10, 64 << 10, 200 << 10)
NUMERIC = (A.I8, A.I16, A.I32, A.I64, A.U8, A.U16, A.U32, A.U64, A.F32, A.F64)
assert len(LENS) == len(OFFSETS) and sum(LENS) == 23266


def input_bytes(cols):
    """What the library counts before it decides to stream (host_input_bytes)."""
    b = 0
    for col in cols:
        for ch in col:
            b += (ch.length + 7) // 8 if ch.dtype == A.BOOL else ch.length * np.dtype(A.NP_OF[ch.dtype]).itemsize
            if ch.validity is not None and ch.length:
                b += (ch.length + 7) // 8
    return b


def slabs_for(cols):
    n = input_bytes(cols)
    return sorted({s if n > 2 * s else n // 3 for s in SLABS})


def column(rng, dtype, values=None, nulls=0.1, lens=LENS, offsets=OFFSETS, all_null=ALL_NULL_BATCH, kind="plain"):
    """A chunk list over the common layout.  values: a vector over all rows (or None: random of `kind`); nulls: the NULL
    fraction (0: no validity buffer at all; > 0: every batch carries one and batch `all_null` is NULL throughout)."""
    n = int(sum(lens))
    if values is None:
        if dtype == A.BOOL:
            values = rng.integers(0, 2, n).astype(bool)
        elif dtype in (A.F32, A.F64):
            values = rng.uniform(-1.0, 1.0, n) if kind == "unit" else rng.uniform(-100.0, 100.0, n)
        else:
            info = np.iinfo(A.NP_OF[dtype])
            if kind == "extreme":
                values = rng.integers(info.min, info.max, n, dtype=A.NP_OF[dtype], endpoint=True)
            else:
                values = rng.integers(max(info.min, -1000), min(info.max, 1000), n, endpoint=True)
    values = np.asarray(values)
    out, at = [], 0
    for i, (ln, off) in enumerate(zip(lens, offsets)):
        valid = None
        if nulls > 0:
            valid = np.zeros(ln, dtype=bool) if i == all_null else rng.uniform(size=ln) >= nulls
        v = values[at:at + ln]
        out.append(A.HostArray.from_numpy(v if dtype == A.BOOL else v.astype(A.NP_OF[dtype]), valid=valid, offset=off, dtype=dtype, rng=rng))
        at += ln
    return out


def agg_case(rng, vdt, values=None, kind="plain"):
    """A value column of `vdt` summed under a predicate on a column of another width, next to a wide Int64 column whose sum
    wraps: -> (expr, cols, value roots, filter root).  Float32 "plain" data is integer-valued in [-100, 100]: sum|x| < 2^24."""
    pdt = A.F64 if vdt in (A.I8, A.U8, A.I16, A.U16) else A.I16
    if values is None and vdt == A.F32 and kind == "plain":
        values = rng.integers(-100, 100, sum(LENS), endpoint=True)
    cols = [column(rng, vdt, values, nulls=0.1, kind=kind), column(rng, pdt, nulls=0.1), column(rng, A.I64, nulls=0.0, kind="extreme")]
    e = A.Expr()
    return e, cols, [e.col(0), e.col(2)], e.op("gt", e.col(1), e.scalar(-30.0))


CASTS = [(A.I8, A.I64), (A.I64, A.U8), (A.F64, A.I32), (A.BOOL, A.I32), (A.I32, A.BOOL)]


def cast_case(rng, src, dst):
    """A nullable column of `src` for rdf_cast to `dst`; I64 -> U8 and F64 -> I32 hold values the target cannot represent (NULLs appear)."""
    n = sum(LENS)
    if (src, dst) == (A.I64, A.U8):
        v = rng.integers(-200, 400, n)
    elif src == A.F64:
        v = rng.uniform(-3e9, 3e9, n)
        v[::5] = rng.uniform(-1000.0, 1000.0, len(v[::5]))
    elif src == A.I32:
        v = rng.integers(-2, 2, n, endpoint=True)
    else:
        v = None
    return column(rng, src, v, nulls=0.1)


def filter_case(rng, selectivity):
    """Columns of 1, 2, 4 and 8 bytes, nullable and not, and both predicate forms over them: -> (cols, {name: (expr, root)}).
    selectivity: 0, 1, 0.5 or 1 / 64 of the rows pass (column 3, uniform in [0, 1), is the one the predicates test)."""
    n = sum(LENS)
    u = rng.uniform(0.0, 1.0, n)
    cols = [column(rng, A.I8, nulls=0.1), column(rng, A.U16, nulls=0.0), column(rng, A.F32, nulls=0.1), column(rng, A.F64, u, nulls=0.0 if selectivity in (0, 1) else 0.1),
            column(rng, A.I64, nulls=0.0, kind="extreme")]
    cut = {0: -1.0, 1: 2.0}.get(selectivity, selectivity)
    e1 = A.Expr()
    one_term = e1.op("lt", e1.col(3), e1.scalar(float(cut)))
    e2 = A.Expr()
    arith = e2.op("and", e2.op("lt", e2.op("multiply", e2.col(3), e2.scalar(2.0)), e2.scalar(2.0 * float(cut))), e2.op("ge", e2.col(4), e2.scalar(np.iinfo(np.int64).min, A.I64)))
    return cols, {"one term": (e1, one_term), "arithmetic inside": (e2, arith)}


def groupby_case(rng, kdt, vdt, ngroups=40):
    """Keys without NULLs (I64 around 0, or U64 above 2^63) and nullable values.  Planted: key `null_everywhere` has no valid
    value at all, key `late_valid` is NULL in every batch but the last, key `last_only` appears in the last batch alone.
    -> (keys, values | None, distinct keys)."""
    n = sum(LENS)
    base = 2 ** 63 + 5 if kdt == A.U64 else -ngroups // 2
    k = rng.integers(0, ngroups, n).astype(A.NP_OF[kdt]) + A.NP_OF[kdt](base)
    last0 = n - LENS[-1]
    null_everywhere, late_valid, last_only = base + ngroups, base + ngroups + 1, base + ngroups + 2
    k[5:last0:211] = null_everywhere
    k[last0 + 5::300] = null_everywhere
    k[9:last0:173] = late_valid
    k[last0 + 9::250] = late_valid
    k[last0 + 100::400] = last_only
    keys = column(rng, kdt, k, nulls=0.0)
    if vdt is None:
        return keys, None, ngroups + 3
    vals = column(rng, vdt, nulls=0.1, kind="unit" if vdt in (A.F32, A.F64) else "plain")
    for i, (kc, vc) in enumerate(zip(keys, vals)):           # NULL out the planted groups' values
        kk = kc.to_numpy()
        ok = vc.valid_mask()
        ok[kk == A.NP_OF[kdt](null_everywhere)] = False
        if i < len(LENS) - 1:
            ok[kk == A.NP_OF[kdt](late_valid)] = False
        else:
            ok[kk == A.NP_OF[kdt](late_valid)] = True
        vals[i] = A.HostArray.from_numpy(vc.to_numpy(), valid=ok, offset=vc.offset, dtype=vdt, rng=rng)
    return keys, vals, ngroups + 3


def marked_f64(rng, n, every=997):
    """Integer-valued f64 data with 2^40 markers: every partial sum is an integer far below 2^53, so every order of additions gives
    the same bits — and a piece that is lost or counted twice moves the sum by at least 1."""
    v = rng.integers(-1000, 1000, n).astype(np.float64)
    v[::every] += 2.0 ** 40
    return v


def cancelling_f64(rng, n):
    """Large values of both signs whose sum is small: sum|x| is 10^9 times the sum."""
    v = rng.uniform(-1.0, 1.0, n) * 1e9
    v[1::2] = -v[0::2][:len(v[1::2])] + rng.uniform(-1.0, 1.0, len(v[1::2]))
    return v
