"""CPU restatement of rdf_window_agg's semantics (include/rdf_mi355x.h, "Window FRAMES") in numpy + math.fsum.

The order comes from window_ref.key_codes and one stable np.lexsort, as in window_ref.  frame_ref then answers every row by
BRUTE FORCE over the positions of its frame: it slices the partition, drops the NULLs and folds what is left — no prefix
differences, no block decomposition, nothing the device path does.  Float sums are math.fsum (correctly rounded).

frame_ref_fast is the vectorised path for the large GPU cases.  It is valid only where cumulative sums are exact: Int64
columns (wrapping) and integer-valued doubles whose partial sums stay below 2^53, without NaN, infinities or -0.0.  Sums and
counts are prefix differences there, min / max come from a sparse table of power-of-two windows.  tests/test_window_frame_ref.py
holds it to frame_ref on small inputs.

Spelling of a call: (name, value index, (unit, start, end)) with unit "rows" / "range" and start / end UNBOUNDED_PRECEDING,
UNBOUNDED_FOLLOWING or an integer — 0 the current row, -s = s preceding, +s = s following (WindowSpec's convention).
Every answer is (values, valid): int64 for count, the value dtype for sum / min / max, float64 for avg, uint32 row indices
for first_value / last_value.
"""
import math

import numpy as np

import window_ref

UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING = "unbounded_preceding", "unbounded_following"
FNS = ("sum", "min", "max", "count", "avg", "first_value", "last_value")
QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def structure(partition_by, order_by, nrows=None):
    """-> order (sorted position -> row), ps (first position of the partition), nn, k, f, l per sorted position."""
    pcodes = [window_ref.key_codes(*window_ref._split(k, False)) for k in partition_by]
    ocodes = [window_ref.key_codes(*window_ref._split(k, True)) for k in order_by]
    allc = pcodes + ocodes
    n = len(allc[0]) if allc else int(nrows)
    order = (np.lexsort(tuple(reversed(allc))) if allc else np.arange(n)).astype(np.int64)
    pos = np.arange(n, dtype=np.int64)
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return order, z, z, z, z, z
    P = np.zeros(n, dtype=bool)
    P[0] = True
    for c in pcodes:
        s = c[order]
        P[1:] |= s[1:] != s[:-1]
    G = P.copy()
    for c in ocodes:
        s = c[order]
        G[1:] |= s[1:] != s[:-1]
    ps = np.maximum.accumulate(np.where(P, pos, 0))
    pid = np.cumsum(P) - 1
    nn = np.bincount(pid)[pid]
    gs = np.maximum.accumulate(np.where(G, pos, 0))
    gid = np.cumsum(G) - 1
    f = gs - ps
    l = f + np.bincount(gid)[gid] - 1
    return order, ps, nn, pos - ps, f, l


def frame_bounds(frame, nn, k, f, l):
    """The closed frame [a, b] of every sorted position, clipped to the partition (empty where a > b)."""
    unit, start, end = frame
    assert unit in ("rows", "range")
    rng = unit == "range"

    def bound(v, is_start):
        if isinstance(v, str):
            assert v in (UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING)
            return np.zeros_like(k) if v == UNBOUNDED_PRECEDING else nn - 1
        v = int(v)
        if v == 0:
            return (f if is_start else l) if rng else k
        assert not rng, "range offsets are not built"
        return k + v
    a, b = bound(start, True), bound(end, False)
    return np.maximum(a, 0), np.minimum(b, nn - 1)


def _total_order_key(x):
    """Non-NaN doubles in IEEE total order: the value, and -0.0 before +0.0."""
    return (x, 0 if math.copysign(1.0, x) < 0 else 1)


def _fold(name, vals, dtype):
    """One frame's answer from its valid values (a list of Python numbers) -> (value, valid)."""
    c = len(vals)
    if name == "count":
        return c, True
    if c == 0:
        return 0, False
    if dtype.kind == "i":
        if name == "sum":
            s = sum(int(v) for v in vals) & 0xFFFFFFFFFFFFFFFF
            return s - (1 << 64) if s >= 1 << 63 else s, True
        if name == "avg":
            return _fold("sum", [float(v) for v in vals], np.dtype(np.float64))[0] / float(c), True
        return (min(vals) if name == "min" else max(vals)), True
    if name in ("sum", "avg"):
        nan = any(math.isnan(v) for v in vals)
        pinf, ninf = any(v == math.inf for v in vals), any(v == -math.inf for v in vals)
        if nan or (pinf and ninf):
            s = QNAN
        elif pinf or ninf:
            s = math.inf if pinf else -math.inf
        else:
            s = math.fsum(vals)
            s = 0.0 if s == 0 else s
        return (s / float(c) if name == "avg" else s), True
    real = [v for v in vals if not math.isnan(v)]
    if not real:
        return QNAN, True
    return (min(real, key=_total_order_key) if name == "min" else max(real, key=_total_order_key)), True


def out_dtype(name, vdtype):
    return np.dtype(np.int64) if name == "count" else np.dtype(np.float64) if name == "avg" else \
        np.dtype(np.uint32) if name in ("first_value", "last_value") else np.dtype(vdtype)


def frame_ref(partition_by, order_by, values, calls, nrows=None):
    """values: [(array, valid | None), ...] Int64 / Float64.  -> [(values, valid)] per call, in the original row order."""
    if nrows is None and not (partition_by or order_by):
        nrows = len(values[0][0])
    order, ps, nn, k, f, l = structure(partition_by, order_by, nrows)
    n = len(order)
    outs = []
    for name, vi, frame in calls:
        assert name in FNS
        a, b = frame_bounds(frame, nn, k, f, l)
        col = valid = None
        if vi >= 0:
            col = np.asarray(values[vi][0])
            valid = np.ones(n, dtype=bool) if values[vi][1] is None else np.asarray(values[vi][1], dtype=bool)
        else:
            assert name in ("count", "first_value", "last_value")
        dt = out_dtype(name, col.dtype if col is not None else np.int64)
        res, ok = np.zeros(n, dtype=dt), np.zeros(n, dtype=bool)
        for j in range(n):
            rows = order[ps[j] + a[j]:ps[j] + b[j] + 1] if a[j] <= b[j] else order[:0]
            r = order[j]
            if name in ("first_value", "last_value"):
                ok[r] = len(rows) > 0
                res[r] = (rows[0] if name == "first_value" else rows[-1]) if ok[r] else 0
            elif vi < 0:
                res[r], ok[r] = len(rows), True
            else:
                res[r], ok[r] = _fold(name, col[rows][valid[rows]].tolist(), col.dtype)
        outs.append((res, ok))
    return outs


def sum_slack(partition_by, order_by, value, frame, nrows=None):
    """8 (m + 1) 2^-106 T per row: m = the partition's rows up to the frame's end, T = the exact sum of |x| over the valid finite
    ones among them (math.fsum, rounded up one ulp).  The second term of the bound a Float64 SUM is held to."""
    col, valid = np.asarray(value[0], dtype=np.float64), value[1]
    if nrows is None and not (partition_by or order_by):
        nrows = len(col)
    order, ps, nn, k, f, l = structure(partition_by, order_by, nrows)
    n = len(order)
    ok = (np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)) & np.isfinite(col)
    a, b = frame_bounds(frame, nn, k, f, l)
    out = np.zeros(n)
    for j in range(n):
        if a[j] > b[j]:
            continue
        rows = order[ps[j]:ps[j] + b[j] + 1]
        t = np.nextafter(math.fsum(np.abs(col[rows][ok[rows]]).tolist()), math.inf)
        out[order[j]] = 8.0 * (b[j] + 2) * 2.0 ** -106 * t
    return out


def exact_for_fast_path(col, valid=None):
    """Is a column inside frame_ref_fast's domain?"""
    col = np.asarray(col)
    if col.dtype.kind == "i":
        return True
    ok = np.ones(len(col), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    x = col[ok]
    return bool(np.isfinite(x).all() and (x == np.round(x)).all() and not (np.signbit(x) & (x == 0)).any() and np.abs(x).sum() < 2.0 ** 53)


def _sparse_table(x, ismax):
    op = np.maximum if ismax else np.minimum
    tabs = [x]
    w = 1
    while 2 * w <= len(x):
        prev = tabs[-1]
        tabs.append(op(prev[:-w], prev[w:]))
        w *= 2
    return tabs


def frame_ref_fast(partition_by, order_by, values, calls, nrows=None):
    """frame_ref, vectorised, for columns where exact_for_fast_path holds."""
    if nrows is None and not (partition_by or order_by):
        nrows = len(values[0][0])
    order, ps, nn, k, f, l = structure(partition_by, order_by, nrows)
    n = len(order)
    outs = []
    for name, vi, frame in calls:
        a, b = frame_bounds(frame, nn, k, f, l)
        some = a <= b
        A, B = np.where(some, ps + a, 0), np.where(some, ps + b, 0)          # global sorted positions
        if vi >= 0:
            col = np.asarray(values[vi][0])
            assert exact_for_fast_path(col, values[vi][1])
            valid = np.ones(n, dtype=bool) if values[vi][1] is None else np.asarray(values[vi][1], dtype=bool)
            sv, sok = col[order], valid[order]
            cc = np.concatenate([[0], np.cumsum(sok.astype(np.int64))])
            cnt = np.where(some, cc[B + 1] - cc[A], 0) if n else np.zeros(0, dtype=np.int64)
        dt = out_dtype(name, col.dtype if vi >= 0 else np.int64)
        if name in ("first_value", "last_value"):
            res, ok = np.where(some, order[A if name == "first_value" else B], 0) if n else np.zeros(0), some
        elif name == "count":
            res, ok = (cnt if vi >= 0 else np.where(some, b - a + 1, 0)), np.ones(n, dtype=bool)
        elif name in ("sum", "avg"):
            x = np.where(sok, sv, 0)
            if name == "avg":
                x = x.astype(np.float64)
                assert np.abs(x).sum() < 2.0 ** 53
            with np.errstate(over="ignore"):
                cs = np.concatenate([np.zeros(1, dtype=x.dtype), np.cumsum(x)])
                s = cs[B + 1] - cs[A]
            ok = cnt > 0
            res = np.where(ok, s, 0)
            if name == "avg":
                res = np.where(ok, res / np.maximum(cnt, 1).astype(np.float64), 0.0)
            elif dt.kind == "f":
                res = res + 0.0
        else:
            ismax = name == "max"
            if col.dtype.kind == "i":
                ident = np.iinfo(np.int64).min if ismax else np.iinfo(np.int64).max
            else:
                ident = -np.inf if ismax else np.inf
            tabs = _sparse_table(np.where(sok, sv, ident), ismax)
            length = np.maximum(B - A + 1, 1)
            lev = np.floor(np.log2(length)).astype(np.int64)
            lev = np.where((1 << lev) > length, lev - 1, lev)
            res = np.zeros(n, dtype=col.dtype)
            op = np.maximum if ismax else np.minimum
            for t in np.unique(lev) if n else []:
                m = lev == t
                res[m] = op(tabs[t][A[m]], tabs[t][B[m] - (1 << t) + 1])
            ok = cnt > 0
            res = np.where(ok, res, 0)
        out_v, out_ok = np.zeros(n, dtype=dt), np.zeros(n, dtype=bool)
        out_v[order] = np.asarray(res).astype(dt)
        out_ok[order] = ok
        outs.append((out_v, out_ok))
    return outs


def sum_slack_fast(partition_by, order_by, value, frame, nrows=None):
    """sum_slack where exact_for_fast_path holds (the cumulative sum of |x| is exact there)."""
    col, valid = np.asarray(value[0], dtype=np.float64), value[1]
    assert exact_for_fast_path(col, valid)
    if nrows is None and not (partition_by or order_by):
        nrows = len(col)
    order, ps, nn, k, f, l = structure(partition_by, order_by, nrows)
    n = len(order)
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    cs = np.concatenate([[0.0], np.cumsum(np.where(ok, np.abs(col), 0.0)[order])])
    a, b = frame_bounds(frame, nn, k, f, l)
    some = a <= b
    B = np.where(some, ps + b, 0)
    out = np.zeros(n)
    out[order] = np.where(some, 8.0 * (b + 2) * 2.0 ** -106 * (cs[B + 1] - cs[ps]), 0.0)
    return out
