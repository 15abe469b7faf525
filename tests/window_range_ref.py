"""CPU restatement of rdf_window_range_agg's semantics (include/rdf_mi355x.h, "Window frames with VALUE offsets").

Order, partitions and the peers f / l come from window_frame_ref.structure.  Every frame end is then answered by BRUTE FORCE
from the rule: a direct predicate over the keys of the row's partition — no search, no monotonicity argument, nothing the device
path does.  Integer bound values are Python ints (no wrap), Float64 bound values are ONE np.float64 operation; results are
window_frame_ref._fold over the frame's valid values (math.fsum for Float64 sums).

range_ref_fast answers from the same bounds with cumulative sums and running extremes, for the large GPU cases; it is valid
where window_frame_ref.exact_for_fast_path holds and tests/test_window_range_ref.py holds it to range_ref.

Spelling of a call: (name, value index, (start, end)); start / end are UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING, a number in the
key's units (0 the current row, -s = s preceding, +s = s following) or (kind, offset) with kind one of PRECEDING, CURRENT_ROW,
FOLLOWING, which is how "0 PRECEDING" is said.  The order key is (values, valid | None, descending).
"""
import math

import numpy as np

import window_frame_ref as F

UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING = F.UNBOUNDED_PRECEDING, F.UNBOUNDED_FOLLOWING
PRECEDING, CURRENT_ROW, FOLLOWING = 1, 2, 3        # rdf_frame_bound
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def norm_bound(b):
    """-> (kind, offset): kind 0 .. 4 as rdf_frame_bound, offset >= 0 (a Python int or float)."""
    if isinstance(b, str):
        return (0 if b == UNBOUNDED_PRECEDING else 4), 0
    if isinstance(b, tuple):
        return int(b[0]), b[1]
    if b == 0:
        return CURRENT_ROW, 0
    return (PRECEDING, -b) if b < 0 else (FOLLOWING, b)


def key_classes(key):
    """-> (values, ordinary): ordinary = the key is neither NULL nor (Float64) NaN."""
    vals = np.asarray(key[0])
    assert vals.dtype in (np.dtype(np.int32), np.dtype(np.int64), np.dtype(np.float64))
    valid = np.ones(len(vals), dtype=bool) if len(key) < 2 or key[1] is None else np.asarray(key[1], dtype=bool)
    ordinary = valid & ~np.isnan(vals) if vals.dtype.kind == "f" else valid.copy()
    return vals, ordinary


def _compare(keys, v, op):
    """keys (int64 / float64 array) `op` v elementwise, exactly: an integer v outside Int64 decides every row at once."""
    if keys.dtype.kind == "f":
        return {">=": keys >= v, "<=": keys <= v}[op]
    if v > I64_MAX:
        return np.full(len(keys), op == "<=")
    if v < I64_MIN:
        return np.full(len(keys), op == ">=")
    v = np.int64(v)
    return {">=": keys >= v, "<=": keys <= v}[op]


def bound_value(o, kind, s, desc, is_float):
    """The bound VALUE of an ordinary row with key o: o - d s for PRECEDING s, o + d s for FOLLOWING s, d = -1 descending."""
    plus = (kind == FOLLOWING) != bool(desc)
    if is_float:
        with np.errstate(over="ignore"):                                                        # (1e300 + 1.7e308 is +inf, by rule)
            return np.float64(o) + np.float64(s) if plus else np.float64(o) - np.float64(s)      # one IEEE operation
    return int(o) + int(s) if plus else int(o) - int(s)


def range_bounds(partition_by, key, frame):
    """-> order, ps, a, b per sorted position: the closed frame [a, b] in positions of the partition (empty where a > b)."""
    desc = bool(key[2]) if len(key) > 2 else False
    order, ps, nn, k, f, l = F.structure(partition_by, [key])
    n = len(order)
    vals, ordinary = key_classes(key)
    is_float = vals.dtype.kind == "f"
    sk = (vals.astype(np.float64) if is_float else vals.astype(np.int64))[order]
    so = ordinary[order]
    (skind, soff), (ekind, eoff) = norm_bound(frame[0]), norm_bound(frame[1])
    a, b = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    j = 0
    while j < n:
        lo, hi = int(ps[j]), int(ps[j] + nn[j])
        pk, po = sk[lo:hi], so[lo:hi]                               # the partition's keys, and which of them are ordinary
        run = np.flatnonzero(po)
        for j in range(lo, hi):
            for is_start, kind, off in ((True, skind, soff), (False, ekind, eoff)):
                if kind == 0:
                    r = 0
                elif kind == 4:
                    r = hi - lo - 1
                elif kind == CURRENT_ROW or not so[j]:
                    r = int(f[j]) if is_start else int(l[j])        # a NULL / NaN row: its own peer group
                else:
                    v = bound_value(sk[j], kind, off, desc, is_float)
                    if is_start:                                    # not before v in the sort direction
                        hit = np.flatnonzero(po & _compare(pk, v, "<=" if desc else ">="))
                        r = int(hit[0]) if len(hit) else int(run[-1]) + 1
                    else:                                           # not after v
                        hit = np.flatnonzero(po & _compare(pk, v, ">=" if desc else "<="))
                        r = int(hit[-1]) if len(hit) else int(run[0]) - 1
                if is_start:
                    a[j] = r
                else:
                    b[j] = r
        j = hi
    return order, ps, a, b


def range_ref(partition_by, key, values, calls):
    """values: [(array, valid | None), ...] Int64 / Float64.  -> [(values, valid)] per call, in the original row order."""
    outs = []
    for name, vi, frame in calls:
        assert name in F.FNS
        order, ps, a, b = range_bounds(partition_by, key, frame)
        n = len(order)
        col = valid = None
        if vi >= 0:
            col = np.asarray(values[vi][0])
            valid = np.ones(n, dtype=bool) if values[vi][1] is None else np.asarray(values[vi][1], dtype=bool)
        else:
            assert name in ("count", "first_value", "last_value")
        dt = F.out_dtype(name, col.dtype if col is not None else np.int64)
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
                res[r], ok[r] = F._fold(name, col[rows][valid[rows]].tolist(), col.dtype)
        outs.append((res, ok))
    return outs


def range_ref_fast(partition_by, key, values, calls):
    """range_ref for columns where window_frame_ref.exact_for_fast_path holds; min / max with one unbounded side only."""
    outs, bounds = [], {}
    for name, vi, frame in calls:
        if repr(frame) not in bounds:                                # calls that share a frame share the brute-force pass
            bounds[repr(frame)] = range_bounds(partition_by, key, frame)
        order, ps, a, b = bounds[repr(frame)]
        n = len(order)
        some = a <= b
        A, B = np.where(some, ps + a, 0), np.where(some, ps + b, 0)
        if vi >= 0:
            col = np.asarray(values[vi][0])
            assert F.exact_for_fast_path(col, values[vi][1])
            valid = np.ones(n, dtype=bool) if values[vi][1] is None else np.asarray(values[vi][1], dtype=bool)
            sv, sok = col[order], valid[order]
            cc = np.concatenate([[0], np.cumsum(sok.astype(np.int64))])
            cnt = np.where(some, cc[B + 1] - cc[A], 0)
        dt = F.out_dtype(name, col.dtype if vi >= 0 else np.int64)
        if name in ("first_value", "last_value"):
            res, ok = np.where(some, order[A if name == "first_value" else B], 0), some
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
            sk, ek = norm_bound(frame[0])[0], norm_bound(frame[1])[0]
            assert sk == 0 or ek == 4, "min / max over a range frame bounded on both sides is not built"
            ident = (np.iinfo(np.int64).min if ismax else np.iinfo(np.int64).max) if col.dtype.kind == "i" else (-np.inf if ismax else np.inf)
            x = np.where(sok, sv, ident)
            op = np.maximum if ismax else np.minimum
            run = np.empty_like(x)                                   # forward (from the partition's start) or backward extremes
            starts = np.flatnonzero(np.concatenate([[True], ps[1:] != ps[:-1]])) if n else np.zeros(0, dtype=np.int64)
            for lo, hi in zip(starts, list(starts[1:]) + [n]):
                run[lo:hi] = op.accumulate(x[lo:hi]) if sk == 0 else op.accumulate(x[lo:hi][::-1])[::-1]
            ok = cnt > 0
            res = np.where(ok, run[B] if sk == 0 else run[A], 0)
        out_v, out_ok = np.zeros(n, dtype=dt), np.zeros(n, dtype=bool)
        out_v[order] = np.asarray(res).astype(dt)
        out_ok[order] = ok
        outs.append((out_v, out_ok))
    return outs


def sum_slack(partition_by, key, value, frame):
    """8 (m + 1) 2^-106 T per row: m = the partition's rows up to the frame's end, T = the exact sum of |x| over the valid finite
    ones among them (math.fsum, rounded up one ulp).  The second term of the bound a Float64 SUM is held to."""
    col, valid = np.asarray(value[0], dtype=np.float64), value[1]
    order, ps, a, b = range_bounds(partition_by, key, frame)
    n = len(order)
    ok = (np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)) & np.isfinite(col)
    out = np.zeros(n)
    for j in range(n):
        if a[j] > b[j]:
            continue
        rows = order[ps[j]:ps[j] + b[j] + 1]
        t = np.nextafter(math.fsum(np.abs(col[rows][ok[rows]]).tolist()), math.inf)
        out[order[j]] = 8.0 * (b[j] + 2) * 2.0 ** -106 * t
    return out


# ---------------------------------------------------------------- the table of tests/cpp/test_window_range_host.cpp
def _positions(keys, classes, o, is_float, desc, is_end, following, s):
    """The search's answer by the direct predicate: the first position that is HIGH or whose ordinary key is not before
    (a start) / is after (an end, one past) the bound value; len(keys) when there is none."""
    v = bound_value(o, FOLLOWING if following else PRECEDING, s, desc, is_float)
    for j, (kk, c) in enumerate(zip(keys, classes)):
        if c == 2:
            return j
        if c == 1:
            continue
        kk = np.float64(kk) if is_float else int(kk)
        after = (kk < v) if desc else (kk > v)
        if after or (not is_end and kk == v):
            return j
    return len(keys)


def write_host_table(path, seed=7):
    """One line per search: f64 desc is_end following offset o nkeys key:class ... expect.  Keys and offsets of Float64 cases
    are written as the hex of their bits.  -> the number of lines."""
    rng = np.random.default_rng(seed)
    lines = []

    def emit(keys, classes, is_float, desc, offsets):
        for o, c in zip(keys, classes):
            if c != 0:
                continue
            for s in offsets:
                for is_end in (0, 1):
                    for following in (0, 1):
                        want = _positions(keys, classes, o, is_float, desc, is_end, following, s)
                        enc = (lambda x: "%016x" % np.array([x], dtype=np.float64).view(np.uint64)[0]) if is_float else (lambda x: str(int(x)))
                        lines.append(" ".join([str(int(is_float)), str(int(desc)), str(is_end), str(following), enc(s), enc(o), str(len(keys))] +
                                              ["%s:%d" % (enc(kk), cc) for kk, cc in zip(keys, classes)] + [str(want)]))

    def laid_out(ordinary, is_float, desc, nlow, nhigh):
        ks = sorted(ordinary, reverse=desc)
        fill = 0.0 if is_float else 0
        return [fill] * nlow + ks + [fill] * nhigh, [1] * nlow + [0] * len(ks) + [2] * nhigh

    i64 = [I64_MIN, I64_MIN + 1, -(1 << 31), -(1 << 31) + 1, -1, 0, 1, 1, 7, (1 << 31) - 1, I64_MAX - 1, I64_MAX, I64_MAX]
    for desc in (False, True):
        for nhigh in (0, 2):
            keys, classes = laid_out(i64, False, desc, 0, nhigh)
            emit(keys, classes, False, desc, [0, 1, 7, (1 << 62), I64_MAX])
        keys, classes = laid_out([I64_MIN], False, desc, 0, 1)
        emit(keys, classes, False, desc, [1, I64_MAX])
        for _ in range(20):
            ks = rng.integers(-20, 20, size=int(rng.integers(1, 40))).tolist()
            keys, classes = laid_out(ks, False, desc, 0, int(rng.integers(0, 3)))
            emit(keys, classes, False, desc, [0, 1, 3, 50])
    sub = float(np.nextafter(0.0, 1.0))
    f64 = [-math.inf, -1e300, -1.0, -0.5, -sub, -0.0, 0.0, sub, 2 * sub, 0.1, 0.2, 0.3, 0.30000000000000004, 0.5, 1.0, 1e300, math.inf, math.inf]
    for desc in (False, True):
        for nlow, nhigh in ((0, 0), (2, 1)) if desc else ((0, 0), (0, 3)):
            keys, classes = laid_out(f64, True, desc, nlow, nhigh)
            emit(keys, classes, True, desc, [0.0, sub, 0.1, 0.2, 0.5, 1e300, 1.7976931348623157e308])
        for _ in range(20):
            ks = (rng.integers(-30, 30, size=int(rng.integers(1, 40))) / 10.0).tolist()
            keys, classes = laid_out(ks, True, desc, int(rng.integers(0, 3)) if desc else 0, int(rng.integers(0, 3)))
            emit(keys, classes, True, desc, [0.0, 0.1, 0.2, 0.5])
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return len(lines)
