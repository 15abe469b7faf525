"""CPU restatement of rdf_groupby_sorted's semantics (include/rdf_mi355x.h, "sorted GROUP BY") in plain Python / numpy.

A column is (values, valid): `values` a numpy array (numeric) or a sequence of bytes objects (Utf8; None = NULL), `valid` a
bool array or None.  The rows are put into a dict of key tuple -> row list; the key of a row is the tuple of its columns'
dense codes from window_ref.key_codes (equal values equal codes, floats canonical, NULL the largest code), so iterating the
dict in sorted key order IS the header's group order.  Per group the distinct values are a Python set of the value column's
codes; sums are exact: Python integers reduced mod 2^64, math.fsum (correctly rounded) for floats.  Nothing here is derived
from the library: no sort of (key, value) pairs, no head list, no segmented reduction.
"""
import math

import numpy as np

from window_ref import canonical, key_codes

FNS = ("count_distinct", "sum_distinct", "first", "last")


def _valid_of(col):
    values, valid = col[0], col[1] if len(col) > 1 else None
    n = len(values)
    if isinstance(values, np.ndarray):
        ok = np.ones(n, dtype=bool)
    else:
        ok = np.array([v is not None for v in values], dtype=bool).reshape(n)
    if valid is not None:
        ok &= np.asarray(valid, dtype=bool)
    return ok


def group_rows_of(keys, n):
    """-> [(key tuple of codes, [rows ascending])] in ascending key order, NULL last.  No keys: one group of all rows."""
    codes = [key_codes(k[0], k[1] if len(k) > 1 else None) for k in keys]
    groups = {}
    for i in range(n):
        groups.setdefault(tuple(int(c[i]) for c in codes), []).append(i)
    return sorted(groups.items())


def ieee_sum(vals):
    """The sum of float64 values as IEEE defines it where it is not finite, correctly rounded (math.fsum) where it is.
    -> (sum, m, sum_abs): m and sum_abs over the finite values."""
    vals = [float(v) for v in vals]
    fin = [v for v in vals if math.isfinite(v)]
    m, sabs = len(fin), math.fsum(abs(v) for v in fin)
    if any(math.isnan(v) for v in vals) or (math.inf in vals and -math.inf in vals):
        return math.nan, m, sabs
    if math.inf in vals:
        return math.inf, m, sabs
    if -math.inf in vals:
        return -math.inf, m, sabs
    return math.fsum(fin), m, sabs


def group_sorted_ref(keys, value, calls, with_terms=False):
    """calls: [name | (name, ignore_nulls)].  -> (group_rows uint32, [result per call]): int64 for count_distinct, int64
    (wrapped) or float64 (exact, rounded once) for sum_distinct, (uint32 row indices, bool valid) for first / last.
    with_terms=True appends {"m": distinct finite values per group, "sum_abs": sum of their magnitudes}."""
    cols = list(keys) + ([value] if value is not None else [])
    n = len(cols[0][0]) if cols else 0
    groups = group_rows_of(keys, n) if n else []
    G = len(groups)
    group_rows = np.array([rows[0] for _, rows in groups], dtype=np.uint32).reshape(G)
    ok = vcodes = vals = None
    is_float = False
    if value is not None:
        ok = _valid_of(value)
        vcodes = key_codes(value[0], value[1] if len(value) > 1 else None)
        if isinstance(value[0], np.ndarray):
            vals = canonical(value[0])
            is_float = vals.dtype.kind == "f"
    m_all, sabs_all = np.zeros(G, dtype=np.int64), np.zeros(G)
    outs = []
    for c in calls:
        name, ign = c if isinstance(c, tuple) else (c, 0)
        if name == "count_distinct":
            outs.append(np.array([len({int(vcodes[i]) for i in rows if ok[i]}) for _, rows in groups], dtype=np.int64).reshape(G))
        elif name == "sum_distinct":
            if vals is None:
                raise ValueError("sum_distinct of a Utf8 column")
            res = np.zeros(G, dtype=np.float64 if is_float else np.int64)
            for g, (_, rows) in enumerate(groups):
                distinct = {}
                for i in rows:
                    if ok[i]:
                        distinct.setdefault(int(vcodes[i]), vals[i])
                if is_float:
                    res[g], m_all[g], sabs_all[g] = ieee_sum([float(v) for v in distinct.values()])   # f32 -> f64 is exact
                else:
                    t = sum(int(v) for v in distinct.values()) % (1 << 64)
                    res[g] = t - (1 << 64) if t >= (1 << 63) else t
            outs.append(res)
        elif name in ("first", "last"):
            idx, valid = np.zeros(G, dtype=np.uint32), np.ones(G, dtype=bool)
            for g, (_, rows) in enumerate(groups):
                cand = [i for i in rows if ok[i]] if ign else rows
                if cand:
                    idx[g] = cand[0] if name == "first" else cand[-1]
                else:
                    valid[g] = False
            outs.append((idx, valid))
        else:
            raise ValueError(name)
    if with_terms:
        return group_rows, outs, {"m": m_all, "sum_abs": sabs_all}
    return group_rows, outs
