"""CPU restatement of rdf_window's semantics (include/rdf_mi355x.h, "window functions") in plain numpy.

A key is (values, valid[, descending]): `values` a numpy array (numeric) or a sequence of bytes objects (Utf8; None = NULL),
`valid` a bool array or None.  Every key is first turned into dense codes — equal values get equal codes, smaller values
smaller codes, floats canonical (-0.0 == +0.0, one NaN after +inf), NULL the largest code in either direction — the rows
are ordered by one stable np.lexsort over the codes, and every quantity of the header's formulas (k, n, f, l, d) is then
computed with cumulative sums and maxima over that order.  Like the device path it finds partition and peer-group starts by
comparing each sorted row with its predecessor — there is no other way to read them off a sorted order — but it shares no
code with it: the comparison runs over dense codes from np.unique / sorted(), not over key bits, and the order comes from
numpy's sort.  tests/test_window_ref.py holds it to pandas, which does neither.
"""
import numpy as np

FNS = ("row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile", "lag", "lead")


def canonical(values):
    """Float arrays with -0.0 -> +0.0 and every NaN -> the quiet NaN; everything else unchanged."""
    v = np.asarray(values)
    if v.dtype.kind != "f":
        return v
    v = v.copy()
    v[v == 0] = 0.0
    v[np.isnan(v)] = np.nan
    return v


def key_codes(values, valid=None, descending=False):
    """-> int64 codes: the rank of each row's value among the distinct values (ascending, or descending), NULLs last."""
    if isinstance(values, np.ndarray) and values.dtype.kind in "iuf":
        v = canonical(values)
        n = len(v)
        ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool).copy()
        codes = np.zeros(n, dtype=np.int64)
        if v.dtype.kind == "f":
            nan = np.isnan(v) & ok
            fin = ok & ~nan
            uniq, inv = np.unique(v[fin], return_inverse=True)
            codes[fin] = inv
            codes[nan] = len(uniq)                      # after +inf
            ncodes = len(uniq) + (1 if nan.any() else 0)
        else:
            uniq, inv = np.unique(v[ok], return_inverse=True)
            codes[ok] = inv
            ncodes = len(uniq)
    else:
        rows = list(values)
        n = len(rows)
        ok = np.array([r is not None for r in rows], dtype=bool)
        if valid is not None:
            ok &= np.asarray(valid, dtype=bool)
        uniq = sorted({bytes(rows[i]) for i in range(n) if ok[i]})      # bytes compare as unsigned bytes, a prefix first
        where = {b: i for i, b in enumerate(uniq)}
        codes = np.array([where[bytes(rows[i])] if ok[i] else 0 for i in range(n)], dtype=np.int64).reshape(n)
        ncodes = len(uniq)
    if descending:
        codes[ok] = ncodes - 1 - codes[ok]
    codes[~ok] = ncodes                                  # NULLs last in both directions, and peers of each other
    return codes


def _split(key, want_desc):
    values, valid = key[0], key[1] if len(key) > 1 else None
    desc = bool(key[2]) if (want_desc and len(key) > 2) else False
    return values, valid, desc


def window_ref(partition_by, order_by, calls, nrows=None):
    """calls: [name | (name, param)].  -> one array per call in the original row order: int64 for row_number / rank /
    dense_rank / ntile, float64 for percent_rank / cume_dist, (uint32 row indices, bool valid) for lag / lead."""
    pcodes = [key_codes(*_split(k, False)) for k in partition_by]
    ocodes = [key_codes(*_split(k, True)) for k in order_by]
    allc = pcodes + ocodes
    n = len(allc[0]) if allc else int(nrows)
    order = np.lexsort(tuple(reversed(allc))) if allc else np.arange(n)      # stable; the last key given is the primary one
    order = order.astype(np.int64)
    outs = []
    if n == 0:
        for c in calls:
            name = c[0] if isinstance(c, tuple) else c
            if name in ("lag", "lead"):
                outs.append((np.zeros(0, np.uint32), np.zeros(0, bool)))
            else:
                outs.append(np.zeros(0, np.float64 if name in ("percent_rank", "cume_dist") else np.int64))
        return outs
    pos = np.arange(n, dtype=np.int64)
    P = np.zeros(n, dtype=bool)
    P[0] = True
    for c in pcodes:
        s = c[order]
        P[1:] |= s[1:] != s[:-1]
    G = P.copy()
    for c in ocodes:
        s = c[order]
        G[1:] |= s[1:] != s[:-1]
    ps = np.maximum.accumulate(np.where(P, pos, 0))          # first position of my partition
    pid = np.cumsum(P) - 1
    nn = np.bincount(pid)[pid]                               # rows of my partition
    k = pos - ps
    gs = np.maximum.accumulate(np.where(G, pos, 0))          # first position of my peer group
    gid = np.cumsum(G) - 1
    f = gs - ps
    l = f + np.bincount(gid)[gid] - 1
    d = gid - gid[ps]

    def scatter(sorted_vals, dtype):
        out = np.zeros(n, dtype=dtype)
        out[order] = sorted_vals
        return out

    for c in calls:
        name, param = c if isinstance(c, tuple) else (c, 0)
        param = int(param)
        if name == "row_number":
            outs.append(scatter(k + 1, np.int64))
        elif name == "rank":
            outs.append(scatter(f + 1, np.int64))
        elif name == "dense_rank":
            outs.append(scatter(d + 1, np.int64))
        elif name == "percent_rank":
            den = np.maximum(nn - 1, 1).astype(np.float64)
            outs.append(scatter(np.where(nn == 1, 0.0, f.astype(np.float64) / den), np.float64))
        elif name == "cume_dist":
            outs.append(scatter((l + 1).astype(np.float64) / nn.astype(np.float64), np.float64))
        elif name == "ntile":
            assert param >= 1
            q, r = nn // param, nn % param
            big = r * (q + 1)                                # rows in the r buckets that hold q + 1
            t = np.where(k < big, k // (q + 1) + 1, r + (k - big) // np.maximum(q, 1) + 1)   # (q == 0: every row is below `big`)
            outs.append(scatter(t, np.int64))
        elif name in ("lag", "lead"):
            assert param >= 0
            ok = (k >= param) if name == "lag" else (param < nn - k)
            src = np.where(ok, pos - param if name == "lag" else pos + param, 0)
            outs.append((scatter(np.where(ok, order[src], 0), np.uint32), scatter(ok, bool)))
        else:
            raise ValueError(name)
    return outs


def gather(values, idx, valid):
    """rdf_take / rdf_utf8_take through a lag / lead result: values[idx] where valid, else None."""
    return [values[int(i)] if v else None for i, v in zip(idx, valid)]


def total_order_argsort(x, descending=False):
    """rdf_sort_to_indices on one non-NULL float column: IEEE total order over the bit patterns (-NaN < -inf < ... < -0.0 <
    +0.0 < ... < +inf < +NaN), stable."""
    x = np.asarray(x)
    u = x.view(np.uint64 if x.dtype == np.float64 else np.uint32)
    top = u.dtype.type(1) << u.dtype.type(8 * u.dtype.itemsize - 1)
    key = np.where(u & top, ~u, u ^ top)
    if descending:
        key = ~key
    return np.argsort(key, kind="stable").astype(np.int64)
