"""A pure-Python reference for text keys: dictionary encoding, GROUP BY and equi-join over columns whose values are
python objects (str / bytes / int, None = NULL).  Dicts keep first-occurrence order, which is the order the codes follow."""
from collections import Counter


def factorize(chunks):
    """chunks: lists of (value | None) -> (codes per chunk with None for NULL, dictionary in first-occurrence order over
    the concatenation of the chunks)."""
    seen = {}
    codes = []
    for chunk in chunks:
        out = []
        for v in chunk:
            if v is None:
                out.append(None)
                continue
            if v not in seen:
                seen[v] = len(seen)
            out.append(seen[v])
        codes.append(out)
    return codes, list(seen)


def groupby(keys, values, agg):
    """keys: list of columns (flat lists, None = NULL), values: flat list or None, agg: sum / min / max / count.
    SQL semantics: a NULL key is a group value of its own, NULL values are skipped; count = non-NULL values of the group (rows
    when values is None or agg == "count").  -> {key tuple: (value, count)}; value is None for min / max of a group without
    a non-NULL value, 0 for its sum; for "count" (or values None) value == count."""
    n = len(keys[0])
    assert all(len(k) == n for k in keys)
    rows_only = values is None or agg == "count"
    groups = {}
    for i in range(n):
        groups.setdefault(tuple(k[i] for k in keys), []).append(None if rows_only else values[i])
    out = {}
    for key, vals in groups.items():
        if rows_only:
            out[key] = (len(vals), len(vals))
            continue
        live = [v for v in vals if v is not None]
        if agg == "sum":
            val = sum(live) if live else 0
        elif agg == "min":
            val = min(live) if live else None
        elif agg == "max":
            val = max(live) if live else None
        else:
            raise ValueError(agg)
        out[key] = (val, len(live))
    return out


def equijoin(left, right, how):
    """left / right: lists of columns (flat lists); a row's key is the tuple over the columns, and a key with a None in it
    never matches.  how: left / right / inner / full.  -> Counter of (left row | None, right row | None) pairs."""
    nl, nr = len(left[0]), len(right[0])
    lkeys = [tuple(c[i] for c in left) for i in range(nl)]
    rkeys = [tuple(c[i] for c in right) for i in range(nr)]
    index = {}
    for j, k in enumerate(rkeys):
        if None not in k:
            index.setdefault(k, []).append(j)
    pairs = Counter()
    matched_right = set()
    for i, k in enumerate(lkeys):
        partners = index.get(k, []) if None not in k else []
        for j in partners:
            pairs[(i, j)] += 1
            matched_right.add(j)
        if not partners and how in ("left", "full"):
            pairs[(i, None)] += 1
    if how in ("right", "full"):
        for j in range(nr):
            if j not in matched_right:
                pairs[(None, j)] += 1
    return pairs


def ordered_pairs(left, right, how):
    """The documented order of the results.  INNER / LEFT / FULL probe with the left rows, RIGHT with the right rows: probe
    rows ascending, every probe row's partners ascending (an outer join's probe row without a partner once, with None),
    then for FULL the unmatched build (right) rows — in unspecified order, listed ascending here: see full_probe_rows."""
    assert how in ("inner", "left", "right", "full")
    probe, build = (right, left) if how == "right" else (left, right)
    np_, nb = len(probe[0]), len(build[0])
    index = {}
    for j in range(nb):
        k = tuple(c[j] for c in build)
        if None not in k:
            index.setdefault(k, []).append(j)
    out = []
    matched = set()
    for i in range(np_):
        k = tuple(c[i] for c in probe)
        partners = index.get(k, []) if None not in k else []
        out.extend((i, j) for j in partners)
        matched.update(partners)
        if not partners and how != "inner":
            out.append((i, None))
    if how == "right":
        return [(b, p) for p, b in out]
    if how == "full":
        out.extend((None, j) for j in range(nb) if j not in matched)
    return out


def full_probe_rows(left, right):
    """Rows of a FULL join's result that come from its probe pass (their order is fixed; the rest is a set)."""
    return len(ordered_pairs(left, right, "left"))


def assert_ordered(pairs, left, right, how):
    """pairs == the documented order; the unmatched build rows behind a FULL join's probe pass compare as a set."""
    exp = ordered_pairs(left, right, how)
    assert len(pairs) == len(exp), (len(pairs), len(exp))
    n = full_probe_rows(left, right) if how == "full" else len(exp)
    assert pairs[:n] == exp[:n], next((i, pairs[i], exp[i]) for i in range(n) if pairs[i] != exp[i])
    assert sorted(pairs[n:], key=lambda p: p[1]) == exp[n:]
