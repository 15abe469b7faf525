"""The executable model of rdf_member_mask and rdf_first_occurrence (include/rdf_mi355x.h, "membership"): pure Python over
canonicalised tuples.  It depends on neither the oracle nor the library.

A side is a list of rows; a row is a tuple with one component per key column: None for NULL, bytes for Utf8, bool / int for
Boolean and integer columns, float for float columns.  canon() maps a component to what the contract compares: -0.0 is
+0.0, every NaN is one NaN (Spark 3's rule for join and grouping keys); everything else compares as itself.  Results are
lists with True / False, and None for a NULL result (IS_IN only)."""
import math

SEMI, ANTI, IS_IN = "semi", "anti", "is_in"
FIRST, LAST, NONE = "first", "last", "none"

_NAN = ("nan",)     # one value for every NaN (float('nan') != float('nan') would make each its own key)


def canon(v):
    if isinstance(v, float):
        if math.isnan(v):
            return _NAN
        return 0.0 if v == 0.0 else v
    return v


def canon_row(row):
    row = row if isinstance(row, tuple) else (row,)
    return tuple(canon(v) for v in row)


def _has_null(row):
    return any(v is None for v in row)


def member_mask(left, right, kind):
    """-> one entry per left row: True / False, or None (IS_IN's NULL)."""
    left = [canon_row(r) for r in left]
    right = [canon_row(r) for r in right]
    members = {r for r in right if not _has_null(r)}
    right_null = any(_has_null(r) for r in right)
    out = []
    for r in left:
        hit = not _has_null(r) and r in members
        if kind == SEMI:
            out.append(hit)
        elif kind == ANTI:
            out.append(not hit)
        elif kind == IS_IN:
            assert len(r) == 1
            if hit:
                out.append(True)
            elif right and (r[0] is None or right_null):
                out.append(None)
            else:
                out.append(False)
        else:
            raise ValueError(kind)
    return out


def first_occurrence(keys, keep):
    """-> one bool per row.  NULL is a key value of its own, component-wise."""
    rows = [canon_row(r) for r in keys]
    first, last = {}, {}
    for i, r in enumerate(rows):
        first.setdefault(r, i)
        last[r] = i
    if keep == FIRST:
        return [first[r] == i for i, r in enumerate(rows)]
    if keep == LAST:
        return [last[r] == i for i, r in enumerate(rows)]
    if keep == NONE:
        return [first[r] == last[r] for r in rows]
    raise ValueError(keep)


def true_rows(mask):
    return sum(1 for b in mask if b is True)
