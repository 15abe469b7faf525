"""CPU restatement of rdf_groupby_collect's and rdf_list_explode's semantics (include/rdf_mi355x.h, "collect per group and
explode") in numpy / plain Python.

A column is (values, valid) as in group_sorted_ref: `values` a numpy array (numeric) or a sequence of bytes objects (Utf8;
None = NULL), `valid` a bool array or None.  Keys and value are turned into window_ref.key_codes (equal values equal codes,
floats canonical, NULL the largest code); ONE stable np.lexsort over (key codes..., [value code,] row) gives the header's
group order, and inside a group the row order (list) or the value order with the smallest row first (set).  Nothing here is
derived from the library: no head list, no tiles, no scans.
"""
import numpy as np

from group_sorted_ref import _valid_of
from window_ref import canonical, key_codes

KINDS = ("list", "set")


def collect_ref(keys, value, kind):
    """-> (group_rows uint32 [G], offsets int32 [G + 1], child_rows uint32 [E], values | None): `values` has the value
    column's dtype (None for Utf8); canonical floats for "set", the rows' own bits for "list".  Zero rows: four empty arrays
    (offsets too: the call writes nothing)."""
    assert kind in KINDS
    n = len(value[0])
    numeric = isinstance(value[0], np.ndarray)
    empty_vals = value[0][:0].copy() if numeric else None
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.uint32), empty_vals
    kcodes = [key_codes(k[0], k[1] if len(k) > 1 else None) for k in keys]
    ok = _valid_of(value)
    vcodes = key_codes(value[0], value[1] if len(value) > 1 else None) if kind == "set" else None
    rows = np.arange(n)
    # np.lexsort: the LAST key is the most significant, and the sort is stable
    minor = [rows] + ([vcodes] if kind == "set" else [])
    order = np.lexsort(tuple(minor + kcodes[::-1]))
    if kcodes:
        kmat = np.stack([c[order] for c in kcodes], axis=1)
        new_group = np.ones(n, dtype=bool)
        new_group[1:] = (kmat[1:] != kmat[:-1]).any(axis=1)
    else:
        new_group = np.zeros(n, dtype=bool)
        new_group[0] = True
    gid = np.cumsum(new_group) - 1                       # group of every sorted position
    G = int(gid[-1]) + 1
    group_rows = np.minimum.reduceat(order, np.flatnonzero(new_group)).astype(np.uint32)   # the group's first row in row order
    keep = ok[order].copy()                              # NULL values are never collected
    if kind == "set":
        first_of_value = np.ones(n, dtype=bool)
        first_of_value[1:] = new_group[1:] | (vcodes[order][1:] != vcodes[order][:-1])
        keep &= first_of_value                           # ties keep ascending rows: the first is the smallest row
    child = order[keep].astype(np.uint32)
    counts = np.bincount(gid[keep], minlength=G)
    offsets = np.zeros(G + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(counts)
    vals = None
    if numeric:
        src = canonical(value[0]) if kind == "set" else value[0]
        vals = src[child]
    return group_rows, offsets, child, vals


def explode_ref(offsets, valid=None, outer=False):
    """offsets: the rows + 1 value_offsets of the list rows (any start), valid: bool per list row or None.
    -> (parent_rows uint32, child_index uint32, pos int32, element_valid bool): one row per element of every non-NULL list,
    and with outer one row (element_valid False, child_index = pos = 0) for every NULL or empty list."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    parent, child, pos, ev = [], [], [], []
    for r in range(n):
        live = valid is None or bool(valid[r])
        ln = int(offsets[r + 1] - offsets[r]) if live else 0
        if ln > 0:
            for k in range(ln):
                parent.append(r); child.append(int(offsets[r]) + k); pos.append(k); ev.append(True)
        elif outer:
            parent.append(r); child.append(0); pos.append(0); ev.append(False)
    return (np.array(parent, dtype=np.uint32), np.array(child, dtype=np.uint32), np.array(pos, dtype=np.int32),
            np.array(ev, dtype=bool))
