"""An executable model of the twelve List entry points (rdf_list_contains .. rdf_list_repeat), written from the contract in
include/rdf_mi355x.h ("ArrayFunctions over List<primitive> columns") and the reference's src/functions/array.rs — not from the
oracle's C and not from the kernels.  numpy and plain Python only.

A list column is (off, valid, child): `off` the rows + 1 value_offsets (any monotone int array; off[0] need not be 0 and
off[-1] need not be len(child)), `valid` a bool vector of the rows or None, `child` the child values as a typed numpy
vector.  Child validity does not exist here: the entry points ignore it.

  contains / position   IEEE ==: a NaN needle matches nothing, -0.0 == 0.0.  A NULL row is NULL (contains) / 0 (position).
  max / min             by the order-preserving bit key (so max{-0.0, +0.0} is +0.0); NaN is skipped unless the row holds
                        nothing else, and then the result is some NaN; an empty or NULL row is NULL and holds 0.
  remove                elements != needle; a NULL row becomes an empty valid row, whatever slice it owns.
  sort                  every row's slice (NULL rows too) by IEEE total order on the bits; offsets do not change.
  set functions         one linear pass with a dict keyed on the value (Python's float keys already fold -0.0 into 0.0):
                        the first occurrence wins and its bits are kept; every NaN is an element of its own — kept by
                        distinct / except / union, never by intersect; b's validity is not looked at.
"""
import numpy as np

_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def bit_key(v):
    """The unsigned key whose order is the type's total order: signed integers with the sign bit flipped, floats with all
    bits flipped when the sign bit is set and the sign bit flipped otherwise (-NaN < -inf < -0.0 < +0.0 < +inf < +NaN)."""
    v = np.ascontiguousarray(v)
    u = v.view(_UINT[v.dtype.itemsize])
    top = u.dtype.type(1 << (8 * v.dtype.itemsize - 1))
    if v.dtype.kind == "f":
        return np.where(u & top != 0, ~u, u ^ top)
    return u ^ top if v.dtype.kind == "i" else u.copy()


def from_bit_key(k, dtype):
    dtype = np.dtype(dtype)
    k = np.ascontiguousarray(k, dtype=_UINT[dtype.itemsize])
    top = k.dtype.type(1 << (8 * dtype.itemsize - 1))
    if dtype.kind == "f":
        return np.where(k & top != 0, k ^ top, ~k).view(dtype)
    return (k ^ top if dtype.kind == "i" else k).view(dtype)


def _rows(off, valid):
    for i in range(len(off) - 1):
        yield i, int(off[i]), int(off[i + 1]), (valid is None or bool(valid[i]))


def _scalar(child, needle):
    """The needle as one element of the child's dtype, bits kept when it already is one."""
    return np.asarray([needle]).astype(child.dtype)[0] if not isinstance(needle, np.generic) or needle.dtype != child.dtype else needle


def find(off, valid, child, needle):
    """-> (contains values [bool], contains validity [bool], position [int32])"""
    n = len(off) - 1
    with np.errstate(invalid="ignore"):
        eq = child == _scalar(child, needle)
    has, ok, pos = np.zeros(n, bool), np.ones(n, bool), np.zeros(n, np.int32)
    for i, b, e, v in _rows(off, valid):
        ok[i] = v
        hit = np.flatnonzero(eq[b:e]) if v else ()
        if len(hit):
            has[i], pos[i] = True, hit[0] + 1
    return has, ok, pos


def extreme(off, valid, child, want_max):
    """-> (values, validity, rows whose result is "some NaN")"""
    n = len(off) - 1
    out, ok, nan_only = np.zeros(n, child.dtype), np.zeros(n, bool), np.zeros(n, bool)
    isnan = np.isnan(child) if child.dtype.kind == "f" else np.zeros(len(child), bool)
    key = bit_key(child)
    for i, b, e, v in _rows(off, valid):
        if not v or e == b:
            continue
        ok[i] = True
        k = key[b:e][~isnan[b:e]]
        if len(k) == 0:
            nan_only[i], out[i] = True, np.nan
        else:
            out[i] = from_bit_key(np.array([k.max() if want_max else k.min()]), child.dtype)[0]
    return out, ok, nan_only


def _assemble(n, pieces, dtype):
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in pieces])
    vals = np.concatenate(pieces).astype(dtype, copy=False) if pieces and off[-1] else np.zeros(0, dtype)
    return off, vals


def remove(off, valid, child, needle):
    """-> (offsets [int64, starting at 0], values)"""
    with np.errstate(invalid="ignore"):
        keep = child != _scalar(child, needle)
    pieces = [child[b:e][keep[b:e]] if v else child[:0] for _, b, e, v in _rows(off, valid)]
    return _assemble(len(off) - 1, pieces, child.dtype)


def sort(off, valid, child):
    """-> child[off[0] : off[-1]] with every row's slice sorted (validity is not looked at)."""
    out = child[int(off[0]):int(off[-1])].copy()
    for _, b, e, _v in _rows(off, None):
        out[b - int(off[0]):e - int(off[0])] = from_bit_key(np.sort(bit_key(child[b:e])), child.dtype)
    return out


def _take(a, idx):
    return a[np.asarray(idx, dtype=np.intp)]


def _first_occurrences(items, seen):
    """Indices of the elements of `items` (Python numbers) not met before; `seen` is updated.  A NaN is never "met"."""
    keep = []
    for i, x in enumerate(items):
        if x != x:
            keep.append(i)
        elif x not in seen:
            seen[x] = i
            keep.append(i)
    return keep


def set_op(op, off, valid, child, off_b=None, child_b=None, count=0):
    """op: distinct / except / intersect / union / repeat -> (offsets [int64, starting at 0], values)"""
    pieces = []
    for i, b, e, v in _rows(off, valid):
        a = child[b:e]
        if not v:
            pieces.append(child[:0])
            continue
        if op == "repeat":
            pieces.append(np.tile(a, count))
            continue
        seen = {}
        ka = _first_occurrences(a.tolist(), seen)
        if op == "distinct":
            pieces.append(_take(a, ka))
            continue
        sb = child_b[int(off_b[i]):int(off_b[i + 1])]
        lb = sb.tolist()
        if op == "union":
            pieces.append(np.concatenate([_take(a, ka), _take(sb, _first_occurrences(lb, seen))]))
            continue
        members = {x for x in lb if x == x}
        la = a.tolist()
        if op == "except":
            pieces.append(_take(a, [j for j in ka if la[j] != la[j] or la[j] not in members]))
        else:
            pieces.append(_take(a, [j for j in ka if la[j] == la[j] and la[j] in members]))
    return _assemble(len(off) - 1, pieces, child.dtype)
