"""An exact numpy model of rdf_sort_to_indices, written from the contract in include/rdf_mi355x.h — not from the kernels and
not from the oracle:

  * column 0 is the most significant criterion;
  * rows that agree on every criterion keep ascending row order, under `descending` too (the sort is stable);
  * NULL rows sort last whatever the direction;
  * floats sort in IEEE total order: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN;
  * unsigned types compare as unsigned.

Input: one list of chunks per column.  A chunk is anything with the fields of an Arrow array slice: `values` (a typed numpy
vector that includes `offset` leading elements), `validity` (an LSB-first uint8 bitmap that includes `offset` leading bits, or
None), `offset`, `length`.  Output: one uint32 array of row numbers over the concatenation of the chunks.

Every value becomes one uint64 "order word" whose unsigned order is the column's order; one np.lexsort over (row number,
word and NULL flag of every column, the last column first) is the whole sort."""
import numpy as np

_TOP = np.uint64(1) << np.uint64(63)


def chunk_values(chunk):
    return np.asarray(chunk.values)[chunk.offset:chunk.offset + chunk.length]


def chunk_valid(chunk):
    if chunk.validity is None:
        return np.ones(chunk.length, dtype=bool)
    bits = np.unpackbits(np.asarray(chunk.validity, dtype=np.uint8), bitorder="little")
    return bits[chunk.offset:chunk.offset + chunk.length].astype(bool)


def order_words(values):
    """uint64 words whose unsigned order is the ascending order of `values` (their dtype decides how)."""
    v = np.ascontiguousarray(values)
    kind, size = v.dtype.kind, v.dtype.itemsize
    if kind == "u":
        return v.astype(np.uint64)
    if kind == "i":
        return v.astype(np.int64).view(np.uint64) ^ _TOP           # two's complement: flip the sign bit
    if kind == "f":
        bits = v.view(np.uint32 if size == 4 else np.uint64).astype(np.uint64)
        sign = np.uint64(1) << np.uint64(8 * size - 1)
        ones = (sign << np.uint64(1)) - np.uint64(1) if size == 4 else ~np.uint64(0)
        neg = (bits & sign) != 0
        # sign-magnitude to ordered: negatives reverse (all bits flipped), the others move above them (sign bit set)
        return np.where(neg, bits ^ ones, bits | sign)
    raise TypeError(f"sort_ref: no order for dtype {v.dtype}")


def sort_to_indices(cols, descending):
    """cols[k] = the chunks of criterion k; descending[k] = its direction.  -> uint32 row numbers."""
    assert len(cols) >= 1 and len(cols) == len(descending)
    keys = []
    n = None
    for chunks, desc in zip(cols, descending):
        words = np.concatenate([order_words(chunk_values(c)) for c in chunks]) if chunks else np.zeros(0, np.uint64)
        valid = np.concatenate([chunk_valid(c) for c in chunks]) if chunks else np.zeros(0, bool)
        assert n is None or len(words) == n, "columns differ in length"
        n = len(words)
        if desc:
            words = ~words
        words = np.where(valid, words, np.uint64(0))                # a NULL row's value takes no part in the order
        keys.append((words, (~valid).astype(np.uint8)))
    lex = [np.arange(n, dtype=np.uint64)]                           # least significant: the row number
    for words, isnull in reversed(keys):
        lex.append(words)
        lex.append(isnull)                                          # NULLs last: above every word of the column
    return np.lexsort(lex).astype(np.uint32)
