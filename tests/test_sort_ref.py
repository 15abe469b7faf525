"""tests/sort_ref.py, the numpy model the GPU sort is held to (test_sort_routes_gpu.py), held itself to two independent
answers on a few hundred rows of every dtype with specials, NULLs, ties, chunks, offsets, several criteria and both
directions: a plain Python `sorted` under an explicit comparator (floats ordered by the sign and magnitude fields of their bit
patterns, read with `struct`), and the CPU oracle."""
import functools
import struct

import numpy as np
import pytest

import sort_ref as R
from rust_dataframe_amd import _abi as A

DTYPES = [A.I8, A.I16, A.I32, A.I64, A.U8, A.U16, A.U32, A.U64, A.F32, A.F64]


def draw(rng, dt, n):
    """Values with ties, both ends of the type's range, and for floats every special of the total order."""
    npdt = np.dtype(A.NP_OF[dt])
    if n == 0:
        return np.zeros(0, dtype=npdt)
    if npdt.kind == "f":
        v = rng.normal(size=n).astype(npdt)
        tiny = np.finfo(npdt).smallest_subnormal
        sp = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, np.finfo(npdt).max, np.finfo(npdt).min, 1.5, 1.5, -1.5], dtype=npdt)
        at = rng.integers(0, n, n // 3)
        v[at] = sp[rng.integers(0, len(sp), len(at))]
        bits = v.view(np.uint32 if npdt.itemsize == 4 else np.uint64)
        nan = np.array([np.nan], dtype=npdt).view(bits.dtype)[0]
        sign = bits.dtype.type(1) << bits.dtype.type(8 * npdt.itemsize - 1)
        for j, pat in enumerate([nan, nan | sign, nan | bits.dtype.type(1), nan | sign | bits.dtype.type(5)]):   # NaNs of both signs, two payloads
            bits[rng.integers(0, n, 4)] = pat
        return v
    info = np.iinfo(npdt)
    v = rng.integers(info.min, info.max, n, dtype=npdt, endpoint=True)
    at = rng.integers(0, n, n // 3)
    sp = np.array([info.min, info.max, 0, 1, info.max // 2, info.max // 2 + 1], dtype=npdt)
    v[at] = sp[rng.integers(0, len(sp), len(at))]
    return v


def column(rng, dt, lens, null_fraction, offsets):
    out = []
    for m, off in zip(lens, offsets):
        valid = rng.uniform(size=m) >= null_fraction if null_fraction else None
        out.append(A.HostArray.from_numpy(draw(rng, dt, m), valid=valid, offset=off, dtype=dt, rng=rng))
    return out


def field_order(x):
    """-1 / 0 / 1 position key of a float in IEEE total order from its fields: (sign, magnitude) read with struct."""
    raw = x.tobytes()
    bits = struct.unpack("<I" if len(raw) == 4 else "<Q", raw)[0]
    width = 8 * len(raw)
    negative = bits >> (width - 1)
    magnitude = bits & ((1 << (width - 1)) - 1)
    return (0, -magnitude) if negative else (1, magnitude)


def python_sorted(cols, descending):
    """sorted() under a comparator that says the contract in so many words."""
    rows = []
    for chunks in cols:
        vals, valid = [], []
        for c in chunks:
            v = R.chunk_values(c)
            vals.extend(field_order(x) if v.dtype.kind == "f" else int(x) for x in v)
            valid.extend(bool(b) for b in R.chunk_valid(c))
        rows.append((vals, valid))
    n = len(rows[0][0])

    def cmp(i, j):
        for (vals, valid), desc in zip(rows, descending):
            if valid[i] != valid[j]:
                return -1 if valid[i] else 1            # NULLs last, whatever the direction
            if not valid[i]:
                continue                                # NULL agrees with NULL
            if vals[i] != vals[j]:
                less = vals[i] < vals[j]
                return -1 if less != bool(desc) else 1
        return -1 if i < j else (1 if i > j else 0)     # ties keep ascending row order

    return np.array(sorted(range(n), key=functools.cmp_to_key(cmp)), dtype=np.uint32)


CASES = [([257], [0]), ([100, 0, 1, 156], [3, 0, 7, 64])]


@pytest.mark.parametrize("dt", DTYPES)
def test_model_against_python_sorted_and_oracle(ora, dt):
    rng = np.random.default_rng(500 + dt)
    for lens, offs in CASES:
        for nf in (0.0, 0.15):
            col = column(rng, dt, lens, nf, offs)
            ties = column(rng, A.I8, lens, 0.1, offs[::-1])
            for t in ties:
                t.values[:] = t.values % 3
            for cols, desc in [([col], [False]), ([col], [True]), ([ties, col], [True, False]), ([ties, col], [False, True]), ([col, ties], [True, True])]:
                got = R.sort_to_indices(cols, desc)
                assert got.dtype == np.uint32 and np.array_equal(np.sort(got), np.arange(sum(lens), dtype=np.uint32))
                assert np.array_equal(got, python_sorted(cols, desc)), (dt, lens, nf, desc, "python sorted")
                assert np.array_equal(got, ora.sort_to_indices(cols, desc).to_numpy()), (dt, lens, nf, desc, "oracle")


def test_model_total_order_of_floats_spelled_out():
    nan = np.float64(np.nan)
    neg_nan = np.array([np.uint64(0xFFF8000000000000)]).view(np.float64)[0]
    v = np.array([nan, np.inf, 1.0, 5e-324, 0.0, -0.0, -5e-324, -1.0, -np.inf, neg_nan], dtype=np.float64)
    col = [A.HostArray.from_numpy(v, dtype=A.F64)]
    assert R.sort_to_indices([col], [False]).tolist() == list(range(9, -1, -1))
    assert R.sort_to_indices([col], [True]).tolist() == list(range(10))
    f = [A.HostArray.from_numpy(v.astype(np.float32), dtype=A.F32)]
    f[0].values.view(np.uint32)[[3, 6, 9]] = [0x00000001, 0x80000001, 0xFFC00000]    # the 4-byte denormals and -NaN
    assert R.sort_to_indices([f], [False]).tolist() == list(range(9, -1, -1))
    u = [A.HostArray.from_numpy(np.array([2 ** 63, 1, 2 ** 64 - 1, 0], dtype=np.uint64), valid=[True, True, True, False], dtype=A.U64)]
    assert R.sort_to_indices([u], [False]).tolist() == [1, 0, 2, 3]
    assert R.sort_to_indices([u], [True]).tolist() == [2, 0, 1, 3]
    all_null = [A.HostArray.from_numpy(np.arange(5, dtype=np.int32)[::-1].copy(), valid=[False] * 5, dtype=A.I32)]
    assert R.sort_to_indices([all_null], [True]).tolist() == [0, 1, 2, 3, 4]
