"""rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32 at the C-ABI boundary, without a GPU: every refusal of the header's
error list by status and message, in the documented order, before any device work; RDF_DEVICE_ERROR with no device;
nchunks == 0."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

INV, MEMERR, COMPUTE, DEVICE = A.RDF_INVALID_ARGUMENT, A.RDF_MEMORY_ERROR, A.RDF_COMPUTE_ERROR, A.RDF_DEVICE_ERROR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rdf_hash_columns", "rdf_utf8_digest", "rdf_utf8_crc32")


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    for n in NAMES:
        getattr(s, n).restype = C.c_int
    return s


H = A.HostUtf8.from_pylist(["ab", None, "cde"])
PLAIN = A.HostUtf8.from_pylist(["ab", "x", "cde"])
SHORT = A.HostUtf8.from_pylist(["ab", "x"])
I64COL = A.HostArray.from_numpy(np.arange(3, dtype=np.int64))
BOOLCOL = A.HostArray.from_numpy(np.array([True, False, True]))


def carr(*hs):
    return (A.rdf_utf8_array * len(hs))(*[h.c_struct() for h in hs])


def narr(*hs):
    return (A.rdf_array * len(hs))(*[h.c_struct() for h in hs])


def key(values=None, utf8=None):
    k = A.rdf_sort_key()
    if values is not None:
        k.values = C.cast(values, C.POINTER(A.rdf_array))
    if utf8 is not None:
        k.utf8 = C.cast(utf8, C.POINTER(A.rdf_utf8_array))
    k._keep = (values, utf8)
    return k


def out(n=1, dtype=A.I32, cap=3, validity=True, mem=A.MEM_HOST):
    keep, o = [], (A.rdf_out * max(1, n))()
    for i in range(n):
        vb, bb = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.uint8)
        keep.append((vb, bb))
        o[i] = A.rdf_out(vb.ctypes.data, bb.ctypes.data if validity else None, cap, -7, -7, dtype, mem)
    o._keep = keep
    return o


def douts(n=1, rows=3, validity=True, cap=0, odt=A.I32, ddt=A.U8, mem=A.MEM_HOST, ocap=None):
    keep, oo, od = [], (A.rdf_out * max(1, n))(), (A.rdf_out * max(1, n))()
    for i in range(n):
        ob, vb, db = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.uint8), np.zeros(1024, dtype=np.uint8)
        keep.append((ob, vb, db))
        oo[i] = A.rdf_out(ob.ctypes.data, vb.ctypes.data if validity else None, rows + 1 if ocap is None else ocap, -7, -7, odt, mem)
        od[i] = A.rdf_out(db.ctypes.data if cap else None, None, cap, -7, -7, ddt, mem)
    oo._keep = keep
    return oo, od


def hash_cols(so, keys, kind=0, n=1, seed=42, o=None, ncols=None):
    arr = (A.rdf_sort_key * max(1, len(keys)))(*keys)
    if o is None:
        o = out(dtype=A.I64 if kind == 1 else A.I32)
    return so.rdf_hash_columns(C.c_int32(kind), arr, C.c_int32(len(keys) if ncols is None else ncols), C.c_int64(n), C.c_int64(seed), o)


def digest(so, chunks, kind=0, n=1, o=None):
    oo, od = douts() if o is None else o
    return so.rdf_utf8_digest(C.c_int32(kind), chunks, C.c_int64(n), oo, od)


def crc(so, chunks, n=1, o=None):
    return so.rdf_utf8_crc32(chunks, C.c_int64(n), out(dtype=A.I64) if o is None else o)


def err(so):
    return so.rdf_last_error().decode()


def no_device():
    return A.RDF_OK if lib.device_count() > 0 else DEVICE


def test_names_enums_and_limits():
    for n in NAMES:
        assert n in lib.EXPORTS
    prog = r'''
#include <stdio.h>
#include "rdf_mi355x.h"
int main(void) {
  printf("%d %d %d %d %d %d %d %d %d\n", RDF_HASH_MURMUR3_32, RDF_HASH_XXHASH64, RDF_DIGEST_MD5, RDF_DIGEST_SHA1, RDF_DIGEST_SHA224, RDF_DIGEST_SHA256,
         RDF_DIGEST_SHA384, RDF_DIGEST_SHA512, RDF_HASH_COLS_MAX);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    K, D = A.HASH_KINDS, A.DIGEST_KINDS
    assert got == [K["murmur3"], K["xxhash64"], D["md5"], D["sha1"], D["sha224"], D["sha256"], D["sha384"], D["sha512"], A.HASH_COLS_MAX]
    assert K["hash"] == K["murmur3"]


def test_1_unknown_kinds_come_first(so):
    g = carr(H)
    for kind in (-1, 2, 9):
        # ... before the column count, the seed and the chunk lists
        assert hash_cols(so, [key(utf8=g)], kind=kind, ncols=0, seed=2**40) == INV and "unknown hash" in err(so)
    for kind in (-1, 6, 256):
        assert digest(so, None, kind=kind, n=-1) == INV and "unknown digest" in err(so)


def test_2_column_counts_and_columns_that_set_both_pointers_or_neither(so):
    g, v = carr(H), narr(I64COL)
    for ncols in (0, -1, 9, 100):
        assert hash_cols(so, [key(utf8=g)] * 9, ncols=ncols, seed=2**40) == INV and "1 .. 8 are taken" in err(so)
    assert so.rdf_hash_columns(C.c_int32(0), None, C.c_int32(1), C.c_int64(1), C.c_int64(42), out()) == INV and "1 .. 8 are taken" in err(so)
    # ... before the seed
    assert hash_cols(so, [key(utf8=g), key()], seed=2**40) == INV and "column 1 must set exactly one" in err(so)
    assert hash_cols(so, [key(values=v, utf8=g)]) == INV and "column 0 must set exactly one" in err(so)


def test_3_a_murmur3_seed_must_fit_int32(so):
    g = carr(H)
    bad_dtype = out(dtype=A.I64)
    for seed in (2**31, -2**31 - 1, 2**40):
        # ... before the dtypes
        assert hash_cols(so, [key(utf8=g)], seed=seed, o=bad_dtype) == INV and "does not fit the Int32" in err(so)
    for seed in (2**31 - 1, -2**31, -1, 0):
        assert hash_cols(so, [key(utf8=g)], seed=seed) == no_device()
    # XXH64 takes every Int64
    for seed in (2**40, -2**63, 2**63 - 1):
        assert hash_cols(so, [key(utf8=g)], kind=1, seed=seed) == no_device()


def test_4_dtypes_then_memory_kinds_then_validity(so):
    g = carr(H)
    # hash_columns: a column of the Null type, chunks of two dtypes, wrong Utf8 buffers, a wrong output dtype
    nullt = A.HostArray.from_numpy(np.arange(3, dtype=np.int64))
    nullt.dtype = A.NULLTYPE if hasattr(A, "NULLTYPE") else 11
    assert hash_cols(so, [key(values=narr(nullt))]) == INV and "one numeric or Boolean dtype" in err(so)
    assert hash_cols(so, [key(values=narr(I64COL, BOOLCOL))], n=2, o=out(n=2)) == INV and "one numeric or Boolean dtype" in err(so)
    assert hash_cols(so, [key(values=narr(BOOLCOL))]) == no_device()
    bad = carr(H)
    bad[0].offsets.dtype = A.I64
    assert hash_cols(so, [key(utf8=bad)]) == INV and "offsets must be an Int32 array" in err(so)
    assert hash_cols(so, [key(utf8=g)], o=out(dtype=A.I64)) == INV and "output dtype" in err(so)
    assert hash_cols(so, [key(utf8=g)], kind=1, o=out(dtype=A.I32)) == INV and "output dtype" in err(so)
    for call, wrong_out in ((lambda c, o: digest(so, c, o=o), lambda **kw: douts(odt=A.I64, **kw)),
                            (lambda c, o: crc(so, c, o=o), lambda **kw: out(dtype=A.I32, **kw))):
        bad = carr(H)
        bad[0].offsets.dtype = A.I64
        assert call(bad, None) == INV and "offsets must be an Int32 array" in err(so)
        bad = carr(H)
        bad[0].data.dtype = A.I8
        assert call(bad, None) == INV and "data must be a UInt8 array" in err(so)
        bad = carr(H)
        bad[0].offsets.length = 0
        assert call(bad, None) == INV and "rows + 1 entries" in err(so)
        assert call(g, wrong_out()) == INV
        # ... dtypes come before memory kinds
        mixed = carr(H)
        mixed[0].data.mem = A.MEM_DEVICE
        assert call(mixed, wrong_out()) == INV and "one memory space" not in err(so)
        assert call(mixed, None) == INV and "one memory space" in err(so)
        assert call(g, wrong_out(mem=A.MEM_DEVICE)) == INV and "same memory space" not in err(so)
    assert digest(so, g, o=douts(mem=A.MEM_DEVICE)) == INV and "same memory space" in err(so)
    assert crc(so, g, o=out(dtype=A.I64, mem=A.MEM_DEVICE)) == INV and "same memory space" in err(so)
    assert hash_cols(so, [key(utf8=g)], o=out(mem=A.MEM_DEVICE)) == INV and "same memory space" in err(so)
    mixed = narr(I64COL)
    mixed[0].mem = A.MEM_DEVICE
    assert hash_cols(so, [key(utf8=g), key(values=mixed)]) == INV and "one memory space" in err(so)
    # ... memory kinds come before the missing validity buffer, which comes before the capacity
    mixed = carr(H)
    mixed[0].data.mem = A.MEM_DEVICE
    assert digest(so, mixed, o=douts(validity=False)) == INV and "one memory space" in err(so)
    assert digest(so, g, o=douts(validity=False, ocap=2)) == INV and "needs a validity buffer" in err(so)
    assert crc(so, g, o=out(dtype=A.I64, validity=False, cap=1)) == INV and "needs a validity buffer" in err(so)
    two = carr(PLAIN, H)
    assert digest(so, two, n=2, o=douts(n=2, validity=False)) == INV and "output 1 needs a validity buffer" in err(so)
    assert crc(so, two, n=2, o=out(n=2, dtype=A.I64, validity=False)) == INV and "output 1 needs a validity buffer" in err(so)
    # a column without a validity bitmap needs none, and hash_columns is never NULL: only the device is missing then
    assert digest(so, carr(PLAIN), o=douts(validity=False)) in (no_device(), MEMERR)
    assert crc(so, carr(PLAIN), o=out(dtype=A.I64, validity=False)) == no_device()
    assert hash_cols(so, [key(utf8=g)], o=out(validity=False)) == no_device()


def test_5_chunk_row_counts_that_differ_between_columns(so):
    a, b = carr(PLAIN), carr(SHORT)
    o = out(cap=1)
    # ... before the capacity
    assert hash_cols(so, [key(utf8=a), key(utf8=b)], o=o) == COMPUTE and "chunk lengths differ" in err(so) and o[0].length == -7
    assert hash_cols(so, [key(values=narr(I64COL)), key(utf8=b)]) == COMPUTE and "chunk lengths differ" in err(so)
    # ... after the dtypes
    assert hash_cols(so, [key(utf8=a), key(utf8=b)], o=out(dtype=A.I64)) == INV


def test_6_capacity(so):
    g = carr(H)
    o = out(cap=2)
    assert hash_cols(so, [key(utf8=g)], o=o) == MEMERR and "below the 3 rows" in err(so) and o[0].length == 3
    o = out(dtype=A.I64, cap=0)
    assert crc(so, g, o=o) == MEMERR and "below the 3 rows" in err(so) and o[0].length == 3
    o = douts(ocap=3)
    assert digest(so, g, o=o) == MEMERR and "offsets need 4 entries" in err(so) and o[0][0].length == 4
    o = douts(ocap=0)
    assert digest(so, g, o=o) == INV and "no offsets buffer" in err(so)


def test_7_no_device_is_the_last_refusal(so):
    g = carr(H)
    for st in (hash_cols(so, [key(utf8=g), key(values=narr(I64COL))]), hash_cols(so, [key(values=narr(I64COL))], kind=1), crc(so, g)):
        assert st == no_device()
    st = digest(so, g)          # with a device: the sizing call
    assert st == (MEMERR if lib.device_count() > 0 else DEVICE)
    api = lib.api()
    for f in (lambda: api.hash_columns("hash", [[H], [I64COL]]), lambda: api.hash_columns("xxhash64", [[I64COL]]), lambda: api.utf8_crc32([H]),
              lambda: api.utf8_digest("md5", [H]), lambda: api.utf8_digest("sha512", [H])):
        if lib.device_count() == 0:
            with pytest.raises(A.RdfError) as ei:
                f()
            assert ei.value.status == DEVICE
        else:
            assert len(f()) == 1


def test_no_chunks_is_ok_and_writes_nothing(so):
    g = carr(H)
    o = out()
    assert hash_cols(so, [key(utf8=g)], n=0, o=o) == A.RDF_OK and o[0].length == -7
    o = out(dtype=A.I64)
    assert crc(so, None, n=0, o=o) == A.RDF_OK and o[0].length == -7
    o = douts()
    assert digest(so, None, n=0, o=o) == A.RDF_OK and o[0][0].length == -7 and o[1][0].length == -7
    api = lib.api()
    assert api.utf8_crc32([]) == [] and api.utf8_digest("sha1", []) == []
    # what is refused with chunks is refused without them; negative chunk counts and null lists
    assert digest(so, None, kind=7, n=0) == INV
    assert hash_cols(so, [key(utf8=g)], kind=3, n=0) == INV
    assert hash_cols(so, [key(utf8=g)], n=0, seed=2**31) == INV
    assert digest(so, g, n=-1) == INV and crc(so, g, n=-1) == INV and hash_cols(so, [key(utf8=g)], n=-1) == INV
    assert so.rdf_utf8_crc32(g, C.c_int64(1), None) == INV and "bad chunk lists" in err(so)
    assert so.rdf_utf8_digest(C.c_int32(0), g, C.c_int64(1), None, None) == INV and "bad chunk lists" in err(so)


def test_python_binding_refuses_what_the_library_refuses():
    api = lib.api()
    with pytest.raises(KeyError):
        api.utf8_digest("sha3", [H])
    with pytest.raises(KeyError):
        api.hash_columns("md5", [[H]])
    with pytest.raises(A.RdfError) as ei:
        api.hash_columns("hash", [[H]] * 9)
    assert ei.value.status == INV
    with pytest.raises(A.RdfError) as ei:
        api.hash_columns("hash", [[H]], seed=2**31)
    assert ei.value.status == INV
