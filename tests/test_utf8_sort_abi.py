"""rdf_lexsort_to_indices at the C-ABI boundary, without a GPU: the rdf_sort_key layout, every argument error before any
device work, and RDF_DEVICE_ERROR for a valid call with no device."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    lib.api()
    s.rdf_lexsort_to_indices.restype = C.c_int
    s.rdf_last_error.restype = C.c_char_p
    return s


def test_sort_key_struct_matches_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rdf_mi355x.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(rdf_sort_key), offsetof(rdf_sort_key, values), offsetof(rdf_sort_key, utf8),
         offsetof(rdf_sort_key, options));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        size, o_values, o_utf8, o_opts = map(int, subprocess.check_output([exe], text=True).split())
    assert size == C.sizeof(A.rdf_sort_key)
    assert o_values == A.rdf_sort_key.values.offset
    assert o_utf8 == A.rdf_sort_key.utf8.offset
    assert o_opts == A.rdf_sort_key.options.offset


class _Keys:
    """Builds rdf_sort_key arrays over host buffers it keeps alive."""

    def __init__(self):
        self.keep = []

    def utf8(self, chunks, desc=0):
        arr = (A.rdf_utf8_array * len(chunks))(*[c.c_struct() for c in chunks])
        self.keep.append(arr)
        return A.rdf_sort_key(None, C.cast(arr, C.POINTER(A.rdf_utf8_array)), A.rdf_sort_options(desc, 0))

    def num(self, chunks, desc=0):
        arr = (A.rdf_array * len(chunks))(*[c.c_struct() for c in chunks])
        self.keep.append(arr)
        return A.rdf_sort_key(C.cast(arr, C.POINTER(A.rdf_array)), None, A.rdf_sort_options(desc, 0))

    def both(self, u, v):
        k = self.utf8(u)
        k.values = self.num(v).values
        return k

    def array(self, *keys):
        arr = (A.rdf_sort_key * max(1, len(keys)))(*keys)
        self.keep.append(arr)
        return arr


def _out(cap, mem=A.MEM_HOST, dtype=A.U32):
    buf = np.zeros(max(cap, 1), dtype=np.uint32)
    return (A.rdf_out * 1)(A.rdf_out(buf.ctypes.data, None, cap, 0, 0, dtype, mem)), buf


def _call(so, keys, nkeys, nchunks, out):
    return so.rdf_lexsort_to_indices(keys, C.c_int32(nkeys), C.c_int64(nchunks), out)


def test_argument_errors_come_before_the_device(so):
    K = _Keys()
    s3 = A.HostUtf8.from_pylist(["b", None, "a"])
    s2 = A.HostUtf8.from_pylist(["b", "a"])
    f3 = A.HostArray.from_numpy(np.array([1.0, 2.0, 3.0]))
    i3 = A.HostArray.from_numpy(np.array([1, 2, 3], dtype=np.int32))
    out, _b = _out(3)
    # no keys
    assert _call(so, None, 0, 1, out) == A.RDF_COMPUTE_ERROR
    assert b"Sort criteria cannot be empty" in so.rdf_last_error()
    assert _call(so, K.array(K.utf8([s3])), 0, 1, out) == A.RDF_COMPUTE_ERROR
    # a key with both pointers or neither
    assert _call(so, K.array(K.both([s3], [f3])), 1, 1, out) == A.RDF_INVALID_ARGUMENT
    assert _call(so, K.array(A.rdf_sort_key(None, None, A.rdf_sort_options(0, 0))), 1, 1, out) == A.RDF_INVALID_ARGUMENT
    # no chunks / no output
    assert _call(so, K.array(K.utf8([s3])), 1, 0, out) == A.RDF_INVALID_ARGUMENT
    assert _call(so, K.array(K.utf8([s3])), 1, 1, None) == A.RDF_INVALID_ARGUMENT
    # wrong dtypes: Utf8 offsets not Int32, data not UInt8, numeric chunks of two dtypes, non-numeric values, output not UInt32
    bad = K.utf8([s3])
    bad.utf8[0].offsets.dtype = A.I64
    assert _call(so, K.array(bad), 1, 1, out) == A.RDF_INVALID_ARGUMENT
    bad = K.utf8([s3])
    bad.utf8[0].data.dtype = A.I8
    assert _call(so, K.array(bad), 1, 1, out) == A.RDF_INVALID_ARGUMENT
    assert _call(so, K.array(K.num([f3, i3])), 1, 2, _out(6)[0]) == A.RDF_INVALID_ARGUMENT
    bad = K.num([f3])
    bad.values[0].dtype = A.BOOL
    assert _call(so, K.array(bad), 1, 1, out) == A.RDF_INVALID_ARGUMENT
    assert _call(so, K.array(K.utf8([s3])), 1, 1, _out(3, dtype=A.I32)[0]) == A.RDF_INVALID_ARGUMENT
    # mixed memory kinds: between keys, inside a Utf8 chunk, between the inputs and the output
    dev = K.num([f3])
    dev.values[0].mem = A.MEM_DEVICE
    assert _call(so, K.array(K.utf8([s3]), dev), 2, 1, out) == A.RDF_INVALID_ARGUMENT
    bad = K.utf8([s3])
    bad.utf8[0].data.mem = A.MEM_DEVICE
    assert _call(so, K.array(bad), 1, 1, out) == A.RDF_INVALID_ARGUMENT
    assert _call(so, K.array(K.utf8([s3])), 1, 1, _out(3, mem=A.MEM_DEVICE)[0]) == A.RDF_INVALID_ARGUMENT
    # chunk row counts that differ between keys
    assert _call(so, K.array(K.utf8([s2]), K.num([f3])), 2, 1, out) == A.RDF_COMPUTE_ERROR
    assert _call(so, K.array(K.num([f3]), K.utf8([s2])), 2, 1, out) == A.RDF_COMPUTE_ERROR
    # 2^32 rows or more (the lengths alone say so; nothing is read)
    big = K.utf8([s3])
    big.utf8[0].offsets.length = (1 << 32) + 1
    assert _call(so, K.array(big), 1, 1, out) == A.RDF_INVALID_ARGUMENT
    # output capacity too small
    assert _call(so, K.array(K.utf8([s3])), 1, 1, _out(2)[0]) == A.RDF_MEMORY_ERROR
    assert _call(so, K.array(K.utf8([s3]), K.num([f3], 1)), 2, 1, _out(2)[0]) == A.RDF_MEMORY_ERROR


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error(so):
    K = _Keys()
    s3 = A.HostUtf8.from_pylist(["b", None, "a"])
    f3 = A.HostArray.from_numpy(np.array([1.0, 2.0, 3.0]))
    out, _b = _out(3)
    assert _call(so, K.array(K.utf8([s3])), 1, 1, out) == A.RDF_DEVICE_ERROR
    assert _call(so, K.array(K.utf8([s3], 1), K.num([f3])), 2, 1, out) == A.RDF_DEVICE_ERROR
    assert _call(so, K.array(K.num([f3])), 1, 1, out) == A.RDF_DEVICE_ERROR
    with pytest.raises(A.RdfError) as ei:
        lib.api().lexsort_to_indices([([s3], True), ([f3], False)])
    assert ei.value.status == A.RDF_DEVICE_ERROR
