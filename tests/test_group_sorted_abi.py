"""rdf_groupby_sorted at the C-ABI boundary, without a GPU: the symbol is exported, the mirrors match the header (checked by
a compiled C snippet), every argument error is a value returned before any device work with nothing written, zero rows is
a valid call, and with no device a valid call fails loudly with RDF_DEVICE_ERROR (no CPU fallback)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = A.RDF_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    lib.api()
    s.rdf_groupby_sorted.restype = C.c_int
    return s


def test_the_symbol_is_exported():
    s = lib.load()
    assert hasattr(s, "rdf_groupby_sorted")
    assert "rdf_groupby_sorted" in lib.EXPORTS


def test_the_struct_and_enum_mirrors_match_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rdf_mi355x.h"
int main(void) {
    printf("sizeof %zu\n", sizeof(rdf_group_call));
    printf("fn %zu\n", offsetof(rdf_group_call, fn));
    printf("ignore_nulls %zu\n", offsetof(rdf_group_call, ignore_nulls));
    printf("count_distinct %d\n", (int)RDF_GRP_COUNT_DISTINCT);
    printf("sum_distinct %d\n", (int)RDF_GRP_SUM_DISTINCT);
    printf("first %d\n", (int)RDF_GRP_FIRST);
    printf("last %d\n", (int)RDF_GRP_LAST);
    printf("max_calls %d\n", (int)RDF_GROUP_MAX_CALLS);
    printf("tile %d\n", (int)RDF_GROUP_SORTED_TILE);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert out["sizeof"] == C.sizeof(A.rdf_group_call) == 8
    assert out["fn"] == A.rdf_group_call.fn.offset and out["ignore_nulls"] == A.rdf_group_call.ignore_nulls.offset
    assert {n: out[n] for n in A.GROUP_FNS} == A.GROUP_FNS
    assert (A.GRP_COUNT_DISTINCT, A.GRP_SUM_DISTINCT, A.GRP_FIRST, A.GRP_LAST) == (0, 1, 2, 3)
    assert out["max_calls"] == A.GROUP_MAX_CALLS and out["tile"] == A.GROUP_SORTED_TILE


class Call:
    """One rdf_groupby_sorted call over host buffers filled with 77, so that "nothing written" can be checked."""

    def __init__(self, ngroup=1, rows=5, calls=((A.GRP_COUNT_DISTINCT, 0),), value="i64", capacity=None, validity=True,
                 value_validity=True, mem=A.MEM_HOST):
        self.cols = [A.HostArray.from_numpy(np.arange(rows, dtype=np.int64) % 3) for _ in range(ngroup)]
        self.arrs = [(A.rdf_array * 1)(c.c_struct()) for c in self.cols]
        self.gk = (A.rdf_sort_key * max(1, ngroup))(*[
            A.rdf_sort_key(C.cast(a, C.POINTER(A.rdf_array)), None, A.rdf_sort_options(0, 0)) for a in self.arrs])
        self.ngroup, self.nchunks = ngroup, 1
        self.vdtype = A.I64
        if value == "utf8":
            self.vcol = A.HostUtf8.from_pylist([("s%d" % (i % 2)) if i else None for i in range(rows)])
            self.varr = (A.rdf_utf8_array * 1)(self.vcol.c_struct())
            self.vk = (A.rdf_sort_key * 1)(A.rdf_sort_key(None, C.cast(self.varr, C.POINTER(A.rdf_utf8_array)), A.rdf_sort_options(0, 0)))
        elif value is not None:
            np_dt = {"i64": np.int64, "f64": np.float64, "f32": np.float32, "u8": np.uint8}[value]
            mask = (np.arange(rows) % 4 != 1) if value_validity else None
            self.vcol = A.HostArray.from_numpy(np.arange(rows).astype(np_dt), mask)
            self.vdtype = self.vcol.dtype
            self.varr = (A.rdf_array * 1)(self.vcol.c_struct())
            self.vk = (A.rdf_sort_key * 1)(A.rdf_sort_key(C.cast(self.varr, C.POINTER(A.rdf_array)), None, A.rdf_sort_options(0, 0)))
        else:
            self.vk = None
        self.calls = (A.rdf_group_call * max(1, len(calls)))(*[A.rdf_group_call(f, i) for f, i in calls])
        self.ncalls = len(calls)
        cap = rows if capacity is None else capacity
        self.bufs = [np.full(max(rows, 1) + 8, 77, dtype=np.int64) for _ in range(len(calls) + 1)]
        self.vbufs = [np.full(16, 77, dtype=np.uint8) for _ in calls]
        self.outs = (A.rdf_out * max(1, len(calls)))(*[
            A.rdf_out(b.ctypes.data, v.ctypes.data if validity else None, cap, -5, -5, A.group_sorted_out_dtype(f, self.vdtype), mem)
            for (f, _i), b, v in zip(calls, self.bufs, self.vbufs)])
        self.rows_out = (A.rdf_out * 1)(A.rdf_out(self.bufs[-1].ctypes.data, None, cap, -5, -5, A.U32, mem))
        self.with_rows = True
        self.groups = C.c_int64(-7)

    def run(self, so):
        return so.rdf_groupby_sorted(self.gk if self.ngroup else None, C.c_int32(self.ngroup), self.vk, C.c_int64(self.nchunks),
                                     self.calls if self.ncalls else None, C.c_int32(self.ncalls),
                                     self.rows_out if self.with_rows else None, self.outs if self.ncalls else None, C.byref(self.groups))

    def untouched(self):
        return all((b == 77).all() for b in self.bufs) and all((v == 77).all() for v in self.vbufs)


def refused(so, call, status=BAD):
    assert call.run(so) == status, so.rdf_last_error()
    assert call.untouched()


def test_calls_are_checked_before_the_device(so):
    refused(so, Call(calls=((A.GRP_COUNT_DISTINCT, 0),) * 9))      # more than 8
    for fn in (-1, 4, 100):
        c = Call()
        c.calls[0].fn = fn
        refused(so, c)                                             # unknown function
    for value in ("i64", "u8", "f64", "f32"):
        for fn in range(4):
            right = A.group_sorted_out_dtype(fn, Call(value=value).vdtype)
            for dt in (A.I64, A.F64, A.U32, A.I32, A.U64, A.F32):
                if dt == right:
                    continue
                c = Call(value=value, calls=((fn, 0),))
                c.outs[0].dtype = dt
                refused(so, c)                                     # wrong output dtype
    c = Call()
    c.rows_out[0].dtype = A.I64
    refused(so, c)                                                 # group rows are UInt32
    refused(so, Call(value="utf8", calls=((A.GRP_SUM_DISTINCT, 0),)))   # no sum of text
    refused(so, Call(calls=((A.GRP_FIRST, 1),), validity=False))   # ignore_nulls over a nullable column needs the bitmap
    refused(so, Call(calls=((A.GRP_LAST, 1),), validity=False))
    refused(so, Call(value="utf8", calls=((A.GRP_LAST, 1),), validity=False))
    c = Call()
    c.outs[0].values = None                                        # a capacity without a buffer
    refused(so, c)
    c = Call()
    c.vk = None                                                    # calls without a value column
    refused(so, c)
    c = Call()
    c.ncalls = 0                                                   # a value column without calls
    refused(so, c)
    c = Call()
    assert so.rdf_groupby_sorted(c.gk, C.c_int32(1), c.vk, C.c_int64(1), None, C.c_int32(1), c.rows_out, c.outs, C.byref(c.groups)) == BAD
    assert so.rdf_groupby_sorted(c.gk, C.c_int32(1), c.vk, C.c_int64(1), c.calls, C.c_int32(1), c.rows_out, None, C.byref(c.groups)) == BAD
    assert so.rdf_groupby_sorted(c.gk, C.c_int32(1), c.vk, C.c_int64(1), c.calls, C.c_int32(1), c.rows_out, c.outs, None) == BAD
    assert c.untouched()


def test_keys_are_checked_before_the_device(so):
    refused(so, Call(ngroup=5))                                    # more than 4 keys
    c = Call()
    c.ngroup = -1
    refused(so, c)
    c = Call()
    c.gk[0].values = None                                          # neither pointer
    refused(so, c)
    c = Call()
    c.vk[0].values = None                                          # ... on the value
    refused(so, c)
    h = A.HostUtf8.from_pylist(["a", "b", "c", "d", "e"])
    u = (A.rdf_utf8_array * 1)(h.c_struct())
    c = Call()
    c.gk[0].utf8 = C.cast(u, C.POINTER(A.rdf_utf8_array))          # both pointers
    refused(so, c)
    c = Call()
    c.vk[0].utf8 = C.cast(u, C.POINTER(A.rdf_utf8_array))
    refused(so, c)
    c = Call()
    c.nchunks = 0
    refused(so, c)
    c = Call()
    c.arrs[0][0].dtype = A.BOOL                                    # a dtype the sort refuses
    refused(so, c)
    c = Call()
    c.varr[0].dtype = A.BOOL
    refused(so, c)
    c = Call()
    c.varr[0].mem = A.MEM_DEVICE                                   # mixed memory kinds among the inputs
    refused(so, c)
    refused(so, Call(mem=A.MEM_DEVICE))                            # ... between inputs and outputs
    c = Call(calls=((A.GRP_FIRST, 0), (A.GRP_COUNT_DISTINCT, 0)))
    c.outs[1].mem = A.MEM_DEVICE
    refused(so, c)
    c = Call()
    c.rows_out[0].mem = A.MEM_DEVICE
    refused(so, c)
    c = Call()
    c.varr[0].length = 4                                           # chunk row counts differ between columns
    refused(so, c, A.RDF_COMPUTE_ERROR)
    c = Call(ngroup=2)
    c.arrs[1][0].length = 6
    refused(so, c, A.RDF_COMPUTE_ERROR)
    c = Call()
    c.arrs[0][0].length = 2**32                                    # 2^32 rows or more
    c.varr[0].length = 2**32
    refused(so, c)


def test_zero_rows_is_a_valid_call_that_writes_nothing(so):
    c = Call(rows=0, calls=((A.GRP_COUNT_DISTINCT, 0), (A.GRP_LAST, 1)))
    assert c.run(so) == A.RDF_OK
    assert c.untouched() and c.groups.value == 0
    assert [c.outs[i].length for i in range(2)] == [0, 0] and c.rows_out[0].length == 0
    c = Call(ngroup=0, rows=0, calls=(), value=None)               # no keys, no value: no rows
    assert c.run(so) == A.RDF_OK
    assert c.untouched() and c.groups.value == 0
    groups, rows, res = lib.api().groupby_sorted([[A.HostArray.from_numpy(np.zeros(0, dtype=np.int32))]],
                                                 [A.HostArray.from_numpy(np.zeros(0))], ["sum_distinct", "first"])
    assert groups == 0 and rows.shape == (0,) and res[0].shape == (0,) and res[1][0].shape == (0,)


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error_for_valid_calls(so):
    api = lib.api()
    k = [A.HostArray.from_numpy(np.array([1, 1, 2], dtype=np.int32))]
    v = [A.HostArray.from_numpy(np.array([0.5, -0.0, 0.0]))]
    t = [A.HostUtf8.from_pylist(["b", None, "a"])]
    calls = [lambda: api.groupby_sorted([k], v, ["count_distinct", "sum_distinct", "first", ("last", 1)]),
             lambda: api.groupby_sorted([t, k], t, ["count_distinct", ("first", 1)]),
             lambda: api.groupby_sorted([], v, ["sum_distinct"]),
             lambda: api.groupby_sorted([t], None, [])]
    for call in calls:
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
        assert "no CPU fallback" in ei.value.message
