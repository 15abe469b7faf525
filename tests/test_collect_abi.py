"""rdf_groupby_collect and rdf_list_explode at the C-ABI boundary, without a GPU: the symbols are exported, the mirrors match
the header (checked by a compiled C snippet), every argument error is a value returned before any device work with
nothing written, zero rows is a valid call, and with no device a valid call fails loudly with RDF_DEVICE_ERROR (no CPU
fallback)."""
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
    s.rdf_groupby_collect.restype = C.c_int
    s.rdf_list_explode.restype = C.c_int
    return s


def test_the_symbols_are_exported():
    s = lib.load()
    for name in ("rdf_groupby_collect", "rdf_list_explode"):
        assert hasattr(s, name) and name in lib.EXPORTS


def test_the_enum_tile_and_struct_mirrors_match_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rdf_mi355x.h"
int main(void) {
    printf("list %d\n", (int)RDF_COLLECT_LIST);
    printf("set %d\n", (int)RDF_COLLECT_SET);
    printf("tile %d\n", (int)RDF_COLLECT_TILE);
    printf("sizeof_list %zu\n", sizeof(rdf_list_array));
    printf("values %zu\n", offsetof(rdf_list_array, values));
    printf("sizeof_key %zu\n", sizeof(rdf_sort_key));
    printf("sizeof_out %zu\n", sizeof(rdf_out));
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert {n: out[n] for n in A.COLLECT_KINDS} == A.COLLECT_KINDS
    assert (A.COLLECT_LIST, A.COLLECT_SET) == (0, 1)
    assert out["tile"] == A.COLLECT_TILE == 1024
    assert out["sizeof_list"] == C.sizeof(A.rdf_list_array) and out["values"] == A.rdf_list_array.values.offset
    assert out["sizeof_key"] == C.sizeof(A.rdf_sort_key) and out["sizeof_out"] == C.sizeof(A.rdf_out)


class Collect:
    """One rdf_groupby_collect call over host buffers filled with 77, so that "nothing written" can be checked."""

    def __init__(self, ngroup=1, rows=5, kind=A.COLLECT_LIST, value="i64", with_values=True, mem=A.MEM_HOST):
        self.cols = [A.HostArray.from_numpy(np.arange(rows, dtype=np.int64) % 3) for _ in range(ngroup)]
        self.arrs = [(A.rdf_array * 1)(c.c_struct()) for c in self.cols]
        self.gk = (A.rdf_sort_key * max(1, ngroup))(*[
            A.rdf_sort_key(C.cast(a, C.POINTER(A.rdf_array)), None, A.rdf_sort_options(0, 0)) for a in self.arrs])
        self.ngroup, self.nchunks, self.kind = ngroup, 1, kind
        if value == "utf8":
            self.vcol = A.HostUtf8.from_pylist([("s%d" % (i % 2)) if i else None for i in range(rows)])
            self.varr = (A.rdf_utf8_array * 1)(self.vcol.c_struct())
            self.vk = (A.rdf_sort_key * 1)(A.rdf_sort_key(None, C.cast(self.varr, C.POINTER(A.rdf_utf8_array)), A.rdf_sort_options(0, 0)))
            self.vdtype = A.U8
        else:
            np_dt = {"i64": np.int64, "f64": np.float64, "u8": np.uint8}[value]
            self.vcol = A.HostArray.from_numpy(np.arange(rows).astype(np_dt), np.arange(rows) % 4 != 1)
            self.varr = (A.rdf_array * 1)(self.vcol.c_struct())
            self.vk = (A.rdf_sort_key * 1)(A.rdf_sort_key(C.cast(self.varr, C.POINTER(A.rdf_array)), None, A.rdf_sort_options(0, 0)))
            self.vdtype = self.vcol.dtype
        self.bufs = [np.full(max(rows, 1) + 8, 77, dtype=np.int64) for _ in range(4)]
        dts = (A.U32, A.I32, A.U32, self.vdtype)
        caps = (rows, rows + 1, rows, rows)
        self.outs = [(A.rdf_out * 1)(A.rdf_out(b.ctypes.data, None, cap, -5, -5, dt, mem)) for b, dt, cap in zip(self.bufs, dts, caps)]
        self.given = [True, True, True, with_values]
        self.groups, self.elements = C.c_int64(-7), C.c_int64(-7)

    def run(self, so):
        o = [x if g else None for x, g in zip(self.outs, self.given)]
        return so.rdf_groupby_collect(self.gk if self.ngroup else None, C.c_int32(self.ngroup), self.vk, C.c_int64(self.nchunks),
                                      C.c_int32(self.kind), o[0], o[1], o[2], o[3], C.byref(self.groups), C.byref(self.elements))

    def untouched(self):
        return all((b == 77).all() for b in self.bufs)


class Explode:
    """One rdf_list_explode call over host buffers filled with 77."""

    def __init__(self, rows=4, outer=0, validity=True, mem=A.MEM_HOST):
        lists = [[1, 2], None, [], [3]][:rows] if rows <= 4 else [[i] for i in range(rows)]
        self.lst = A.HostList.from_lists(lists, A.I64)
        self.cl = self.lst.c_struct()
        self.outer = outer
        self.bufs = [np.full(16, 77, dtype=np.int64) for _ in range(3)]
        self.vbufs = [np.full(16, 77, dtype=np.uint8) for _ in range(3)]
        self.outs = [(A.rdf_out * 1)(A.rdf_out(b.ctypes.data, v.ctypes.data if validity else None, 16, -5, -5, dt, mem))
                     for b, v, dt in zip(self.bufs, self.vbufs, (A.U32, A.U32, A.I32))]
        self.given = [True, True, True]
        self.rows = C.c_int64(-7)

    def run(self, so):
        o = [x if g else None for x, g in zip(self.outs, self.given)]
        return so.rdf_list_explode(C.byref(self.cl), C.c_int32(self.outer), o[0], o[1], o[2], C.byref(self.rows))

    def untouched(self):
        return all((b == 77).all() for b in self.bufs) and all((v == 77).all() for v in self.vbufs)


def refused(so, call, status=BAD):
    assert call.run(so) == status, so.rdf_last_error()
    assert call.untouched()


def test_collect_arguments_are_checked_before_the_device(so):
    for kind in (-1, 2, 100):
        refused(so, Collect(kind=kind))                            # unknown kind
    refused(so, Collect(ngroup=5))                                 # more than 4 keys
    c = Collect()
    c.ngroup = -1
    refused(so, c)
    c = Collect()
    c.gk[0].values = None                                          # neither pointer
    refused(so, c)
    c = Collect()
    c.vk[0].values = None                                          # ... on the value
    refused(so, c)
    h = A.HostUtf8.from_pylist(["a", "b", "c", "d", "e"])
    u = (A.rdf_utf8_array * 1)(h.c_struct())
    c = Collect()
    c.gk[0].utf8 = C.cast(u, C.POINTER(A.rdf_utf8_array))          # both pointers
    refused(so, c)
    c = Collect()
    c.vk[0].utf8 = C.cast(u, C.POINTER(A.rdf_utf8_array))
    refused(so, c)
    c = Collect()
    c.vk = None                                                    # no value column
    refused(so, c)
    c = Collect()
    c.nchunks = 0
    refused(so, c)
    for i, wrong in enumerate((A.I64, A.U32, A.I32, A.F64)):       # wrong output dtypes: group rows, offsets, child rows, values
        c = Collect()
        c.outs[i][0].dtype = wrong
        refused(so, c)
    for kind in (A.COLLECT_LIST, A.COLLECT_SET):
        refused(so, Collect(value="utf8", kind=kind))              # out_values with a Utf8 value
    c = Collect()
    c.outs[2][0].values = None                                     # a capacity without a buffer
    refused(so, c)
    c = Collect()
    c.arrs[0][0].dtype = A.BOOL                                    # a dtype the sort refuses
    refused(so, c)
    c = Collect()
    c.varr[0].dtype = A.BOOL
    refused(so, c)
    c = Collect()
    c.varr[0].mem = A.MEM_DEVICE                                   # mixed memory kinds among the inputs
    refused(so, c)
    refused(so, Collect(mem=A.MEM_DEVICE))                         # ... between inputs and outputs
    for i in range(4):
        c = Collect()
        c.outs[i][0].mem = A.MEM_DEVICE
        refused(so, c)
    c = Collect()
    c.varr[0].length = 4                                           # chunk row counts differ between columns
    refused(so, c, A.RDF_COMPUTE_ERROR)
    c = Collect(ngroup=2)
    c.arrs[1][0].length = 6
    refused(so, c, A.RDF_COMPUTE_ERROR)
    c = Collect()
    c.arrs[0][0].length = 2**32                                    # 2^32 rows or more
    c.varr[0].length = 2**32
    refused(so, c)
    c = Collect()
    o = [x for x in c.outs]
    assert so.rdf_groupby_collect(c.gk, C.c_int32(1), c.vk, C.c_int64(1), C.c_int32(0), o[0], o[1], o[2], o[3], None, C.byref(c.elements)) == BAD
    assert so.rdf_groupby_collect(c.gk, C.c_int32(1), c.vk, C.c_int64(1), C.c_int32(0), o[0], o[1], o[2], o[3], C.byref(c.groups), None) == BAD
    assert c.untouched()


def test_explode_arguments_are_checked_before_the_device(so):
    refused(so, Explode(outer=1, validity=False))                  # outer without bitmaps
    e = Explode(outer=1)
    e.outs[2][0].validity = None                                   # ... on the positions alone
    refused(so, e)
    for i, wrong in enumerate((A.I32, A.I64, A.U32)):              # wrong output dtypes: parent rows, child indices, positions
        e = Explode()
        e.outs[i][0].dtype = wrong
        refused(so, e)
    e = Explode()
    e.cl.offsets.dtype = A.I64                                     # value_offsets are Int32
    refused(so, e)
    e = Explode()
    e.cl.offsets.length = 0
    refused(so, e)
    refused(so, Explode(mem=A.MEM_DEVICE))                         # mixed memory kinds
    e = Explode()
    e.outs[1][0].mem = A.MEM_DEVICE
    refused(so, e)
    e = Explode()
    e.outs[0][0].values = None                                     # a capacity without a buffer
    refused(so, e)
    e = Explode()
    e.cl.offsets.length = 2**32 + 1                                # 2^32 list rows
    refused(so, e)
    e = Explode()
    assert so.rdf_list_explode(None, C.c_int32(0), e.outs[0], e.outs[1], e.outs[2], C.byref(e.rows)) == BAD
    assert so.rdf_list_explode(C.byref(e.cl), C.c_int32(0), e.outs[0], e.outs[1], e.outs[2], None) == BAD
    assert e.untouched()


def test_zero_rows_is_a_valid_call_that_writes_nothing(so):
    for kind in (A.COLLECT_LIST, A.COLLECT_SET):
        for ngroup in (0, 1, 2):
            c = Collect(ngroup=ngroup, rows=0, kind=kind)
            assert c.run(so) == A.RDF_OK
            assert c.untouched() and c.groups.value == 0 and c.elements.value == 0
            assert [o[0].length for o in c.outs] == [0, 0, 0, 0]
    e = Explode(rows=0, outer=1)
    assert e.run(so) == A.RDF_OK
    assert e.untouched() and e.rows.value == 0 and [o[0].length for o in e.outs] == [0, 0, 0]
    api = lib.api()
    groups, rows, offs, child, vals = api.groupby_collect([[A.HostArray.from_numpy(np.zeros(0, dtype=np.int32))]],
                                                          [A.HostArray.from_numpy(np.zeros(0))], "set")
    assert groups == 0 and rows.shape == offs.shape == child.shape == vals.shape == (0,) and vals.dtype == np.float64
    parent, (idx, valid), pos = api.list_explode(A.HostList.from_lists([], A.I32), outer=True, pos=True)
    assert parent.shape == idx.shape == valid.shape == pos[0].shape == (0,)


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error_for_valid_calls(so):
    api = lib.api()
    k = [A.HostArray.from_numpy(np.array([1, 1, 2], dtype=np.int32))]
    v = [A.HostArray.from_numpy(np.array([0.5, -0.0, 0.0]), np.array([True, False, True]))]
    t = [A.HostUtf8.from_pylist(["b", None, "a"])]
    lst = A.HostList.from_lists([[1, 2], None, []], A.I64)
    calls = [lambda: api.groupby_collect([k], v, "list"),
             lambda: api.groupby_collect([k], v, "set"),
             lambda: api.groupby_collect([t, k], t, "set"),
             lambda: api.groupby_collect([], t, "list"),
             lambda: api.groupby_collect([], v, "list", outs=(None, None, None, None)),
             lambda: api.list_explode(lst),
             lambda: api.list_explode(lst, outer=True, pos=True)]
    for call in calls:
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
        assert "no CPU fallback" in ei.value.message
