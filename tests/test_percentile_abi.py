"""rdf_groupby_percentile at the C-ABI boundary, without a GPU: the symbol is exported, the mirrors match the header (checked
by a compiled C snippet), every argument error is a value returned before any device work with nothing written and in the
order the header documents, zero rows is a valid call, and with no device a valid call fails loudly with RDF_DEVICE_ERROR
(no CPU fallback)."""
import ctypes as C
import math
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
    s.rdf_groupby_percentile.restype = C.c_int
    yield s
    lib.set_option("percentile_route", 0)


def test_the_symbol_is_exported():
    s = lib.load()
    assert hasattr(s, "rdf_groupby_percentile")
    assert "rdf_groupby_percentile" in lib.EXPORTS


def test_the_struct_and_enum_mirrors_match_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rdf_mi355x.h"
int main(void) {
    printf("sizeof %zu\n", sizeof(rdf_percentile_call));
    printf("kind %zu\n", offsetof(rdf_percentile_call, kind));
    printf("reserved %zu\n", offsetof(rdf_percentile_call, reserved));
    printf("p %zu\n", offsetof(rdf_percentile_call, p));
    printf("cont %d\n", (int)RDF_PCT_CONT);
    printf("disc %d\n", (int)RDF_PCT_DISC);
    printf("max_calls %d\n", (int)RDF_PERCENTILE_MAX_CALLS);
    printf("pick_block %d\n", (int)RDF_PERCENTILE_PICK_BLOCK);
    printf("bits %d\n", (int)RDF_PCT_SELECT_BITS);
    printf("tile %d\n", (int)RDF_PCT_SELECT_TILE);
    printf("finish %d\n", (int)RDF_PCT_SELECT_FINISH);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert out["sizeof"] == C.sizeof(A.rdf_percentile_call) == 16
    assert (out["kind"], out["reserved"], out["p"]) == (A.rdf_percentile_call.kind.offset, A.rdf_percentile_call.reserved.offset, A.rdf_percentile_call.p.offset) == (0, 4, 8)
    assert {n: out[n] for n in A.PERCENTILE_KINDS} == A.PERCENTILE_KINDS and (A.PCT_CONT, A.PCT_DISC) == (0, 1)
    assert out["max_calls"] == A.PERCENTILE_MAX_CALLS and out["pick_block"] == A.PERCENTILE_PICK_BLOCK
    assert (out["bits"], out["tile"], out["finish"]) == (A.PCT_SELECT_BITS, A.PCT_SELECT_TILE, A.PCT_SELECT_FINISH)
    assert A.PCT_SELECT_TILE % 256 == 0 and A.PCT_SELECT_FINISH & (A.PCT_SELECT_FINISH - 1) == 0      # whole blocks per tile; the finish is a bitonic sort
    assert A.percentile_calls(["median", ("disc", 0.25), ("cont", 1)]) == [(A.PCT_CONT, 0.5), (A.PCT_DISC, 0.25), (A.PCT_CONT, 1.0)]


class Call:
    """One rdf_groupby_percentile call over host buffers filled with 77, so that "nothing written" can be checked."""

    def __init__(self, ngroup=1, rows=5, calls=((A.PCT_CONT, 0.5),), value="i64", capacity=None, validity=True, value_validity=True,
                 mem=A.MEM_HOST, counts=True):
        self.cols = [A.HostArray.from_numpy(np.arange(rows, dtype=np.int64) % 3) for _ in range(ngroup)]
        self.arrs = [(A.rdf_array * 1)(c.c_struct()) for c in self.cols]
        self.gk = (A.rdf_sort_key * max(1, ngroup))(*[
            A.rdf_sort_key(C.cast(a, C.POINTER(A.rdf_array)), None, A.rdf_sort_options(0, 0)) for a in self.arrs])
        self.ngroup, self.nchunks = ngroup, 1
        if value == "utf8":
            self.vcol = A.HostUtf8.from_pylist([("s%d" % (i % 2)) if i else None for i in range(rows)])
            self.varr = (A.rdf_utf8_array * 1)(self.vcol.c_struct())
            self.vk = (A.rdf_sort_key * 1)(A.rdf_sort_key(None, C.cast(self.varr, C.POINTER(A.rdf_utf8_array)), A.rdf_sort_options(0, 0)))
        elif value is not None:
            np_dt = {"i64": np.int64, "f64": np.float64, "f32": np.float32, "u8": np.uint8}[value]
            mask = (np.arange(rows) % 4 != 1) if value_validity else None
            self.vcol = A.HostArray.from_numpy(np.arange(rows).astype(np_dt), mask)
            self.varr = (A.rdf_array * 1)(self.vcol.c_struct())
            self.vk = (A.rdf_sort_key * 1)(A.rdf_sort_key(C.cast(self.varr, C.POINTER(A.rdf_array)), None, A.rdf_sort_options(0, 0)))
        else:
            self.vk = None
        self.calls = (A.rdf_percentile_call * max(1, len(calls)))(*[A.rdf_percentile_call(k, 0, p) for k, p in calls])
        self.ncalls = len(calls)
        cap = rows if capacity is None else capacity
        self.bufs = [np.full(max(rows, 1) + 8, 77, dtype=np.int64) for _ in range(len(calls) + 2)]
        self.vbufs = [np.full(16, 77, dtype=np.uint8) for _ in calls]
        self.outs = (A.rdf_out * max(1, len(calls)))(*[
            A.rdf_out(b.ctypes.data, v.ctypes.data if validity else None, cap, -5, -5, A.F64 if k == A.PCT_CONT else A.U32, mem)
            for (k, _p), b, v in zip(calls, self.bufs, self.vbufs)])
        self.rows_out = (A.rdf_out * 1)(A.rdf_out(self.bufs[-1].ctypes.data, None, cap, -5, -5, A.U32, mem))
        self.counts_out = (A.rdf_out * 1)(A.rdf_out(self.bufs[-2].ctypes.data, None, cap, -5, -5, A.I64, mem))
        self.with_rows, self.with_counts = True, counts
        self.groups = C.c_int64(-7)

    def run(self, so):
        return so.rdf_groupby_percentile(self.gk if self.ngroup else None, C.c_int32(self.ngroup), self.vk, C.c_int64(self.nchunks),
                                         self.calls if self.ncalls else None, C.c_int32(self.ncalls),
                                         self.rows_out if self.with_rows else None, self.outs if self.ncalls else None,
                                         self.counts_out if self.with_counts else None, C.byref(self.groups))

    def untouched(self):
        return all((b == 77).all() for b in self.bufs) and all((v == 77).all() for v in self.vbufs)


def last_error():
    return (lib.load().rdf_last_error() or b"").decode("utf-8", "replace")


def refused(so, call, status=BAD, says=None):
    assert call.run(so) == status, last_error()
    assert call.untouched()
    if says is not None:
        assert says in last_error(), last_error()


def test_calls_are_checked_before_the_device(so):
    refused(so, Call(calls=((A.PCT_CONT, 0.5),) * 9), says="at most 8")
    for kind in (-1, 2, 100):
        refused(so, Call(calls=((kind, 0.5),)), says="unknown kind")
    for p in (-1e-300, float(np.nextafter(1.0, 2.0)), 2.0, -1.0, math.inf, -math.inf, math.nan):
        for kind in (A.PCT_CONT, A.PCT_DISC):
            refused(so, Call(calls=((kind, p),)), says="[0, 1]")
    for p in (0.0, -0.0, 1.0):                                     # the ends are inside: these get as far as the device
        assert Call(calls=((A.PCT_CONT, p),)).run(so) != BAD or lib.device_count() > 0
    for value in ("i64", "u8", "f64", "f32"):
        for kind, right in ((A.PCT_CONT, A.F64), (A.PCT_DISC, A.U32)):
            for dt in (A.I64, A.F64, A.U32, A.I32, A.U64, A.F32):
                if dt == right:
                    continue
                c = Call(value=value, calls=((kind, 0.5),))
                c.outs[0].dtype = dt
                refused(so, c, says="wrong output dtype")
    c = Call()
    c.rows_out[0].dtype = A.I64
    refused(so, c, says="group rows are UInt32")
    c = Call()
    c.counts_out[0].dtype = A.U32
    refused(so, c, says="counts are Int64")
    refused(so, Call(value="utf8", calls=((A.PCT_CONT, 0.5),)), says="Utf8")          # no interpolation of text
    refused(so, Call(calls=((A.PCT_CONT, 0.5),), validity=False), says="validity bitmap")      # a nullable value needs the bitmap
    refused(so, Call(calls=((A.PCT_DISC, 0.5),), validity=False), says="validity bitmap")
    refused(so, Call(value="utf8", calls=((A.PCT_DISC, 0.5),), validity=False), says="validity bitmap")
    c = Call()
    c.outs[0].values = None                                        # a capacity without a buffer
    refused(so, c)
    c = Call()
    c.vk = None                                                    # calls without a value column
    refused(so, c)
    c = Call(counts=False)
    c.ncalls = 0                                                   # a value column without calls or counts
    refused(so, c)
    c = Call()
    for args in ((None, 1, c.outs, c.groups), (c.calls, 1, None, c.groups)):
        assert so.rdf_groupby_percentile(c.gk, C.c_int32(1), c.vk, C.c_int64(1), args[0], C.c_int32(args[1]), c.rows_out, args[2], c.counts_out, C.byref(args[3])) == BAD
    assert so.rdf_groupby_percentile(c.gk, C.c_int32(1), c.vk, C.c_int64(1), c.calls, C.c_int32(1), c.rows_out, c.outs, c.counts_out, None) == BAD
    assert c.untouched()


def test_the_refusals_come_in_the_documented_order(so):
    c = Call(ngroup=5, calls=((7, 2.0),))                          # keys before kinds
    refused(so, c, says="grouping keys")
    c = Call(calls=((7, 2.0),))                                    # kind before p
    refused(so, c, says="unknown kind")
    c = Call(calls=((A.PCT_CONT, 2.0),))
    c.varr[0].dtype = A.BOOL                                       # p before the columns' own rules
    refused(so, c, says="[0, 1]")
    c = Call(value="utf8")
    c.outs[0].dtype = A.I32                                        # CONT of text before the output dtype
    refused(so, c, says="Utf8")
    c = Call(validity=False)
    c.outs[0].dtype = A.I32                                        # the output dtype before the bitmap
    refused(so, c, says="wrong output dtype")
    lib.set_option("percentile_route", 2)
    try:
        refused(so, Call(), says="select route")                   # grouping keys: not the select route's
        refused(so, Call(ngroup=0, value="utf8", calls=((A.PCT_DISC, 0.5),)), says="select route")
        c = Call(calls=((A.PCT_CONT, 2.0),))
        refused(so, c, says="[0, 1]")                              # p before the route
        c = Call()
        c.arrs[0][0].dtype = A.BOOL
        refused(so, c, says="select route")                        # the route before the keys are looked at
    finally:
        lib.set_option("percentile_route", 0)


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
    c = Call(calls=((A.PCT_CONT, 0.5), (A.PCT_DISC, 0.5)))
    c.outs[1].mem = A.MEM_DEVICE
    refused(so, c)
    c = Call()
    c.rows_out[0].mem = A.MEM_DEVICE
    refused(so, c)
    c = Call()
    c.counts_out[0].mem = A.MEM_DEVICE
    refused(so, c)
    c = Call()
    c.varr[0].length = 4                                           # chunk row counts differ between columns
    refused(so, c, A.RDF_COMPUTE_ERROR)
    c = Call()
    c.arrs[0][0].length = 2**32                                    # 2^32 rows or more
    c.varr[0].length = 2**32
    refused(so, c)


def test_zero_rows_and_the_count_only_call_write_nothing(so):
    for route in (0, 1, 2):
        lib.set_option("percentile_route", route)
        try:
            c = Call(ngroup=0 if route == 2 else 1, rows=0, calls=((A.PCT_CONT, 0.5), (A.PCT_DISC, 1.0)))
            assert c.run(so) == A.RDF_OK, last_error()
            assert c.untouched() and c.groups.value == 0
            assert [c.outs[i].length for i in range(2)] == [0, 0] and c.rows_out[0].length == 0 and c.counts_out[0].length == 0
        finally:
            lib.set_option("percentile_route", 0)
    c = Call(ngroup=0, rows=0, calls=(), value=None, counts=False)  # no keys, no value: no rows
    assert c.run(so) == A.RDF_OK
    assert c.untouched() and c.groups.value == 0
    c = Call(rows=0, calls=(), value=None, counts=False)            # the count-only call over zero rows
    c.with_rows = False
    assert c.run(so) == A.RDF_OK and c.groups.value == 0 and c.untouched()
    groups, rows, res, cnt = lib.api().groupby_percentile([[A.HostArray.from_numpy(np.zeros(0, dtype=np.int32))]],
                                                          [A.HostArray.from_numpy(np.zeros(0))], ["median", ("disc", 0.5)], counts=True)
    assert groups == 0 and rows.shape == (0,) and res[0][0].shape == (0,) and res[1][0].shape == (0,) and cnt.shape == (0,)


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error_for_valid_calls(so):
    api = lib.api()
    k = [A.HostArray.from_numpy(np.array([1, 1, 2], dtype=np.int32))]
    v = [A.HostArray.from_numpy(np.array([0.5, -0.0, 0.0]))]
    t = [A.HostUtf8.from_pylist(["b", None, "a"])]
    calls = [lambda: api.groupby_percentile([k], v, ["median", ("disc", 0.5)]),
             lambda: api.groupby_percentile([t, k], t, [("disc", 1.0)]),
             lambda: api.groupby_percentile([], v, ["median"]),                 # the select route
             lambda: api.groupby_percentile([t], None, [])]
    for call in calls:
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
        assert "no CPU fallback" in ei.value.message
    c = Call(calls=(), value=None, counts=False)                   # the count-only call reaches the device too
    c.with_rows = False
    assert c.run(so) == A.RDF_DEVICE_ERROR
