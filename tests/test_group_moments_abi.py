"""rdf_groupby_moments at the C-ABI boundary, without a GPU: the symbol is exported, the mirrors match the header (checked by
a compiled C snippet), every argument error is RDF_INVALID_ARGUMENT returned before any device work with nothing written —
and in the order the header states, shown by calls that carry two faults and are refused for the earlier one — zero rows is
a valid call, and with no device a valid call fails loudly with RDF_DEVICE_ERROR (no CPU fallback)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib
import group_moments_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = A.RDF_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    lib.api()
    s.rdf_groupby_moments.restype = C.c_int
    return s


def test_the_symbol_is_exported():
    assert hasattr(lib.load(), "rdf_groupby_moments")
    assert "rdf_groupby_moments" in lib.EXPORTS


def test_the_struct_and_constants_match_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rdf_mi355x.h"
int main(void) {
    printf("sizeof %zu\n", sizeof(rdf_group_stat_call));
    printf("stat %zu\n", offsetof(rdf_group_stat_call, stat));
    printf("reserved %zu\n", offsetof(rdf_group_stat_call, reserved));
    printf("max_calls %d\n", (int)RDF_GROUP_MOMENTS_MAX_CALLS);
    printf("tile %d\n", (int)RDF_GROUP_MOMENTS_TILE);
    printf("state %zu\n", sizeof(rdf_moments_state));
    printf("costate %zu\n", sizeof(rdf_comoments_state));
    printf("kurtosis %d\n", (int)RDF_STAT_KURTOSIS);
    printf("corr %d\n", (int)RDF_COSTAT_CORR);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
    assert out["sizeof"] == C.sizeof(A.rdf_group_stat_call) == 8
    assert out["stat"] == A.rdf_group_stat_call.stat.offset and out["reserved"] == A.rdf_group_stat_call.reserved.offset
    assert out["max_calls"] == A.GROUP_MOMENTS_MAX_CALLS == 8
    assert out["tile"] == A.GROUP_MOMENTS_TILE == R.T
    assert out["state"] == C.sizeof(A.rdf_moments_state) == 48 and out["costate"] == C.sizeof(A.rdf_comoments_state) == 64
    assert out["kurtosis"] == A.STAT_KURTOSIS and out["corr"] == A.COSTAT_CORR


class Call:
    """One rdf_groupby_moments call over host buffers filled with 77, so that "nothing written" can be checked."""

    def __init__(self, ngroup=1, rows=5, stats=(A.STAT_VAR_SAMP,), pair=False, x="f64", capacity=None, mem=A.MEM_HOST):
        self.cols = [A.HostArray.from_numpy(np.arange(rows, dtype=np.int64) % 3) for _ in range(ngroup)]
        self.arrs = [(A.rdf_array * 1)(c.c_struct()) for c in self.cols]
        self.gk = (A.rdf_sort_key * max(1, ngroup))(*[
            A.rdf_sort_key(C.cast(a, C.POINTER(A.rdf_array)), None, A.rdf_sort_options(0, 0)) for a in self.arrs])
        self.ngroup, self.nchunks = ngroup, 1
        np_dt = {"f64": np.float64, "i8": np.int8, "u64": np.uint64}[x]
        self.xcol = A.HostArray.from_numpy(np.arange(rows).astype(np_dt), np.arange(rows) % 4 != 1)
        self.ycol = A.HostArray.from_numpy(np.arange(rows).astype(np.float32))
        self.x = (A.rdf_array * 1)(self.xcol.c_struct())
        self.y = (A.rdf_array * 1)(self.ycol.c_struct())
        self.with_x, self.with_y = True, pair
        self.calls = (A.rdf_group_stat_call * max(1, len(stats)))(*[A.rdf_group_stat_call(s, 0) for s in stats])
        self.ncalls = len(stats)
        cap = rows if capacity is None else capacity
        self.bufs = [np.full(max(rows, 1) + 8, 77, dtype=np.int64) for _ in range(len(stats) + 2)]
        self.vbufs = [np.full(16, 77, dtype=np.uint8) for _ in stats]
        self.outs = (A.rdf_out * max(1, len(stats)))(*[
            A.rdf_out(b.ctypes.data, v.ctypes.data, cap, -5, -5, A.F64, mem) for b, v in zip(self.bufs, self.vbufs)])
        self.rows_out = (A.rdf_out * 1)(A.rdf_out(self.bufs[-1].ctypes.data, None, cap, -5, -5, A.U32, mem))
        self.counts_out = (A.rdf_out * 1)(A.rdf_out(self.bufs[-2].ctypes.data, None, cap, -5, -5, A.I64, mem))
        self.states = np.full(64 * (max(rows, 1) + 1), 77, dtype=np.uint8)
        self.states_capacity = cap
        self.with_rows = self.with_counts = self.with_states = True
        self.groups = C.c_int64(-7)

    def run(self, so, groups=True):
        return so.rdf_groupby_moments(self.gk if self.ngroup else None, C.c_int32(self.ngroup), self.x if self.with_x else None,
                                      self.y if self.with_y else None, C.c_int64(self.nchunks),
                                      self.calls if self.ncalls else None, C.c_int32(self.ncalls),
                                      self.rows_out if self.with_rows else None, self.outs if self.ncalls else None,
                                      self.counts_out if self.with_counts else None,
                                      C.c_void_p(self.states.ctypes.data) if self.with_states else None, C.c_int64(self.states_capacity),
                                      C.byref(self.groups) if groups else None)

    def untouched(self):
        return all((b == 77).all() for b in self.bufs) and all((v == 77).all() for v in self.vbufs) and (self.states == 77).all()


def refused(so, call, status=BAD, says=None, **kw):
    assert call.run(so, **kw) == status, so.rdf_last_error()
    assert call.untouched()
    if says is not None:
        assert says in so.rdf_last_error().decode(), so.rdf_last_error()


# every fault of the header's list, in its order: (name, how to put it into a call, a word of its message)
def f_groups(c): return dict(groups=False)
def f_keys(c): c.ngroup = 5
def f_calls(c): c.ncalls = 9
def f_x(c): c.with_x = False
def f_stat(c): c.calls[0].stat = A.STAT_KURTOSIS + 1
def f_key_rules(c): c.arrs[0][0].dtype = A.BOOL
def f_x_dtype(c): c.x[0].dtype = A.BOOL
def f_out_dtype(c): c.outs[0].dtype = A.I64
def f_bitmap(c): c.outs[0].validity = None
def f_counts_dtype(c): c.counts_out[0].dtype = A.F64
def f_states(c): c.states_capacity = -1
def f_mem(c): c.x[0].mem = A.MEM_DEVICE


FAULTS = [("out_groups", f_groups, "null out_groups"), ("key count", f_keys, "grouping keys"), ("call count", f_calls, "at most 8 calls"),
          ("x missing", f_x, "x is given exactly when"), ("unknown stat", f_stat, "unknown statistic"), ("key rules", f_key_rules, "key 0"),
          ("x dtype", f_x_dtype, "x: numeric chunks"), ("output dtype", f_out_dtype, "wrong output dtype"),
          ("bitmap", f_bitmap, "validity bitmap"), ("counts dtype", f_counts_dtype, "counts are Int64"),
          ("states capacity", f_states, "states_capacity"), ("memory kinds", f_mem, "memory space")]


@pytest.mark.parametrize("i", range(len(FAULTS)), ids=[f[0] for f in FAULTS])
def test_every_refusal_and_its_place_in_the_order(so, i):
    c = Call()
    kw = FAULTS[i][1](c) or {}
    refused(so, c, says=FAULTS[i][2], **kw)
    for j in range(i + 1, len(FAULTS)):            # with a later fault in the same call, the earlier one is reported
        c = Call()
        kw = FAULTS[i][1](c) or {}
        kw.update(FAULTS[j][1](c) or {})
        refused(so, c, says=FAULTS[i][2], **kw)


def test_the_other_forms_of_each_refusal(so):
    c = Call()
    c.ngroup = -1
    refused(so, c)
    c = Call()
    assert so.rdf_groupby_moments(None, C.c_int32(1), c.x, None, C.c_int64(1), c.calls, C.c_int32(1), c.rows_out, c.outs, None, None,
                                  C.c_int64(0), C.byref(c.groups)) == BAD                     # keys counted, none given
    c = Call()
    c.ncalls = -1
    refused(so, c)
    c = Call()
    assert so.rdf_groupby_moments(c.gk, C.c_int32(1), c.x, None, C.c_int64(1), None, C.c_int32(1), c.rows_out, c.outs, None, None,
                                  C.c_int64(0), C.byref(c.groups)) == BAD                     # calls counted, none given
    assert so.rdf_groupby_moments(c.gk, C.c_int32(1), c.x, None, C.c_int64(1), c.calls, C.c_int32(1), c.rows_out, None, None, None,
                                  C.c_int64(0), C.byref(c.groups)) == BAD                     # ... or no outputs
    assert c.untouched()
    c = Call(stats=())                                             # x given with nothing asked
    c.with_counts = c.with_states = False
    refused(so, c, says="x is given exactly when")
    c = Call(stats=())                                             # counts alone ask for x
    c.with_x = c.with_states = False
    refused(so, c, says="x is given exactly when")
    c = Call(stats=())                                             # states alone ask for x
    c.with_x = c.with_counts = False
    refused(so, c, says="x is given exactly when")
    c = Call(pair=True, stats=(A.COSTAT_CORR,))                    # y without x
    c.with_x = False
    refused(so, c, says="x is given exactly when")
    refused(so, Call(stats=(-1,)), says="unknown statistic")
    refused(so, Call(pair=True, stats=(A.STAT_KURTOSIS,)), says="unknown statistic")     # an rdf_stat number with y
    refused(so, Call(stats=(A.COSTAT_CORR + 1,), pair=True), says="unknown statistic")
    c = Call()
    c.gk[0].values = None                                          # a key with neither pointer
    refused(so, c)
    c = Call()
    c.nchunks = 0
    refused(so, c)
    c = Call(pair=True, stats=(A.COSTAT_CORR,))
    c.y[0].dtype = A.BOOL
    refused(so, c, says="y: numeric chunks")
    for dt in (A.I64, A.U32, A.F32):
        c = Call()
        c.outs[0].dtype = dt
        refused(so, c, says="wrong output dtype")
    c = Call()
    c.rows_out[0].dtype = A.I64
    refused(so, c, says="group rows are UInt32")
    refused(so, Call(mem=A.MEM_DEVICE))                            # inputs on the host, outputs on the device
    c = Call(pair=True, stats=(A.COSTAT_CORR,))
    c.y[0].mem = A.MEM_DEVICE
    refused(so, c, says="memory space")
    c = Call()
    c.counts_out[0].mem = A.MEM_DEVICE
    refused(so, c)
    c = Call()
    c.outs[0].values = None                                        # a capacity without a buffer
    refused(so, c)


def test_chunk_lengths_that_differ_are_a_compute_error(so):
    c = Call()
    c.x[0].length = 4
    refused(so, c, A.RDF_COMPUTE_ERROR)
    c = Call(pair=True, stats=(A.COSTAT_COVAR_POP,))
    c.y[0].length = 4
    refused(so, c, A.RDF_COMPUTE_ERROR)
    c = Call()
    c.arrs[0][0].length = 2**32                                    # 2^32 rows or more
    c.x[0].length = 2**32
    refused(so, c)


def test_zero_rows_is_a_valid_call_that_writes_nothing(so):
    c = Call(rows=0, stats=(A.STAT_VAR_SAMP, A.STAT_SKEWNESS))
    assert c.run(so) == A.RDF_OK
    assert c.untouched() and c.groups.value == 0
    assert [c.outs[i].length for i in range(2)] == [0, 0] and c.rows_out[0].length == 0 and c.counts_out[0].length == 0
    c = Call(ngroup=0, rows=0, stats=())                           # no keys, no x: no rows
    c.with_x = c.with_counts = c.with_states = False
    assert c.run(so) == A.RDF_OK
    assert c.untouched() and c.groups.value == 0
    groups, rows, res, counts, states = lib.api().groupby_moments([[A.HostArray.from_numpy(np.zeros(0, dtype=np.int32))]],
                                                                  [A.HostArray.from_numpy(np.zeros(0))], stats=["var_samp", "kurtosis"], states=True)
    assert groups == 0 and rows.shape == (0,) and counts.shape == (0,) and res[0][0].shape == (0,) and len(states) == 0


def test_a_valid_call_needs_the_device(so):
    """Without a GPU a valid call is RDF_DEVICE_ERROR: there is no CPU path.  With one, the same calls succeed."""
    api = lib.api()
    k = [A.HostArray.from_numpy(np.array([1, 1, 2], dtype=np.int32))]
    v = [A.HostArray.from_numpy(np.array([0.5, -0.0, 2.0]))]
    t = [A.HostUtf8.from_pylist(["b", None, "a"])]
    calls = [lambda: api.groupby_moments([k], v, stats=["var_samp", "stddev_pop", "skewness", "kurtosis"]),
             lambda: api.groupby_moments([t, k], v, v, stats=["corr", "covar_samp"], states=True),
             lambda: api.groupby_moments([], v, stats=["mean"]),
             lambda: api.groupby_moments([t], None, stats=[])]
    for call in calls:
        if lib.device_count() > 0:
            assert call()[0] >= 1
            continue
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
        assert "no CPU fallback" in ei.value.message
