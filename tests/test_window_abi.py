"""rdf_window at the C-ABI boundary, without a GPU: the symbol is exported, every argument error is a value returned before
any device work with nothing written, short capacities report the rows, zero rows is a valid call, and with no device a
valid call fails loudly with RDF_DEVICE_ERROR (no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

BAD = A.RDF_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    lib.api()
    s.rdf_window.restype = C.c_int
    return s


def test_the_symbol_is_exported():
    s = lib.load()
    assert hasattr(s, "rdf_window")
    assert "rdf_window" in lib.EXPORTS


def test_the_struct_and_enum_mirrors_match_the_header():
    assert C.sizeof(A.rdf_window_call) == 16 and A.rdf_window_call.param.offset == 8
    assert [A.WINDOW_FNS[n] for n in ("row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile", "lag", "lead")] == list(range(8))
    assert (A.WINDOW_MAX_KEYS, A.WINDOW_MAX_CALLS) == (4, 8)


class Call:
    """One rdf_window call over host buffers filled with 77, so that "nothing written" can be checked."""

    def __init__(self, nkeys_p=1, nkeys_o=1, rows=5, calls=((A.WIN_ROW_NUMBER, 0),), capacity=None, validity=True, mem=A.MEM_HOST):
        self.cols = [A.HostArray.from_numpy(np.arange(rows, dtype=np.int64) % 3) for _ in range(nkeys_p + nkeys_o)]
        self.arrs = [(A.rdf_array * 1)(c.c_struct()) for c in self.cols]
        keys = [A.rdf_sort_key(C.cast(a, C.POINTER(A.rdf_array)), None, A.rdf_sort_options(0, 0)) for a in self.arrs]
        self.pk = (A.rdf_sort_key * max(1, nkeys_p))(*keys[:nkeys_p])
        self.ok = (A.rdf_sort_key * max(1, nkeys_o))(*keys[nkeys_p:])
        self.np, self.no = nkeys_p, nkeys_o
        self.nchunks, self.nrows = 1, 0
        self.calls = (A.rdf_window_call * max(1, len(calls)))(*[A.rdf_window_call(f, 0, p) for f, p in calls])
        self.ncalls = len(calls)
        cap = rows if capacity is None else capacity
        self.bufs = [np.full(max(rows, 1) + 8, 77, dtype=np.int64) for _ in calls]
        self.vbufs = [np.full(16, 77, dtype=np.uint8) for _ in calls]
        self.outs = (A.rdf_out * max(1, len(calls)))(*[
            A.rdf_out(b.ctypes.data, v.ctypes.data if validity else None, cap, -5, -5, A.window_out_dtype(f), mem)
            for (f, _p), b, v in zip(calls, self.bufs, self.vbufs)])

    def run(self, so):
        return so.rdf_window(self.pk if self.np else None, C.c_int32(self.np), self.ok if self.no else None, C.c_int32(self.no),
                             C.c_int64(self.nchunks), C.c_int64(self.nrows), self.calls, C.c_int32(self.ncalls), self.outs)

    def untouched(self):
        return all((b == 77).all() for b in self.bufs) and all((v == 77).all() for v in self.vbufs)


def refused(so, call, status=BAD):
    assert call.run(so) == status, so.rdf_last_error()
    assert call.untouched()


def test_calls_are_checked_before_the_device(so):
    c = Call()
    c.ncalls = 0
    refused(so, c)                                             # no calls
    c = Call(calls=((A.WIN_ROW_NUMBER, 0),) * 9)
    refused(so, c)                                             # more than 8
    for fn in (-1, 8, 100):
        c = Call()
        c.calls[0].fn = fn
        refused(so, c)                                         # unknown function
    for fn, p in ((A.WIN_NTILE, 0), (A.WIN_NTILE, -3), (A.WIN_LAG, -1), (A.WIN_LEAD, -1)):
        refused(so, Call(calls=((fn, p),)))                    # param out of range
    for fn, dt in ((A.WIN_ROW_NUMBER, A.F64), (A.WIN_RANK, A.U32), (A.WIN_DENSE_RANK, A.I32), (A.WIN_NTILE, A.U64),
                   (A.WIN_PERCENT_RANK, A.I64), (A.WIN_CUME_DIST, A.F32), (A.WIN_LAG, A.I64), (A.WIN_LEAD, A.I32)):
        c = Call(calls=((fn, 1),))
        c.outs[0].dtype = dt
        refused(so, c)                                         # wrong output dtype
    refused(so, Call(calls=((A.WIN_LAG, 1),), validity=False))     # lag / lead with an offset need the bitmap
    refused(so, Call(calls=((A.WIN_LEAD, 2),), validity=False))
    c = Call()
    c.outs[0].values = None                                    # a capacity without a buffer
    refused(so, c)
    c = Call()
    assert so.rdf_window(c.pk, C.c_int32(1), c.ok, C.c_int32(1), C.c_int64(1), C.c_int64(0), None, C.c_int32(1), c.outs) == BAD
    assert so.rdf_window(c.pk, C.c_int32(1), c.ok, C.c_int32(1), C.c_int64(1), C.c_int64(0), c.calls, C.c_int32(1), None) == BAD


def test_keys_are_checked_before_the_device(so):
    refused(so, Call(nkeys_p=5))                               # more than 4 keys of a kind
    refused(so, Call(nkeys_o=5))
    c = Call()
    c.np = -1
    refused(so, c)
    c = Call()
    c.pk[0].values = None                                      # neither pointer
    refused(so, c)
    c = Call()
    h = A.HostUtf8.from_pylist(["a", "b", "c", "d", "e"])
    u = (A.rdf_utf8_array * 1)(h.c_struct())
    c.ok[0].utf8 = C.cast(u, C.POINTER(A.rdf_utf8_array))      # both pointers
    refused(so, c)
    c = Call()
    c.nchunks = 0
    refused(so, c)
    c = Call()
    c.arrs[0][0].dtype = A.BOOL                                # a dtype the sort refuses
    refused(so, c)
    c = Call()
    c.arrs[1][0].mem = A.MEM_DEVICE                            # mixed memory kinds among the keys
    refused(so, c)
    c = Call(mem=A.MEM_DEVICE)                                 # ... and between keys and outputs
    refused(so, c)
    c = Call(calls=((A.WIN_RANK, 0), (A.WIN_ROW_NUMBER, 0)))
    c.outs[1].mem = A.MEM_DEVICE
    refused(so, c)
    c = Call()
    c.arrs[1][0].length = 4                                    # chunk row counts differ between keys
    refused(so, c, A.RDF_COMPUTE_ERROR)
    c = Call()
    c.nrows = 4                                                # contradicts the keys' 5 rows
    refused(so, c)
    c = Call(nkeys_p=0, nkeys_o=0)
    c.nrows = -1
    refused(so, c)
    c = Call(nkeys_p=0, nkeys_o=0, rows=1, capacity=2**32)
    c.nrows = 2**32                                            # 2^32 rows or more
    refused(so, c)
    c = Call(nkeys_p=0, nkeys_o=0)
    c.outs[0].mem = 7
    c.nrows = 5
    refused(so, c)


def test_short_capacities_report_the_rows_and_write_nothing(so):
    for cap in (4, 0):
        c = Call(calls=((A.WIN_RANK, 0), (A.WIN_CUME_DIST, 0), (A.WIN_LAG, 1)), capacity=cap)
        c.outs[0].capacity = 5                                 # one short output is enough
        refused(so, c, A.RDF_MEMORY_ERROR)
        assert [c.outs[i].length for i in range(3)] == [5, 5, 5]
    c = Call(nkeys_p=0, nkeys_o=0, capacity=9)
    c.nrows = 10
    refused(so, c, A.RDF_MEMORY_ERROR)
    assert c.outs[0].length == 10


def test_zero_rows_is_a_valid_call_that_writes_nothing(so):
    c = Call(rows=0, calls=((A.WIN_ROW_NUMBER, 0), (A.WIN_LEAD, 1)))
    assert c.run(so) == A.RDF_OK
    assert c.untouched() and [c.outs[i].length for i in range(2)] == [0, 0] and c.outs[1].null_count == 0
    c = Call(nkeys_p=0, nkeys_o=0, rows=0)
    assert c.run(so) == A.RDF_OK
    assert c.untouched() and c.outs[0].length == 0
    assert lib.api().window([], [], ["row_number"], mem="host", nrows=0)[0].shape == (0,)


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error_for_valid_calls(so):
    api = lib.api()
    p = [A.HostArray.from_numpy(np.array([1, 1, 2], dtype=np.int32))]
    o = [A.HostArray.from_numpy(np.array([0.5, -0.0, 0.0]))]
    t = [A.HostUtf8.from_pylist(["b", None, "a"])]
    calls = [lambda: api.window([p], [(o, True)], ["rank"]),
             lambda: api.window([t], [o], ["row_number", ("ntile", 2), ("lag", 1), ("lead", 0)]),
             lambda: api.window([], [t], ["cume_dist"]),
             lambda: api.window([], [], ["row_number"], mem="host", nrows=3)]
    for call in calls:
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
        assert "no CPU fallback" in ei.value.message
