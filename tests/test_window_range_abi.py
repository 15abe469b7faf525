"""rdf_window_range_agg at the C-ABI boundary, without a GPU: the symbol is exported, the struct mirrors match the header, every
refusal the header lists is a value returned before any device work with nothing written, short capacities report the rows,
zero rows is a valid call, and with no device a valid call fails loudly with RDF_DEVICE_ERROR (no CPU fallback)."""
import ctypes as C
import math

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

BAD = A.RDF_INVALID_ARGUMENT
UP, PREC, CUR, FOLL, UF = A.BOUND_UNBOUNDED_PRECEDING, A.BOUND_PRECEDING, A.BOUND_CURRENT_ROW, A.BOUND_FOLLOWING, A.BOUND_UNBOUNDED_FOLLOWING
MINMAX = "min / max over a range frame bounded on both sides is not built"


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    lib.api()
    s.rdf_window_range_agg.restype = C.c_int
    s.rdf_last_error.restype = C.c_char_p
    return s


def test_the_symbol_is_exported():
    s = lib.load()
    assert hasattr(s, "rdf_window_range_agg")
    assert "rdf_window_range_agg" in lib.EXPORTS


def test_the_struct_mirrors_and_constants_match_the_header():
    fr, call = A.rdf_window_range_frame, A.rdf_window_range_call
    assert C.sizeof(fr) == 40 and (fr.start_kind.offset, fr.end_kind.offset, fr.start_i.offset, fr.end_i.offset, fr.start_f.offset, fr.end_f.offset) == (0, 4, 8, 16, 24, 32)
    assert C.sizeof(call) == 48 and (call.fn.offset, call.value.offset, call.frame.offset) == (0, 4, 8)
    hdr = open(lib._HERE + "/csrc/rdf_window_range.h").read()
    assert "kWRangeTile = kWRangeThreads * kWRangePer" in hdr and "kWRangeThreads = 256;" in hdr and "kWRangePer = 4;" in hdr and A.WINDOW_RANGE_TILE == 256 * 4
    assert f"kWRangeLdsKeys = {A.WINDOW_RANGE_LDS_KEYS};" in hdr
    f = A.window_range_frame(-7, 0)
    assert (f.start_kind, f.start_i, f.start_f, f.end_kind) == (PREC, 7, 7.0, CUR)
    f = A.window_range_frame(A.UNBOUNDED_PRECEDING, 0.5)
    assert (f.start_kind, f.end_kind, f.end_i, f.end_f) == (UP, FOLL, 0, 0.5)
    f = A.window_range_frame((PREC, 0), A.UNBOUNDED_FOLLOWING)
    assert (f.start_kind, f.start_i, f.end_kind) == (PREC, 0, UF)
    f = A.window_range_frame(-(2 ** 63 - 1), 2 ** 62)
    assert (f.start_i, f.end_i) == (2 ** 63 - 1, 2 ** 62)


def frame(sk=UP, ek=CUR, si=0, ei=0, sf=0.0, ef=0.0):
    return A.rdf_window_range_frame(sk, ek, si, ei, sf, ef)


class Call:
    """One rdf_window_range_agg call over host buffers filled with 77, so that "nothing written" can be checked."""

    def __init__(self, nkeys_p=1, nkeys_o=1, nvalues=1, rows=5, calls=((A.WAGG_SUM, 0, None),), capacity=None, validity=True,
                 mem=A.MEM_HOST, vdtype=np.float64, kdtype=np.int64):
        self.cols = [A.HostArray.from_numpy(np.arange(rows, dtype=np.int64) % 3) for _ in range(nkeys_p)] + \
                    [A.HostArray.from_numpy((np.arange(rows) % 3).astype(kdtype)) for _ in range(nkeys_o)]
        self.arrs = [(A.rdf_array * 1)(c.c_struct()) for c in self.cols]
        keys = [A.rdf_sort_key(C.cast(a, C.POINTER(A.rdf_array)), None, A.rdf_sort_options(0, 0)) for a in self.arrs]
        self.pk = (A.rdf_sort_key * max(1, nkeys_p))(*keys[:nkeys_p])
        self.ok = (A.rdf_sort_key * max(1, nkeys_o))(*keys[nkeys_p:])
        self.np, self.no = nkeys_p, nkeys_o
        self.vcols = [A.HostArray.from_numpy(np.arange(rows).astype(vdtype)) for _ in range(nvalues)]
        self.varrs = [(A.rdf_array * 1)(c.c_struct()) for c in self.vcols]
        self.values = (C.POINTER(A.rdf_array) * max(1, nvalues))(*[C.cast(a, C.POINTER(A.rdf_array)) for a in self.varrs])
        self.nv = nvalues
        self.nchunks = 1
        self.calls = (A.rdf_window_range_call * max(1, len(calls)))(*[A.rdf_window_range_call(f, v, fr or frame()) for f, v, fr in calls])
        self.ncalls = len(calls)
        cap = rows if capacity is None else capacity
        self.bufs = [np.full(max(rows, 1) + 8, 77, dtype=np.int64) for _ in calls]
        self.vbufs = [np.full(16, 77, dtype=np.uint8) for _ in calls]
        vdt = A.F64 if vdtype == np.float64 else A.I64
        self.outs = (A.rdf_out * max(1, len(calls)))(*[
            A.rdf_out(b.ctypes.data, v.ctypes.data if validity else None, cap, -5, -5, A.window_agg_out_dtype(f, vdt), mem)
            for (f, _v, _fr), b, v in zip(calls, self.bufs, self.vbufs)])

    def run(self, so):
        return so.rdf_window_range_agg(self.pk if self.np else None, C.c_int32(self.np), self.ok if self.no else None, C.c_int32(self.no),
                                       self.values if self.nv else None, C.c_int32(self.nv), C.c_int64(self.nchunks),
                                       self.calls, C.c_int32(self.ncalls), self.outs)

    def untouched(self):
        return all((b == 77).all() for b in self.bufs) and all((v == 77).all() for v in self.vbufs)


def refused(so, call, status=BAD, says=None):
    assert call.run(so) == status, so.rdf_last_error()
    assert call.untouched()
    if says:
        assert says in so.rdf_last_error().decode()


def test_frames_are_checked_before_the_device(so):
    for kd in (np.int64, np.int32, np.float64):
        one = lambda **kw: Call(calls=((A.WAGG_SUM, 0, frame(**kw)),), kdtype=kd)
        refused(so, one(sk=UF, ek=UF))                                                   # a start of UNBOUNDED FOLLOWING
        refused(so, one(sk=UP, ek=UP))                                                   # an end of UNBOUNDED PRECEDING
        for sk, ek in ((CUR, PREC), (FOLL, CUR), (FOLL, PREC)):                          # start kind > end kind
            refused(so, one(sk=sk, ek=ek, si=1, ei=1, sf=1.0, ef=1.0))
        refused(so, one(sk=PREC, ek=PREC, si=1, ei=2, sf=1.0, ef=2.0))                   # 1 PRECEDING .. 2 PRECEDING
        refused(so, one(sk=FOLL, ek=FOLL, si=3, ei=2, sf=3.0, ef=2.0))                   # 3 FOLLOWING .. 2 FOLLOWING
        for kind in (-1, 5, 77):
            refused(so, one(sk=kind))                                                    # unknown kinds
            refused(so, one(ek=kind))
    refused(so, Call(calls=((A.WAGG_SUM, 0, frame(sk=PREC, si=-1)),)), says="negative")              # a negative integer offset
    refused(so, Call(calls=((A.WAGG_SUM, 0, frame(sk=CUR, ek=FOLL, ei=-1)),)), says="negative")
    refused(so, Call(calls=((A.WAGG_SUM, 0, frame(sk=PREC, si=-(2 ** 63))),), kdtype=np.int32), says="negative")
    for bad, says in ((-0.5, "negative"), (math.nan, "finite"), (math.inf, "finite"), (-math.inf, "finite")):
        refused(so, Call(calls=((A.WAGG_SUM, 0, frame(sk=PREC, sf=bad)),), kdtype=np.float64), says=says)   # Float64 offsets
        refused(so, Call(calls=((A.WAGG_SUM, 0, frame(sk=CUR, ek=FOLL, ef=bad)),), kdtype=np.float64), says=says)
    # MIN / MAX need an unbounded side
    for fn in (A.WAGG_MIN, A.WAGG_MAX):
        for fr in (frame(sk=PREC, ek=CUR, si=1), frame(sk=CUR, ek=CUR), frame(sk=PREC, ek=FOLL, si=1, ei=1), frame(sk=FOLL, ek=FOLL, si=1, ei=2)):
            refused(so, Call(calls=((fn, 0, fr),)), says=MINMAX)
        refused(so, Call(calls=((fn, 0, frame(sk=PREC, ek=CUR, sf=0.5)),), kdtype=np.float64), says=MINMAX)
    # what is allowed passes the checks (and then needs a device, or succeeds where there is one); the pair of the other key
    # type is not read
    ok = [frame(sk=PREC, ek=PREC, si=2, ei=1), frame(sk=FOLL, ek=FOLL, si=2, ei=5), frame(sk=CUR, ek=CUR), frame(sk=UP, ek=UF),
          frame(sk=PREC, ek=FOLL, si=2 ** 63 - 1, ei=2 ** 62), frame(sk=PREC, ek=CUR, si=7, sf=math.nan), frame(sk=PREC, ek=CUR, si=0)]
    for fr in ok:
        assert Call(calls=((A.WAGG_SUM, 0, fr),)).run(so) in (A.RDF_OK, A.RDF_DEVICE_ERROR), so.rdf_last_error()
    for fr in (frame(sk=PREC, ek=FOLL, sf=0.1, ef=1e300), frame(sk=PREC, ek=CUR, si=-3, sf=0.5)):
        assert Call(calls=((A.WAGG_SUM, 0, fr),), kdtype=np.float64).run(so) in (A.RDF_OK, A.RDF_DEVICE_ERROR), so.rdf_last_error()
    for fn, fr in ((A.WAGG_MIN, frame(sk=UP, ek=FOLL, ei=3)), (A.WAGG_MAX, frame(sk=PREC, ek=UF, si=3))):
        assert Call(calls=((fn, 0, fr),)).run(so) in (A.RDF_OK, A.RDF_DEVICE_ERROR), so.rdf_last_error()


def test_the_order_key_is_checked_before_the_device(so):
    refused(so, Call(nkeys_o=0))                               # exactly one order key
    refused(so, Call(nkeys_o=2))
    for kd in (np.int8, np.int16, np.uint32, np.uint64, np.float32):
        refused(so, Call(kdtype=kd), says="Int32, Int64 or Float64")
    c = Call()
    words = A.HostUtf8.from_pylist(["a", "b", "c", "d", "e"])
    uarr = (A.rdf_utf8_array * 1)(words.c_struct())
    c.ok[0] = A.rdf_sort_key(None, C.cast(uarr, C.POINTER(A.rdf_utf8_array)), A.rdf_sort_options(0, 0))
    refused(so, c, says="numeric")                             # a Utf8 order key
    c = Call()
    c.ok[0].values = None
    refused(so, c)
    assert Call(nkeys_p=0).run(so) in (A.RDF_OK, A.RDF_DEVICE_ERROR)       # no partition keys is fine


def test_calls_and_values_are_checked_before_the_device(so):
    c = Call()
    c.ncalls = 0
    refused(so, c)                                             # no calls
    refused(so, Call(calls=((A.WAGG_COUNT, 0, None),) * 9))    # more than 8
    for fn in (-1, 7, 100):
        c = Call()
        c.calls[0].fn = fn
        refused(so, c)                                         # unknown function
    for fn in (A.WAGG_SUM, A.WAGG_MIN, A.WAGG_MAX, A.WAGG_AVG):
        refused(so, Call(calls=((fn, -1, None),)))             # these read values
        refused(so, Call(calls=((fn, 1, None),)))              # out of range
        refused(so, Call(calls=((fn, -2, None),)))
    refused(so, Call(calls=((A.WAGG_COUNT, 1, None),)))
    refused(so, Call(nvalues=5))                               # more than 4 value columns
    c = Call()
    c.nv = -1
    refused(so, c)
    for dt in (A.I32, A.U64, A.F32, A.BOOL):
        c = Call()
        c.varrs[0][0].dtype = dt                               # Int64 or Float64 only
        refused(so, c)
    for fn, dt in ((A.WAGG_SUM, A.I64), (A.WAGG_COUNT, A.F64), (A.WAGG_AVG, A.I64), (A.WAGG_FIRST_VALUE, A.I64)):
        c = Call(calls=((fn, 0, None),))
        c.outs[0].dtype = dt
        refused(so, c)                                         # wrong output dtype
    for fn in (A.WAGG_SUM, A.WAGG_MIN, A.WAGG_MAX, A.WAGG_AVG, A.WAGG_FIRST_VALUE, A.WAGG_LAST_VALUE):
        refused(so, Call(calls=((fn, 0, None),), validity=False))   # the result can be NULL: the bitmap is required
    c = Call()
    c.outs[0].values = None                                    # a capacity without a buffer
    refused(so, c)
    c = Call()
    assert so.rdf_window_range_agg(c.pk, C.c_int32(1), c.ok, C.c_int32(1), c.values, C.c_int32(1), C.c_int64(1), None, C.c_int32(1), c.outs) == BAD
    assert so.rdf_window_range_agg(c.pk, C.c_int32(1), c.ok, C.c_int32(1), c.values, C.c_int32(1), C.c_int64(1), c.calls, C.c_int32(1), None) == BAD
    assert so.rdf_window_range_agg(c.pk, C.c_int32(1), c.ok, C.c_int32(1), None, C.c_int32(1), C.c_int64(1), c.calls, C.c_int32(1), c.outs) == BAD
    assert so.rdf_window_range_agg(c.pk, C.c_int32(1), None, C.c_int32(1), c.values, C.c_int32(1), C.c_int64(1), c.calls, C.c_int32(1), c.outs) == BAD


def test_keys_and_memory_kinds_are_checked_as_rdf_window_checks_them(so):
    refused(so, Call(nkeys_p=5))
    c = Call()
    c.pk[0].values = None
    refused(so, c)
    c = Call()
    c.nchunks = 0
    refused(so, c)
    c = Call()
    c.arrs[0][0].dtype = A.BOOL
    refused(so, c)
    c = Call()
    c.varrs[0][0].mem = A.MEM_DEVICE                           # mixed memory kinds between keys and values
    refused(so, c)
    refused(so, Call(mem=A.MEM_DEVICE))                        # ... and between inputs and outputs
    c = Call()
    c.varrs[0][0].length = 4                                   # the value chunk's rows differ from the keys'
    refused(so, c, A.RDF_COMPUTE_ERROR)


def test_short_capacities_report_the_rows_and_write_nothing(so):
    for cap in (4, 0):
        c = Call(calls=((A.WAGG_SUM, 0, frame(sk=PREC, si=1)), (A.WAGG_COUNT, -1, None), (A.WAGG_LAST_VALUE, -1, None)), capacity=cap)
        c.outs[0].capacity = 5                                 # one short output is enough
        refused(so, c, A.RDF_MEMORY_ERROR)
        assert [c.outs[i].length for i in range(3)] == [5, 5, 5]


def test_zero_rows_is_a_valid_call_that_writes_nothing(so):
    c = Call(rows=0, calls=((A.WAGG_SUM, 0, frame(sk=PREC, si=7)), (A.WAGG_COUNT, 0, None)))
    assert c.run(so) == A.RDF_OK
    assert c.untouched() and [c.outs[i].length for i in range(2)] == [0, 0] and c.outs[0].null_count == 0
    key = [A.HostArray.from_numpy(np.zeros(0, dtype=np.int32))]
    got = lib.api().window_range_agg([], [key], [], [("count", -1, (-1, 1))])
    assert got[0][0].shape == (0,)


def test_rdf_window_agg_still_refuses_range_offsets(so):
    import test_window_agg_abi as W
    so.rdf_window_agg.restype = C.c_int
    W.refused(so, W.Call(calls=((A.WAGG_SUM, 0, W.frame(unit=A.FRAME_RANGE, sk=PREC, ek=CUR, start=1)),)), says="range offsets are not built")


def test_the_route_option_is_known():
    for v in (1, 2, 0):
        lib.set_option("window_range_route", v)


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error_for_valid_calls(so):
    api = lib.api()
    p = [A.HostUtf8.from_pylist(["b", None, "a"])]
    d = [A.HostArray.from_numpy(np.array([19000, 19003, 19001], dtype=np.int32))]
    t = [A.HostArray.from_numpy(np.array([0.5, -0.0, np.nan]), np.array([True, False, True]))]
    x = [A.HostArray.from_numpy(np.array([3, 2, 1], dtype=np.int64))]
    calls = [lambda: api.window_range_agg([p], [d], [x], [("sum", 0, (-7, 0))]),
             lambda: api.window_range_agg([], [(t, True)], [x, t], [("min", 0, (A.UNBOUNDED_PRECEDING, 0.5)), ("avg", 1, (-0.5, 0.5)), ("count", -1, (0, 0))]),
             lambda: api.window_range_agg([p], [d], [], [("first_value", -1, (1, 2))])]
    for call in calls:
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
        assert "no CPU fallback" in ei.value.message
