"""rdf_member_mask / rdf_first_occurrence without a GPU: every refusal the header lists comes back before any device work,
with its status and message, and `length` / *out_rows are what the header says even then (on a machine without a device
RDF_DEVICE_ERROR would otherwise mask a check that runs too late)."""
import ctypes as C

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib


@pytest.fixture(autouse=True)
def _default_options():
    yield
    lib.set_option("member_route", 0)
    lib.set_option("member_slots", 0)
    lib.set_option("member_table_bits", 0)


def num(values, dtype=np.int64, valid=None):
    return A.HostArray.from_numpy(np.asarray(values, dtype=dtype), valid)


def text(rows):
    return A.HostUtf8.from_pylist(rows)


def refused(call, status, words):
    with pytest.raises(A.RdfError) as ei:
        call()
    assert ei.value.status == status, ei.value
    assert words in ei.value.message, ei.value.message


def raw_member(lk, lnc, rk, rnc, nk, kind, outs, rows):
    fn = lib.load().rdf_member_mask
    fn.restype = C.c_int
    return fn(lk, C.c_int64(lnc), rk, C.c_int64(rnc), C.c_int32(nk), C.c_int32(kind), outs, rows)


def test_member_mask_refusals_need_no_device():
    api = lib.api()
    L, R = [num([1, 2, 3])], [num([2])]
    refused(lambda: api.member_mask([L], [R], 7), A.RDF_INVALID_ARGUMENT, "bad kind")
    refused(lambda: api.member_mask([L], [R], -1), A.RDF_INVALID_ARGUMENT, "bad kind")
    refused(lambda: api.member_mask([L] * 5, [R] * 5, "semi"), A.RDF_INVALID_ARGUMENT, "1 to 4 key columns")
    refused(lambda: api.member_mask([L, L], [R, R], "is_in"), A.RDF_INVALID_ARGUMENT, "IS_IN takes one key column")
    refused(lambda: api.member_mask([L], [[num([2], np.int32)]], "semi"), A.RDF_INVALID_ARGUMENT, "share one dtype")
    refused(lambda: api.member_mask([L], [[text(["a"])]], "semi"), A.RDF_INVALID_ARGUMENT, "a Utf8 key pairs with a Utf8 key only")
    refused(lambda: api.member_mask([[num([1]), num([2], np.int32)]], [R + R], "semi"), A.RDF_INVALID_ARGUMENT, "chunks of one dtype")
    refused(lambda: api.member_mask([L, [num([1, 2])]], [R, R], "semi"), A.RDF_COMPUTE_ERROR, "differ in their chunks' rows")
    refused(lambda: api.member_mask([L, L], [R, [num([2, 3])]], "anti"), A.RDF_COMPUTE_ERROR, "differ in their chunks' rows")
    # mixed memory kinds
    dev = A.DeviceArray(64, None, 0, 1, A.I64, 0)
    refused(lambda: api.member_mask([L], [[dev]], "semi", count_only=True), A.RDF_INVALID_ARGUMENT, "one memory space")
    # outputs: dtype, buffer, validity (IS_IN), memory kind
    bad = [A.HostArray.empty_out(A.U8, 3, False)]
    refused(lambda: api.member_mask([L], [R], "semi", outs=bad), A.RDF_INVALID_ARGUMENT, "the mask is Boolean")
    refused(lambda: api.member_mask([L], [R], "is_in", outs=[A.HostArray.empty_out(A.BOOL, 3, False)]), A.RDF_INVALID_ARGUMENT, "validity buffer required")
    # forcing the LDS form on a call it cannot serve: tuples, or more build rows than its capacity
    lib.set_option("member_route", 1)
    refused(lambda: api.member_mask([L, L], [R, R], "semi"), A.RDF_INVALID_ARGUMENT, "LDS route")
    lib.set_option("member_slots", 64)
    refused(lambda: api.member_mask([L], [[num(np.arange(33))]], "semi"), A.RDF_INVALID_ARGUMENT, "at most 32 build rows")
    lib.set_option("member_route", 0)
    # null pointers and chunk counts
    rows = C.c_int64(-5)
    lk, keep = A.Api._sort_keys([L])
    assert raw_member(None, 1, lk, 1, 1, 0, None, C.byref(rows)) == A.RDF_INVALID_ARGUMENT
    assert raw_member(lk, 1, None, 1, 1, 0, None, C.byref(rows)) == A.RDF_INVALID_ARGUMENT
    assert raw_member(lk, 0, lk, 1, 1, 0, None, C.byref(rows)) == A.RDF_INVALID_ARGUMENT
    assert raw_member(lk, 1, lk, 1, 1, 0, None, None) == A.RDF_INVALID_ARGUMENT
    assert rows.value == -5                                   # nothing is written through a call that has no place to write
    both = (A.rdf_sort_key * 1)(lk[0])
    both[0].utf8 = C.cast(C.pointer(text(["a"]).c_struct()), C.POINTER(A.rdf_utf8_array))
    assert raw_member(both, 1, lk, 1, 1, 0, None, C.byref(rows)) == A.RDF_INVALID_ARGUMENT
    assert b"exactly one of values / utf8" in lib.load().rdf_last_error() and rows.value == 0


def test_out_rows_and_lengths_of_refused_calls():
    api = lib.api()
    L = [num([1, 2, 3]), num([4, 5])]
    R = [num([2])]
    # a refusal sets *out_rows = 0
    rows = C.c_int64(-5)
    lk, k1 = A.Api._sort_keys([L])
    rk, k2 = A.Api._sort_keys([R])
    assert raw_member(lk, 2, rk, 1, 1, 9, None, C.byref(rows)) == A.RDF_INVALID_ARGUMENT and rows.value == 0
    # a short capacity: RDF_MEMORY_ERROR before the device, every length set, nothing written
    outs = [A.HostArray.empty_out(A.BOOL, 3, True), A.HostArray.empty_out(A.BOOL, 1, True)]
    for o in outs:
        o.values[:] = 0xA5
        o.validity[:] = 0x5A
    with pytest.raises(A.RdfError) as ei:
        api.member_mask([L], [R], "is_in", outs=outs)
    assert ei.value.status == A.RDF_MEMORY_ERROR and "shorter than its chunk" in ei.value.message
    assert [o.length for o in outs] == [3, 2] and api.last_out_rows == 0
    assert all((o.values == 0xA5).all() and (o.validity == 0x5A).all() for o in outs)
    outs = [A.HostArray.empty_out(A.BOOL, 3, False), A.HostArray.empty_out(A.BOOL, 1, False)]
    with pytest.raises(A.RdfError) as ei:
        api.first_occurrence([L], "last", outs=outs)
    assert ei.value.status == A.RDF_MEMORY_ERROR and [o.length for o in outs] == [3, 2] and api.last_out_rows == 0


def test_first_occurrence_refusals_need_no_device():
    api = lib.api()
    K = [num([1, 1, 2])]
    refused(lambda: api.first_occurrence([K], 3), A.RDF_INVALID_ARGUMENT, "bad keep")
    refused(lambda: api.first_occurrence([K] * 5, "first"), A.RDF_INVALID_ARGUMENT, "1 to 4 key columns")
    refused(lambda: api.first_occurrence([K, [text(["a", "b"])]], "first"), A.RDF_COMPUTE_ERROR, "differ in their chunks' rows")
    refused(lambda: api.first_occurrence([K], "first", outs=[A.HostArray.empty_out(A.I32, 3, False)]), A.RDF_INVALID_ARGUMENT, "the mask is Boolean")
    bad_offsets = text(["a", "b", "c"])
    bad_offsets.offsets = bad_offsets.offsets.astype(np.int64)
    st = bad_offsets.c_struct()
    st.offsets.dtype = A.I64
    ck = (A.rdf_sort_key * 1)()
    ck[0].utf8 = C.cast(C.pointer(st), C.POINTER(A.rdf_utf8_array))
    fn = lib.load().rdf_first_occurrence
    fn.restype = C.c_int
    rows = C.c_int64(-1)
    assert fn(ck, C.c_int32(1), C.c_int64(1), C.c_int32(0), None, C.byref(rows)) == A.RDF_INVALID_ARGUMENT
    assert b"Int32 array of rows + 1" in lib.load().rdf_last_error() and rows.value == 0
    # "member_route" is rdf_member_mask's: a forced LDS form does not refuse this call's arguments
    lib.set_option("member_route", 1)
    refused(lambda: api.first_occurrence([K], 3), A.RDF_INVALID_ARGUMENT, "bad keep")


def test_zero_left_rows_need_no_device():
    api = lib.api()
    outs, rows = api.member_mask([[num([])]], [[num([1, 2])]], "anti")
    assert rows == 0 and [o.length for o in outs] == [0] and outs[0].null_count == 0
    assert api.member_mask([[text([])]], [[text(["a"])]], "semi", count_only=True) == 0
    outs, rows = api.first_occurrence([[num([]), num([])]], "none")
    assert rows == 0 and [o.length for o in outs] == [0, 0]


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_valid_calls_fail_loudly_without_a_gpu():
    api = lib.api()
    for call in (lambda: api.member_mask([[num([1, 2])]], [[num([2])]], "semi"), lambda: api.first_occurrence([[num([1, 1])]], "first")):
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR and "no CPU fallback" in ei.value.message


def test_unknown_option_values_fall_back():
    lib.set_option("member_route", 9)        # not a route: planned
    lib.set_option("member_table_bits", 99)  # clamped
    lib.set_option("member_slots", -1)
    api = lib.api()
    assert api.member_mask([[num([])]], [[num([1])]], "semi", count_only=True) == 0
