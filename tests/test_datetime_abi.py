"""rdf_datetime_fields / rdf_datetime_trunc / rdf_date_shift / rdf_date_diff at the C-ABI boundary, without a GPU: the four
symbols are exported and listed, the enum mirrors match the header, every refusal the header lists is a value returned
before any device work with nothing written, zero chunks is RDF_OK, and with no device a valid call fails loudly with
RDF_DEVICE_ERROR."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, MEMORY, COMPUTE = A.RDF_INVALID_ARGUMENT, A.RDF_MEMORY_ERROR, A.RDF_COMPUTE_ERROR
NAMES = ["rdf_datetime_fields", "rdf_datetime_trunc", "rdf_date_shift", "rdf_date_diff"]


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    for n in NAMES:
        getattr(s, n).restype = C.c_int
    return s


@pytest.fixture(scope="module")
def api():
    return lib.api()


def test_the_symbols_are_exported():
    s = lib.load()
    for n in NAMES:
        assert hasattr(s, n) and n in lib.EXPORTS


def test_the_enum_mirrors_match_the_header():
    prog = r'''
#include <stdio.h>
#include "rdf_mi355x.h"
int main(void) {
  rdf_datetime_field f = RDF_DT_DATE; rdf_trunc_level l = RDF_TRUNC_SECOND; rdf_date_shift_op o = RDF_SHIFT_NEXT_DAY;
  printf("fields %d %d %d %d %d %d %d %d %d %d %d\n", RDF_DT_YEAR, RDF_DT_QUARTER, RDF_DT_MONTH, RDF_DT_DAY_OF_MONTH, RDF_DT_DAY_OF_WEEK,
         RDF_DT_DAY_OF_YEAR, RDF_DT_WEEK_OF_YEAR, RDF_DT_HOUR, RDF_DT_MINUTE, RDF_DT_SECOND, (int)f);
  printf("levels %d %d %d %d %d %d %d %d\n", RDF_TRUNC_YEAR, RDF_TRUNC_QUARTER, RDF_TRUNC_MONTH, RDF_TRUNC_WEEK, RDF_TRUNC_DAY,
         RDF_TRUNC_HOUR, RDF_TRUNC_MINUTE, (int)l);
  printf("shifts %d %d %d %d\n", RDF_SHIFT_DAYS, RDF_SHIFT_MONTHS, RDF_SHIFT_LAST_DAY, (int)o);
  printf("units %d %d %d %d %d\n", RDF_TIME_SECOND, RDF_TIME_MILLISECOND, RDF_TIME_MICROSECOND, RDF_TIME_NANOSECOND, RDF_TIME_DAY);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        lines = subprocess.check_output([exe], text=True).splitlines()
    names = ["year", "quarter", "month", "day_of_month", "day_of_week", "day_of_year", "week_of_year", "hour", "minute", "second", "date"]
    assert lines[0] == "fields " + " ".join(str(A.DT_FIELDS[n]) for n in names) and len(A.DT_FIELDS) == 11
    levels = ["year", "quarter", "month", "week", "day", "hour", "minute", "second"]
    assert lines[1] == "levels " + " ".join(str(A.TRUNC_LEVELS[n]) for n in levels) and len(A.TRUNC_LEVELS) == 8
    assert lines[2] == "shifts " + " ".join(str(A.DATE_SHIFTS[n]) for n in ["days", "months", "last_day", "next_day"]) and len(A.DATE_SHIFTS) == 4
    assert lines[3] == "units " + " ".join(str(u) for u in (A.TIME_SECOND, A.TIME_MILLISECOND, A.TIME_MICROSECOND, A.TIME_NANOSECOND, A.TIME_DAY))


def arr(chunks):
    return (A.rdf_array * len(chunks))(*[x.c_struct() for x in chunks])


class Outs:
    """Output chunks whose every byte (buffers and descriptors) can be compared before and after a refused call."""

    def __init__(self, dtype, lens, validity=True, nout=1):
        self.arrays = [A.HostArray.empty_out(dtype, n, validity) for _ in range(nout) for n in lens]
        for a in self.arrays:
            a.values[:] = 77
            if a.validity is not None:
                a.validity[:] = 0x5A
        self.c = (A.rdf_out * len(self.arrays))(*[a.out_struct() for a in self.arrays])
        for o in self.c:
            o.length, o.null_count = -5, -6
        self.before = self.snapshot()

    def snapshot(self):
        return [(a.values.tobytes(), None if a.validity is None else a.validity.tobytes(), o.length, o.null_count) for a, o in zip(self.arrays, self.c)]

    def untouched(self):
        return self.snapshot() == self.before


def test_argument_errors_come_back_before_the_device(so):
    x64 = [A.HostArray.from_numpy(np.arange(5, dtype=np.int64)), A.HostArray.from_numpy(np.arange(3, dtype=np.int64))]
    x32 = [A.HostArray.from_numpy(np.arange(5, dtype=np.int32)), A.HostArray.from_numpy(np.arange(3, dtype=np.int32))]
    xf = [A.HostArray.from_numpy(np.arange(5.0)), A.HostArray.from_numpy(np.arange(3.0))]
    xn = [A.HostArray.from_numpy(np.arange(5, dtype=np.int64), valid=[1, 0, 1, 1, 1]), A.HostArray.from_numpy(np.arange(3, dtype=np.int64))]
    k32 = [A.HostArray.from_numpy(np.arange(1, 6, dtype=np.int32)), A.HostArray.from_numpy(np.arange(1, 4, dtype=np.int32))]
    kn = [A.HostArray.from_numpy(np.arange(1, 6, dtype=np.int32), valid=[1, 1, 0, 1, 1]), A.HostArray.from_numpy(np.arange(1, 4, dtype=np.int32))]
    c64, c32, cf, cn, ck, ckn = arr(x64), arr(x32), arr(xf), arr(xn), arr(k32), arr(kn)
    swapped, kswapped, mixed = arr(x64[::-1]), arr(k32[::-1]), arr([x64[0], x32[1]])
    n, S, DAY = C.c_int64(2), C.c_int32(A.TIME_SECOND), C.c_int32(A.TIME_DAY)
    lens = [5, 3]
    o32, o64, o32x2, plain32 = Outs(A.I32, lens), Outs(A.I64, lens), Outs(A.I32, lens, nout=2), Outs(A.I32, lens, validity=False)
    small = Outs(A.I32, [4, 3])
    one = (C.c_int32 * 8)(A.DT_YEAR, A.DT_MONTH, 0, 0, 0, 0, 0, 0)
    nine = (C.c_int32 * 9)(*range(9))
    results = []

    def refused(status, want, text=None):
        results.append(status)
        assert status == want, (status, so.rdf_last_error())
        if text:
            assert text in so.rdf_last_error().decode(), so.rdf_last_error()

    fields = lambda a, unit, f, nf, o, nch=n: so.rdf_datetime_fields(a, nch, unit, f, C.c_int32(nf), o)
    trunc = lambda a, unit, level, o, nch=n: so.rdf_datetime_trunc(a, nch, unit, C.c_int32(level), o)
    shift = lambda a, unit, op, k, amount, o, nch=n: so.rdf_date_shift(a, nch, unit, C.c_int32(op), k, C.c_int32(amount), o)
    diff = lambda a, ua, b, ub, o, nch=n: so.rdf_date_diff(a, ua, b, ub, nch, o)

    # an unknown unit, field, level or operation
    for bad_unit in (-1, 5, 100):
        u = C.c_int32(bad_unit)
        refused(fields(c64, u, one, 1, o32.c), BAD, "unit")
        refused(trunc(c64, u, A.TRUNC_MONTH, o64.c), BAD, "unit")
        refused(shift(c64, u, A.SHIFT_DAYS, None, 1, o32.c), BAD, "unit")
        refused(diff(c64, u, c64, S, o32.c), BAD, "unit")
        refused(diff(c64, S, c64, u, o32.c), BAD, "unit")
    for bad_field in (-1, 11, 99):
        refused(fields(c64, S, (C.c_int32 * 1)(bad_field), 1, o32.c), BAD, "field")
    for bad_level in (-1, 8):
        refused(trunc(c64, S, bad_level, o64.c), BAD, "level")
    for bad_op in (-1, 4):
        refused(shift(c64, S, bad_op, None, 1, o32.c), BAD, "operation")
    # nfields outside 1..8, a NULL field list, a repeated field
    refused(fields(c64, S, one, 0, o32.c), BAD)
    refused(fields(c64, S, nine, 9, o32.c), BAD)
    refused(fields(c64, S, None, 1, o32.c), BAD)
    refused(fields(c64, S, (C.c_int32 * 2)(A.DT_YEAR, A.DT_YEAR), 2, o32x2.c), BAD, "repeats")
    # a NULL list with nchunks > 0, negative nchunks
    neg = C.c_int64(-1)
    refused(fields(None, S, one, 1, o32.c), BAD)
    refused(fields(c64, S, one, 1, None), BAD)
    refused(fields(c64, S, one, 1, o32.c, neg), BAD)
    refused(trunc(None, S, A.TRUNC_DAY, o64.c), BAD)
    refused(trunc(c64, S, A.TRUNC_DAY, None), BAD)
    refused(trunc(c64, S, A.TRUNC_DAY, o64.c, neg), BAD)
    refused(shift(None, S, A.SHIFT_DAYS, None, 1, o32.c), BAD)
    refused(shift(c64, S, A.SHIFT_DAYS, None, 1, None), BAD)
    refused(shift(c64, S, A.SHIFT_DAYS, None, 1, o32.c, neg), BAD)
    refused(diff(None, S, c64, S, o32.c), BAD)
    refused(diff(c64, S, None, S, o32.c), BAD)
    refused(diff(c64, S, c64, S, None), BAD)
    refused(diff(c64, S, c64, S, o32.c, neg), BAD)
    # a level finer than the unit; last_day with amounts; a scalar weekday outside 1..7; per-row weekdays without an output bitmap
    for level in (A.TRUNC_HOUR, A.TRUNC_MINUTE, A.TRUNC_SECOND):
        refused(trunc(c32, DAY, level, o32.c), BAD, "finer")
    refused(shift(c64, S, A.SHIFT_LAST_DAY, ck, 0, o32.c), BAD, "last_day")
    for wd in (0, 8, -1):
        refused(shift(c64, S, A.SHIFT_NEXT_DAY, None, wd, o32.c), BAD, "weekday")
    refused(shift(c64, S, A.SHIFT_NEXT_DAY, ck, 0, plain32.c), BAD, "validity")
    # chunk lengths that differ between paired columns; amounts that are not Int32
    refused(shift(c64, S, A.SHIFT_DAYS, kswapped, 0, o32.c), BAD, "lengths differ")
    refused(diff(c64, S, swapped, S, o32.c), BAD, "lengths differ")
    refused(shift(c64, S, A.SHIFT_DAYS, c64, 0, o32.c), BAD, "Int32")
    # two memory kinds in one call (inputs against inputs, outputs against inputs)
    dev = arr(k32)
    dev[0].mem = dev[1].mem = A.MEM_DEVICE
    refused(shift(c64, S, A.SHIFT_DAYS, dev, 0, o32.c), BAD, "memory space")
    dev64 = arr(x64)
    dev64[0].mem = dev64[1].mem = A.MEM_DEVICE
    refused(diff(c64, S, dev64, S, o32.c), BAD, "memory space")
    refused(fields(dev64, S, one, 1, o32.c), BAD, "memory space")
    # an input with validity but an output without
    refused(fields(cn, S, one, 1, plain32.c), BAD, "validity")
    refused(trunc(cn, S, A.TRUNC_DAY, Outs(A.I64, lens, validity=False).c), BAD, "validity")
    refused(shift(c64, S, A.SHIFT_DAYS, ckn, 0, plain32.c), BAD, "validity")
    refused(diff(c64, S, cn, S, plain32.c), BAD, "validity")
    # an output of the wrong dtype, too small a capacity
    refused(fields(c64, S, one, 1, o64.c), BAD, "dtype")
    refused(trunc(c64, S, A.TRUNC_DAY, o32.c), BAD, "dtype")
    refused(trunc(c32, S, A.TRUNC_DAY, o64.c), BAD, "dtype")
    refused(shift(c64, S, A.SHIFT_MONTHS, None, 1, o64.c), BAD, "dtype")
    refused(diff(c64, S, c32, S, o64.c), BAD, "dtype")
    refused(fields(c64, S, one, 1, small.c), MEMORY, "capacity")
    refused(shift(c64, S, A.SHIFT_MONTHS, None, 1, small.c), MEMORY, "capacity")
    refused(diff(c64, S, c32, DAY, small.c), MEMORY, "capacity")
    # storage that is not Int32 / Int64; Int64 with RDF_TIME_DAY; chunks of two storage types
    refused(fields(cf, S, one, 1, o32.c), COMPUTE, "does not support type")
    refused(trunc(cf, S, A.TRUNC_DAY, Outs(A.F64, lens).c), COMPUTE, "does not support type")
    refused(shift(cf, S, A.SHIFT_DAYS, None, 1, o32.c), COMPUTE, "does not support type")
    refused(diff(c64, S, cf, S, o32.c), COMPUTE, "does not support type")
    refused(fields(c64, DAY, one, 1, o32.c), BAD, "Int32 day numbers")
    refused(diff(c32, DAY, c64, DAY, o32.c), BAD, "Int32 day numbers")
    refused(fields(mixed, S, one, 1, o32.c), BAD, "one storage type")
    assert len(results) > 60
    for o in (o32, o64, o32x2, plain32, small):                  # nothing was written by any refused call
        assert o.untouched()


def test_zero_chunks_are_ok(so, api):
    zero, S = C.c_int64(0), C.c_int32(A.TIME_SECOND)
    one = (C.c_int32 * 1)(A.DT_YEAR)
    assert so.rdf_datetime_fields(None, zero, S, one, C.c_int32(1), None) == A.RDF_OK
    assert so.rdf_datetime_trunc(None, zero, S, C.c_int32(A.TRUNC_WEEK), None) == A.RDF_OK
    assert so.rdf_date_shift(None, zero, S, C.c_int32(A.SHIFT_MONTHS), None, C.c_int32(3), None) == A.RDF_OK
    assert so.rdf_date_diff(None, S, None, S, zero, None) == A.RDF_OK
    assert so.rdf_datetime_fields(None, zero, C.c_int32(9), one, C.c_int32(1), None) == BAD        # the enums are checked first
    # chunks without rows: lengths and NULL counts are set, no device is needed
    empty = [A.HostArray.from_numpy(np.zeros(0, dtype=np.int64)), A.HostArray.from_numpy(np.zeros(0, dtype=np.int64), valid=np.zeros(0, dtype=bool))]
    for outs in (api.datetime_fields(empty, A.TIME_NANOSECOND, ["year", "hour"]), [api.datetime_trunc(empty, A.TIME_NANOSECOND, "month")],
                 [api.date_shift(empty, A.TIME_NANOSECOND, "months", 1)], [api.date_diff(empty, A.TIME_NANOSECOND, empty, A.TIME_SECOND)]):
        assert all(o.length == 0 and o.null_count == 0 for per in outs for o in per)


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error_for_valid_calls(api):
    x = [A.HostArray.from_numpy(np.array([1, 2, 4], dtype=np.int64), valid=[1, 0, 1])]
    d = [A.HostArray.from_numpy(np.array([3, 2, 1], dtype=np.int32))]
    for call in (lambda: api.datetime_fields(x, A.TIME_MILLISECOND, ["year", "month", "day_of_month"]), lambda: api.datetime_fields(d, A.TIME_DAY, ["week_of_year"]),
                 lambda: api.datetime_trunc(x, A.TIME_MICROSECOND, "week"), lambda: api.datetime_trunc(d, A.TIME_DAY, "quarter"),
                 lambda: api.date_shift(x, A.TIME_SECOND, "months", -2), lambda: api.date_shift(d, A.TIME_DAY, "next_day", d),
                 lambda: api.date_shift(d, A.TIME_DAY, "last_day"), lambda: api.date_diff(x, A.TIME_NANOSECOND, d, A.TIME_DAY)):
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
        assert "no CPU fallback" in ei.value.message
