"""rdf_null_test / rdf_coalesce / rdf_case_when / rdf_extremum / rdf_nanvl / rdf_utf8_coalesce / rdf_utf8_case_when at the C-ABI
boundary, without a GPU: the seven symbols
are exported and listed, rdf_value_part and the enum have the header's layout, every refusal the header lists comes back in
the header's order before any device work with nothing written (the outputs sit in guard bytes; a short capacity sets the
lengths and nothing else), zero chunks is RDF_OK, and with no device a valid call fails loudly with RDF_DEVICE_ERROR."""
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
NAMES = ["rdf_null_test", "rdf_coalesce", "rdf_case_when", "rdf_extremum", "rdf_nanvl", "rdf_utf8_coalesce", "rdf_utf8_case_when"]


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


def test_the_part_struct_and_the_enum_match_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rdf_mi355x.h"
int main(void) {
  rdf_null_test_op o = RDF_IS_NAN;
  printf("part %zu %zu %zu %zu\n", sizeof(rdf_value_part), offsetof(rdf_value_part, column), offsetof(rdf_value_part, literal_bits), offsetof(rdf_value_part, literal_is_null));
  printf("tests %d %d %d max %d\n", RDF_IS_NULL, RDF_IS_NOT_NULL, (int)o, RDF_SELECT_PARTS_MAX);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        lines = subprocess.check_output([exe], text=True).splitlines()
    P = A.rdf_value_part
    assert lines[0] == f"part {C.sizeof(P)} {P.column.offset} {P.literal_bits.offset} {P.literal_is_null.offset}" == "part 24 0 8 16"
    assert lines[1] == f"tests {A.NULL_TESTS['is_null']} {A.NULL_TESTS['is_not_null']} {A.NULL_TESTS['is_nan']} max {A.SELECT_PARTS_MAX}" and len(A.NULL_TESTS) == 3


def arr(chunks):
    return (A.rdf_array * len(chunks))(*[x.c_struct() for x in chunks])


def part(chunks=None, literal=0, null=0):
    return A.rdf_value_part(None if chunks is None else C.cast(chunks, C.POINTER(A.rdf_array)), literal, null)


def parts(*ps):
    return (A.rdf_value_part * max(1, len(ps)))(*ps)


def cond_list(*cs):
    return (C.POINTER(A.rdf_array) * max(1, len(cs)))(*[C.cast(c, C.POINTER(A.rdf_array)) if c is not None else None for c in cs])


class Outs:
    """Output chunks between guard bytes whose every byte (buffers, guards and descriptors) can be compared before and after a refused call."""
    GUARD = 64

    def __init__(self, dtype, lens, validity=True, caps=None):
        g = self.GUARD
        self.bufs = []
        structs = []
        for n, cap in zip(lens, caps or lens):
            nbytes = max(cap, 1) * 8                                     # room for any dtype; BOOL values are bits
            v = np.full(g + nbytes + 16 + g, 0x4D, dtype=np.uint8)
            b = np.full(g + (cap + 63) // 64 * 8 + 8 + g, 0x5A, dtype=np.uint8) if validity else None
            self.bufs.append((v, b))
            structs.append(A.rdf_out(v.ctypes.data + g, b.ctypes.data + g if b is not None else None, cap, -5, -6, dtype, A.MEM_HOST))
        self.c = (A.rdf_out * len(structs))(*structs)
        self.before = self.snapshot()

    def snapshot(self, lengths=True):
        return [(v.tobytes(), None if b is None else b.tobytes(), o.length if lengths else None, o.null_count) for (v, b), o in zip(self.bufs, self.c)]

    def untouched(self):
        return self.snapshot() == self.before

    def only_lengths_set(self, lens):
        ok = self.snapshot(False) == [(v, b, None, nc) for v, b, _, nc in self.before] and [o.length for o in self.c] == list(lens)
        for o in self.c:
            o.length = -5
        return ok


def test_argument_errors_come_back_in_the_stated_order_before_the_device(so):
    lens = [5, 3]
    H = A.HostArray.from_numpy
    x64 = [H(np.arange(5, dtype=np.int64)), H(np.arange(3, dtype=np.int64))]
    x32 = [H(np.arange(5, dtype=np.int32)), H(np.arange(3, dtype=np.int32))]
    xf = [H(np.arange(5.0)), H(np.arange(3.0))]
    xn = [H(np.arange(5, dtype=np.int64), valid=[1, 0, 1, 1, 1]), H(np.arange(3, dtype=np.int64))]
    xfn = [H(np.arange(5.0), valid=[1, 0, 1, 1, 1]), H(np.arange(3.0), valid=[1, 1, 0])]
    xb = [H(np.array([1, 0, 1, 1, 0], dtype=bool)), H(np.array([1, 0, 1], dtype=bool))]
    xbn = [H(np.array([1, 0, 1, 1, 0], dtype=bool), valid=[1, 1, 0, 1, 1]), H(np.array([1, 0, 1], dtype=bool))]
    c64, c32, cf, cn, cfn, cb, cbn = arr(x64), arr(x32), arr(xf), arr(xn), arr(xfn), arr(xb), arr(xbn)
    swapped, bswapped, mixed = arr(x64[::-1]), arr(xb[::-1]), arr([x64[0], x32[1]])
    dev64 = arr(x64)
    dev64[0].mem = dev64[1].mem = A.MEM_DEVICE
    devb = arr(xb)
    devb[0].mem = devb[1].mem = A.MEM_DEVICE
    n, neg = C.c_int64(2), C.c_int64(-1)
    o64, o32, of, ob = Outs(A.I64, lens), Outs(A.I32, lens), Outs(A.F64, lens), Outs(A.BOOL, lens)
    plain64, plainf, obool_as_value = Outs(A.I64, lens, validity=False), Outs(A.F64, lens, validity=False), Outs(A.BOOL, lens)
    small64, smallf, smallb = Outs(A.I64, lens, caps=[4, 3]), Outs(A.F64, lens, caps=[5, 2]), Outs(A.BOOL, lens, caps=[4, 3])
    everything = [o64, o32, of, ob, plain64, plainf, obool_as_value, small64, smallf, smallb]
    results = []

    def refused(status, want, text=None):
        results.append(status)
        assert status == want, (status, want, so.rdf_last_error())
        if text:
            assert text in so.rdf_last_error().decode(), so.rdf_last_error()
        if want != MEMORY:
            assert all(o.untouched() for o in everything), so.rdf_last_error()

    test = lambda op, a, o, nch=n: so.rdf_null_test(C.c_int32(op), a, nch, o)
    coalesce = lambda p, k, o, nch=n: so.rdf_coalesce(p, C.c_int32(k), nch, o)
    when = lambda cs, vs, k, other, o, nch=n: so.rdf_case_when(cs, vs, C.c_int32(k), other, nch, o)
    extremum = lambda g, p, k, o, nch=n: so.rdf_extremum(C.c_int32(g), p, C.c_int32(k), nch, o)
    nanvl = lambda a, b, o, nch=n: so.rdf_nanvl(a, b, nch, o)
    two = parts(part(c64), part(cn))
    nine = parts(*[part(c64)] * 9)
    lit7 = parts(part(literal=7))
    conds1, conds2 = cond_list(cb), cond_list(cb, cbn)
    pf, pfn, plit = parts(part(cf)), parts(part(cfn)), parts(part(literal=0x405EC00000000000))

    # 1. an unknown test (first: every other argument is bad as well)
    for op in (-1, 3, 99):
        refused(test(op, None, None, neg), BAD, "unknown test")
    # 2. nparts / nbranches outside their range
    for k in (0, 9, -1):
        refused(coalesce(None, k, None, neg), BAD, "1 to 8 parts")
        refused(when(None, None, k, None, None, neg), BAD, "1 to 8 branches")
    for k in (0, 1, 9):
        refused(extremum(1, None, k, None, neg), BAD, "2 to 8 parts")
    refused(coalesce(nine, 9, o64.c), BAD, "parts")
    # 3. a NULL list with nchunks > 0, negative nchunks (before the parts are looked at: these have no column part)
    refused(test(A.IS_NULL, None, ob.c), BAD, "chunk lists")
    refused(test(A.IS_NULL, c64, None), BAD, "chunk lists")
    refused(test(A.IS_NULL, c64, ob.c, neg), BAD, "nchunks")
    refused(coalesce(None, 1, o64.c), BAD, "chunk lists")
    refused(coalesce(lit7, 1, None), BAD, "chunk lists")
    refused(coalesce(lit7, 1, o64.c, neg), BAD, "nchunks")
    refused(when(None, lit7, 1, None, o64.c), BAD, "chunk lists")
    refused(when(conds1, None, 1, None, o64.c), BAD, "chunk lists")
    refused(when(cond_list(None), lit7, 1, None, o64.c), BAD, "chunk lists")
    refused(when(conds1, lit7, 1, None, None), BAD, "chunk lists")
    refused(when(conds1, lit7, 1, None, o64.c, neg), BAD, "nchunks")
    refused(extremum(1, None, 2, o64.c), BAD, "chunk lists")
    refused(extremum(0, two, 2, None), BAD, "chunk lists")
    refused(nanvl(None, plit, of.c), BAD, "chunk lists")
    refused(nanvl(pf, None, of.c), BAD, "chunk lists")
    refused(nanvl(pf, plit, None), BAD, "chunk lists")
    refused(nanvl(pf, plit, of.c, neg), BAD, "nchunks")
    # 4. no column part (the conditions are not RDF_BOOL, the output has another dtype: reported later)
    refused(coalesce(parts(part(literal=1), part(null=1)), 2, o32.c), BAD, "no column part")
    refused(when(cond_list(c64), lit7, 1, lit7, o32.c), BAD, "no column part")
    refused(extremum(1, parts(part(literal=1), part(literal=2)), 2, o32.c), BAD, "no column part")
    refused(nanvl(plit, plit, o32.c), BAD, "no column part")
    # 5. a column part that also says it is the NULL literal (with conditions that are not RDF_BOOL)
    refused(coalesce(parts(part(c64), part(c64, null=1)), 2, o32.c), BAD, "NULL literal")
    refused(when(cond_list(c64), parts(part(c64, null=1)), 1, None, o32.c), BAD, "NULL literal")
    refused(when(conds1, lit7, 1, parts(part(c64, null=1)), o32.c), BAD, "NULL literal")
    refused(extremum(0, parts(part(c64, null=1), part(literal=2)), 2, o32.c), BAD, "NULL literal")
    refused(nanvl(pf, parts(part(cf, null=1)), o32.c), BAD, "NULL literal")
    # 8. a condition that is not RDF_BOOL (with value dtypes that differ)
    refused(when(cond_list(c64), parts(part(c64)), 1, parts(part(c32)), o64.c), BAD, "not RDF_BOOL")
    refused(when(cond_list(cb, cf), parts(part(c64), part(c32)), 2, None, o64.c), BAD, "not RDF_BOOL")
    # 9. value dtypes that differ from each other or from the output (with mixed memory kinds)
    refused(coalesce(parts(part(c64), part(c32)), 2, o64.c), BAD, "dtypes differ")
    refused(coalesce(parts(part(mixed)), 1, o64.c), BAD, "dtypes differ")
    refused(coalesce(parts(part(dev64), part(c32)), 2, o64.c), BAD, "dtypes differ")
    refused(coalesce(two, 2, o32.c), BAD, "output dtype")
    refused(when(conds1, parts(part(c64)), 1, parts(part(cf)), o64.c), BAD, "dtypes differ")
    refused(when(cond_list(devb), parts(part(c64)), 1, None, of.c), BAD, "output dtype")
    refused(extremum(1, parts(part(c64), part(cf)), 2, o64.c), BAD, "dtypes differ")
    refused(extremum(1, two, 2, of.c), BAD, "output dtype")
    refused(nanvl(pf, parts(part(c64)), of.c), BAD, "dtypes differ")
    refused(nanvl(pf, plit, o64.c), BAD, "output dtype")
    refused(test(A.IS_NULL, mixed, ob.c), BAD, "dtypes differ")
    refused(test(A.IS_NAN, cf, of.c), BAD, "output dtype")
    refused(test(A.IS_NOT_NULL, dev64, o64.c), BAD, "output dtype")
    # 10. mixed memory kinds: inputs against inputs, conditions against values, outputs against inputs (and no bitmap where one is required)
    refused(coalesce(parts(part(cn), part(dev64)), 2, plain64.c), BAD, "memory space")
    refused(when(cond_list(devb), parts(part(c64)), 1, None, plain64.c), BAD, "memory space")
    refused(extremum(1, parts(part(dev64), part(cn)), 2, plain64.c), BAD, "memory space")
    refused(coalesce(parts(part(dev64)), 1, o64.c), BAD, "memory space")
    refused(test(A.IS_NULL, dev64, ob.c), BAD, "memory space")
    devf = arr(xfn)
    devf[0].mem = devf[1].mem = A.MEM_DEVICE
    refused(nanvl(pfn, parts(part(devf)), plainf.c), BAD, "memory space")
    # 11. a missing required bitmap (with an unsupported dtype / differing row counts, reported later)
    refused(coalesce(parts(part(cn)), 1, plain64.c), BAD, "validity")
    refused(coalesce(parts(part(cn), part(null=1)), 2, plain64.c), BAD, "validity")
    refused(when(conds1, parts(part(c64)), 1, None, plain64.c), BAD, "validity")                       # no otherwise: NULL
    refused(when(conds1, lit7, 1, parts(part(cn)), plain64.c), BAD, "validity")
    refused(when(conds2, parts(part(cn), part(literal=1)), 2, lit7, plain64.c), BAD, "validity")
    refused(when(conds1, parts(part(null=1)), 1, parts(part(c64)), plain64.c), BAD, "validity")
    refused(extremum(1, parts(part(cn), part(cn)), 2, plain64.c), BAD, "validity")
    refused(extremum(0, parts(part(cn), part(null=1)), 2, plain64.c), BAD, "validity")
    refused(nanvl(pfn, plit, plainf.c), BAD, "validity")
    refused(nanvl(pf, pfn, plainf.c), BAD, "validity")
    refused(nanvl(pf, parts(part(null=1)), plainf.c), BAD, "validity")
    bool_plain = Outs(A.BOOL, lens, validity=False)
    everything.append(bool_plain)
    refused(coalesce(parts(part(cbn)), 1, bool_plain.c), BAD, "validity")                              # (Boolean values: refused under 12 once the bitmap is there)
    # 12. an unsupported dtype: Boolean-valued results, nanvl / is_nan of integers (with differing row counts)
    refused(coalesce(parts(part(cb), part(bswapped)), 2, obool_as_value.c), COMPUTE, "does not support type")
    refused(when(conds1, parts(part(cb)), 1, parts(part(cbn)), obool_as_value.c), COMPUTE, "does not support type")
    refused(extremum(1, parts(part(cb), part(bswapped)), 2, obool_as_value.c), COMPUTE, "does not support type")
    refused(nanvl(parts(part(c64)), parts(part(swapped)), o64.c), COMPUTE, "does not support type")
    refused(nanvl(parts(part(cb)), parts(part(literal=1)), obool_as_value.c), COMPUTE, "does not support type")
    refused(test(A.IS_NAN, c64, ob.c), COMPUTE, "does not support type")
    refused(test(A.IS_NAN, cb, ob.c), COMPUTE, "does not support type")
    # 13. chunk row counts that differ between parts or conditions (with too small a capacity)
    refused(coalesce(parts(part(cn), part(swapped)), 2, small64.c), COMPUTE, "row counts differ")
    refused(when(cond_list(bswapped), parts(part(c64)), 1, lit7, small64.c), COMPUTE, "row count differs")
    refused(when(conds1, parts(part(c64)), 1, parts(part(swapped)), small64.c), COMPUTE, "row counts differ")
    refused(extremum(0, parts(part(literal=1), part(c64), part(swapped)), 3, small64.c), COMPUTE, "row counts differ")
    refused(nanvl(pf, parts(part(arr(xf[::-1]))), smallf.c), COMPUTE, "row counts differ")
    # 14. a capacity below the rows: every length is set, nothing else is written
    refused(coalesce(two, 2, small64.c), MEMORY, "capacity")
    assert small64.only_lengths_set(lens)
    refused(when(conds1, parts(part(c64)), 1, lit7, small64.c), MEMORY, "capacity")
    assert small64.only_lengths_set(lens)
    refused(extremum(1, two, 2, small64.c), MEMORY, "capacity")
    assert small64.only_lengths_set(lens)
    refused(nanvl(pf, plit, smallf.c), MEMORY, "capacity")
    assert smallf.only_lengths_set(lens)
    refused(test(A.IS_NULL, cn, smallb.c), MEMORY, "capacity")
    assert smallb.only_lengths_set(lens)
    assert len(results) > 80
    assert all(o.untouched() for o in everything)


def test_zero_chunks_are_ok(so, api):
    zero = C.c_int64(0)
    assert so.rdf_null_test(C.c_int32(A.IS_NAN), None, zero, None) == A.RDF_OK
    assert so.rdf_coalesce(None, C.c_int32(3), zero, None) == A.RDF_OK
    assert so.rdf_case_when(None, None, C.c_int32(8), None, zero, None) == A.RDF_OK
    assert so.rdf_extremum(C.c_int32(1), None, C.c_int32(2), zero, None) == A.RDF_OK
    assert so.rdf_nanvl(None, None, zero, None) == A.RDF_OK
    assert so.rdf_null_test(C.c_int32(7), None, zero, None) == BAD                     # the test and the counts are checked first
    assert so.rdf_coalesce(None, C.c_int32(0), zero, None) == BAD
    assert so.rdf_extremum(C.c_int32(1), None, C.c_int32(1), zero, None) == BAD
    # chunks without rows: lengths and NULL counts are set, no device is needed
    e = [A.HostArray.from_numpy(np.zeros(0)), A.HostArray.from_numpy(np.zeros(0), valid=np.zeros(0, dtype=bool))]
    b = [A.HostArray.from_numpy(np.zeros(0, dtype=bool)), A.HostArray.from_numpy(np.zeros(0, dtype=bool))]
    for outs in (api.null_test("is_null", e), api.null_test("is_nan", e), api.coalesce([e, 1.0]), api.coalesce([e, e]), api.case_when([b], [e], 2.0),
                 api.case_when([b, b], [1.0, e], None), api.greatest([e, e, 3.0]), api.least([e, None]), api.nanvl(e, 0.0), api.nanvl(1.0, e)):
        assert len(outs) == 2 and all(o.length == 0 and o.null_count == 0 for o in outs)


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error_for_valid_calls(api):
    H = A.HostArray.from_numpy
    x = [H(np.array([1.0, np.nan, 4.0]), valid=[1, 0, 1])]
    y = [H(np.array([3.0, 2.0, 1.0]))]
    i = [H(np.array([3, 2, 1], dtype=np.int8), valid=[0, 1, 1])]
    c = [H(np.array([1, 0, 1], dtype=bool), valid=[1, 1, 0])]
    for call in (lambda: api.null_test("is_null", x), lambda: api.null_test("is_not_null", c), lambda: api.null_test("is_nan", x),
                 lambda: api.coalesce([x, 0.0]), lambda: api.coalesce([i, i, None]), lambda: api.case_when([c], [x], y), lambda: api.case_when([c, c], [1, i], None),
                 lambda: api.greatest([x, y]), lambda: api.least([i, 5]), lambda: api.nanvl(x, y), lambda: api.nanvl(x, 123.0)):
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
        assert "no CPU fallback" in ei.value.message


def text_outs(rows, validity=True):
    """(out_offsets, out_data, the buffers) of one text output chunk, everything 0x4D, for a call that must write nothing"""
    offs = np.full(4 * (rows + 1) + 16, 0x4D, dtype=np.uint8)
    bits = np.full(16, 0x4D, dtype=np.uint8) if validity else None
    co = (A.rdf_out * 1)(A.rdf_out(offs.ctypes.data, bits.ctypes.data if validity else None, rows + 1, -5, -6, A.I32, A.MEM_HOST))
    cd = (A.rdf_out * 1)(A.rdf_out(None, None, 0, -5, -6, A.U8, A.MEM_HOST))
    return co, cd, (offs, bits)


def test_argument_errors_of_the_text_forms_in_the_stated_order(so):
    a = [A.HostUtf8.from_pylist(["x", None, "yz"])]
    carr = (A.rdf_utf8_array * 1)(a[0].c_struct())
    buf = (C.c_uint8 * 2048)()
    co, cd, keep = text_outs(3)
    plain_co, plain_cd, plain_keep = text_outs(3, validity=False)
    P = A.rdf_utf8_part
    lit = lambda n: P(None, C.cast(buf, C.POINTER(C.c_uint8)), n)  # noqa: E731
    col, both, null = P(carr, None, 0), P(carr, C.cast(buf, C.POINTER(C.c_uint8)), 1), P(None, None, 0)
    one, neg, zero = C.c_int64(1), C.c_int64(-1), C.c_int64(0)
    notbool = (A.rdf_array * 1)(A.HostArray.from_numpy(np.zeros(3, dtype=np.int32)).c_struct())
    short = (A.rdf_array * 1)(A.HostArray.from_numpy(np.zeros(2, dtype=bool)).c_struct())
    good = (A.rdf_array * 1)(A.HostArray.from_numpy(np.zeros(3, dtype=bool)).c_struct())
    ptr = lambda c: (C.POINTER(A.rdf_array) * 1)(C.cast(c, C.POINTER(A.rdf_array)))  # noqa: E731
    coalesce = lambda ps, k, nch=one, o=co, d=cd: so.rdf_utf8_coalesce((P * max(1, len(ps)))(*ps) if ps is not None else None, C.c_int32(k), nch, o, d)  # noqa: E731
    when = lambda cs, vs, k, other, nch=one, o=co, d=cd: so.rdf_utf8_case_when(cs, (P * max(1, len(vs)))(*vs) if vs is not None else None, C.c_int32(k),  # noqa: E731
                                                                             (P * 1)(other) if other is not None else None, nch, o, d)
    seen = []

    def refused(status, want, text):
        seen.append(status)
        assert status == want and text in so.rdf_last_error().decode(), (status, so.rdf_last_error())

    # 2. the counts (every other argument bad as well); 3. lists; 4. no column part; 6. both pointers; 7. a literal too long;
    # 8. a condition that is not Boolean; 9. dtypes; 11. the bitmap; 13. row counts -- each with the later errors present
    refused(coalesce(None, 0, neg, None, None), BAD, "parts")
    refused(coalesce(None, 9, neg, None, None), BAD, "parts")
    refused(when(None, None, 0, None, neg, None, None), BAD, "branches")
    refused(coalesce(None, 1, neg), BAD, "nchunks")
    refused(coalesce(None, 1), BAD, "chunk lists")
    refused(coalesce([lit(1)], 1, one, None, cd), BAD, "chunk lists")
    refused(when(None, [lit(1)], 1, None), BAD, "chunk lists")
    refused(when((C.POINTER(A.rdf_array) * 1)(None), [lit(1)], 1, None), BAD, "chunk lists")
    refused(coalesce([lit(2000), null], 2), BAD, "no column part")
    refused(when(ptr(notbool), [lit(2000)], 1, null), BAD, "no column part")
    refused(coalesce([both, lit(2000)], 2), BAD, "both")
    refused(when(ptr(notbool), [col], 1, both), BAD, "both")
    refused(coalesce([col, lit(1025)], 2, one, plain_co, plain_cd), BAD, "at most")
    refused(coalesce([col, lit(-1)], 2), BAD, "negative")
    refused(when(ptr(notbool), [lit(1025)], 1, col), BAD, "at most")
    refused(when(ptr(notbool), [col], 1, None, one, plain_co, plain_cd), BAD, "RDF_BOOL")
    bad_out = (A.rdf_out * 1)(A.rdf_out(keep[0].ctypes.data, None, 4, -5, -6, A.I64, A.MEM_HOST))
    refused(coalesce([col], 1, one, bad_out, cd), BAD, "Int32 offsets")
    # 10. mixed memory kinds: a device-tagged condition / column against host text and host outputs (no bitmap, wrong row count: later)
    devcond = (A.rdf_array * 1)(A.HostArray.from_numpy(np.zeros(2, dtype=bool)).c_struct())
    devcond[0].mem = A.MEM_DEVICE
    refused(when(ptr(devcond), [col], 1, None, one, plain_co, plain_cd), BAD, "memory space")
    devtext = (A.rdf_utf8_array * 1)(a[0].c_struct())
    devtext[0].offsets.mem = devtext[0].data.mem = A.MEM_DEVICE
    refused(coalesce([col, P(devtext, None, 0)], 2, one, plain_co, plain_cd), BAD, "memory space")
    refused(coalesce([P(devtext, None, 0)], 1, one, plain_co, plain_cd), BAD, "memory space")       # host outputs of a device call
    refused(coalesce([col], 1, one, plain_co, plain_cd), BAD, "validity")
    refused(coalesce([col, null], 2, one, plain_co, plain_cd), BAD, "validity")
    refused(when(ptr(short), [lit(3)], 1, col, one, plain_co, plain_cd), BAD, "validity")
    refused(when(ptr(short), [col], 1, lit(2)), COMPUTE, "row count differs")
    small = (A.rdf_out * 1)(A.rdf_out(keep[0].ctypes.data, keep[1].ctypes.data, 3, -5, -6, A.I32, A.MEM_HOST))
    refused(coalesce([col, lit(1)], 2, one, small, cd), MEMORY, "offsets need")
    assert small[0].length == 4
    assert len(seen) >= 20
    assert so.rdf_utf8_coalesce(None, C.c_int32(1), zero, None, None) == A.RDF_OK
    assert so.rdf_utf8_case_when(None, None, C.c_int32(8), None, zero, None, None) == A.RDF_OK
    for bufs in (keep, plain_keep):
        assert all(b is None or (b == 0x4D).all() for b in bufs), "a refused call wrote"
    assert (co[0].length, co[0].null_count, cd[0].length) == (-5, -6, -5)


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error_for_the_text_forms(api):
    a = [A.HostUtf8.from_pylist(["x", None, "yz"])]
    c = [A.HostArray.from_numpy(np.array([1, 0, 1], dtype=bool))]
    for call in (lambda: api.utf8_coalesce([a, "unknown"]), lambda: api.utf8_coalesce([a, a, None]), lambda: api.utf8_case_when([c], ["low"], a),
                 lambda: api.utf8_case_when([c, c], [a, None], None)):
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
