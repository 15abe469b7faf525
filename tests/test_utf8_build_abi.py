"""rdf_utf8_concat / _pad / _repeat / _reverse / _substring_index at the C-ABI boundary, without a GPU: every refusal of the
header's error list by status and message, in the documented order, before any device work; RDF_DEVICE_ERROR with no
device; nchunks == 0."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

INV, MEMERR, COMPUTE, DEVICE = A.RDF_INVALID_ARGUMENT, A.RDF_MEMORY_ERROR, A.RDF_COMPUTE_ERROR, A.RDF_DEVICE_ERROR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("concat", "pad", "repeat", "reverse", "substring_index")


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    for n in NAMES:
        getattr(s, "rdf_utf8_" + n).restype = C.c_int
    return s


H = A.HostUtf8.from_pylist(["ab", None, "cde"])
PLAIN = A.HostUtf8.from_pylist(["ab", "x", "cde"])


def carr(*hs):
    return (A.rdf_utf8_array * len(hs))(*[h.c_struct() for h in hs])


def outs(n=1, rows=3, validity=True, cap=64, odt=A.I32, ddt=A.U8, mem=A.MEM_HOST, ocap=None):
    """(out_offsets, out_data) of n chunks"""
    keep, oo, od = [], (A.rdf_out * max(1, n))(), (A.rdf_out * max(1, n))()
    for i in range(n):
        ob, vb, db = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
        keep.append((ob, vb, db))
        oo[i] = A.rdf_out(ob.ctypes.data, vb.ctypes.data if validity else None, rows + 1 if ocap is None else ocap, -7, -7, odt, mem)
        od[i] = A.rdf_out(db.ctypes.data, None, cap, -7, -7, ddt, mem)
    oo._keep = keep
    return oo, od


def lit(b):
    return (C.c_uint8 * max(1, len(b))).from_buffer_copy(b or b"\0")


def part(col=None, literal=None, nbytes=None):
    p = A.rdf_utf8_part()
    if col is not None:
        p.utf8 = C.cast(col, C.POINTER(A.rdf_utf8_array))
    if literal is not None:
        buf = lit(literal)
        p._keep = buf
        p.literal = C.cast(buf, C.POINTER(C.c_uint8))
    p.literal_bytes = len(literal or b"") if nbytes is None else nbytes
    return p


def concat(so, parts, n=1, ws=0, sep=b"", o=None, nparts=None, sep_bytes=None, null_sep=False):
    arr = (A.rdf_utf8_part * max(1, len(parts)))(*parts)
    oo, od = outs() if o is None else o
    return so.rdf_utf8_concat(arr, C.c_int32(len(parts) if nparts is None else nparts), C.c_int64(n), C.c_int32(ws), None if null_sep else lit(sep),
                              C.c_int64(len(sep) if sep_bytes is None else sep_bytes), oo, od)


def pad(so, chunks, n=1, side=0, length=5, p=b"x", o=None, nbytes=None, null_pad=False):
    oo, od = outs() if o is None else o
    return so.rdf_utf8_pad(C.c_int32(side), chunks, C.c_int64(n), C.c_int64(length), None if null_pad else lit(p), C.c_int64(len(p) if nbytes is None else nbytes), oo, od)


def subidx(so, chunks, n=1, d=b".", count=1, o=None, nbytes=None, null_delim=False):
    oo, od = outs() if o is None else o
    return so.rdf_utf8_substring_index(chunks, C.c_int64(n), None if null_delim else lit(d), C.c_int64(len(d) if nbytes is None else nbytes), C.c_int64(count), oo, od)


def err(so):
    return so.rdf_last_error().decode()


def no_device():
    return A.RDF_OK if lib.device_count() > 0 else DEVICE


def test_names_and_the_part_struct():
    for n in NAMES:
        assert "rdf_utf8_" + n in lib.EXPORTS
    assert A.UTF8_PARTS_MAX == 8
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rdf_mi355x.h"
int main(void) {
  printf("%zu %zu %zu %zu %d %d\n", sizeof(rdf_utf8_part), offsetof(rdf_utf8_part, utf8), offsetof(rdf_utf8_part, literal), offsetof(rdf_utf8_part, literal_bytes),
         RDF_UTF8_PARTS_MAX, RDF_UTF8_PATTERN_MAX);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    P = A.rdf_utf8_part
    assert got == [C.sizeof(P), P.utf8.offset, P.literal.offset, P.literal_bytes.offset, A.UTF8_PARTS_MAX, A.UTF8_PATTERN_MAX]


def test_1_part_counts_and_sides(so):
    g = carr(H)
    for nparts in (0, -1, 9, 100):
        assert concat(so, [part(g)] * 9, nparts=nparts) == INV and "1 .. 8 are taken" in err(so)
    for side in (-1, 2, 7):
        assert pad(so, g, side=side) == INV and "side" in err(so)
    # ... before anything else: a bad part and a bad pad with them are still this refusal
    assert concat(so, [part()], nparts=0, sep_bytes=-1) == INV and "1 .. 8 are taken" in err(so)
    assert pad(so, g, side=3, nbytes=-1) == INV and "side" in err(so)


def test_2_parts_set_exactly_one_pointer_and_one_is_a_column(so):
    g = carr(H)
    both = part(g, b"x")
    assert concat(so, [part(g), both]) == INV and "part 1 must set exactly one" in err(so)
    assert concat(so, [part(), part(g)]) == INV and "part 0 must set exactly one" in err(so)
    assert concat(so, [part(None, None, nbytes=3)]) == INV and "exactly one" in err(so)          # NULL literal with a positive length: no part at all
    assert concat(so, [part(literal=b"a"), part(literal=b"")]) == INV and "at least one part must be a column" in err(so)
    # ... before the lengths
    assert concat(so, [part(literal=b"a", nbytes=-1)]) == INV and "at least one part must be a column" in err(so)
    assert concat(so, [part(g), both], sep_bytes=-1) == INV and "exactly one" in err(so)


def test_3_lengths_of_literals_separator_pad_and_delimiter(so):
    g = carr(H)
    assert concat(so, [part(g), part(literal=b"a", nbytes=-1)]) == INV and "negative length" in err(so) and "literal part" in err(so)
    assert concat(so, [part(g), part(literal=b"a" * 1025)]) == INV and "at most 1024" in err(so)
    assert concat(so, [part(g), part(literal=b"a" * 1024)], n=0) == A.RDF_OK
    assert concat(so, [part(g)], ws=1, sep_bytes=-1) == INV and "separator" in err(so) and "negative" in err(so)
    assert concat(so, [part(g)], ws=1, sep=b"s" * 1025) == INV and "at most 1024" in err(so)
    assert concat(so, [part(g)], ws=1, sep_bytes=2, null_sep=True) == INV and "null pointer" in err(so)
    assert pad(so, g, nbytes=-1) == INV and "the pad" in err(so)
    assert pad(so, g, p=b"p" * 1025) == INV and "at most 1024" in err(so)
    assert pad(so, g, nbytes=1, null_pad=True) == INV and "null pointer" in err(so)
    assert subidx(so, g, nbytes=-1) == INV and "the delimiter" in err(so)
    assert subidx(so, g, d=b"d" * 1025) == INV and "at most 1024" in err(so)
    assert subidx(so, g, nbytes=1, null_delim=True) == INV and "null pointer" in err(so)
    # ... before the separator rule and before the arrays
    assert concat(so, [part(g), part(literal=b"a", nbytes=-1)], ws=0, sep=b"-") == INV and "negative length" in err(so)
    bad = carr(H)
    bad[0].offsets.dtype = A.I64
    assert pad(so, bad, nbytes=-1) == INV and "the pad" in err(so)
    assert subidx(so, bad, nbytes=2000) == INV and "the delimiter" in err(so)


def test_4_a_separator_needs_with_separator(so):
    g = carr(H)
    assert concat(so, [part(g)], ws=0, sep=b"-") == INV and "without with_separator" in err(so)
    bad = carr(H)
    bad[0].offsets.dtype = A.I64
    assert concat(so, [part(bad)], ws=0, sep=b"-") == INV and "without with_separator" in err(so)      # before the arrays


def calls(so):
    """(name in the message, call(chunks, (out_offsets, out_data), n)) for every entry point over one chunk list"""
    return [("utf8_concat", lambda c, o, n=1: concat(so, [part(c), part(literal=b"-")], n=n, o=o)),
            ("utf8_lpad", lambda c, o, n=1: pad(so, c, n=n, o=o)),
            ("utf8_rpad", lambda c, o, n=1: pad(so, c, n=n, side=1, o=o)),
            ("utf8_repeat", lambda c, o, n=1: so.rdf_utf8_repeat(c, C.c_int64(n), C.c_int64(2), o[0], o[1])),
            ("utf8_reverse", lambda c, o, n=1: so.rdf_utf8_reverse(c, C.c_int64(n), o[0], o[1])),
            ("utf8_substring_index", lambda c, o, n=1: subidx(so, c, n=n, o=o))]


def test_5_array_refusals_in_order(so):
    for name, call in calls(so):
        bad = carr(H)
        bad[0].offsets.dtype = A.I64
        assert call(bad, outs()) == INV and "offsets must be an Int32 array" in err(so) and name in err(so)
        bad = carr(H)
        bad[0].data.dtype = A.I8
        assert call(bad, outs()) == INV and "data must be a UInt8 array" in err(so)
        assert call(carr(H), outs(odt=A.I64)) == INV and "outputs are (Int32 offsets, UInt8 data)" in err(so)
        assert call(carr(H), outs(ddt=A.I8)) == INV and "outputs are" in err(so)
        # ... come before mixed memory kinds
        bad = carr(H)
        bad[0].data.mem = A.MEM_DEVICE
        assert call(bad, outs(odt=A.I64)) == INV and "outputs are" in err(so)
        assert call(bad, outs()) == INV and "one memory space" in err(so)
        assert call(carr(H), outs(mem=A.MEM_DEVICE)) == INV and "same memory space" in err(so)
        # ... which come before the missing validity buffer
        assert call(bad, outs(validity=False)) == INV and "one memory space" in err(so)
        assert call(carr(H), outs(validity=False)) == INV and "needs a validity buffer" in err(so)
        two = carr(PLAIN, H)
        assert call(two, outs(n=2, validity=False), 2) == INV and "output 1 needs a validity buffer" in err(so)
        # ... which comes before the offsets' capacity
        o = outs(validity=False, ocap=2)
        assert call(carr(H), o) == INV and "needs a validity buffer" in err(so) and o[0][0].length == -7
        o = outs(ocap=3)
        assert call(carr(H), o) == MEMERR and "offsets need 4 entries" in err(so) and o[0][0].length == 4
        # null lists, negative chunk counts
        assert call(None, outs()) == INV
        assert call(carr(H), (None, None)) == INV and "bad chunk lists" in err(so)
        assert call(carr(H), outs(), -1) == INV
    # concat_ws is never NULL: it needs no validity buffer, and only the device is missing then
    assert concat(so, [part(carr(H))], ws=1, sep=b"-", o=outs(validity=False)) == no_device()


def test_6_chunk_row_counts_that_differ_between_parts(so):
    a, b = carr(PLAIN), carr(A.HostUtf8.from_pylist(["ab", "x"]))
    assert concat(so, [part(a), part(literal=b"-"), part(b)]) == COMPUTE and "chunk lengths differ" in err(so)
    # the missing validity buffer is found first, the offsets' capacity afterwards
    assert concat(so, [part(carr(H)), part(b)], o=outs(validity=False)) == INV and "validity buffer" in err(so)
    o = outs(ocap=1)
    assert concat(so, [part(a), part(b)], o=o) == COMPUTE and o[0][0].length == -7


def test_7_no_device_is_the_last_refusal(so):
    for name, call in calls(so):
        st, msg = call(carr(H), outs()), err(so)
        assert st == no_device(), name
        assert st == A.RDF_OK or "no CPU fallback" in msg
    api = lib.api()
    for f in (lambda: api.utf8_concat([[H], ", ", [PLAIN]]), lambda: api.utf8_concat([[H], [PLAIN]], sep="-"), lambda: api.utf8_build("lpad", [H], 5, "0"),
              lambda: api.utf8_build("repeat", [H], 2), lambda: api.utf8_build("reverse", [H]), lambda: api.utf8_build("substring_index", [H], ".", -1)):
        if lib.device_count() == 0:
            with pytest.raises(A.RdfError) as ei:
                f()
            assert ei.value.status == DEVICE
        else:
            assert len(f()) == 1


def test_no_chunks_is_ok_and_writes_nothing(so):
    for name, call in calls(so):
        o = outs()
        # (a concat part is a column by its pointer, so it has one even without chunks)
        assert call(carr(H) if name == "utf8_concat" else None, o, 0) == A.RDF_OK and o[0][0].length == -7 and o[1][0].length == -7, name
    api = lib.api()
    assert api.utf8_concat([[], "x"]) == [] and api.utf8_build("reverse", []) == [] and api.utf8_build("lpad", [], 3, "x") == []
    # what is refused with chunks is refused without them
    assert pad(so, None, n=0, nbytes=-1) == INV and subidx(so, None, n=0, nbytes=1025) == INV
    assert concat(so, [part(literal=b"a")], n=0) == INV


def test_python_binding_refuses_what_the_library_refuses():
    api = lib.api()
    with pytest.raises(ValueError):
        api.utf8_build("translate", [H])
    with pytest.raises(ValueError):
        api.utf8_concat([[H], [H, H]])
    with pytest.raises(A.RdfError) as ei:
        api.utf8_concat(["a", "b"])
    assert ei.value.status == INV
    with pytest.raises(A.RdfError) as ei:
        api.utf8_build("lpad", [H], 5, "p" * 1025)
    assert ei.value.status == INV
