"""rdf_utf8_replace / _translate / _initcap / _split at the C-ABI boundary, without a GPU: every refusal of the header's
error list by status and message, in the documented order, before any device work; RDF_DEVICE_ERROR with no device;
nchunks == 0; the four names in lib.EXPORTS."""
import ctypes as C

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

INV, MEMERR, DEVICE = A.RDF_INVALID_ARGUMENT, A.RDF_MEMORY_ERROR, A.RDF_DEVICE_ERROR
NAMES = ("replace", "translate", "initcap", "split")


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    for n in NAMES:
        getattr(s, "rdf_utf8_" + n).restype = C.c_int
    return s


H = A.HostUtf8.from_pylist(["ab", None, "c,de"])
PLAIN = A.HostUtf8.from_pylist(["ab", "x", "c,de"])


def carr(*hs):
    return (A.rdf_utf8_array * len(hs))(*[h.c_struct() for h in hs])


def outs(n=1, rows=3, validity=True, cap=64, odt=A.I32, ddt=A.U8, ldt=A.I32, mem=A.MEM_HOST, ocap=None, data=True, lmem=None):
    """(out_list_offsets, out_offsets, out_data) of n chunks; the first is used by split only, where out_offsets is the child's"""
    keep = []
    ol, oo, od = (A.rdf_out * max(1, n))(), (A.rdf_out * max(1, n))(), (A.rdf_out * max(1, n))()
    for i in range(n):
        lb, ob, vb, db = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
        keep.append((lb, ob, vb, db))
        ol[i] = A.rdf_out(lb.ctypes.data, vb.ctypes.data if validity else None, rows + 1 if ocap is None else ocap, -7, -7, ldt, mem if lmem is None else lmem)
        oo[i] = A.rdf_out(ob.ctypes.data, vb.ctypes.data if validity else None, rows + 1 if ocap is None else ocap, -7, -7, odt, mem)
        od[i] = A.rdf_out(db.ctypes.data if data else None, None, cap, -7, -7, ddt, mem)
    ol._keep = keep
    return ol, oo, od


def lit(b):
    return (C.c_uint8 * max(1, len(b))).from_buffer_copy(b or b"\0")


def run(so, name, chunks, n=1, a=b",", b=b"x", o=None, abytes=None, bbytes=None, null_a=False, null_b=False, limit=-1, split_child=None):
    ol, oo, od = outs() if o is None else o
    la = (None if null_a else lit(a), C.c_int64(len(a) if abytes is None else abytes))
    lb = (None if null_b else lit(b), C.c_int64(len(b) if bbytes is None else bbytes))
    if name == "initcap":
        return so.rdf_utf8_initcap(chunks, C.c_int64(n), oo, od)
    if name == "split":
        if split_child is None:   # the child's offsets: room for every element
            oo = outs(n=max(1, n), rows=63, validity=False, mem=oo[0].mem, odt=oo[0].dtype)[1]
            ol._child = oo
        return so.rdf_utf8_split(chunks, C.c_int64(n), *la, C.c_int64(limit), ol, oo, od)
    return getattr(so, "rdf_utf8_" + name)(chunks, C.c_int64(n), *la, *lb, oo, od)


def err(so):
    return so.rdf_last_error().decode()


def no_device():
    return A.RDF_OK if lib.device_count() > 0 else DEVICE


WITH_LITERALS = ("replace", "translate", "split")


def test_names():
    for n in NAMES:
        assert "rdf_utf8_" + n in lib.EXPORTS
    assert A.UTF8_PATTERN_MAX == 1024


def test_1_literals(so):
    g = carr(H)
    what = {"replace": ("search string", "replacement"), "translate": ("matching string", "replace string"), "split": ("delimiter", None)}
    for name in WITH_LITERALS:
        first, second = what[name]
        assert run(so, name, g, abytes=-1) == INV and "negative length" in err(so) and first in err(so)
        assert run(so, name, g, a=b"a" * 1025) == INV and "at most 1024" in err(so) and first in err(so)
        assert run(so, name, g, null_a=True, abytes=2) == INV and "null pointer with 2 bytes" in err(so)
        if second:
            assert run(so, name, g, bbytes=-1) == INV and "negative length" in err(so) and second in err(so)
            assert run(so, name, g, b=b"b" * 1025) == INV and "at most 1024" in err(so) and second in err(so)
            assert run(so, name, g, null_b=True, bbytes=1) == INV and "null pointer with 1 bytes" in err(so)
            # in argument order
            assert run(so, name, g, abytes=-1, b=b"b" * 1025) == INV and first in err(so)
        # ... before the chunk lists
        assert run(so, name, None, n=-1, abytes=-1) == INV and "negative length" in err(so)
    # a literal of the full length is taken; a NULL pointer with no bytes is the empty literal
    assert run(so, "replace", g, a=b"a" * 1024, n=0) == A.RDF_OK
    assert run(so, "replace", g, null_a=True, abytes=0, null_b=True, bbytes=0, n=0) == A.RDF_OK


def test_2_an_empty_delimiter(so):
    g = carr(H)
    assert run(so, "split", g, a=b"") == INV and "empty delimiter" in err(so)
    assert run(so, "split", g, null_a=True, abytes=0) == INV and "empty delimiter" in err(so)
    assert run(so, "split", None, n=-1, a=b"") == INV and "empty delimiter" in err(so)   # before the chunk lists
    assert run(so, "replace", g, a=b"", n=0) == A.RDF_OK                                   # replace takes an empty search


def test_3_chunk_lists_and_nchunks_zero(so):
    g = carr(H)
    for name in NAMES:
        assert run(so, name, g, n=-1) == INV and "bad chunk lists" in err(so)
        assert run(so, name, None, n=1) == INV and "bad chunk lists" in err(so)
        ol, oo, od = outs()
        assert run(so, name, g, o=(ol, None, od), split_child=True) == INV and "bad chunk lists" in err(so)
        assert run(so, name, g, o=(ol, oo, None)) == INV and "bad chunk lists" in err(so)
        assert run(so, name, None, n=0, o=(None, None, None), split_child=True) == A.RDF_OK
        # ... nchunks == 0 before the dtypes
        assert run(so, name, g, n=0, o=outs(odt=A.F64)) == A.RDF_OK
    ol, oo, od = outs()
    assert run(so, "split", g, o=(None, oo, od), split_child=True) == INV and "bad chunk lists" in err(so)


def test_4_dtypes(so):
    bad_offs = A.HostUtf8.from_pylist(["a"]).c_struct()
    bad_offs.offsets.dtype = A.I64
    bad_data = A.HostUtf8.from_pylist(["a"]).c_struct()
    bad_data.data.dtype = A.I8
    no_rows = A.HostUtf8.from_pylist(["a"]).c_struct()
    no_rows.offsets.length = 0
    for name in NAMES:
        assert run(so, name, (A.rdf_utf8_array * 1)(bad_offs), o=outs(rows=1)) == INV and "offsets must be an Int32 array" in err(so)
        assert run(so, name, (A.rdf_utf8_array * 1)(no_rows), o=outs(rows=1)) == INV and "rows + 1 entries" in err(so)
        assert run(so, name, (A.rdf_utf8_array * 1)(bad_data), o=outs(rows=1)) == INV and "data must be a UInt8 array" in err(so)
        g = carr(H)
        assert run(so, name, g, o=outs(ddt=A.I8)) == INV and "outputs are" in err(so)
        assert run(so, name, g, o=outs(odt=A.I64), split_child=True) == INV and "outputs are" in err(so)
        # ... the inputs first, and before the memory kinds
        assert run(so, name, (A.rdf_utf8_array * 1)(bad_offs), o=outs(rows=1, ddt=A.I8, mem=A.MEM_DEVICE)) == INV and "offsets must be" in err(so)
    assert run(so, "split", carr(H), o=outs(ldt=A.U32)) == INV and "Int32 list offsets" in err(so)


def test_5_memory_kinds(so):
    g = carr(H)
    mixed = H.c_struct()
    mixed.data.mem = A.MEM_DEVICE
    for name in NAMES:
        assert run(so, name, (A.rdf_utf8_array * 1)(mixed)) == INV and "share one memory space" in err(so)
        assert run(so, name, g, o=outs(mem=A.MEM_DEVICE), split_child=True) == INV and "same memory space as the inputs" in err(so)
        assert run(so, name, g, o=outs(mem=A.MEM_DEVICE, validity=False, ocap=0), split_child=True) == INV and "same memory space" in err(so)   # before the buffers
    assert run(so, "split", g, o=outs(lmem=A.MEM_DEVICE)) == INV and "same memory space as the inputs" in err(so)


def test_6_buffers_and_bitmaps(so):
    g = carr(H)
    for name in NAMES:
        ol, oo, od = outs()
        rows_out = ol if name == "split" else oo
        rows_out[0].values = None
        assert run(so, name, g, o=(ol, oo, od), split_child=True) == INV and "has no offsets buffer" in err(so)
        assert run(so, name, g, o=outs(ocap=0)) == INV and "has no offsets buffer" in err(so)
        assert run(so, name, g, o=outs(cap=-1)) == INV and "negative capacity" in err(so)
        assert run(so, name, g, o=outs(validity=False)) == INV and "needs a validity buffer" in err(so)
        # ... the buffers before the bitmaps
        assert run(so, name, g, o=outs(validity=False, cap=-1)) == INV and "negative capacity" in err(so)
        # a column without validity needs none
        assert run(so, name, carr(PLAIN), o=outs(validity=False)) == no_device()
    for name in ("replace", "translate", "initcap"):
        assert run(so, name, g, o=outs(data=False)) == INV and "data capacity without a buffer" in err(so)
    # split: a NULL data / child-offsets buffer is the sizing call, not a refusal (it gets as far as the device)
    assert run(so, "split", g, o=outs(data=False)) in (no_device(), MEMERR)


def test_7_the_rows_offsets_capacity(so):
    g = carr(H)
    for name in NAMES:
        ol, oo, od = outs(ocap=3)
        assert run(so, name, g, o=(ol, oo, od)) == MEMERR and "offsets need 4 entries" in err(so)
        assert (ol if name == "split" else oo)[0].length == 4
        assert od[0].length == -7                       # nothing else was touched
        # ... after the bitmaps
        assert run(so, name, g, o=outs(ocap=3, validity=False)) == INV and "validity buffer" in err(so)


def test_8_no_device_is_an_error_and_the_last_check(so):
    if lib.device_count() > 0:
        pytest.skip("a device is visible")
    g = carr(H)
    for name in NAMES:
        assert run(so, name, g) == DEVICE and "no HIP device" in err(so)
    api = lib.api()
    for call in (lambda: api.utf8_replace([H], "a", "b"), lambda: api.utf8_translate([H], "a", "b"), lambda: api.utf8_initcap([H]),
                 lambda: api.utf8_split([H], ",")):
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == DEVICE


def test_9_the_python_layer_refuses_like_the_abi():
    api = lib.api()
    with pytest.raises(A.RdfError) as ei:
        api.utf8_split([H], "")
    assert ei.value.status == INV and "empty delimiter" in ei.value.message
    with pytest.raises(A.RdfError) as ei:
        api.utf8_replace([H], "a" * 1025, "")
    assert ei.value.status == INV and "at most 1024" in ei.value.message
    assert api.utf8_replace([], "a", "b") == [] and api.utf8_split([], ",") == [] and api.utf8_initcap([]) == []
