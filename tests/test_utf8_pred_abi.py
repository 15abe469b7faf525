"""rdf_utf8_predicate / rdf_utf8_compare / rdf_utf8_measure at the C-ABI boundary, without a GPU: every refusal of the
header's error list by status and message, in the documented order, before any device work; RDF_DEVICE_ERROR with no
device; nchunks == 0."""
import ctypes as C

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

INV, MEMERR, COMPUTE, DEVICE = A.RDF_INVALID_ARGUMENT, A.RDF_MEMORY_ERROR, A.RDF_COMPUTE_ERROR, A.RDF_DEVICE_ERROR


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    for n in ("predicate", "compare", "measure"):
        getattr(s, "rdf_utf8_" + n).restype = C.c_int
    return s


H = A.HostUtf8.from_pylist(["ab", None, "cde"])
PLAIN = A.HostUtf8.from_pylist(["ab", "x", "cde"])


def carr(*hs):
    return (A.rdf_utf8_array * len(hs))(*[h.c_struct() for h in hs])


def outs(n=1, rows=3, dtype=A.BOOL, validity=True, cap=None, mem=A.MEM_HOST):
    keep, o = [], (A.rdf_out * max(1, n))()
    for i in range(n):
        vb, bb = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
        keep.append((vb, bb))
        o[i] = A.rdf_out(vb.ctypes.data, bb.ctypes.data if validity else None, rows if cap is None else cap, -7, -7, dtype, mem)
    o._keep = keep
    return o


def pat(b):
    return (C.c_uint8 * max(1, len(b))).from_buffer_copy(b or b"\0"), C.c_int64(len(b))


def predicate(so, op, chunks, n, pattern=b"a", escape=-1, o=None, nbytes=None, null_pattern=False):
    p, k = pat(pattern)
    return so.rdf_utf8_predicate(C.c_int32(op), chunks, C.c_int64(n), None if null_pattern else p, k if nbytes is None else C.c_int64(nbytes),
                                 C.c_int32(escape), outs() if o is None else o)


def measure(so, what, chunks, n, pattern=b"a", pos=1, o=None, nbytes=None, null_pattern=False):
    p, k = pat(pattern)
    return so.rdf_utf8_measure(C.c_int32(what), chunks, C.c_int64(n), None if null_pattern else p, k if nbytes is None else C.c_int64(nbytes),
                               C.c_int64(pos), outs(dtype=A.I32) if o is None else o)


def err(so):
    return so.rdf_last_error().decode()


def test_enums_and_names():
    assert A.UTF8_PRED_OPS == {n: i for i, n in enumerate(["eq", "ne", "lt", "le", "gt", "ge", "starts_with", "ends_with", "contains", "like"])}
    assert A.UTF8_MEASURE_OPS == {"length": 0, "octet_length": 1, "locate": 2}
    assert A.UTF8_PATTERN_MAX == 1024
    for n in ("rdf_utf8_predicate", "rdf_utf8_compare", "rdf_utf8_measure"):
        assert n in lib.EXPORTS


def test_unknown_ops(so):
    g = carr(H)
    for op in (-1, 10, 99):
        assert predicate(so, op, g, 1) == INV and "unknown operation" in err(so)
    for what in (-1, 3):
        assert measure(so, what, g, 1) == INV and "unknown operation" in err(so)
    for op in (-1, 6, 7, 8, 9, 10):       # starts_with .. like are not comparisons
        assert so.rdf_utf8_compare(C.c_int32(op), g, g, C.c_int64(1), outs()) == INV and "six comparisons" in err(so)
    # the op is looked at before anything else: a null chunk list with a bad op is still the op's refusal
    assert predicate(so, 42, None, 1) == INV and "unknown operation" in err(so)


def test_pattern_refusals(so):
    g = carr(H)
    for op in range(10):
        assert predicate(so, op, g, 1, nbytes=-1) == INV and "negative pattern length" in err(so)
        assert predicate(so, op, g, 1, pattern=b"a" * 1025) == INV and "at most 1024" in err(so)
        assert predicate(so, op, g, 1, nbytes=3, null_pattern=True) == INV and "null pattern" in err(so)
        for esc in (0, ord("%"), ord("_"), 128, 255, -2, 1000):
            assert predicate(so, op, g, 1, escape=esc) == INV and "escape" in err(so), (op, esc)
    assert predicate(so, 9, g, 1, pattern=b"ab\\", escape=ord("\\")) == INV and "lone escape" in err(so)
    assert predicate(so, 9, g, 1, pattern=b"%".join([b"a"] * 33)) == INV and "more than 32 segments" in err(so)
    assert measure(so, 2, g, 1, nbytes=-1) == INV and "negative pattern length" in err(so)
    assert measure(so, 2, g, 1, pattern=b"a" * 1025) == INV and "at most 1024" in err(so)
    assert measure(so, 2, g, 1, nbytes=1, null_pattern=True) == INV and "null pattern" in err(so)
    # the pattern comes before the arrays: a bad pattern with bad dtypes is the pattern's refusal
    bad = carr(H)
    bad[0].offsets.dtype = A.I64
    assert predicate(so, 0, bad, 1, nbytes=-1) == INV and "negative pattern length" in err(so)


def calls(so):
    """(name, call(chunks, out)) for one entry point of each kind over one chunk list; compare uses the list twice"""
    return [("utf8_predicate", lambda c, o: predicate(so, 9, c, len(c), pattern=b"a%", o=o), A.BOOL),
            ("utf8_predicate", lambda c, o: predicate(so, 0, c, len(c), o=o), A.BOOL),
            ("utf8_compare", lambda c, o: so.rdf_utf8_compare(C.c_int32(2), c, c, C.c_int64(len(c)), o), A.BOOL),
            ("utf8_measure", lambda c, o: measure(so, 0, c, len(c), o=o), A.I32),
            ("utf8_measure", lambda c, o: measure(so, 2, c, len(c), o=o), A.I32)]


def test_array_refusals_in_order(so):
    for name, call, dt in calls(so):
        # wrong dtypes: offsets, data, output
        bad = carr(H)
        bad[0].offsets.dtype = A.I64
        assert call(bad, outs(dtype=dt)) == INV and "offsets must be an Int32 array" in err(so) and name in err(so)
        bad = carr(H)
        bad[0].data.dtype = A.I8
        assert call(bad, outs(dtype=dt)) == INV and "data must be a UInt8 array" in err(so)
        assert call(carr(H), outs(dtype=A.I64)) == INV and "output dtype" in err(so)
        # ... come before mixed memory kinds
        bad = carr(H)
        bad[0].data.mem = A.MEM_DEVICE
        assert call(bad, outs(dtype=A.I64)) == INV and "output dtype" in err(so)
        assert call(bad, outs(dtype=dt)) == INV and "one memory space" in err(so)
        assert call(carr(H), outs(dtype=dt, mem=A.MEM_DEVICE)) == INV and "same memory space" in err(so)
        # ... which come before the missing validity buffer
        assert call(bad, outs(dtype=dt, validity=False)) == INV and "one memory space" in err(so)
        assert call(carr(H), outs(dtype=dt, validity=False)) == INV and "needs a validity buffer" in err(so)
        # ... which comes before the capacity
        o = outs(dtype=dt, validity=False, cap=2)
        assert call(carr(H), o) == INV and "needs a validity buffer" in err(so) and o[0].length == -7
        o = outs(dtype=dt, cap=2)
        assert call(carr(H), o) == MEMERR and "capacity 2 below the 3 rows" in err(so)
        assert o[0].length == 3
        # a chunk without validity needs no validity buffer: only the device is missing then
        two = carr(PLAIN, H)
        o = outs(n=2, dtype=dt, validity=False)
        assert call(two, o) == INV and "output 1 needs a validity buffer" in err(so)
    # null lists, negative chunk counts
    assert predicate(so, 0, None, 1) == INV and "bad chunk lists" in err(so)
    assert so.rdf_utf8_predicate(C.c_int32(0), carr(H), C.c_int64(1), None, C.c_int64(0), C.c_int32(-1), None) == INV
    assert predicate(so, 0, carr(H), -1) == INV
    assert so.rdf_utf8_compare(C.c_int32(0), carr(H), None, C.c_int64(1), outs()) == INV
    assert measure(so, 0, None, 1) == INV


def test_compare_row_counts_and_either_side_nullable(so):
    a, b = carr(PLAIN), carr(A.HostUtf8.from_pylist(["ab", "x"]))
    assert so.rdf_utf8_compare(C.c_int32(0), a, b, C.c_int64(1), outs()) == COMPUTE and "chunk lengths differ" in err(so)
    # the missing validity buffer is found first
    nb = carr(A.HostUtf8.from_pylist(["ab", None]))
    assert so.rdf_utf8_compare(C.c_int32(0), a, nb, C.c_int64(1), outs(validity=False)) == INV and "validity buffer" in err(so)
    # validity on the right side alone asks for the buffer too
    assert so.rdf_utf8_compare(C.c_int32(0), carr(PLAIN), carr(H), C.c_int64(1), outs(validity=False)) == INV and "validity buffer" in err(so)
    # the row counts come before the capacity
    o = outs(cap=1)
    assert so.rdf_utf8_compare(C.c_int32(0), a, b, C.c_int64(1), o) == COMPUTE and o[0].length == -7


def test_no_chunks_is_ok_and_writes_nothing(so):
    o = outs()
    assert predicate(so, 9, None, 0, pattern=b"a%", o=o) == A.RDF_OK
    assert so.rdf_utf8_compare(C.c_int32(0), None, None, C.c_int64(0), o) == A.RDF_OK
    assert measure(so, 2, None, 0, o=outs(dtype=A.I32)) == A.RDF_OK
    assert o[0].length == -7
    api = lib.api()
    assert api.utf8_predicate("like", [], "a%") == [] and api.utf8_compare("eq", [], []) == [] and api.utf8_measure("length", []) == []
    # a refused pattern is refused with no chunks too
    assert predicate(so, 9, None, 0, pattern=b"a\\", escape=ord("\\")) == INV


def test_chunks_without_rows_need_no_device(so):
    e = A.HostUtf8.from_pylist([])
    o = outs(n=2, rows=0)
    assert predicate(so, 8, carr(e, e), 2, o=o) == A.RDF_OK and o[0].length == 0 and o[1].null_count == 0


def test_length_and_octet_length_ignore_pattern_and_pos(so):
    # (whatever they are: they are not even looked at; without a GPU the call then gets as far as the device)
    expect = A.RDF_OK if lib.device_count() > 0 else DEVICE
    for what in (0, 1):
        assert measure(so, what, carr(H), 1, nbytes=-5, null_pattern=True, pos=-9) == expect


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error(so):
    for name, call, dt in calls(so):
        assert call(carr(H), outs(dtype=dt)) == DEVICE, name
        assert "no CPU fallback" in err(so)
    api = lib.api()
    for f in (lambda: api.utf8_predicate("like", [H], "a%"), lambda: api.utf8_compare("lt", [H], [PLAIN]), lambda: api.utf8_measure("locate", [H], "a", 2),
              lambda: api.utf8_predicate("eq", [H], b"\xff\x00"), lambda: api.utf8_predicate("like", [H], "a#%", escape="#")):
        with pytest.raises(A.RdfError) as ei:
            f()
        assert ei.value.status == DEVICE


def test_python_binding_refuses_what_the_library_refuses():
    api = lib.api()
    with pytest.raises(KeyError):
        api.utf8_predicate("regex", [H], "a")
    with pytest.raises(A.RdfError) as ei:
        api.utf8_predicate("like", [H], "a", escape="%")
    assert ei.value.status == INV
    with pytest.raises(A.RdfError) as ei:
        api.utf8_compare("like", [H], [H])
    assert ei.value.status == INV
    with pytest.raises(ValueError):
        api.utf8_compare("eq", [H], [])
