"""rdf_utf8_dictionary_encode / rdf_groupby_agg_keys / rdf_equijoin_indices_keys at the C-ABI boundary, without a GPU: the
symbols are exported, every argument error is a value returned before any device work, and with no device a valid call
fails loudly with RDF_DEVICE_ERROR (no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

NAMES = ["rdf_utf8_dictionary_encode", "rdf_groupby_agg_keys", "rdf_equijoin_indices_keys"]
BAD = A.RDF_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    lib.api()
    for n in NAMES:
        getattr(s, n).restype = C.c_int
    return s


def _out(dtype, capacity, mem=A.MEM_HOST, values=True, validity=True):
    buf = np.zeros(max(capacity, 1) + 8, dtype=np.int64)
    vbuf = np.zeros(max(capacity, 1) // 8 + 16, dtype=np.uint8)
    o = (A.rdf_out * 1)(A.rdf_out(buf.ctypes.data if values else None, vbuf.ctypes.data if validity else None, capacity, 0, 0, dtype, mem))
    return o, (buf, vbuf)


def _utf8_arr(chunks):
    return (A.rdf_utf8_array * len(chunks))(*[c.c_struct() for c in chunks])


def _key(values=None, utf8=None):
    return A.rdf_sort_key(C.cast(values, C.POINTER(A.rdf_array)) if values is not None else None,
                          C.cast(utf8, C.POINTER(A.rdf_utf8_array)) if utf8 is not None else None, A.rdf_sort_options(0, 0))


def _num_arr(chunks):
    return (A.rdf_array * len(chunks))(*[c.c_struct() for c in chunks])


TEXT = A.HostUtf8.from_pylist(["b", None, "a", "b", ""])
TEXT2 = A.HostUtf8.from_pylist(["x", "y"])
INTS = A.HostArray.from_numpy(np.arange(5, dtype=np.int64))


def test_the_three_symbols_are_exported():
    s = lib.load()
    for n in NAMES:
        assert hasattr(s, n), n
        assert n in lib.EXPORTS
    api = lib.api()
    for m in ("utf8_dictionary_encode", "groupby_agg_keys", "equijoin_indices_keys"):
        assert callable(getattr(api, m))


# ---------------------------------------------------------------- encode

def _encode(so, arr, n, codes, offs, data, count=None):
    count = count if count is not None else C.c_int64(-7)
    return so.rdf_utf8_dictionary_encode(arr, C.c_int64(n), codes, offs, data, C.byref(count))


def test_encode_checks_its_arguments_before_the_device(so):
    arr = _utf8_arr([TEXT])
    codes, _k1 = _out(A.U32, 5)
    offs, _k2 = _out(A.I32, 6, validity=False)
    data, _k3 = _out(A.U8, 16, validity=False)
    # null lists / outputs
    assert _encode(so, None, 1, codes, offs, data) == BAD
    assert _encode(so, arr, -1, codes, offs, data) == BAD
    assert _encode(so, arr, 1, None, offs, data) == BAD
    assert _encode(so, arr, 1, codes, None, data) == BAD
    assert _encode(so, arr, 1, codes, offs, None) == BAD
    assert so.rdf_utf8_dictionary_encode(arr, C.c_int64(1), codes, offs, data, None) == BAD
    # wrong dtypes for codes, offsets, data — outputs and inputs
    for dt in (A.I32, A.U64, A.I64):
        c2, _k = _out(dt, 5)
        assert _encode(so, arr, 1, c2, offs, data) == BAD, dt
    o2, _k = _out(A.I64, 6, validity=False)
    assert _encode(so, arr, 1, codes, o2, data) == BAD
    d2, _k = _out(A.I8, 16, validity=False)
    assert _encode(so, arr, 1, codes, offs, d2) == BAD
    bad_in = _utf8_arr([TEXT])
    bad_in[0].offsets.dtype = A.I64
    assert _encode(so, bad_in, 1, codes, offs, data) == BAD
    bad_in = _utf8_arr([TEXT])
    bad_in[0].data.dtype = A.I8
    assert _encode(so, bad_in, 1, codes, offs, data) == BAD
    bad_in = _utf8_arr([TEXT])
    bad_in[0].offsets.length = 0
    assert _encode(so, bad_in, 1, codes, offs, data) == BAD
    # mixed memory kinds: chunk against chunk, input against each output
    mixed = _utf8_arr([TEXT, TEXT2])
    mixed[1].offsets.mem = A.MEM_DEVICE
    mixed[1].data.mem = A.MEM_DEVICE
    two, _k = _out(A.U32, 5)
    codes2 = (A.rdf_out * 2)(two[0], two[0])
    assert _encode(so, mixed, 2, codes2, offs, data) == BAD
    for which in range(3):
        c3, _ka = _out(A.U32, 5, mem=A.MEM_DEVICE if which == 0 else A.MEM_HOST)
        o3, _kb = _out(A.I32, 6, mem=A.MEM_DEVICE if which == 1 else A.MEM_HOST, validity=False)
        d3, _kc = _out(A.U8, 16, mem=A.MEM_DEVICE if which == 2 else A.MEM_HOST, validity=False)
        assert _encode(so, arr, 1, c3, o3, d3) == BAD, which
    # a nullable chunk needs a validity buffer for its codes; buffers must exist
    c4, _k = _out(A.U32, 5, validity=False)
    assert _encode(so, arr, 1, c4, offs, data) == BAD
    c5, _k = _out(A.U32, 5, values=False)
    assert _encode(so, arr, 1, c5, offs, data) == BAD
    o5, _k = _out(A.I32, 6, values=False, validity=False)
    assert _encode(so, arr, 1, codes, o5, data) == BAD
    d5, _k = _out(A.U8, 16, values=False, validity=False)
    assert _encode(so, arr, 1, codes, offs, d5) == BAD
    # 2^32 rows or more (only the descriptor says so: nothing is read before the check)
    huge = _utf8_arr([TEXT2])
    huge[0].offsets.validity = None
    huge[0].offsets.length = 2**32 + 1
    big, _k = _out(A.U32, 2**32, validity=False)
    assert _encode(so, huge, 1, big, offs, data) == BAD
    assert b"2^32" in so.rdf_last_error()


# ---------------------------------------------------------------- group by

def _groupby(so, keys, nkeys, values, nchunks, agg, max_groups, kouts, ov, oc):
    return so.rdf_groupby_agg_keys(keys, C.c_int32(nkeys), values, C.c_int64(nchunks), C.c_int32(agg), C.c_int64(max_groups), kouts, ov, oc)


def _text_key_out(cap=8, nbytes=32, validity=True):
    o, k1 = _out(A.I32, cap + 1, validity=validity)
    d, k2 = _out(A.U8, nbytes, validity=False)
    return A.rdf_key_out(None, C.cast(o, C.POINTER(A.rdf_out)), C.cast(d, C.POINTER(A.rdf_out))), (o, d, k1, k2)


def _num_key_out(dtype, cap=8):
    o, k = _out(dtype, cap)
    return A.rdf_key_out(C.cast(o, C.POINTER(A.rdf_out)), None, None), (o, k)


def test_groupby_keys_checks_its_arguments_before_the_device(so):
    uarr, narr, varr = _utf8_arr([TEXT]), _num_arr([INTS]), _num_arr([INTS])
    keys = (A.rdf_sort_key * 1)(_key(utf8=uarr))
    ko, _k1 = _text_key_out()
    kouts = (A.rdf_key_out * 1)(ko)
    ov, _k2 = _out(A.I64, 8)
    oc, _k3 = _out(A.I64, 8)
    # null lists / outputs, counts out of range
    assert _groupby(so, None, 1, varr, 1, 0, 6, kouts, ov, oc) == BAD
    assert _groupby(so, keys, 1, varr, 1, 0, 6, None, ov, oc) == BAD
    assert _groupby(so, keys, 1, varr, 1, 0, 6, kouts, None, oc) == BAD
    assert _groupby(so, keys, 1, varr, 1, 0, 6, kouts, ov, None) == BAD
    assert _groupby(so, keys, 1, varr, 0, 0, 6, kouts, ov, oc) == BAD
    assert _groupby(so, keys, 1, varr, 1, 0, 0, kouts, ov, oc) == BAD
    assert _groupby(so, keys, 1, varr, 1, 9, 6, kouts, ov, oc) == BAD
    for nk in (0, 5, -1):
        many = (A.rdf_sort_key * 5)(*[_key(utf8=uarr)] * 5)
        mouts = (A.rdf_key_out * 5)(*[ko] * 5)
        assert _groupby(so, many, nk, varr, 1, 0, 6, mouts, ov, oc) == BAD, nk
    # a key that sets both pointers, or neither
    both = (A.rdf_sort_key * 1)(_key(values=narr, utf8=uarr))
    assert _groupby(so, both, 1, varr, 1, 0, 6, kouts, ov, oc) == BAD
    neither = (A.rdf_sort_key * 1)(_key())
    assert _groupby(so, neither, 1, varr, 1, 0, 6, kouts, ov, oc) == BAD
    # a key output that does not match its key: a Utf8 key with `values`, a numeric key with the pair, both, neither
    nko, _k4 = _num_key_out(A.I64)
    assert _groupby(so, keys, 1, varr, 1, 0, 6, (A.rdf_key_out * 1)(nko), ov, oc) == BAD
    nkeys_ = (A.rdf_sort_key * 1)(_key(values=narr))
    assert _groupby(so, nkeys_, 1, varr, 1, 0, 6, kouts, ov, oc) == BAD
    allset = A.rdf_key_out(nko.values, ko.utf8_offsets, ko.utf8_data)
    assert _groupby(so, keys, 1, varr, 1, 0, 6, (A.rdf_key_out * 1)(allset), ov, oc) == BAD
    assert _groupby(so, keys, 1, varr, 1, 0, 6, (A.rdf_key_out * 1)(A.rdf_key_out(None, None, None)), ov, oc) == BAD
    # wrong dtypes: key output offsets / data, value output, a Float64 grouping column, Utf8 input offsets
    wo, _k5 = _out(A.I64, 9)
    wrong = A.rdf_key_out(None, C.cast(wo, C.POINTER(A.rdf_out)), ko.utf8_data)
    assert _groupby(so, keys, 1, varr, 1, 0, 6, (A.rdf_key_out * 1)(wrong), ov, oc) == BAD
    wd, _k6 = _out(A.I8, 32, validity=False)
    wrong = A.rdf_key_out(None, ko.utf8_offsets, C.cast(wd, C.POINTER(A.rdf_out)))
    assert _groupby(so, keys, 1, varr, 1, 0, 6, (A.rdf_key_out * 1)(wrong), ov, oc) == BAD
    ovf, _k7 = _out(A.F64, 8)
    assert _groupby(so, keys, 1, varr, 1, 0, 6, kouts, ovf, oc) == BAD
    ocf, _k8 = _out(A.F64, 8)
    assert _groupby(so, keys, 1, varr, 1, 0, 6, kouts, ov, ocf) == BAD
    farr = _num_arr([A.HostArray.from_numpy(np.arange(5.0))])
    fko, _k9 = _num_key_out(A.F64)
    two = (A.rdf_sort_key * 2)(_key(utf8=uarr), _key(values=farr))
    assert _groupby(so, two, 2, varr, 1, 0, 6, (A.rdf_key_out * 2)(ko, fko), ov, oc) == BAD
    bad_in = _utf8_arr([TEXT])
    bad_in[0].offsets.dtype = A.I64
    assert _groupby(so, (A.rdf_sort_key * 1)(_key(utf8=bad_in)), 1, varr, 1, 0, 6, kouts, ov, oc) == BAD
    # a nullable Utf8 key needs a validity buffer on its output
    nv, _k10 = _text_key_out(validity=False)
    assert _groupby(so, keys, 1, varr, 1, 0, 6, (A.rdf_key_out * 1)(nv), ov, oc) == BAD
    # mixed memory kinds: key against key, keys against values, keys against outputs
    dnarr = _num_arr([INTS])
    dnarr[0].mem = A.MEM_DEVICE
    ik, _k11 = _num_key_out(A.I64)
    mixed = (A.rdf_sort_key * 2)(_key(utf8=uarr), _key(values=dnarr))
    assert _groupby(so, mixed, 2, varr, 1, 0, 6, (A.rdf_key_out * 2)(ko, ik), ov, oc) == BAD
    assert _groupby(so, keys, 1, dnarr, 1, 0, 6, kouts, ov, oc) == BAD
    ovd, _k12 = _out(A.I64, 8, mem=A.MEM_DEVICE)
    assert _groupby(so, keys, 1, varr, 1, 0, 6, kouts, ovd, oc) == BAD
    dko, _k13 = _text_key_out()
    dko.utf8_data.contents.mem = A.MEM_DEVICE
    assert _groupby(so, keys, 1, varr, 1, 0, 6, (A.rdf_key_out * 1)(dko), ov, oc) == BAD
    # chunk row counts that differ between key columns, and between keys and values
    short = _num_arr([A.HostArray.from_numpy(np.arange(4, dtype=np.int64))])
    two = (A.rdf_sort_key * 2)(_key(utf8=uarr), _key(values=short))
    assert _groupby(so, two, 2, varr, 1, 0, 6, (A.rdf_key_out * 2)(ko, ik), ov, oc) == A.RDF_COMPUTE_ERROR
    assert _groupby(so, keys, 1, short, 1, 0, 6, kouts, ov, oc) == A.RDF_COMPUTE_ERROR
    # capacities of the numeric outputs below min(max_groups, rows) + 2
    small, _k14 = _out(A.I64, 6)
    assert _groupby(so, keys, 1, varr, 1, 0, 6, kouts, small, oc) == A.RDF_MEMORY_ERROR
    assert _groupby(so, keys, 1, varr, 1, 0, 6, kouts, ov, small) == A.RDF_MEMORY_ERROR


# ---------------------------------------------------------------- join

def _join(so, lk, lnc, rk, rnc, nkeys, jt, ol, orr, rows=None):
    rows = rows if rows is not None else C.c_int64(-7)
    return so.rdf_equijoin_indices_keys(lk, C.c_int64(lnc), rk, C.c_int64(rnc), C.c_int32(nkeys), C.c_int32(jt), ol, orr, C.byref(rows))


def test_join_keys_checks_its_arguments_before_the_device(so):
    larr, rarr, narr = _utf8_arr([TEXT]), _utf8_arr([TEXT2]), _num_arr([INTS])
    lk, rk = (A.rdf_sort_key * 1)(_key(utf8=larr)), (A.rdf_sort_key * 1)(_key(utf8=rarr))
    ol, _k1 = _out(A.U32, 16)
    orr, _k2 = _out(A.U32, 16)
    # null lists / outputs
    assert _join(so, None, 1, rk, 1, 1, 2, ol, orr) == BAD
    assert _join(so, lk, 1, None, 1, 1, 2, ol, orr) == BAD
    assert _join(so, lk, 0, rk, 1, 1, 2, ol, orr) == BAD
    assert _join(so, lk, 1, rk, 0, 1, 2, ol, orr) == BAD
    assert _join(so, lk, 1, rk, 1, 1, 2, ol, None) == BAD
    assert _join(so, lk, 1, rk, 1, 1, 2, None, orr) == BAD
    assert so.rdf_equijoin_indices_keys(lk, C.c_int64(1), rk, C.c_int64(1), C.c_int32(1), C.c_int32(2), ol, orr, None) == BAD
    assert _join(so, lk, 1, rk, 1, 1, 4, ol, orr) == BAD
    for nk in (0, 5, -1):
        l5, r5 = (A.rdf_sort_key * 5)(*[_key(utf8=larr)] * 5), (A.rdf_sort_key * 5)(*[_key(utf8=rarr)] * 5)
        assert _join(so, l5, 1, r5, 1, nk, 2, ol, orr) == BAD, nk
    # a key that sets both pointers, or neither
    assert _join(so, (A.rdf_sort_key * 1)(_key(values=narr, utf8=larr)), 1, rk, 1, 1, 2, ol, orr) == BAD
    assert _join(so, lk, 1, (A.rdf_sort_key * 1)(_key()), 1, 1, 2, ol, orr) == BAD
    # a Utf8 key paired with a numeric one; numeric pairs of two dtypes
    nk1 = (A.rdf_sort_key * 1)(_key(values=narr))
    assert _join(so, lk, 1, nk1, 1, 1, 2, ol, orr) == BAD
    assert _join(so, nk1, 1, rk, 1, 1, 2, ol, orr) == BAD
    i32 = _num_arr([A.HostArray.from_numpy(np.arange(5, dtype=np.int32))])
    assert _join(so, nk1, 1, (A.rdf_sort_key * 1)(_key(values=i32)), 1, 1, 2, ol, orr) == BAD
    # wrong dtypes: inputs and outputs
    bad_in = _utf8_arr([TEXT])
    bad_in[0].data.dtype = A.I8
    assert _join(so, (A.rdf_sort_key * 1)(_key(utf8=bad_in)), 1, rk, 1, 1, 2, ol, orr) == BAD
    o64, _k3 = _out(A.U64, 16)
    assert _join(so, lk, 1, rk, 1, 1, 2, o64, orr) == BAD
    # mixed memory kinds
    drarr = _utf8_arr([TEXT2])
    drarr[0].offsets.mem = A.MEM_DEVICE
    drarr[0].data.mem = A.MEM_DEVICE
    assert _join(so, lk, 1, (A.rdf_sort_key * 1)(_key(utf8=drarr)), 1, 1, 2, ol, orr) == BAD
    od, _k4 = _out(A.U32, 16, mem=A.MEM_DEVICE)
    assert _join(so, lk, 1, rk, 1, 1, 2, od, orr) == BAD
    # chunk row counts that differ between the key columns of one side
    short = _num_arr([A.HostArray.from_numpy(np.arange(4, dtype=np.int64))])
    two = _num_arr([A.HostArray.from_numpy(np.arange(2, dtype=np.int64))])
    l2 = (A.rdf_sort_key * 2)(_key(utf8=larr), _key(values=short))
    r2 = (A.rdf_sort_key * 2)(_key(utf8=rarr), _key(values=two))
    assert _join(so, l2, 1, r2, 1, 2, 2, ol, orr) == A.RDF_COMPUTE_ERROR


# ---------------------------------------------------------------- no device

@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_loud_device_error_not_a_fallback(so):
    api = lib.api()
    calls = [lambda: api.utf8_dictionary_encode([TEXT]),
             lambda: api.utf8_dictionary_encode([]),
             lambda: api.groupby_agg_keys([[TEXT]], [INTS], "sum", 8),
             lambda: api.groupby_agg_keys([[TEXT], [INTS]], None, "count", 8),
             lambda: api.equijoin_indices_keys([[TEXT]], [[TEXT2]], "inner"),
             lambda: api.equijoin_indices_keys([[TEXT], [INTS]], [[TEXT2], [A.HostArray.from_numpy(np.arange(2, dtype=np.int64))]], "full")]
    for call in calls:
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
        assert "no CPU fallback" in ei.value.message
