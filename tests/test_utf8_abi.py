"""Utf8 columns at the C-ABI boundary, without a GPU: the rdf_utf8_array layout, argument checks before any device work,
RDF_DEVICE_ERROR with no device, and the committed case tables (rdf_unicode_case.h) against Python's own case mapping."""
import bisect
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import unicodedata

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_H = os.path.join(ROOT, "rust_dataframe_amd", "csrc", "rdf_unicode_case.h")
UNARY = ["trim", "ltrim", "rtrim", "substring", "lower", "upper"]


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    lib.api()
    for n in ["filter", "take"] + UNARY:
        getattr(s, "rdf_utf8_" + n).restype = C.c_int
    return s


def _outs(n, rows, validity=True, cap=0):
    keep = []
    oo, od = (A.rdf_out * max(1, n))(), (A.rdf_out * max(1, n))()
    for i in range(n):
        ob = np.zeros(rows + 1, dtype=np.int32)
        vb = np.zeros(64, dtype=np.uint8)
        db = np.zeros(max(cap, 1), dtype=np.uint8)
        keep.append((ob, vb, db))
        oo[i] = A.rdf_out(ob.ctypes.data, vb.ctypes.data if validity else None, rows + 1, 0, 0, A.I32, A.MEM_HOST)
        od[i] = A.rdf_out(db.ctypes.data if cap else None, None, cap, 0, 0, A.U8, A.MEM_HOST)
    return oo, od, keep


def _call(so, name, carr, n, oo, od, mask=None, idx=None):
    fn = getattr(so, "rdf_utf8_" + name)
    if name == "filter":
        return fn(carr, mask, C.c_int64(n), oo, od)
    if name == "take":
        return fn(carr, C.c_int64(n), idx, oo, od)
    if name == "substring":
        return fn(carr, C.c_int64(n), C.c_int64(1), C.c_int64(2), oo, od)
    return fn(carr, C.c_int64(n), oo, od)


def test_utf8_struct_matches_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rdf_mi355x.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(rdf_utf8_array), offsetof(rdf_utf8_array, offsets), offsetof(rdf_utf8_array, data));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        size, o_off, o_data = map(int, subprocess.check_output([exe], text=True).split())
    assert size == C.sizeof(A.rdf_utf8_array)
    assert o_off == A.rdf_utf8_array.offsets.offset
    assert o_data == A.rdf_utf8_array.data.offset


def test_every_entry_point_checks_its_arguments_before_the_device(so):
    h = A.HostUtf8.from_pylist(["ab", None, "cde"])
    good = (A.rdf_utf8_array * 1)(h.c_struct())
    mask_h = A.HostArray.from_numpy(np.array([1, 0, 1], dtype=bool), dtype=A.BOOL)   # (the arrays own the buffers)
    idx_h = A.HostArray.from_numpy(np.array([2, 0], dtype=np.uint32))
    mask = (A.rdf_array * 1)(mask_h.c_struct())
    idx = (A.rdf_array * 1)(idx_h.c_struct())
    for name in ["filter", "take"] + UNARY:
        rows = 2 if name == "take" else 3
        # null chunk list / null outputs
        oo, od, _k = _outs(1, rows)
        assert _call(so, name, None, 1, oo, od, mask, idx) == A.RDF_INVALID_ARGUMENT, name
        assert _call(so, name, good, 1, None, None, mask, idx) == A.RDF_INVALID_ARGUMENT, name
        assert _call(so, name, good, -1, oo, od, mask, idx) == A.RDF_INVALID_ARGUMENT, name
        # offsets must be Int32, data UInt8
        bad = (A.rdf_utf8_array * 1)(h.c_struct())
        bad[0].offsets.dtype = A.I64
        assert _call(so, name, bad, 1, oo, od, mask, idx) == A.RDF_INVALID_ARGUMENT, name
        bad = (A.rdf_utf8_array * 1)(h.c_struct())
        bad[0].data.dtype = A.I8
        assert _call(so, name, bad, 1, oo, od, mask, idx) == A.RDF_INVALID_ARGUMENT, name
        # mixed memory spaces
        bad = (A.rdf_utf8_array * 1)(h.c_struct())
        bad[0].data.mem = A.MEM_DEVICE
        assert _call(so, name, bad, 1, oo, od, mask, idx) == A.RDF_INVALID_ARGUMENT, name
        # NULL rows without an output validity buffer
        oo2, od2, _k2 = _outs(1, rows, validity=False)
        assert _call(so, name, good, 1, oo2, od2, mask, idx) == A.RDF_INVALID_ARGUMENT, name
        # wrong output dtypes
        oo3, od3, _k3 = _outs(1, rows)
        od3[0].dtype = A.I32
        assert _call(so, name, good, 1, oo3, od3, mask, idx) == A.RDF_INVALID_ARGUMENT, name
        assert b"utf8_" in so.rdf_last_error()
    oo, od, _k = _outs(1, 3)
    # filter: mask of the wrong length / type, no mask
    short_h = A.HostArray.from_numpy(np.array([1, 0], dtype=bool), dtype=A.BOOL)
    short = (A.rdf_array * 1)(short_h.c_struct())
    assert so.rdf_utf8_filter(good, short, C.c_int64(1), oo, od) == A.RDF_INVALID_ARGUMENT
    ints_h = A.HostArray.from_numpy(np.array([1, 0, 1], dtype=np.int32))
    ints = (A.rdf_array * 1)(ints_h.c_struct())
    assert so.rdf_utf8_filter(good, ints, C.c_int64(1), oo, od) == A.RDF_INVALID_ARGUMENT
    assert so.rdf_utf8_filter(good, None, C.c_int64(1), oo, od) == A.RDF_INVALID_ARGUMENT
    # take: signed / missing indices
    sidx_h = A.HostArray.from_numpy(np.array([0], dtype=np.int32))
    sidx = (A.rdf_array * 1)(sidx_h.c_struct())
    assert so.rdf_utf8_take(good, C.c_int64(1), sidx, oo, od) == A.RDF_INVALID_ARGUMENT
    assert so.rdf_utf8_take(good, C.c_int64(1), None, oo, od) == A.RDF_INVALID_ARGUMENT
    # substring: negative position or length
    assert so.rdf_utf8_substring(good, C.c_int64(1), C.c_int64(-1), C.c_int64(1), oo, od) == A.RDF_INVALID_ARGUMENT
    assert so.rdf_utf8_substring(good, C.c_int64(1), C.c_int64(0), C.c_int64(-2), oo, od) == A.RDF_INVALID_ARGUMENT
    # offsets too short for the rows: the rows are known up front, so this is the sizing rule's error before any device work
    oo4, od4, _k4 = _outs(1, 1)
    assert so.rdf_utf8_lower(good, C.c_int64(1), oo4, od4) == A.RDF_MEMORY_ERROR
    assert oo4[0].length == 4


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error_for_every_utf8_entry_point(so):
    h = A.HostUtf8.from_pylist(["ab", None, "cde"])
    good = (A.rdf_utf8_array * 1)(h.c_struct())
    mask_h = A.HostArray.from_numpy(np.array([1, 0, 1], dtype=bool), dtype=A.BOOL)   # (the arrays own the buffers)
    idx_h = A.HostArray.from_numpy(np.array([2, 0], dtype=np.uint32))
    mask = (A.rdf_array * 1)(mask_h.c_struct())
    idx = (A.rdf_array * 1)(idx_h.c_struct())
    for name in ["filter", "take"] + UNARY:
        oo, od, _k = _outs(1, 2 if name == "take" else 3)
        assert _call(so, name, good, 1, oo, od, mask, idx) == A.RDF_DEVICE_ERROR, name
        assert b"no CPU fallback" in so.rdf_last_error()
    api = lib.api()
    with pytest.raises(A.RdfError) as ei:
        api.utf8_unary("lower", [h])
    assert ei.value.status == A.RDF_DEVICE_ERROR


def _table(src, name):
    m = re.search(r"\b%s\[\d+\] = \{(.*?)\};" % name, src, re.S)
    return [int(x, 0) for x in m.group(1).replace("\n", " ").split(",") if x.strip()]


def test_case_tables_reproduce_python_case_mapping_for_every_code_point():
    src = open(CASE_H).read()
    assert f'RDF_UNICODE_VERSION "{unicodedata.unidata_version}"' in src
    flag_stride2 = int(re.search(r"RDF_CASE_FLAG_STRIDE2 (0x[0-9a-f]+)u", src).group(1), 16)
    flag_multi = int(re.search(r"RDF_CASE_FLAG_MULTI (0x[0-9a-f]+)u", src).group(1), 16)

    def mapper(name):
        st, info, delta, multi = (_table(src, f"k_{name}_{t}") for t in ("start", "info", "delta", "multi"))

        def f(c):   # the device's lookup (rdf_utf8.hip: case_map)
            i = bisect.bisect_right(st, c) - 1
            if i < 0:
                return chr(c)
            d, stride = c - st[i], 2 if info[i] & flag_stride2 else 1
            if d % stride or d // stride >= (info[i] & 0xFFFF):
                return chr(c)
            if info[i] & flag_multi:
                e = multi[4 * delta[i]:4 * delta[i] + 4]
                return "".join(chr(x) for x in e[1:1 + e[0]])
            return chr(c + delta[i])
        return f
    lower, upper = mapper("lower"), mapper("upper")
    bad = [c for c in range(0x110000) if not 0xD800 <= c <= 0xDFFF and (lower(c) != chr(c).lower() or upper(c) != chr(c).upper())]
    assert bad == []
    # the one-to-many mappings the issue names
    assert lower(0x130) == "i̇" and upper(0xDF) == "SS" and upper(0x149) == "ʼN" and len(upper(0x390)) == 3


def test_final_sigma_sets_describe_pythons_rule():
    src = open(CASE_H).read()
    cl, ch = _table(src, "k_cased_lo"), _table(src, "k_cased_hi")
    il, ih = _table(src, "k_case_ignorable_lo"), _table(src, "k_case_ignorable_hi")

    def member(lo, hi, c):
        i = bisect.bisect_right(lo, c) - 1
        return i >= 0 and c <= hi[i]
    for c in (ord("A"), ord("z"), 0x3A3, 0x1F88):
        assert member(cl, ch, c)
    for c in (ord("'"), ord("."), 0x300, 0xAD):
        assert member(il, ih, c) and not member(cl, ch, c)
    assert not member(cl, ch, ord(" ")) and not member(il, ih, ord(" "))


def test_generator_reproduces_the_committed_header():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_unicode_case.py"), "--check"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr


def test_host_utf8_round_trips_python_and_arrow():
    pa = pytest.importorskip("pyarrow")
    rows = ["a", None, "", "农历新年", "ß"]
    h = A.HostUtf8.from_pylist(rows, row_offset=3, data_offset=5)
    assert h.to_pylist() == rows
    assert h.to_arrow().to_pylist() == rows
    arr = pa.array(["x", "yy", None, "zzz", "w"], type=pa.string()).slice(1, 3)
    assert A.HostUtf8.from_arrow(arr).to_pylist() == ["yy", None, "zzz"]
