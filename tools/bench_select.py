#!/usr/bin/env python3
"""The conditional and NULL functions (rdf_coalesce / rdf_case_when / rdf_extremum / rdf_null_test) on device-resident columns,
set against two yardsticks taken in the same process: rdf_probe_stream's bare copy moving as many bytes as the entry must
read and write together, and rdf_binary(ADD) of two Float64 columns, the existing path that moves the same 24 bytes per row as
coalesce(a, b).

  entries    coalesce(a, 0) of Float64 and Int32 with 0 %, 1 % and 50 % NULLs; coalesce(a, b) of Float64 with 0 %, 1 % and
             50 % NULLs in a (--variant names the build: the A/B of skipping the parts no row of a pass takes is a second
             library built with -DRDF_SELECT_READ_ALL, run in alternation with the product build); case_when of three branches;
             greatest of 2 and of 8 Float64 columns; is_null; rdf_binary(ADD); rdf_utf8_coalesce(col, 'unknown') over --text-rows
             rows of ~24 bytes in 4 chunks with 10 % NULL rows, against rdf_utf8_trim of the same column (the existing writer:
             the same passes with one source span)
  timing     the library's own kernel timing (HIP events around the call's kernels on the library's stream), --warmup calls,
             then --reps (>= 10) repetitions: best, median and the spread (max - min) / median
  bytes      what the call MUST move: every column whose rows can matter, the output, + 1 bit per row for every bitmap read
             or written; of coalesce(a, b) the rows of b are counted only where a is NULL (8 bytes each)

One JSON line per measurement on stdout, appended to --out.

    python tools/bench_select.py [--rows 250000000] [--reps 10] [--variant NAME] [--out profiles/select_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rust_dataframe_amd import _abi as A  # noqa: E402
from rust_dataframe_amd import lib  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_utf8 import device_column, pool  # noqa: E402


def text_entries(args, api, torch, emit, copy_gbps):
    """rdf_utf8_coalesce(col, 'unknown') and rdf_utf8_trim on one text column: kernel ms, and the bytes both must move (offsets in and
    out, the row bytes in, the output bytes out) against the best copy rate the probe reached in this process."""
    so = lib.load()
    so.rdf_utf8_trim.restype = C.c_int
    nch = 4
    cr = args.text_rows // nch
    strings = pool(np.random.default_rng(31), 1 << 20, False)
    x, xb = device_column(torch, strings, cr)
    vx = torch.zeros((cr + 63) // 64 * 8 + 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib.fill_validity(vx.data_ptr(), cr, 7, 0, 0, 0.1)
    xn = [A.DeviceUtf8(x.offsets_ptr, x.data_ptr, x.data_length, cr, vx.data_ptr(), 0, 0, -1, keep=(x.keep, vx))] * nch
    ot = [torch.empty(cr + 1 + 64, dtype=torch.int32, device="cuda") for _ in range(nch)]
    vt = [torch.empty((cr + 63) // 64 * 8 + 8, dtype=torch.uint8, device="cuda") for _ in range(nch)]

    def timed(call, oo, od):
        ms = []
        for i in range(args.warmup + args.reps):
            lib.kernel_timing_reset(True)
            assert call(oo, od) == A.RDF_OK, so.rdf_last_error()
            ms.append(lib.kernel_timing_get()[0])
        lib.kernel_timing_reset(False)
        ms = ms[args.warmup:]
        med = float(np.median(ms))
        return {"kernel_ms": round(min(ms), 4), "kernel_ms_median": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 3)}

    def sized(call, nullable):
        oo = (A.rdf_out * nch)(*[A.rdf_out(t.data_ptr(), v.data_ptr() if nullable else None, cr + 1, 0, 0, A.I32, A.MEM_DEVICE) for t, v in zip(ot, vt)])
        od = (A.rdf_out * nch)(*[A.rdf_out(None, None, 0, 0, 0, A.U8, A.MEM_DEVICE) for _ in range(nch)])
        assert call(oo, od) in (A.RDF_OK, A.RDF_MEMORY_ERROR), so.rdf_last_error()
        out_bytes = [od[i].length for i in range(nch)]
        dt = [torch.empty(b + 64, dtype=torch.uint8, device="cuda") for b in out_bytes]
        od = (A.rdf_out * nch)(*[A.rdf_out(t.data_ptr(), None, b, 0, 0, A.U8, A.MEM_DEVICE) for t, b in zip(dt, out_bytes)])
        return oo, od, sum(out_bytes), dt

    carr = (A.rdf_utf8_array * nch)(*[c.c_struct() for c in xn])
    for op, call, nullable in (("utf8_trim_10pct_nulls", lambda oo, od: so.rdf_utf8_trim(carr, C.c_int64(nch), oo, od), True),
                               ("utf8_coalesce_col_literal_10pct_nulls", api.utf8_select_call([xn, "unknown"])[0], False)):
        oo, od, out_bytes, keep = sized(call, nullable)
        t = timed(call, oo, od)
        moved = 4 * (cr + 1) * nch * 2 + xb * nch + out_bytes + 2 * (cr // 8) * nch
        emit({"op": op, "rows": cr * nch, "chunks": nch, "in_bytes": xb * nch, "out_bytes": out_bytes, **t, "kernel": lib.last_kernel(), "bytes_moved": moved,
              "GBps": round(moved / t["kernel_ms"] / 1e6, 1), "copy_GBps": round(copy_gbps, 1), "frac_of_copy": round(moved / copy_gbps / 1e6 / t["kernel_ms"], 3),
              "variant": args.variant})
        del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--text-rows", type=int, default=100_000_000)
    ap.add_argument("--ab-only", action="store_true", help="only coalesce(a, b): the entries the two builds of the A/B differ in")
    ap.add_argument("--variant", default="skip unneeded parts", help="the build under test (recorded with coalesce(a, b))")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.jsonl"))
    args = ap.parse_args()
    import torch
    api = lib.api()
    assert lib.device_count() >= 1, "needs a GPU"
    lib.set_device(0)
    n = args.rows

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def one(call):
        lib.kernel_timing_reset(True)
        call()
        ms, _ = lib.kernel_timing_get()
        return ms

    def stats(ker):
        med = float(np.median(ker))
        return {"kernel_ms": round(min(ker), 4), "kernel_ms_median": round(med, 4), "spread": round((max(ker) - min(ker)) / med, 3)}

    def timed(call, ab=False):
        if args.ab_only and not ab:
            return None
        for _ in range(args.warmup):
            call()
        ker = [one(call) for _ in range(args.reps)]
        lib.kernel_timing_reset(False)
        return stats(ker)

    copies = {}
    src = torch.empty(40 * n + 64, dtype=torch.uint8, device="cuda")
    dst = torch.empty(40 * n + 64, dtype=torch.uint8, device="cuda")

    def copy_gbps(moved):
        half = int(moved // 2) // 16 * 16
        assert half <= 40 * n, "the probe's buffers hold 40 bytes per row"
        if half not in copies:
            copies[half] = lib.probe_stream(1, src.data_ptr(), dst.data_ptr(), 0, half, 10)
        return copies[half]

    f = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(8)]
    for k, t in enumerate(f):
        lib.fill_uniform_f64(t.data_ptr(), n, 42, k, 0, -1.0, 1.0)
    i32 = torch.randint(-1000, 1000, (n,), dtype=torch.int32, device="cuda")
    nbytes = (n + 63) // 64 * 8 + 64
    share = {"nulls_0pct": None, "nulls_1pct": 0.01, "nulls_50pct": 0.5}
    bitmaps = {}
    for k, (label, p) in enumerate(share.items()):
        if p is not None:
            bitmaps[label] = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            lib.fill_validity(bitmaps[label].data_ptr(), n, 7, k, 0, p)
    conds = []
    for k in range(3):                                               # three conditions, each true for a quarter of the rows
        c = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        lib.fill_validity(c.data_ptr(), n, 9, k, 0, 0.75)
        conds.append([A.DeviceArray(c.data_ptr(), None, 0, n, A.BOOL, 0, keep=(c, None))])
    lib.synchronize()
    bitmap = n / 8.0

    def col(t, dt, v=None):
        return [A.DeviceArray(t.data_ptr(), v.data_ptr() if v is not None else None, 0, n, dt, -1 if v is not None else 0, keep=(t, v))]

    o64 = [api._window_out(A.F64, n, True, True)]
    o32 = [api._window_out(A.I32, n, True, True)]
    ob = [api._window_out(A.BOOL, n, True, False)]

    def record(op, data, t, moved, **more):
        if t is None:
            return None
        gbps, shape = copy_gbps(moved)
        emit({"op": op, "data": data, "rows": n, **t, "kernel": lib.last_kernel(), "bytes_moved": int(moved), "GBps": round(moved / t["kernel_ms"] / 1e6, 1),
              "copy_GBps": round(gbps, 1), "copy_floor_ms": round(moved / gbps / 1e6, 4), "frac_of_copy": round(moved / gbps / 1e6 / t["kernel_ms"], 3), **more})
        return shape

    b = col(f[1], A.F64)
    shape = record("binary_add_f64", "nulls_0pct", timed(lambda: api.binary("add", col(f[0], A.F64), b, outs=o64)), 24.0 * n)
    for label, p in share.items():
        v = bitmaps.get(label)
        bm = 0.0 if v is None else bitmap
        a, ai = col(f[0], A.F64, v), col(i32, A.I32, v)
        record("coalesce_f64_literal", label, timed(lambda: api.coalesce([a, 0.0], outs=o64)), 16.0 * n + 2 * bm)
        record("coalesce_i32_literal", label, timed(lambda: api.coalesce([ai, 0], outs=o32)), 8.0 * n + 2 * bm)
        record("is_null_f64", label, timed(lambda: api.null_test("is_null", a, outs=ob)), 2 * bm if v is not None else bitmap)
        # coalesce(a, b): b's rows are counted where a is NULL (a build that reads every part moves all of b)
        moved = 16.0 * n + 8.0 * n * (p or 0.0) + 2 * bm
        record("coalesce_f64_two_columns", label, timed(lambda: api.coalesce([a, b], outs=o64), ab=True), moved, variant=args.variant)
    va = bitmaps["nulls_1pct"]
    vals = [col(f[k], A.F64, va if k == 0 else None) for k in range(4)]
    record("case_when_3_branches_f64", "conditions true for 1/4 each, 1 % NULLs in the first value",
           timed(lambda: api.case_when(conds, vals[:3], vals[3], outs=o64)), 40.0 * n + 3 * bitmap + 2 * bitmap)
    cols8 = [col(f[k], A.F64) for k in range(8)]
    record("greatest_2_f64", "nulls_0pct", timed(lambda: api.greatest(cols8[:2], outs=o64)), 24.0 * n)
    record("greatest_8_f64", "nulls_0pct", timed(lambda: api.greatest(cols8, outs=o64)), 72.0 * n)
    del f, i32, src, dst, o64, o32, ob, cols8, vals
    if not args.ab_only:
        text_entries(args, api, torch, emit, copies and max(v[0] for v in copies.values()))
    emit({"op": "copy_probe", "rows": n, "shape": shape, "sizes": {str(k): round(v[0], 1) for k, v in copies.items()}})


if __name__ == "__main__":
    main()
