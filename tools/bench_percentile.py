#!/usr/bin/env python3
"""rdf_groupby_percentile on device-resident columns.

  group   --rows (5e7) rows, one Int64 key, a Float64 and an Int64 value column, G in {1, 1e2, 1e6, rows} groups; row i holds
          key = (i * 2654435761) mod G.  The call (median + p90 + a DISC median, group rows and counts) is set against its own
          front — the count-only call with key AND value as grouping columns: the same sort_core, flag pass, scan and start
          tables — and against rdf_groupby_sorted(COUNT_DISTINCT) on the same input in the same process, the yardstick.
          "pick_own_ms" = call - front is the pick kernel, the fold for the group rows and the packing.
  whole   one column of Int8 / Int16 / Int32 / Int64 / Float64 with 10 % NULLs in four distributions — uniform, lognormal, all-equal,
          two-valued — with 1 call (the median) and 8 calls (4 CONT + 4 DISC), on the select route and with the sorted route
          forced, next to the library's bare reader (rdf_probe_stream, read-only) over the same value bytes: the floor of the
          select route is one read of the column, "bytes_moved" = its values and its validity bitmap, at the reader's rate.
          "select_over_floor" = select kernel time / (bytes_moved / reader GB/s).  The reader repeats its read, so over a column
          that fits the last-level cache (256 MiB: every dtype at 5e7 rows but the 8-byte ones' 400 MB only in part) its rate
          is a CACHE rate and the floor a cache floor ("floor_kind"); at 1e9 rows of 8 bytes it is an HBM floor.

Timing: the library's own kernel timer (rdf_kernel_timing_*: HIP events around the kernels of a call) and HIP events around the
whole call, after --warmup calls, --reps repetitions; best, median and spread (max - min) / median of each.  One JSON line per
measurement on stdout (and --out).

    python tools/bench_percentile.py [--rows 50000000] [--reps 5] [--only group,whole] [--dtypes i8,i16,i32,i64,f64] [--out profiles/percentile_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rust_dataframe_amd import _abi as A  # noqa: E402
from rust_dataframe_amd import lib  # noqa: E402

GROUP_CALLS = ["median", ("cont", 0.9), ("disc", 0.5)]
ONE = ["median"]
EIGHT = ["median", ("cont", 0.25), ("cont", 0.75), ("cont", 0.99), ("disc", 0.5), ("disc", 0.05), ("disc", 0.95), ("disc", 0.999)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="group,whole")
    ap.add_argument("--dtypes", default="i8,i16,i32,i64,f64")
    ap.add_argument("--dists", default="uniform,lognormal,equal,two")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    api = lib.api()
    assert lib.device_count() >= 1, "needs a GPU"
    lib.set_device(0)
    stream = torch.cuda.Stream()
    lib.set_stream(stream.cuda_stream)
    n = args.rows
    only = set(args.only.split(","))

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def once(call):
        """-> (kernel ms by the library's timer, ms by HIP events around the call)"""
        with torch.cuda.stream(stream):
            lib.synchronize()
            lib.kernel_timing_reset(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            lib.synchronize()
            kms, _ = lib.kernel_timing_get()
            lib.kernel_timing_reset(False)
        return kms, e0.elapsed_time(e1)

    def stats(xs):
        med = float(np.median(xs))
        return {"best": round(min(xs), 3), "median": round(med, 3), "spread": round((max(xs) - min(xs)) / med, 3) if med > 0 else 0.0}

    def timed(call):
        for _ in range(args.warmup):
            call()
        runs = [once(call) for _ in range(args.reps)]
        return [r[0] for r in runs], [r[1] for r in runs]

    def device_array(t, dtype, bitmap=None):
        return A.DeviceArray(t.data_ptr(), bitmap.data_ptr() if bitmap is not None else None, 0, n, dtype, 0, keep=(t, bitmap))

    def percentile_call(K, V, calls, route):
        outs = [api._window_out(A.F64 if kind == A.PCT_CONT else A.U32, n if K else 1, True, True) for kind, _ in A.percentile_calls(calls)]
        rows_out = api._window_out(A.U32, n if K else 1, True, False)
        counts_out = api._window_out(A.I64, n if K else 1, True, False)

        def call():
            lib.set_option("percentile_route", route)
            try:
                api.groupby_percentile(K, V, calls, outs=outs, rows_out=rows_out, counts_out=counts_out, raw=True)
            finally:
                lib.set_option("percentile_route", 0)
        return call

    if "group" in only:
        for f64 in (True, False):
            for G in (1, 100, 1_000_000, n):
                i = torch.arange(n, dtype=torch.int64, device="cuda")
                kt = torch.empty(n + 64, dtype=torch.int64, device="cuda")
                kt[:n] = (i * 2654435761) % G
                vt = torch.empty(n + 64, dtype=torch.float64 if f64 else torch.int64, device="cuda")
                v = (i * 40503) % 1_000_003
                vt[:n] = v.to(torch.float64) * 0.5 if f64 else v
                del i, v
                torch.cuda.synchronize()
                K, V = [device_array(kt, A.I64)], [device_array(vt, A.F64 if f64 else A.I64)]
                pk, pe = timed(percentile_call([K], V, GROUP_CALLS, 1))
                kernels, groups = lib.last_kernel(), api.last_groups
                fk, fe = timed(lambda: api.groupby_percentile([K, V], None, [], group_rows=False, raw=True))
                cd_outs = [api._window_out(A.I64, n, True, False)]
                cd_rows = api._window_out(A.U32, n, True, False)
                ck, ce = timed(lambda: api.groupby_sorted([K], V, ["count_distinct"], outs=cd_outs, rows_out=cd_rows, raw=True))
                emit({"op": "groupby_percentile", "rows": n, "groups": groups, "value": "f64" if f64 else "i64", "calls": len(GROUP_CALLS),
                      "kernel_ms": stats(pk), "call_ms": stats(pe), "front_kernel_ms": stats(fk), "front_call_ms": stats(fe),
                      "count_distinct_kernel_ms": stats(ck), "count_distinct_call_ms": stats(ce),
                      "pick_own_ms": round(min(pk) - min(fk), 3), "minus_count_distinct_ms": round(min(pk) - min(ck), 3), "kernels": kernels})
                del K, V, kt, vt

    if "whole" in only:
        TORCH = {"i8": (torch.int8, A.I8), "i16": (torch.int16, A.I16), "i32": (torch.int32, A.I32), "i64": (torch.int64, A.I64), "f64": (torch.float64, A.F64)}
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7)
        nb = (n + 7) // 8
        bits = (torch.rand(nb * 8, device="cuda", generator=gen) > 0.1).to(torch.uint8).reshape(nb, 8)
        bitmap = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        bitmap[:nb] = (bits * torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], device="cuda", dtype=torch.uint8)).sum(dim=1).to(torch.uint8)
        del bits
        for name in args.dtypes.split(","):
            tdt, adt = TORCH[name]
            top = 100.0 if name == "i8" else 3e4 if name == "i16" else 1e9
            for dist in args.dists.split(","):
                if dist == "uniform":
                    x = (torch.rand(n, device="cuda", generator=gen, dtype=torch.float64) * 2 - 1) * top
                elif dist == "lognormal":
                    x = torch.exp(torch.randn(n, device="cuda", generator=gen, dtype=torch.float64) * 2.0).clamp(max=top)
                elif dist == "equal":
                    x = torch.full((n,), 42.0, device="cuda", dtype=torch.float64)
                else:
                    x = torch.where(torch.rand(n, device="cuda", generator=gen) < 0.3, 7.0, -7.0).to(torch.float64)
                vt = torch.zeros(n + 64, dtype=tdt, device="cuda")
                vt[:n] = x.to(tdt)
                del x
                torch.cuda.synchronize()
                V = [device_array(vt, adt, bitmap)]
                nbytes = n * vt.element_size()
                gbps, shape = lib.probe_stream(0, vt.data_ptr(), nbytes=nbytes // 16 * 16)
                bytes_moved = nbytes + nb                  # one read: the values and the validity bitmap
                floor_ms = bytes_moved / (gbps * 1e9) * 1e3
                floor_kind = "cache" if nbytes <= 256 * 1024 * 1024 else "hbm"      # a column below the 256 MiB of last-level cache is re-read from it
                for label, calls in (("1", ONE), ("8", EIGHT)):
                    sk, se = timed(percentile_call([], V, calls, 2))
                    sel_kernels = lib.last_kernel()
                    ok, oe = timed(percentile_call([], V, calls, 1))
                    emit({"op": "percentile_whole_column", "rows": n, "dtype": name, "dist": dist, "calls": int(label), "nulls": 0.1,
                          "select_kernel_ms": stats(sk), "select_call_ms": stats(se), "sorted_kernel_ms": stats(ok), "sorted_call_ms": stats(oe),
                          "reader_gbps": round(gbps, 1), "bytes_moved": bytes_moved, "floor_ms": round(floor_ms, 4), "floor_kind": floor_kind, "select_over_floor": round(min(sk) / floor_ms, 2),
                          "sorted_over_select": round(min(ok) / min(sk), 2), "select_kernels": sel_kernels, "sorted_kernels": lib.last_kernel()})
                del V, vt
    lib.set_stream(0)


if __name__ == "__main__":
    main()
