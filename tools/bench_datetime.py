#!/usr/bin/env python3
"""The date and time functions (rdf_datetime_fields / rdf_datetime_trunc / rdf_date_shift / rdf_date_diff) on device-resident
columns, set against two yardsticks taken in the same process: rdf_probe_stream's bare copy moving as many bytes as the
entry reads and writes together, and rdf_hour (the interpreter's three opcodes) on the same column.

  entries    Timestamp(ns) -> year; Timestamp(ns) -> 8 fields in one call, against eight one-field calls; Date32 -> month;
             date_trunc(MONTH) of ns; add_months by a scalar; date_diff of two ns columns — each without NULLs and with 10 %
  timing     the library's own kernel timing (rdf_kernel_timing_reset / _get: HIP events around the call's kernels on the
             library's stream), --warmup calls, then --reps (>= 10) repetitions: best, median and the spread (max - min) /
             median; the whole call (tables, kernels, the NULL counts' copy) by the host clock next to it
  bytes      what the call must move: the column(s) read, the outputs written, + 1 bit per row for every bitmap read or written

One JSON line per measurement on stdout, appended to --out.

    python tools/bench_datetime.py [--rows 250000000] [--reps 10] [--out profiles/datetime_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rust_dataframe_amd import _abi as A  # noqa: E402
from rust_dataframe_amd import lib  # noqa: E402

FIELDS8 = ["year", "quarter", "month", "day_of_month", "day_of_week", "day_of_year", "week_of_year", "hour"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "datetime_bench.jsonl"))
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

    def timed(call):
        """-> kernel ms (best, median, spread), whole-call ms (best)"""
        for _ in range(args.warmup):
            call()
        ker, wall = [], []
        for _ in range(args.reps):
            lib.kernel_timing_reset(True)
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms, _ = lib.kernel_timing_get()
            ker.append(ms)
        lib.kernel_timing_reset(False)
        med = float(np.median(ker))
        return {"kernel_ms": round(min(ker), 4), "kernel_ms_median": round(med, 4), "spread": round((max(ker) - min(ker)) / med, 3),
                "call_ms": round(min(wall), 3)}

    # the copy yardstick, for the number of bytes an entry moves (half read, half written)
    copies = {}
    src = torch.empty(24 * n + 64, dtype=torch.uint8, device="cuda")
    dst = torch.empty(24 * n + 64, dtype=torch.uint8, device="cuda")

    def copy_gbps(moved):
        half = int(moved // 2) // 16 * 16
        assert half <= 24 * n, "the probe's buffers hold 24 bytes per row"
        if half not in copies:
            copies[half] = lib.probe_stream(1, src.data_ptr(), dst.data_ptr(), 0, half, 10)
        return copies[half]

    ts = torch.empty(n, dtype=torch.int64, device="cuda")
    ts2 = torch.empty(n, dtype=torch.int64, device="cuda")
    lib.fill_uniform_i64(ts.data_ptr(), n, 42, 0, 0, 0, 4_102_444_800_000_000_000)            # 1970 .. 2100 in nanoseconds
    lib.fill_uniform_i64(ts2.data_ptr(), n, 42, 1, 0, 0, 4_102_444_800_000_000_000)
    dates = torch.randint(-20_000, 50_000, (n,), dtype=torch.int32, device="cuda")
    nbytes = (n + 63) // 64 * 8 + 64
    v1, v2 = (torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2))
    lib.fill_validity(v1.data_ptr(), n, 7, 2, 0, 0.1)
    lib.fill_validity(v2.data_ptr(), n, 7, 3, 0, 0.1)
    lib.synchronize()
    bitmap = n / 8.0

    def col(t, dt, v=None):
        return [A.DeviceArray(t.data_ptr(), v.data_ptr() if v is not None else None, 0, n, dt, -1 if v is not None else 0, keep=(t, v))]

    o32 = [[api._window_out(A.I32, n, True, True)] for _ in range(8)]
    o64 = [api._window_out(A.I64, n, True, True)]
    NS, DAY = A.TIME_NANOSECOND, A.TIME_DAY

    for label, va, vb in (("no_nulls", None, None), ("nulls_10pct", v1, v2)):
        bm = 0.0 if va is None else bitmap
        a, b, d = col(ts, A.I64, va), col(ts2, A.I64, vb), col(dates, A.I32, va)
        t = timed(lambda: api.hour(a, NS, outs=o32[0]))
        hour_ms = t["kernel_ms"]
        moved = 12.0 * n + 2 * bm
        gbps, shape = copy_gbps(moved)
        emit({"op": "rdf_hour", "data": label, "rows": n, **t, "kernel": lib.last_kernel(), "bytes_moved": int(moved), "GBps": round(moved / t["kernel_ms"] / 1e6, 1),
              "copy_GBps": round(gbps, 1), "frac_of_copy": round(moved / gbps / 1e6 / t["kernel_ms"], 3)})
        eight = None
        cases = [("ns_to_year", lambda: api.datetime_fields(a, NS, ["year"], outs=o32[:1]), 12.0 * n + 2 * bm),
                 ("ns_to_hour", lambda: api.datetime_fields(a, NS, ["hour"], outs=o32[:1]), 12.0 * n + 2 * bm),
                 ("ns_to_8_fields_one_call", lambda: api.datetime_fields(a, NS, FIELDS8, outs=o32), 40.0 * n + 9 * bm),
                 ("ns_to_8_fields_eight_calls", lambda: [api.datetime_fields(a, NS, [f], outs=[o]) for f, o in zip(FIELDS8, o32)], 96.0 * n + 16 * bm),
                 ("date32_to_month", lambda: api.datetime_fields(d, DAY, ["month"], outs=o32[:1]), 8.0 * n + 2 * bm),
                 ("date_trunc_month_ns", lambda: api.datetime_trunc(a, NS, "month", outs=o64), 16.0 * n + 2 * bm),
                 ("add_months_scalar_ns", lambda: api.date_shift(a, NS, "months", 7, outs=o32[0]), 12.0 * n + 2 * bm),
                 ("date_diff_ns_ns", lambda: api.date_diff(a, NS, b, NS, outs=o32[0]), 20.0 * n + (0.0 if va is None else 3 * bitmap))]
        for op, call, moved in cases:
            if op == "ns_to_8_fields_eight_calls":      # eight calls: the kernel time of the call is that of its last kernel; time the calls one by one
                per = [timed(lambda f=f, o=o: api.datetime_fields(a, NS, [f], outs=[o])) for f, o in zip(FIELDS8, o32)]
                t = {"kernel_ms": round(sum(p["kernel_ms"] for p in per), 4), "kernel_ms_median": round(sum(p["kernel_ms_median"] for p in per), 4),
                     "spread": round(max(p["spread"] for p in per), 3), "call_ms": round(sum(p["call_ms"] for p in per), 3)}
            else:
                t = timed(call)
            gbps, shape = copy_gbps(moved / 8 if op == "ns_to_8_fields_eight_calls" else moved)   # (eight calls: eight copies of an eighth)
            rec = {"op": op, "data": label, "rows": n, **t, "kernel": lib.last_kernel(), "bytes_moved": int(moved), "GBps": round(moved / t["kernel_ms"] / 1e6, 1),
                   "copy_GBps": round(gbps, 1), "copy_floor_ms": round(moved / gbps / 1e6, 4), "frac_of_copy": round(moved / gbps / 1e6 / t["kernel_ms"], 3),
                   "over_hour_kernel": round(t["kernel_ms"] / hour_ms, 3)}
            if op == "ns_to_8_fields_one_call":
                eight = t["kernel_ms"]
            if op == "ns_to_8_fields_eight_calls":
                rec["over_one_call"] = round(t["kernel_ms"] / eight, 3)
            emit(rec)
    emit({"op": "copy_probe", "rows": n, "shape": shape, "sizes": {str(k): round(v[0], 1) for k, v in copies.items()}})


if __name__ == "__main__":
    main()
