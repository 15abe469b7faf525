#!/usr/bin/env python3
"""rdf_moments / rdf_comoments on a device-resident Float64 column, set against two yardsticks taken in the same process:
rdf_avg's kernel on the same column (the nearest existing whole-column aggregate) and rdf_probe_stream's bare read.

  variants   no NULLs, 10 % NULLs, and with a mask (a Boolean column with 10 % NULLs of its own that keeps half the rows)
  timing     the library's own kernel timing (rdf_kernel_timing_reset / _get: HIP events around the kernel on the library's
             stream), --warmup calls, then --reps (>= 10) repetitions: best, median and the spread (max - min) / median; the
             whole call (staging tables, the kernel, the states' copy and the host fold) by the host clock next to it
  bytes      8 B/row and column, + 1 bit per row and bitmap: the least the call must read

One JSON line per measurement on stdout, appended to --out.

    python tools/bench_moments.py [--rows 250000000] [--reps 10] [--out profiles/moments_bench.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=250_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_bench.jsonl"))
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
        """-> kernel ms (best, median, spread), launches per call, whole-call ms (best)"""
        for _ in range(args.warmup):
            call()
        ker, wall, launches = [], [], 0
        for _ in range(args.reps):
            lib.kernel_timing_reset(True)
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms, launches = lib.kernel_timing_get()
            ker.append(ms)
        lib.kernel_timing_reset(False)
        med = float(np.median(ker))
        return {"kernel_ms": round(min(ker), 4), "kernel_ms_median": round(med, 4), "spread": round((max(ker) - min(ker)) / med, 3),
                "launches": launches, "call_ms": round(min(wall), 3)}

    pbytes = 8 * n
    pt = torch.empty(pbytes, dtype=torch.uint8, device="cuda")
    read_gbps, read_shape = lib.probe_stream(0, pt.data_ptr(), 0, 0, pbytes, 10)
    del pt
    emit({"op": "read_probe", "rows": n, "GBps": round(read_gbps, 1), "shape": read_shape})

    x = torch.empty(n, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    lib.fill_uniform_f64(x.data_ptr(), n, 42, 0, 0, 1e9, 1e9 + 1.0)            # the column the textbook formula loses
    lib.fill_uniform_f64(y.data_ptr(), n, 42, 1, 0, -1.0, 1.0)
    nbytes = (n + 63) // 64 * 8 + 64
    vx, vm, bits = (torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(3))
    lib.fill_validity(vx.data_ptr(), n, 7, 2, 0, 0.1)
    lib.fill_validity(vm.data_ptr(), n, 7, 3, 0, 0.1)
    lib.fill_validity(bits.data_ptr(), n, 7, 4, 0, 0.5)
    lib.synchronize()

    plain = [A.DeviceArray(x.data_ptr(), None, 0, n, A.F64, 0, keep=x)]
    nulls = [A.DeviceArray(x.data_ptr(), vx.data_ptr(), 0, n, A.F64, -1, keep=(x, vx))]
    other = [A.DeviceArray(y.data_ptr(), None, 0, n, A.F64, 0, keep=y)]
    mask = [A.DeviceArray(bits.data_ptr(), vm.data_ptr(), 0, n, A.BOOL, -1, keep=(bits, vm))]
    bitmap = n / 8.0

    avg = {}
    for label, col, must in (("no_nulls", plain, 8.0 * n), ("nulls_10pct", nulls, 8.0 * n + bitmap)):
        t = timed(lambda: api.avg(col))
        avg[label] = t["kernel_ms"]
        emit({"op": "avg", "data": label, "rows": n, **t, "kernel": lib.last_kernel(), "bytes_read": int(must),
              "GBps": round(must / t["kernel_ms"] / 1e6, 1), "frac_of_read": round(must / read_gbps / 1e6 / t["kernel_ms"], 3)})

    cases = [("moments", "no_nulls", lambda: api.moments(plain), 8.0 * n, "no_nulls"),
             ("moments", "nulls_10pct", lambda: api.moments(nulls), 8.0 * n + bitmap, "nulls_10pct"),
             ("moments", "masked", lambda: api.moments(nulls, mask), 8.0 * n + 3 * bitmap, "nulls_10pct"),
             ("comoments", "no_nulls", lambda: api.comoments(plain, other), 16.0 * n, "no_nulls"),
             ("comoments", "nulls_10pct", lambda: api.comoments(nulls, other), 16.0 * n + bitmap, "nulls_10pct"),
             ("comoments", "masked", lambda: api.comoments(nulls, other, mask), 16.0 * n + 3 * bitmap, "nulls_10pct")]
    for op, label, call, must, against in cases:
        st = call()
        t = timed(call)
        emit({"op": op, "data": label, "rows": n, "counted": st.count, **t, "kernel": lib.last_kernel(), "bytes_read": int(must),
              "GBps": round(must / t["kernel_ms"] / 1e6, 1), "read_floor_ms": round(must / read_gbps / 1e6, 4),
              "frac_of_read": round(must / read_gbps / 1e6 / t["kernel_ms"], 3), "over_avg_kernel": round(t["kernel_ms"] / avg[against], 3)})


if __name__ == "__main__":
    main()
