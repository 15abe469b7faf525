#!/usr/bin/env python3
"""rdf_window_range_agg on device-resident keys and values, each call set against rdf_window_agg with the EQUIVALENT ROWS frame
in the same process.  The order keys are dense and unique inside every partition (0 .. rows / partitions - 1, shuffled), so
`s PRECEDING .. e FOLLOWING` in key units is the ROWS frame of the same numbers: the two calls give the same answer (checked
here, byte for byte) from the same sort and the same scans, and the difference of their times is what the value frame adds —
the sorted key gather, the window pass, the bounds pass, and 8 B per row and call more in the emit.

  --rows (5e7) rows, one Int64 partition key with 1e2 / 1e4 / 1e6 distinct values, the order key as Int64 and as Float64, one
  Float64 value column, SUM over
      narrow    7 PRECEDING .. CURRENT ROW               one distinct bound; every tile's window fits LDS
      narrow2   7 PRECEDING .. 7 FOLLOWING               two distinct bounds: the difference to `narrow` prices one bounds array
      wide      2 * WINDOW_RANGE_LDS_KEYS PRECEDING .. CURRENT ROW   wider than the window wherever partitions are that long:
                the global search
      narrow under rdf_set_option("window_range_route", 2)           the same frame on the global search: the LDS window's A/B

Byte model, written down before the first run.  Gather: 4 B of perm read, one random 128-byte line for the key, 8 B of key and
1 B of class written per row.  Bounds pass, per row and distinct bound: 8 B of key (and 1 B of class) read — once per tile for
the LDS route, the searches then probe LDS; per probe in L2 / HBM for the global route — and 4 B written; 12 B of scan word and
table entries per row.  Emit: 4 B per row and resolved frame end read.  Streamed at this process's rdf_probe_stream copy rate,
lines at the 6.4 TB/s DESIGN.md 4.0a quotes.

Timing: HIP events on the stream the library is told to use, around the WHOLE call, after --warmup calls, --reps (>= 10)
repetitions; best, median and the spread (max - min) / median.  One JSON line per measurement on stdout (and --out).

    python tools/bench_window_range.py [--rows 50000000] [--reps 10] [--out profiles/window_range.jsonl]
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

LINE_RATE = 6.4e12 / 128          # random 128-byte lines per second
NARROW = 7
WIDE = 2 * A.WINDOW_RANGE_LDS_KEYS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--partitions", default="100,10000,1000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    api = lib.api()
    assert lib.device_count() >= 1, "needs a GPU"
    lib.set_device(0)
    stream = torch.cuda.Stream()
    lib.set_stream(stream.cuda_stream)

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def timed(call):
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                call()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        return min(ms), med, (max(ms) - min(ms)) / med

    n = args.rows
    pbytes = min(8 * n, 1 << 32)
    pa, pb = torch.empty(pbytes, dtype=torch.uint8, device="cuda"), torch.empty(pbytes, dtype=torch.uint8, device="cuda")
    read_gbps, _ = lib.probe_stream(0, pa.data_ptr(), 0, 0, pbytes, 10)
    copy_gbps, _ = lib.probe_stream(1, pa.data_ptr(), pb.data_ptr(), 0, pbytes, 10)
    del pa, pb
    emit({"op": "probe", "read_GBps": round(read_gbps, 1), "copy_GBps": round(copy_gbps, 1)})

    def model_ms(nbounds):
        gather = (4 + 8 + 1) * n / (copy_gbps * 1e9) + n / LINE_RATE
        bounds = nbounds * (8 + 1 + 4) * n / (copy_gbps * 1e9) + 12 * n / (copy_gbps * 1e9)
        return gather * 1e3, bounds * 1e3

    def arr(t, dtype):
        return [A.DeviceArray(t.data_ptr(), None, 0, n, dtype, 0, keep=t)]

    def out():
        return [api._window_out(A.F64, n, True, True)]

    vt = torch.empty(n + 64, dtype=torch.float64, device="cuda")
    lib.fill_uniform_f64(vt.data_ptr(), n, 42, 3, 0, 0.0, 1.0)
    value = arr(vt, A.F64)
    for distinct in [int(p) for p in args.partitions.split(",")]:
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        perm = torch.randperm(n, device="cuda", generator=g)
        pt = (perm % distinct).contiguous()
        kt = torch.div(perm, distinct, rounding_mode="floor").contiguous()
        del perm
        part = arr(pt, A.I64)
        for kname, order in (("int64", arr(kt, A.I64)), ("float64", arr(kt.double(), A.F64))):
            conv = float if kname == "float64" else int
            cases = (("narrow", (-NARROW, 0), 1, 0), ("narrow2", (-NARROW, NARROW), 2, 0), ("wide", (-WIDE, 0), 1, 0), ("narrow", (-NARROW, 0), 1, 2))
            rows_ms = {}
            for label, (s, e), nbounds, route in cases:
                if (s, e) not in rows_ms:
                    ro = out()
                    rows_ms[(s, e)] = (timed(lambda: api.window_agg([part], [order], [value], [("sum", 0, ("rows", s, e))], outs=ro, raw=True)), ro)
                base, ro = rows_ms[(s, e)]
                go = out()
                lib.set_option("window_range_route", route)
                try:
                    ms = timed(lambda: api.window_range_agg([part], [order], [value], [("sum", 0, (conv(s), conv(e)))], outs=go, raw=True))
                    kernels = lib.last_kernel()
                finally:
                    lib.set_option("window_range_route", 0)
                torch.cuda.synchronize()
                same = bool(torch.equal(go[0].keep[0][:n], ro[0].keep[0][:n]) and torch.equal(go[0].keep[1][:n // 8], ro[0].keep[1][:n // 8]))
                gm, bm = model_ms(nbounds)
                emit({"op": "window_range_agg", "data": label, "key": kname, "route_option": route, "rows": n, "partitions": distinct, "frame": [s, e],
                      "ms": round(ms[0], 3), "ms_median": round(ms[1], 3), "spread": round(ms[2], 3), "rows_frame_ms": round(base[0], 3),
                      "rows_frame_spread": round(base[2], 3), "extra_ms": round(ms[0] - base[0], 3), "model_gather_ms": round(gm, 3),
                      "model_bounds_ms": round(bm, 3), "same_answer": same, "kernels": kernels})
                del go
            del rows_ms, order
        del part, pt, kt
        torch.cuda.empty_cache()
    lib.set_stream(0)


if __name__ == "__main__":
    main()
