#!/usr/bin/env python3
"""rdf_window_agg on device-resident keys and values, each call set against rdf_window(row_number) over the same keys in the
same process: the shared front (sort, flag pass, scan, start tables) plus one scattered Int64 output.

  partitions   --rows (1e8) rows, one Int64 partition key with 1e2 / 1e4 / 1e6 distinct values + one Float64 order key, one
               Float64 value column: SUM over ROWS UNBOUNDED PRECEDING .. CURRENT ROW alone, MIN over ROWS 99 PRECEDING ..
               CURRENT ROW alone (w = 100), and SUM + MIN + MAX + COUNT + AVG over ROWS 99 PRECEDING .. CURRENT ROW in one call
               against the same five as five calls

Byte model, written down before the first run.  Per row and per scan, streamed at this process's rdf_probe_stream copy rate:
12 B read in the segment pass (perm 4, scan word 8) and the payload written — 32 B for a Float64 sum (double-double 16 + two
packed count words 16), 16 B for an Int64 sum, 8 B for a min / max scan — plus, in the add-back pass, the payload read and
written again for the positions ahead of their segment's first restart: none of them when partitions are far shorter than a
4096-position segment, all of them (2 x payload more) when they are far longer.  One random 128-byte line per row per scan for
the value gathered through the permutation, at the 6.4 TB/s of lines DESIGN.md 4.0a quotes.  The emit pass: 28 B (scan word 8,
perm 4, up to 16 of table entries), per call the payload words at the frame's two ends (neighbouring lanes read neighbouring
words: streamed; sum 2 x 32 or 2 x 16 B, min / max 8 - 16 B), one random line for the scattered output, one for its scattered
validity byte (not for COUNT) and 1.125 B for the pack pass.  The yardstick's own emit (28 B + one line) is subtracted.

Timing: HIP events on the stream the library is told to use, around the WHOLE call, after --warmup calls, --reps (>= 10)
repetitions; best, median and the spread (max - min) / median.  One JSON line per measurement on stdout (and --out).

    python tools/bench_window_agg.py [--rows 100000000] [--reps 10] [--out profiles/window_agg.jsonl]
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
SEG = 4096
W = 100
RUNNING = ("rows", A.UNBOUNDED_PRECEDING, 0)
TRAILING = ("rows", -(W - 1), 0)
PAYLOAD = {"sumf": 32, "sumi": 16, "ext": 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
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

    def model_ms(rows, partitions, scans, calls):
        """scans: payload names; calls: (payload bytes read per frame end, scattered lines).  The value passes alone."""
        carried = min(1.0, max(0.0, 1.0 - SEG / (rows / partitions)))       # share of positions whose run began before their segment
        streamed = sum(12 + PAYLOAD[s] * (1 + 2 * carried) for s in scans)
        streamed += sum(2 * b + 1.125 * (lines - 1) for b, lines in calls)
        lines = len(scans) + sum(ln for _b, ln in calls) - 1                  # the yardstick's one scattered output is subtracted
        return (streamed * rows / (copy_gbps * 1e9) + lines * rows / LINE_RATE) * 1e3

    def dev_f64(rows, col):
        t = torch.empty(rows + 64, dtype=torch.float64, device="cuda")
        lib.fill_uniform_f64(t.data_ptr(), rows, 42, col, 0, 0.0, 1.0)
        return [A.DeviceArray(t.data_ptr(), None, 0, rows, A.F64, 0, keep=t)]

    def dev_i64(rows, col, distinct):
        t = torch.empty(rows + 64, dtype=torch.int64, device="cuda")
        lib.fill_uniform_i64(t.data_ptr(), rows, 42, col, 0, 0, distinct)
        return [A.DeviceArray(t.data_ptr(), None, 0, rows, A.I64, 0, keep=t)]

    def outs_for(calls):
        return [api._window_out(A.window_agg_out_dtype(A.WINDOW_AGG_FNS[f], A.F64), n, True, f != "count") for f, _v, _fr in calls]

    order, value = dev_f64(n, 0), dev_f64(n, 3)
    for distinct in [int(p) for p in args.partitions.split(",")]:
        part = dev_i64(n, 1, distinct)
        rn = [api._window_out(A.I64, n, True, False)]
        base = timed(lambda: api.window([part], [order], ["row_number"], outs=rn, raw=True))
        emit({"op": "window_row_number", "rows": n, "partitions": distinct, "ms": round(base[0], 3), "ms_median": round(base[1], 3),
              "spread": round(base[2], 3)})
        del rn
        five = [(f, 0, TRAILING) for f in ("sum", "min", "max", "count", "avg")]
        cases = (("sum_running", [("sum", 0, RUNNING)], ["sumf"], [(32, 2)]),
                 ("min_w100", [("min", 0, TRAILING)], ["ext", "ext"], [(8, 2)]),
                 ("five_in_one_w100", five, ["sumf", "ext", "ext", "ext", "ext"], [(32, 2), (8, 2), (8, 2), (8, 1), (32, 2)]))
        got = {}
        for label, calls, scans, reads in cases:
            outs = outs_for(calls)
            ms = timed(lambda: api.window_agg([part], [order], [value], calls, outs=outs, raw=True))
            got[label] = ms
            emit({"op": "window_agg", "data": label, "rows": n, "partitions": distinct, "calls": len(calls), "ms": round(ms[0], 3),
                  "ms_median": round(ms[1], 3), "spread": round(ms[2], 3), "row_number_ms": round(base[0], 3),
                  "value_passes_ms": round(ms[0] - base[0], 3), "model_ms": round(model_ms(n, distinct, scans, reads), 3),
                  "kernels": lib.last_kernel()})
            del outs
        outs = [outs_for([c]) for c in five]
        sep = timed(lambda: [api.window_agg([part], [order], [value], [c], outs=o, raw=True) for c, o in zip(five, outs)])
        emit({"op": "window_agg_calls", "rows": n, "partitions": distinct, "five_in_one_ms": round(got["five_in_one_w100"][0], 3),
              "five_separate_ms": round(sep[0], 3), "five_separate_spread": round(sep[2], 3),
              "five_separate_over_in_one": round(sep[0] / got["five_in_one_w100"][0], 3)})
        del outs, part
        torch.cuda.empty_cache()
    lib.set_stream(0)


if __name__ == "__main__":
    main()
