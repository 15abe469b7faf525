#!/usr/bin/env python3
"""rdf_window on device-resident keys, each call set against the sort of the same keys taken in the same process.

  int_partitions  --rows (1e8) rows, one Int64 partition key with 1e2 / 1e4 / 1e6 / 1e8 distinct values + one Float64 order key
  no_partition    the Float64 order key alone
  utf8_partition  --utf8-rows (1e7) rows, a Utf8 partition key over 1000 distinct city-like values + the Float64 order key
  calls           1e4 partitions: one call (rank), all eight in one rdf_window, and the eight one after the other
  host            --host-rows (1e7) rows, keys and outputs in host memory: the transfer share

Yardstick: rdf_lexsort_to_indices over the same keys (partition keys, then order keys) — the sort the window call runs
first; the difference is what the window passes cost.  That difference is set against a byte model written down before the
first run.  Per row, streamed at this process's rdf_probe_stream copy rate: 12 B in the flag pass (perm 4, flag word 8),
32 B in the scan's two passes, 8 B in the start tables' pass, 12 B in the emit pass (scan word 8, perm 4), up to 16 B more
there for pstart[pid], pstart[pid + 1], gstart[gid], gstart[gid + 1] and scan[ps + 1] (neighbouring lanes share them: the
bound is reached when every row is its own partition), and per lag / lead output 4 B for perm[j -/+ o] and 1.125 B for the
pack pass over the validity bytes.  Random 128-byte lines at the 6.4 TB/s of lines DESIGN.md 4.0a quotes: one per key gather,
one per output scatter, and one more per lag / lead output for its scattered validity byte.

Timing: HIP events on the stream the library is told to use, around the WHOLE call, after --warmup calls, --reps (>= 10)
repetitions; best, median and the spread (max - min) / median.  One JSON line per measurement on stdout (and --out).

    python tools/bench_window.py [--rows 100000000] [--reps 10] [--only int,nopart,utf8,calls,host] [--out profiles/window.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rust_dataframe_amd import _abi as A  # noqa: E402
from rust_dataframe_amd import lib  # noqa: E402
from bench_utf8 import city_like  # noqa: E402

ALL = ["row_number", "rank", "dense_rank", "percent_rank", "cume_dist", ("ntile", 100), ("lag", 1), ("lead", 1)]
LINE_RATE = 6.4e12 / 128          # random 128-byte lines per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--utf8-rows", type=int, default=10_000_000)
    ap.add_argument("--host-rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="int,nopart,utf8,calls,host")
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
    only = set(args.only.split(","))
    pbytes = min(8 * n, 1 << 32)
    pa, pb = torch.empty(pbytes, dtype=torch.uint8, device="cuda"), torch.empty(pbytes, dtype=torch.uint8, device="cuda")
    read_gbps, _ = lib.probe_stream(0, pa.data_ptr(), 0, 0, pbytes, 10)
    copy_gbps, _ = lib.probe_stream(1, pa.data_ptr(), pb.data_ptr(), 0, pbytes, 10)
    del pa, pb
    emit({"op": "probe", "read_GBps": round(read_gbps, 1), "copy_GBps": round(copy_gbps, 1)})

    def model_ms(rows, nkeys, calls):
        nshift = sum((c[0] if isinstance(c, tuple) else c) in ("lag", "lead") for c in calls)
        streamed = 12 + 32 + 8 + 12 + 16 + nshift * (4 + 1.125)
        lines = nkeys + len(calls) + nshift
        return (streamed * rows / (copy_gbps * 1e9) + lines * rows / LINE_RATE) * 1e3

    def outs_for(calls, rows):
        return [api._window_out(A.window_out_dtype(A.WINDOW_FNS[c[0] if isinstance(c, tuple) else c]), rows, True,
                                (c[0] if isinstance(c, tuple) else c) in ("lag", "lead")) for c in calls]

    def case(label, part, order, rows, calls, extra=None):
        """part / order: key lists as Api.window takes them (device chunks)."""
        keys = [(k, False) for k in part] + [k if isinstance(k, tuple) else (k, False) for k in order]
        idx_t = torch.empty(rows + 64, dtype=torch.int32, device="cuda")
        idx = A.DeviceArray(idx_t.data_ptr(), None, 0, rows, A.U32, 0, keep=idx_t)
        ms_s = timed(lambda: api.lexsort_to_indices(keys, out=idx))
        outs = outs_for(calls, rows)
        ms_w = timed(lambda: api.window(part, order, calls, outs=outs, raw=True))
        rec = {"op": "window", "data": label, "rows": rows, "partition_keys": len(part), "order_keys": len(order), "calls": len(calls),
               "ms": round(ms_w[0], 3), "ms_median": round(ms_w[1], 3), "spread": round(ms_w[2], 3),
               "lexsort_ms": round(ms_s[0], 3), "lexsort_ms_median": round(ms_s[1], 3), "lexsort_spread": round(ms_s[2], 3),
               "window_passes_ms": round(ms_w[0] - ms_s[0], 3), "model_ms": round(model_ms(rows, len(keys), calls), 3),
               "window_over_lexsort": round(ms_w[0] / ms_s[0], 3), "kernels": lib.last_kernel()}
        rec.update(extra or {})
        emit(rec)
        return ms_w, ms_s

    def dev_f64(rows, col):
        t = torch.empty(rows + 64, dtype=torch.float64, device="cuda")
        lib.fill_uniform_f64(t.data_ptr(), rows, 42, col, 0, 0.0, 1.0)
        return [A.DeviceArray(t.data_ptr(), None, 0, rows, A.F64, 0, keep=t)]

    def dev_i64(rows, col, distinct):
        t = torch.empty(rows + 64, dtype=torch.int64, device="cuda")
        lib.fill_uniform_i64(t.data_ptr(), rows, 42, col, 0, 0, distinct)
        return [A.DeviceArray(t.data_ptr(), None, 0, rows, A.I64, 0, keep=t)]

    order = dev_f64(n, 0)
    if "int" in only:
        for distinct in (100, 10_000, 1_000_000, 100_000_000):
            case(f"int64_{distinct}_partitions", [dev_i64(n, 1, distinct)], [order], n, ["rank"], {"partitions": distinct})
    if "nopart" in only:
        case("no_partition_key", [], [order], n, ["rank"])
    if "calls" in only:
        part = [dev_i64(n, 1, 10_000)]
        one, sort_ms = case("1_call", part, [order], n, ["rank"], {"partitions": 10_000})
        eight, _ = case("8_calls_in_one", part, [order], n, ALL, {"partitions": 10_000})
        outs = [outs_for([c], n) for c in ALL]
        sep = timed(lambda: [api.window(part, [order], [c], outs=o, raw=True) for c, o in zip(ALL, outs)])
        emit({"op": "window_calls", "rows": n, "one_call_ms": round(one[0], 3), "eight_in_one_ms": round(eight[0], 3),
              "eight_separate_ms": round(sep[0], 3), "eight_separate_spread": round(sep[2], 3),
              "eight_in_one_over_one": round(eight[0] / one[0], 3), "eight_separate_over_in_one": round(sep[0] / eight[0], 3)})
        del outs
    if "utf8" in only:
        m = args.utf8_rows
        rng = np.random.default_rng(23)
        woffs, wdata, _v = city_like(rng, 1000, null_frac=0.0)
        pick = rng.integers(0, 1000, m)
        lens = np.diff(woffs)[pick]
        offs = np.zeros(m + 1, dtype=np.int64)
        offs[1:] = np.cumsum(lens)
        assert offs[-1] < 2**31
        d = torch.empty(int(offs[-1]) + 64, dtype=torch.uint8, device="cuda")
        row_of = torch.repeat_interleave(torch.arange(m, device="cuda"), torch.from_numpy(lens).cuda())
        pos = torch.arange(int(offs[-1]), device="cuda", dtype=torch.int64)
        pk = torch.from_numpy(pick).cuda()
        d[:int(offs[-1])] = torch.from_numpy(wdata).cuda()[torch.from_numpy(woffs[:-1]).cuda()[pk[row_of]] + (pos - torch.from_numpy(offs[:-1]).cuda()[row_of])]
        del row_of, pos
        ot = torch.from_numpy(offs.astype(np.int32)).cuda()
        text = [A.DeviceUtf8(ot.data_ptr(), d.data_ptr(), int(offs[-1]), m, None, 0, 0, 0, keep=(ot, d, None))]
        case("utf8_1000_partitions", [text], [dev_f64(m, 2)], m, ["rank"], {"partitions": 1000, "bytes": int(offs[-1])})
        case("int64_1000_partitions_same_rows", [dev_i64(m, 3, 1000)], [dev_f64(m, 2)], m, ["rank"], {"partitions": 1000})
    if "host" in only:
        h = args.host_rows
        rng = np.random.default_rng(5)
        part = [[A.HostArray.from_numpy(rng.integers(0, 10_000, h))]]
        ordr = [[A.HostArray.from_numpy(rng.random(h))]]
        for calls, label in ((["rank"], "host_1_call"), (ALL, "host_8_calls")):
            outs = [A.HostArray.empty_out(A.window_out_dtype(A.WINDOW_FNS[c[0] if isinstance(c, tuple) else c]), h,
                                          (c[0] if isinstance(c, tuple) else c) in ("lag", "lead")) for c in calls]
            ms = timed(lambda: api.window(part, ordr, calls, outs=outs, raw=True))
            dp = [[A.DeviceArray(t.data_ptr(), None, 0, h, c[0].dtype, 0, keep=t)] for c in (part[0], ordr[0])
                  for t in [torch.from_numpy(c[0].values).cuda()]]
            douts = outs_for(calls, h)
            ms_d = timed(lambda: api.window([dp[0]], [dp[1]], calls, outs=douts, raw=True))
            emit({"op": "window_host", "data": label, "rows": h, "calls": len(calls), "ms": round(ms[0], 3), "ms_median": round(ms[1], 3),
                  "spread": round(ms[2], 3), "device_resident_ms": round(ms_d[0], 3), "transfer_share": round(1 - ms_d[0] / ms[0], 3)})
    lib.set_stream(0)


if __name__ == "__main__":
    main()
