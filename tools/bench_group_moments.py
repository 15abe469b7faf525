#!/usr/bin/env python3
"""rdf_groupby_moments on device-resident columns, each call set against its own front (the count-only call on the same
keys), against rdf_moments' kernel on the same value column, and against the yardstick rdf_groupby_sorted(COUNT_DISTINCT)
on the same keys and value — all taken in the same process (this call changes no kernel or host path of the yardstick).

  data   --rows (5e7) rows, one Int64 key and one Float64 value 1e9 + U[0, 1); groups G in {1, 1e2, 1e6, rows}: row i holds
         key (i * 2654435761) mod G, so the groups are spread over the rows without a sort-friendly order; 0 and 10 % NULL
         values (rdf_fill_validity).
  call   rdf_groupby_moments with var_samp, stddev_samp, skewness and kurtosis, the first rows and the counts
  states the call without a statistic (counts only): front + level 0 + the levels of partials + a finish that writes the
         counts.  "levels_ms" = states - front, "statistics_ms" = call - states: what the four statistics, their validity
         bytes, the first rows and the packing cost.
  front  the count-only call (no outputs, no calls, no x) on the same key: sort_core over the key, the flag pass, the scan,
         the start tables and the 8-byte readback.  "fold_ms" = call - front: level 0, the levels of partials, the finish
         kernel and the packing of the validity bits.
  moments  rdf_moments on the value column: the streaming kernel that reads x once, in row order, without a gather

Timing: the library's own kernel timer (rdf_kernel_timing_*: HIP events around the kernels of a call) and HIP events around
the whole call, after --warmup calls, --reps repetitions; best, median and spread (max - min) / median of each.  One JSON
line per configuration on stdout (and --out).

    python tools/bench_group_moments.py [--rows 50000000] [--reps 5] [--out profiles/group_moments_bench.jsonl]
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

STATS = ["var_samp", "stddev_samp", "skewness", "kurtosis"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--groups", default="1,100,1000000,rows")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    api = lib.api()
    assert lib.device_count() >= 1, "needs a GPU"
    lib.set_device(0)
    stream = torch.cuda.Stream()
    lib.set_stream(stream.cuda_stream)
    n = args.rows

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
        return {"best": round(min(xs), 3), "median": round(med, 3), "spread": round((max(xs) - min(xs)) / med, 3)}

    def timed(call):
        for _ in range(args.warmup):
            call()
        runs = [once(call) for _ in range(args.reps)]
        return [r[0] for r in runs], [r[1] for r in runs]

    vt = torch.empty(n + 64, dtype=torch.float64, device="cuda")
    lib.fill_uniform_f64(vt.data_ptr(), n, 7, 1, 0, 0.0, 1.0)
    vt += 1e9
    bits = torch.zeros((n + 63) // 64 * 8 + 8, dtype=torch.uint8, device="cuda")
    lib.fill_validity(bits.data_ptr(), n, 7, 2, 0, 0.1)
    torch.cuda.synchronize()
    for G in [n if g == "rows" else int(g) for g in args.groups.split(",")]:
        i = torch.arange(n, dtype=torch.int64, device="cuda")
        kt = torch.empty(n + 64, dtype=torch.int64, device="cuda")
        kt[:n] = (i * 2654435761) % G
        del i
        torch.cuda.synchronize()
        K = [A.DeviceArray(kt.data_ptr(), None, 0, n, A.I64, 0, keep=kt)]
        for nulls in (0.0, 0.1):
            V = [A.DeviceArray(vt.data_ptr(), bits.data_ptr() if nulls else None, 0, n, A.F64, -1 if nulls else 0, keep=(vt, bits))]
            if nulls:
                V[0]._unknown_nc = True
            outs = [api._window_out(A.F64, n, True, True) for _ in STATS]
            rows_out, counts_out = api._window_out(A.U32, n, True, False), api._window_out(A.I64, n, True, False)
            ck, ce = timed(lambda: api.groupby_moments([K], V, stats=STATS, outs=outs, rows_out=rows_out, counts_out=counts_out, raw=True))
            kernels, groups = lib.last_kernel(), api.last_groups
            fk, fe = timed(lambda: api.groupby_moments([K], None, stats=[], group_rows=False, raw=True))
            assert api.last_groups == groups == min(G, n)
            sk, _ = timed(lambda: api.groupby_moments([K], V, stats=[], group_rows=False, counts_out=counts_out, raw=True))   # states and counts, no statistic
            mk, me = timed(lambda: api.moments(V))
            ys_outs, ys_rows = [api._window_out(A.I64, n, True, False)], api._window_out(A.U32, n, True, False)
            yk, ye = timed(lambda: api.groupby_sorted([K], V, ["count_distinct"], outs=ys_outs, rows_out=ys_rows, raw=True))
            emit({"op": "groupby_moments", "rows": n, "groups": groups, "null_fraction": nulls, "stats": len(STATS),
                  "kernel_ms": stats(ck), "call_ms": stats(ce), "front_kernel_ms": stats(fk), "front_call_ms": stats(fe),
                  "fold_ms": round(min(ck) - min(fk), 3), "states_kernel_ms": stats(sk), "levels_ms": round(min(sk) - min(fk), 3),
                  "statistics_ms": round(min(ck) - min(sk), 3), "moments_kernel_ms": stats(mk), "moments_call_ms": stats(me),
                  "sorted_count_distinct_kernel_ms": stats(yk), "sorted_count_distinct_call_ms": stats(ye),
                  "call_over_yardstick": round(min(ck) / min(yk), 3), "kernels": kernels})
        del kt, K
    lib.set_stream(0)


if __name__ == "__main__":
    main()
