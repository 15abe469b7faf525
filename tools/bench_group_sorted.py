#!/usr/bin/env python3
"""rdf_groupby_sorted on device-resident columns, each call set against its own front (the count-only call) and against
rdf_window's DENSE_RANK over the same keys, all taken in the same process.

  grid   --rows (5e7) rows, one Int64 key and one Int64 (or Float64, --f64) value column; groups G in {1, 1e2, 1e6, rows},
         distinct (key, value) pairs D in {G, sqrt(G * rows), rows}.  Row i holds pair p = (i * 2654435761) mod D, key = p mod G,
         value = p div G: the pairs are spread over the rows without a sort-friendly order.
  skew   D = rows, G = 1e4: the keys uniform, or ONE group holding half of the pairs; --alternate (>= 5) runs of each in turn
  hash   rdf_groupby_agg(COUNT) on the same key column: what the order and the exactness cost until a hash route exists

Front: the count-only call (no outputs, no calls) with the key AND the value column as grouping columns.  It runs the same
sort_core over (key, value), the flag pass, the scan, the start tables and the 8-byte readback, and stops there: its D groups
are the call's D pairs.  (The flag pass marks every pair as a partition start instead of a peer start and the partition
start table gets D entries instead of G: the same reads, at most 4 B more written per pair.)  "fold_own_ms" = call - front
is the fold alone: the zeroing of the NULL counters, the fold's levels and the packing of the validity bits.

Yardstick: rdf_window with one DENSE_RANK call, partition key = the grouping key, order key = the value column.  It runs the
identical front and then its emit pass over all rows (12 B streamed and one scattered 8-byte store per row), with no readback
in the middle.  "emit_ms" = yardstick - front is that pass; "fold_minus_emit_ms" = call - yardstick.

Timing: the library's own kernel timer (rdf_kernel_timing_*: HIP events around the kernels of a call) and HIP events around
the whole call, after --warmup calls, --reps repetitions; best, median and spread (max - min) / median of each.  One JSON
line per measurement on stdout (and --out).

    python tools/bench_group_sorted.py [--rows 50000000] [--reps 5] [--only grid,skew,hash] [--out profiles/group_sorted_bench.jsonl]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rust_dataframe_amd import _abi as A  # noqa: E402
from rust_dataframe_amd import lib  # noqa: E402

CALLS = ["count_distinct", "sum_distinct", "first", "last"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--alternate", type=int, default=5)
    ap.add_argument("--only", default="grid,skew,hash")
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
        return {"best": round(min(xs), 3), "median": round(med, 3), "spread": round((max(xs) - min(xs)) / med, 3)}

    def timed(call, reps=None):
        for _ in range(args.warmup):
            call()
        runs = [once(call) for _ in range(reps or args.reps)]
        return [r[0] for r in runs], [r[1] for r in runs]

    def columns(G, D, f64, skew=False):
        i = torch.arange(n, dtype=torch.int64, device="cuda")
        p = (i * 2654435761) % D
        if skew:      # one group holds the pairs below D / 2, the others share the rest
            key = torch.where(p < D // 2, torch.zeros_like(p), 1 + p % (G - 1))
            val = p
        else:
            key, val = p % G, p // G
        del i, p
        kt = torch.empty(n + 64, dtype=torch.int64, device="cuda")
        kt[:n] = key
        vt = torch.empty(n + 64, dtype=torch.float64 if f64 else torch.int64, device="cuda")
        vt[:n] = val.to(vt.dtype) * 0.5 if f64 else val
        del key, val
        torch.cuda.synchronize()
        return ([A.DeviceArray(kt.data_ptr(), None, 0, n, A.I64, 0, keep=kt)],
                [A.DeviceArray(vt.data_ptr(), None, 0, n, A.F64 if f64 else A.I64, 0, keep=vt)])

    def sorted_call(K, V):
        vdt = V[0].dtype
        outs = [api._window_out(A.group_sorted_out_dtype(A.GROUP_FNS[c], vdt), n, True, c in ("first", "last")) for c in CALLS]
        rows_out = api._window_out(A.U32, n, True, False)
        return lambda: api.groupby_sorted([K], V, CALLS, outs=outs, rows_out=rows_out, raw=True)

    def front_call(K, V):
        return lambda: api.groupby_sorted([K, V], None, [], group_rows=False, raw=True)

    def window_call(K, V):
        out = [api._window_out(A.I64, n, True, False)]
        return lambda: api.window([K], [V], ["dense_rank"], outs=out, raw=True)

    def case(label, G, D, f64, skew=False):
        K, V = columns(G, D, f64, skew)
        gs, fs, ws = sorted_call(K, V), front_call(K, V), window_call(K, V)
        gk, ge = timed(gs)
        kernels = lib.last_kernel()
        groups = api.last_groups
        fk, fe = timed(fs)
        assert api.last_groups == D, (api.last_groups, D)
        wk, we = timed(ws)
        emit({"op": "groupby_sorted", "data": label, "rows": n, "groups": groups, "pairs": D, "value": "f64" if f64 else "i64", "calls": len(CALLS),
              "kernel_ms": stats(gk), "call_ms": stats(ge), "front_kernel_ms": stats(fk), "front_call_ms": stats(fe),
              "window_dense_rank_kernel_ms": stats(wk), "window_dense_rank_call_ms": stats(we),
              "fold_own_ms": round(min(gk) - min(fk), 3), "emit_ms": round(min(wk) - min(fk), 3),
              "fold_minus_emit_ms": round(min(gk) - min(wk), 3), "kernels": kernels})
        return K, V

    if "grid" in only:
        for G in (1, 100, 1_000_000, n):
            for D in sorted({G, int(math.sqrt(G * n)), n}):
                if D < G:
                    continue
                case(f"G{G}_D{D}", G, D, False)
            case(f"G{G}_D{n}_f64", G, n, True)
    if "skew" in only:
        G = 10_000
        Ku, Vu = columns(G, n, False)
        Ks, Vs = columns(G, n, False, skew=True)
        calls = {"uniform": (sorted_call(Ku, Vu), front_call(Ku, Vu), window_call(Ku, Vu)),
                 "skewed": (sorted_call(Ks, Vs), front_call(Ks, Vs), window_call(Ks, Vs))}
        for gs, fs, ws in calls.values():
            gs(), fs(), ws()
        runs = {"uniform": [], "skewed": []}
        for _ in range(max(5, args.alternate)):
            for name, (gs, fs, ws) in calls.items():
                g, f, w = once(gs)[0], once(fs)[0], once(ws)[0]
                runs[name].append((g, f, w, g - f, g - w))

        def span(xs):
            return {"min": round(min(xs), 3), "median": round(float(np.median(xs)), 3), "max": round(max(xs), 3)}

        rec = {"op": "groupby_sorted_skew", "rows": n, "groups": G, "pairs": n, "runs": len(runs["uniform"])}
        for name, r in runs.items():
            rec[name] = {"kernel_ms": stats([x[0] for x in r]), "front_kernel_ms": stats([x[1] for x in r]),
                         "window_dense_rank_kernel_ms": stats([x[2] for x in r]),
                         "fold_own_ms": span([x[3] for x in r]), "fold_minus_emit_ms": span([x[4] for x in r])}
        emit(rec)
    if "hash" in only:
        for G in (100, 1_000_000):
            K, V = columns(G, n, False)
            outs = ([api._window_out(A.I64, G + 2, True, False)], api._window_out(A.I64, G + 2, True, False), api._window_out(A.I64, G + 2, True, False))
            hk, he = timed(lambda: api.groupby_agg([K], None, "count", G, outs=outs))
            kernels = lib.last_kernel()
            gk, ge = timed(sorted_call(K, V))
            emit({"op": "groupby_agg_count_vs_sorted", "rows": n, "groups": G, "pairs": n, "hash_count_kernel_ms": stats(hk), "hash_count_call_ms": stats(he),
                  "sorted_kernel_ms": stats(gk), "sorted_call_ms": stats(ge), "sorted_over_hash": round(min(gk) / min(hk), 2), "hash_kernels": kernels})
    lib.set_stream(0)


if __name__ == "__main__":
    main()
