#!/usr/bin/env python3
"""rdf_groupby_collect and rdf_list_explode on device-resident columns, each call set against its own front and against a
yardstick of the library that touches the same items, all taken in the same process.

  set      --rows (5e7) rows, one Int64 key, G in {1, 1e2, 1e6, rows} groups, an Int64 value with D in {G, rows} distinct
           (key, value) pairs (row i holds pair p = (i * 2654435761) mod D, key = p mod G, value = p div G).
           call = collect_set with all four outputs; front = rdf_groupby_sorted's count-only call over (key, value) as
           grouping columns (the identical sort, flags, scan, start tables); yardstick = rdf_groupby_sorted(COUNT_DISTINCT)
           with group rows.  "collect_own_ms" = call - front, "fold_own_ms" = yardstick - front; "compaction_ms" = the
           call without out_group_rows - front (SET takes the groups' first rows from a fold of their own).
  list     the same keys, value = the row number, with 0 % (the fast path: no validity) and 10 % NULL values.
           call = collect_list with all four outputs; front = the count-only rdf_groupby_sorted over the key alone;
           yardstick = rdf_window(ROW_NUMBER) partitioned by the key, whose emit pass also touches all rows once.
           "collect_own_ms" = call - front, "emit_ms" = yardstick - front.
  explode  --rows elements in three length distributions: every list of length 1, uniform lengths 0..20, one list holding
           everything among 1e6 empty ones; parent rows and child indices written.  The three times, their max / min ratio,
           and the bytes the passes move per element (model: per list row 4 read + 8 written by the count pass, 8 + 8 by the
           scan, 8 read by the expansion; per element 8 written) as a rate next to rdf_probe_stream's copy rate.

Timing: the library's own kernel timer (rdf_kernel_timing_*: HIP events around the kernels of a call) after --warmup calls,
--reps repetitions; best, median and spread (max - min) / median.  One JSON line per measurement on stdout (and --out).

    python tools/bench_collect.py [--rows 50000000] [--reps 5] [--only set,list,explode] [--out profiles/collect_bench.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="set,list,explode")
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
        with torch.cuda.stream(stream):
            lib.synchronize()
            lib.kernel_timing_reset(True)
            call()
            lib.synchronize()
            kms, _ = lib.kernel_timing_get()
            lib.kernel_timing_reset(False)
        return kms

    def stats(xs):
        med = float(np.median(xs))
        return {"best": round(min(xs), 3), "median": round(med, 3), "spread": round((max(xs) - min(xs)) / med, 3) if med else 0.0}

    def timed(call):
        for _ in range(args.warmup):
            call()
        return [once(call) for _ in range(args.reps)]

    def dev(t, dtype, validity=None):
        return [A.DeviceArray(t.data_ptr(), validity.data_ptr() if validity is not None else None, 0, n, dtype, -1 if validity is not None else 0,
                              keep=(t, validity))]

    def key_value(G, D):
        i = torch.arange(n, dtype=torch.int64, device="cuda")
        p = (i * 2654435761) % D
        kt, vt = torch.empty(n + 64, dtype=torch.int64, device="cuda"), torch.empty(n + 64, dtype=torch.int64, device="cuda")
        kt[:n], vt[:n] = p % G, p // G
        del i, p
        torch.cuda.synchronize()
        return kt, vt

    def collect_call(K, V, kind):
        outs = (api._window_out(A.U32, n, True, False), api._window_out(A.I32, n + 1, True, False),
                api._window_out(A.U32, n, True, False), api._window_out(A.I64, n, True, False))
        return lambda: api.groupby_collect([K], V, kind, outs=outs, raw=True)

    if "set" in only:
        for G in (1, 100, 1_000_000, n):
            for D in sorted({G, n}):
                kt, vt = key_value(G, D)
                K, V = dev(kt, A.I64), dev(vt, A.I64)
                ck = timed(collect_call(K, V, "set"))
                kernels, groups, elements = lib.last_kernel(), api.last_groups, api.last_elements
                fk = timed(lambda: api.groupby_sorted([K, V], None, [], group_rows=False, raw=True))
                yo, yr = [api._window_out(A.I64, n, True, False)], api._window_out(A.U32, n, True, False)
                yk = timed(lambda: api.groupby_sorted([K], V, ["count_distinct"], outs=yo, rows_out=yr, raw=True))
                nr = (None,) + tuple(api._window_out(dt, n + 1, True, False) for dt in (A.I32, A.U32, A.I64))
                nk = timed(lambda: api.groupby_collect([K], V, "set", outs=nr, raw=True))   # no group rows: the compaction alone
                own, fold = min(ck) - min(fk), min(yk) - min(fk)
                emit({"op": "collect_set", "rows": n, "groups": groups, "pairs": D, "elements": elements, "kernel_ms": stats(ck),
                      "front_kernel_ms": stats(fk), "count_distinct_kernel_ms": stats(yk), "collect_own_ms": round(own, 3),
                      "no_group_rows_kernel_ms": stats(nk), "compaction_ms": round(min(nk) - min(fk), 3), "fold_own_ms": round(fold, 3), "own_over_fold": round(own / fold, 2) if fold > 0 else None, "kernels": kernels})
    if "list" in only:
        for G in (1, 100, 1_000_000, n):
            kt, _ = key_value(G, n)
            K = dev(kt, A.I64)
            vt = torch.arange(n + 64, dtype=torch.int64, device="cuda")
            fk = timed(lambda: api.groupby_sorted([K], None, [], group_rows=False, raw=True))
            wo = [api._window_out(A.I64, n, True, False)]
            wk = timed(lambda: api.window([K], [], ["row_number"], outs=wo, raw=True))
            for nulls in (0.0, 0.1):
                bits = None
                if nulls:
                    bits = torch.zeros((n + 63) // 64 * 8 + 64, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    lib.fill_validity(bits.data_ptr(), n, 11, 3, 0, nulls)
                V = dev(vt, A.I64, bits)
                ck = timed(collect_call(K, V, "list"))
                own, em = min(ck) - min(fk), min(wk) - min(fk)
                emit({"op": "collect_list", "rows": n, "groups": api.last_groups, "null_fraction": nulls, "elements": api.last_elements,
                      "kernel_ms": stats(ck), "front_kernel_ms": stats(fk), "window_row_number_kernel_ms": stats(wk),
                      "collect_own_ms": round(own, 3), "emit_ms": round(em, 3), "own_over_emit": round(own / em, 2) if em > 0 else None,
                      "kernels": lib.last_kernel()})
    if "explode" in only:
        nb = 1 << 30
        a, b = torch.empty(nb, dtype=torch.uint8, device="cuda"), torch.empty(nb, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        copy_gbps, shape = lib.probe_stream(1, a.data_ptr(), b.data_ptr(), 0, nb, 5)
        del a, b
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        dists = {"ones": torch.ones(n, dtype=torch.int64, device="cuda"),
                 "uniform_0_20": torch.randint(0, 21, (n // 10,), generator=g, device="cuda", dtype=torch.int64),
                 "one_long_among_1e6_empty": torch.zeros(1_000_001, dtype=torch.int64, device="cuda")}
        dists["one_long_among_1e6_empty"][500_000] = n
        best = {}
        for name, lens in dists.items():
            rows = int(lens.numel())
            offs = torch.zeros(rows + 1 + 64, dtype=torch.int32, device="cuda")
            offs[1:rows + 1] = torch.cumsum(lens, 0).to(torch.int32)
            elements = int(offs[rows].item())
            child = A.DeviceArray(offs.data_ptr(), None, 0, 0, A.I64, 0)            # the child is never read
            lst = A.DeviceList(offs.data_ptr(), rows, child, None, 0, keep=offs)
            outs = (api._window_out(A.U32, elements, True, False), api._window_out(A.U32, elements, True, False), None)
            ek = timed(lambda: api.list_explode(lst, outs=outs, raw=True))
            assert api.last_rows == elements
            moved = rows * (4 + 8 + 16 + 8) + elements * 8
            best[name] = min(ek)
            emit({"op": "list_explode", "lengths": name, "list_rows": rows, "elements": elements, "kernel_ms": stats(ek),
                  "model_bytes_per_element": round(moved / elements, 2), "model_gbps": round(moved / min(ek) / 1e6, 1),
                  "probe_copy_gbps": round(copy_gbps, 1), "probe_shape": shape, "kernels": lib.last_kernel()})
        emit({"op": "list_explode_balance", "best_kernel_ms": {k: round(v, 3) for k, v in best.items()},
              "max_over_min": round(max(best.values()) / min(best.values()), 2)})
    lib.set_stream(0)


if __name__ == "__main__":
    main()
