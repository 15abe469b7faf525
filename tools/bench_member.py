#!/usr/bin/env python3
"""rdf_member_mask and rdf_first_occurrence on device-resident Int64 columns.

  semi    --left (1e8) Int64 left rows, key = (i * 2654435761) mod (2 * D), against a right side of D distinct keys 0 .. D - 1
          (about half the left rows match), D in --right (1e3, 1e5, 1e7, 1e8), once distinct and once every key ten times.
          Both forms of the probe where both can run ("member_route" 1 / 2).  Set against the library's bare reader
          (rdf_probe_stream, read-only) over the same left bytes in the same process — the floor: one read of the left keys —
          and against rdf_equijoin_indices(INNER) over the same keys, count-only and with the pairs written: what a caller
          had to do before (followed by a de-duplication of the left indices, which is not timed here).
  first   --rows (5e7) Int64 rows, key = (i * 2654435761) mod G, G in (1, 1e2, 1e6, rows): rdf_first_occurrence(KEEP_FIRST)
          against rdf_groupby_sorted(FIRST) and rdf_groupby_agg(COUNT) over the same keys; "folds_without_atomic" is what
          the load-and-compare in front of the atomic saved (from rdf_last_kernel).

Timing: the library's own kernel timer (rdf_kernel_timing_*: HIP events around the kernels of a call), after --warmup calls,
--reps repetitions of every measurement in alternation (one round runs every variant once); best, median and spread
(max - min) / median.  One JSON line per measurement on stdout (and --out).

    python tools/bench_member.py [--left 100000000] [--rows 50000000] [--reps 5] [--only semi,first] [--out profiles/member_bench.jsonl]
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rust_dataframe_amd import _abi as A  # noqa: E402
from rust_dataframe_amd import lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--left", type=int, default=100_000_000)
    ap.add_argument("--right", default="1000,100000,10000000,100000000")
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="semi,first")
    ap.add_argument("--join", type=int, default=1, help="0: skip the rdf_equijoin_indices comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    api = lib.api()
    assert lib.device_count() >= 1, "needs a GPU"
    lib.set_device(0)
    stream = torch.cuda.Stream()
    lib.set_stream(stream.cuda_stream)
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
        return {"best": round(min(xs), 3), "median": round(med, 3), "spread": round((max(xs) - min(xs)) / med, 3) if med > 0 else 0.0}

    def alternate(variants):
        """variants: name -> call.  Every round runs every variant once.  -> name -> kernel ms of every round"""
        for _ in range(args.warmup):
            for call in variants.values():
                call()
        runs = {name: [] for name in variants}
        for _ in range(args.reps):
            for name, call in variants.items():
                runs[name].append(once(call))
        return runs

    def column(values):
        n = values.numel()
        t = torch.empty(n + 64, dtype=torch.int64, device="cuda")
        t[:n] = values
        return A.DeviceArray(t.data_ptr(), None, 0, n, A.I64, 0, keep=(t, None))

    def keys(n, mod):
        i = torch.arange(n, dtype=torch.int64, device="cuda")
        return column((i * 2654435761) % mod)

    if "semi" in only:
        n = args.left
        mask = [api._window_out(A.BOOL, n, True, False)]
        for D in [int(x) for x in args.right.split(",")]:
            L = [keys(n, 2 * D)]
            gbps, _shape = lib.probe_stream(0, L[0].values_ptr, nbytes=n * 8)
            floor_ms = n * 8 / (gbps * 1e9) * 1e3
            for dup in (1, 10):
                if D * dup > 200_000_000:
                    continue
                Rr = [column(torch.arange(D * dup, dtype=torch.int64, device="cuda") % D)]
                plan_lds = D * dup <= 4096

                def member(route):
                    def call():
                        lib.set_option("member_route", route)
                        try:
                            api.member_mask([L], [Rr], "semi", outs=mask)
                        finally:
                            lib.set_option("member_route", 0)
                    return call
                variants = {"hbm": member(2)}
                if plan_lds:
                    variants["lds"] = member(1)
                if args.join:
                    variants["inner_join_count"] = lambda: api.equijoin_indices_keys([L], [Rr], "inner", count_only=True)
                    pairs = api.equijoin_indices_keys([L], [Rr], "inner", count_only=True)
                    if pairs <= 1_500_000_000:
                        jo = (api._window_out(A.U32, pairs, True, True), api._window_out(A.U32, pairs, True, True))
                        variants["inner_join"] = lambda: api.equijoin_indices_keys([L], [Rr], "inner", outs=jo)
                runs = alternate(variants)
                member(0)()
                rec = {"op": "member_mask_semi", "left_rows": n, "right_rows": D * dup, "right_distinct": D, "planned": "lds" if plan_lds else "hbm",
                       "true_rows": api.last_out_rows, "reader_gbps": round(gbps, 1), "floor_ms": round(floor_ms, 3), "kernels": lib.last_kernel()}
                for name, xs in runs.items():
                    rec[name + "_kernel_ms"] = stats(xs)
                    rec[name + "_over_floor"] = round(min(xs) / floor_ms, 2)
                emit(rec)
                del Rr
            del L

    if "first" in only:
        n = args.rows
        mask = [api._window_out(A.BOOL, n, True, False)]
        for G in (1, 100, 1_000_000, n):
            K = [keys(n, G)]
            gs_outs = [api._window_out(A.U32, n, True, False)]
            gs_rows = api._window_out(A.U32, n, True, False)
            cap = min(G, n) + 2
            ga_outs = ([api._window_out(A.I64, cap, True, False)], api._window_out(A.I64, cap, True, False), api._window_out(A.I64, cap, True, False))
            variants = {
                "first_occurrence": lambda: api.first_occurrence([K], "first", outs=mask),
                "groupby_sorted_first": lambda: api.groupby_sorted([K], K, ["first"], outs=gs_outs, rows_out=gs_rows, raw=True),
                "groupby_agg_count": lambda: api.groupby_agg([K], None, "count", min(G, n), outs=ga_outs),
            }
            runs = alternate(variants)
            variants["first_occurrence"]()
            m = re.search(r"\((\d+) of (\d+) folds without an atomic\)", lib.last_kernel())
            gbps, _shape = lib.probe_stream(0, K[0].values_ptr, nbytes=n * 8)
            rec = {"op": "first_occurrence_keep_first", "rows": n, "distinct": api.last_out_rows, "reader_gbps": round(gbps, 1),
                   "floor_ms": round(n * 8 / (gbps * 1e9) * 1e3, 3), "folds_without_atomic": int(m.group(1)) if m else None,
                   "folds": int(m.group(2)) if m else None}
            for name, xs in runs.items():
                rec[name + "_kernel_ms"] = stats(xs)
            rec["sorted_over_first_occurrence"] = round(min(runs["groupby_sorted_first"]) / min(runs["first_occurrence"]), 2)
            rec["count_over_first_occurrence"] = round(min(runs["groupby_agg_count"]) / min(runs["first_occurrence"]), 2)
            emit(rec)
            del K
    lib.set_stream(0)


if __name__ == "__main__":
    main()
