#!/usr/bin/env python3
"""rdf_groupby_multi beside its yardstick, on device-resident columns: ONE call with K aggregates against K calls of
rdf_groupby_agg (the single-aggregate engine, unchanged) over the same columns in the same process.

  shape     --rows (5e7) rows, one Int64 key of G distinct sparse values, K value columns alternating Float64 / Int64, call c =
            (sum, min, max)[c % 3] of column c.  G in {100, rdf_groupby_multi_capacity(K), 1e5, 1e6}, K in {2, 4, 8}.
  multi     api.groupby_multi(..., max_groups = G): the planned route (the LDS route up to the capacity, the table beyond);
            --route 1 / 2 forces one.
  single    K x api.groupby_agg(..., max_groups = G).
Both sides allocate their outputs inside the timed call and end in the library's own stream synchronise, so a host clock
around the call is the call time.  After --warmup calls of each, --reps (>= 10) repetitions ALTERNATING the two sides; best,
median and spread (max - min) / median of each, and the ratio of the medians (single / multi: above 1, the one call wins).
Before timing, the two sides' integer results are compared group for group.  One JSON line per (G, K) on stdout, appended to
--out (default profiles/groupby_multi_bench.jsonl).

    python tools/bench_groupby_multi.py [--rows 50000000] [--reps 10] [--route 0] [--out profiles/groupby_multi_bench.jsonl]
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

AGGS = ("sum", "min", "max")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route", type=int, default=0)
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--groups", default="100,capacity,100000,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupby_multi_bench.jsonl"))
    args = ap.parse_args()
    import torch
    api = lib.api()
    assert lib.device_count() >= 1, "needs a GPU"
    lib.set_device(0)
    n = args.rows
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)

    def dev(t, dtype):
        return A.DeviceArray(t.data_ptr(), None, 0, t.numel(), dtype, 0, keep=(t, None))

    vals = []
    for v in range(max(int(k) for k in args.ks.split(","))):
        if v % 2 == 0:
            vals.append([dev(torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) * 200.0 - 100.0, A.F64)])
        else:
            vals.append([dev(torch.randint(-1_000_000, 1_000_000, (n,), generator=gen, device="cuda", dtype=torch.int64), A.I64)])

    def host(o):
        t, _ = o.keep
        return t.cpu().numpy().view(A.NP_OF[o.dtype])[:o.length].copy()

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def stats(ms):
        med = float(np.median(ms))
        return round(min(ms), 3), round(med, 3), round((max(ms) - min(ms)) / med, 3)

    lib.set_option("groupby_multi_route", args.route)
    for k in [int(x) for x in args.ks.split(",")]:
        calls = [(AGGS[c % 3], c) for c in range(k)]
        for gs in args.groups.split(","):
            g = api.groupby_multi_capacity(k) if gs == "capacity" else int(gs)
            keys = [[dev(torch.randint(0, g, (n,), generator=gen, device="cuda", dtype=torch.int64) * 7919 - 1234567, A.I64)]]

            def multi():
                return api.groupby_multi(keys, vals[:k], calls, g, with_rows=False)

            def single():
                res = []
                for c in range(k):
                    odt = A.F64 if c % 2 == 0 else A.I64
                    outs = ([A.Api._window_out(A.I64, g + 2, True, False)], A.Api._window_out(odt, g + 2, True, False), A.Api._window_out(A.I64, g + 2, True, False))
                    res.append(api.groupby_agg(keys, vals[c], AGGS[c % 3], g, outs=outs))
                return res

            # the same answers first: integer aggregates group for group (float sums differ in their last bits by design)
            mk, mo, mc, _ = multi()
            multi_kernel = lib.last_kernel()
            order = np.argsort(host(mk[0]), kind="stable")
            for c, (sk, so, sc) in enumerate(single()):
                so_order = np.argsort(host(sk[0]), kind="stable")
                assert (host(mk[0])[order] == host(sk[0])[so_order]).all(), "keys differ"
                assert (host(mc[c])[order] == host(sc)[so_order]).all(), f"counts of call {c} differ"
                if c % 2 == 1 or AGGS[c % 3] != "sum":
                    assert (host(mo[c])[order].view(np.uint64) == host(so)[so_order].view(np.uint64)).all(), f"values of call {c} differ"
            single_kernel = lib.last_kernel()
            for _ in range(args.warmup):
                multi()
                single()
            tm, ts = [], []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                multi()
                t1 = time.perf_counter()
                single()
                t2 = time.perf_counter()
                tm.append((t1 - t0) * 1e3)
                ts.append((t2 - t1) * 1e3)
            m, s = stats(tm), stats(ts)
            emit({"op": "groupby_multi_vs_k_calls", "rows": n, "groups": g, "k": k, "route_option": args.route, "multi_kernel": multi_kernel,
                  "single_kernel": single_kernel, "multi_ms": m[0], "multi_ms_median": m[1], "multi_spread": m[2],
                  "single_ms": s[0], "single_ms_median": s[1], "single_spread": s[2], "single_over_multi": round(s[1] / m[1], 3)})
            del keys
    lib.set_option("groupby_multi_route", 0)


if __name__ == "__main__":
    main()
