#!/usr/bin/env python3
"""Column::hist / Column::uniques on device-resident columns, each set against a yardstick taken in the same process.

  hist          --rows (1e9) Float64 rows, uniform on [0, 1) and one-hot (a constant column), nbins 10 / 1000 / 1e5 / 2^20,
                with range = (0, 1) and without (then a min / max pass comes first).  Yardstick: rdf_probe_stream's read
                rate x the bytes the call must read (8 B/row with a range, 16 B/row without).
  uniques       --rows Int64 rows x {10, 1e6} distinct values and --distinct-rows (1e8) rows all distinct.  Yardstick: the
                only other device route to the same answer, rdf_groupby_agg(COUNT, values = NULL, max_groups = the true
                count), run here on the same column.
  utf8_uniques  the three --utf8-rows (1e7) inputs of tools/bench_utf8.py --sort (city-like rows with 10 % NULLs, the same
                behind a 1 KiB common prefix — cut to the rows whose distinct values still fit ONE output chunk of 2^31 - 1
                bytes —, rows over 1000 distinct values), hash route and forced exact route.
                Yardstick: rdf_lexsort_to_indices on the same input.

Timing: HIP events on the stream the library is told to use (rdf_set_stream), recorded around the WHOLE call, after
--warmup calls, --reps (>= 10) repetitions; best, median and the spread (max - min) / median are reported.
One JSON line per measurement on stdout (and appended to --out).

    python tools/bench_colstats.py [--rows 1000000000] [--reps 10] [--only hist,uniques,utf8] [--out profiles/colstats.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--distinct-rows", type=int, default=100_000_000)
    ap.add_argument("--utf8-rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="hist,uniques,utf8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    api = lib.api()
    assert lib.device_count() >= 1, "needs a GPU"
    lib.set_device(0)
    stream = torch.cuda.Stream()
    lib.set_stream(stream.cuda_stream)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def timed(call):
        """-> (best, median, spread) in ms of HIP events around the whole call."""
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

    def stats(ms):
        return {"ms": round(ms[0], 3), "ms_median": round(ms[1], 3), "spread": round(ms[2], 3)}

    n = args.rows
    only = set(args.only.split(","))

    # the read rate this process reaches (rdf_probe_stream kind 0)
    pbytes = min(8 * n, 1 << 33)
    pt = torch.empty(pbytes, dtype=torch.uint8, device="cuda")
    read_gbps, read_shape = lib.probe_stream(0, pt.data_ptr(), 0, 0, pbytes, 10)
    del pt
    emit({"op": "read_probe", "GBps": round(read_gbps, 1), "shape": read_shape})

    if "hist" in only:
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        lib.fill_uniform_f64(x.data_ptr(), n, 42, 0, 0, 0.0, 1.0)
        hot = torch.full((n,), 0.375, dtype=torch.float64, device="cuda")
        for name, t in (("uniform", x), ("one_hot", hot)):
            col = [A.DeviceArray(t.data_ptr(), None, 0, n, A.F64, 0, keep=t)]
            for nbins in (10, 1000, 100_000, 2**20):
                outs = (api._stats_out(A.I64, nbins, True), api._stats_out(A.F64, nbins + 1, True))
                for rng in ((0.0, 1.0), None):
                    ms = timed(lambda: api.hist(col, nbins, rng, outs=outs))
                    must = (8 if rng else 16) * n
                    floor_ms = must / read_gbps / 1e6
                    emit({"op": "hist", "data": name, "rows": n, "nbins": nbins, "range": bool(rng), **stats(ms),
                          "bytes_read": must, "GBps": round(must / ms[0] / 1e6, 1), "read_floor_ms": round(floor_ms, 3),
                          "frac_of_read": round(floor_ms / ms[0], 3)})
        del x, hot

    if "uniques" in only:
        def uniq_case(label, t, rows, expect):
            col = [A.DeviceArray(t.data_ptr(), None, 0, rows, A.I64, 0, keep=t)]
            torch.cuda.synchronize()
            true_count = api.uniques(col, count_only=True)
            assert true_count == expect, (true_count, expect)
            out = api._stats_out(A.I64, true_count, True)
            got = api.uniques(col, out=out).length
            assert got == true_count, (got, true_count)
            ms_u = timed(lambda: api.uniques(col, out=out))
            route = lib.last_kernel()
            cap = true_count + 2
            gouts = ([api._stats_out(A.I64, cap, True)], api._stats_out(A.I64, cap, True), api._stats_out(A.I64, cap, True))
            ms_g = timed(lambda: api.groupby_agg([col], None, "count", true_count, outs=gouts))
            assert gouts[0][0].length == true_count
            emit({"op": "uniques", "data": label, "rows": rows, "distinct": true_count, "route": route, **stats(ms_u),
                  "groupby_count_ms": round(ms_g[0], 3), "groupby_count_ms_median": round(ms_g[1], 3), "groupby_count_spread": round(ms_g[2], 3),
                  "uniques_over_groupby": round(ms_u[0] / ms_g[0], 3), "read_floor_ms": round(8 * rows / read_gbps / 1e6, 3)})

        k = torch.empty(n, dtype=torch.int64, device="cuda")
        for distinct in (10, 1_000_000):
            lib.fill_uniform_i64(k.data_ptr(), n, 7, 1, 0, 0, distinct)
            uniq_case(f"{distinct}_distinct", k, n, distinct)
        del k
        m = args.distinct_rows
        p = torch.randperm(m, device="cuda", dtype=torch.int64) * 3 - 11
        uniq_case("all_distinct", p, m, m)
        del p

    if "utf8" in only:
        rng = np.random.default_rng(23)
        m = args.utf8_rows

        def dev_chunks(offs, data, valid, nch):
            dd = torch.from_numpy(data).cuda() if isinstance(data, np.ndarray) else data
            per = (len(offs) - 1 + nch - 1) // nch
            out = []
            for c in range(nch):
                r0, r1 = c * per, min((c + 1) * per, len(offs) - 1)
                o = offs[r0:r1 + 1] - offs[r0]
                assert o[-1] < 2**31
                ot = torch.from_numpy(o.astype(np.int32)).cuda()
                vt = torch.from_numpy(A.pack_bits(valid[r0:r1])).cuda() if valid is not None else None
                out.append(A.DeviceUtf8(ot.data_ptr(), dd.data_ptr() + int(offs[r0]), int(o[-1]), r1 - r0,
                                        vt.data_ptr() if vt is not None else None, 0, 0, -1, keep=(ot, dd, vt)))
            return out

        def utf8_case(label, col, nbytes):
            m = sum(c.length for c in col)
            idx_t = torch.empty(m + 64, dtype=torch.int32, device="cuda")
            idx = A.DeviceArray(idx_t.data_ptr(), None, 0, m, A.U32, 0, keep=idx_t)
            ms_s = timed(lambda: api.lexsort_to_indices([(col, False)], out=idx))
            rec = {"op": "utf8_uniques", "data": label, "rows": m, "bytes": int(nbytes), "lexsort_ms": round(ms_s[0], 3),
                   "lexsort_ms_median": round(ms_s[1], 3), "lexsort_spread": round(ms_s[2], 3)}
            for route, key in ((0, "hash"), (1, "exact")):
                lib.set_option("uniques_route", route)
                r = api.utf8_uniques(col)
                rec["distinct"] = r.length
                ms = timed(lambda: api.utf8_uniques(col))          # (one call: the outputs are sized from the input)
                rec[key + "_route"] = lib.last_kernel()
                rec[key + "_ms"], rec[key + "_ms_median"], rec[key + "_spread"] = round(ms[0], 3), round(ms[1], 3), round(ms[2], 3)
                rec[key + "_over_lexsort"] = round(ms[0] / ms_s[0], 3)
            lib.set_option("uniques_route", 0)
            emit(rec)

        offs, data, valid = city_like(rng, m)
        utf8_case("city_like", dev_chunks(offs, data, valid, 1), offs[-1])
        # the same rows behind a 1 KiB common prefix (built on the device, 8 chunks).  Nearly every row is distinct and the
        # distinct values come back as ONE chunk with Int32 offsets: only as many rows as stay below 2^31 bytes are used.
        P = 1024
        m = min(m, (2**31 - 2**24) // (P + 24))
        valid = valid[:m]
        offs = offs[:m + 1]
        data = data[:int(offs[-1])]
        lens = np.diff(offs)
        offs2 = np.zeros(m + 1, dtype=np.int64)
        offs2[1:] = np.cumsum(lens + P)
        d2 = torch.full((int(offs2[-1]) + 64,), ord("p"), dtype=torch.uint8, device="cuda")
        src = torch.from_numpy(data).cuda()
        row_of = torch.repeat_interleave(torch.arange(m, device="cuda"), torch.from_numpy(lens).cuda())
        o1, o2 = torch.from_numpy(offs[:-1]).cuda(), torch.from_numpy(offs2[:-1]).cuda()
        pos = torch.arange(int(offs[-1]), device="cuda", dtype=torch.int64)
        d2[o2[row_of] + P + (pos - o1[row_of])] = src
        del row_of, pos, o1, o2, src
        utf8_case("city_like_1k_prefix", dev_chunks(offs2, d2, valid, 8), offs2[-1])
        del d2
        # rows over 1000 distinct values
        m = args.utf8_rows
        woffs, wdata, _v = city_like(rng, 1000, null_frac=0.0)
        pick = rng.integers(0, 1000, m)
        lens3 = np.diff(woffs)[pick]
        offs3 = np.zeros(m + 1, dtype=np.int64)
        offs3[1:] = np.cumsum(lens3)
        d3 = torch.empty(int(offs3[-1]) + 64, dtype=torch.uint8, device="cuda")
        row_of = torch.repeat_interleave(torch.arange(m, device="cuda"), torch.from_numpy(lens3).cuda())
        pos = torch.arange(int(offs3[-1]), device="cuda", dtype=torch.int64)
        wsrc = torch.from_numpy(wdata).cuda()
        pk = torch.from_numpy(pick).cuda()
        d3[:int(offs3[-1])] = wsrc[torch.from_numpy(woffs[:-1]).cuda()[pk[row_of]] + (pos - torch.from_numpy(offs3[:-1]).cuda()[row_of])]
        del row_of, pos
        utf8_case("1000_distinct", dev_chunks(offs3, d3, None, 1), offs3[-1])

    lib.set_stream(0)


if __name__ == "__main__":
    main()
