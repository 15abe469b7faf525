#!/usr/bin/env python3
"""Text keys on device-resident columns: rdf_utf8_dictionary_encode (hash route and forced exact route),
rdf_groupby_agg_keys(COUNT) on one text key and rdf_equijoin_indices_keys on one text pair, each beside its yardstick taken in
the same process, on the three Utf8 inputs of tools/bench_colstats.py (city-like rows with 10 % NULLs, the same behind a
1 KiB common prefix, rows over 1000 distinct values).

  encode    yardstick: rdf_utf8_uniques on the same input (the same two reads of the bytes; encode adds the flags, the scan
            and the codes).
  groupby   yardstick: rdf_groupby_agg(COUNT) on the column's UInt32 codes, made beforehand: the difference is the price
            of the text.
  join      --utf8-rows x --join-rows on one text pair (the right side: every 10th row of the left); yardstick:
            rdf_equijoin_indices on the two sides' UInt32 codes, made beforehand.
  uniques   rdf_utf8_uniques alone (--only uniques runs against a library without the new entry points too: with
            tools/ab_libs.py this is the parent-against-this-commit comparison of the entry point whose passes encode shares).

Timing as tools/bench_colstats.py: HIP events on the stream the library is told to use, recorded around the WHOLE call, after
--warmup calls, --reps (>= 10) repetitions; best (`ms`, repeated as `kernel_ms` for tools/ab_libs.py), median and the spread
(max - min) / median.  The read probe runs in the same process.  One JSON line per measurement on stdout (and appended to --out).

    python tools/bench_text_keys.py [--utf8-rows 10000000] [--join-rows 1000000] [--only encode,groupby,join,uniques] [--out profiles/text_keys.jsonl]
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
    ap.add_argument("--utf8-rows", type=int, default=10_000_000)
    ap.add_argument("--join-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="encode,groupby,join,uniques")
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

    def put(rec, key, ms):
        rec[key + "_ms"], rec[key + "_ms_median"], rec[key + "_spread"] = round(ms[0], 3), round(ms[1], 3), round(ms[2], 3)

    pbytes = 1 << 32
    pt = torch.empty(pbytes, dtype=torch.uint8, device="cuda")
    read_gbps, read_shape = lib.probe_stream(0, pt.data_ptr(), 0, 0, pbytes, 10)
    del pt
    emit({"op": "read_probe", "GBps": round(read_gbps, 1), "shape": read_shape})

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

    def every_10th(col):
        """The right side of the join: --join-rows rows of the column's first chunk, every 10th one, as one device chunk."""
        c = col[0]
        ot, dd, vt = c.keep
        take = min(args.join_rows, c.length // 10)
        rows = torch.arange(take, device="cuda", dtype=torch.int64) * 10
        o = ot.to(torch.int64)
        lens = o[rows + 1] - o[rows]
        no = torch.zeros(take + 1, dtype=torch.int64, device="cuda")
        no[1:] = torch.cumsum(lens, 0)
        row_of = torch.repeat_interleave(torch.arange(take, device="cuda"), lens)
        pos = torch.arange(int(no[-1]), device="cuda", dtype=torch.int64)
        base = (c.data_ptr - dd.data_ptr())
        nd = torch.zeros(int(no[-1]) + 64, dtype=torch.uint8, device="cuda")
        nd[:int(no[-1])] = dd[base + o[rows][row_of] + (pos - no[:-1][row_of])]
        nv = None
        if vt is not None:
            bits = torch.from_numpy(A.unpack_bits(vt.cpu().numpy(), 0, c.length)).cuda()[rows]
            nv = torch.from_numpy(A.pack_bits(bits.cpu().numpy())).cuda()
        no32 = no.to(torch.int32)
        return [A.DeviceUtf8(no32.data_ptr(), nd.data_ptr(), int(no[-1]), take, nv.data_ptr() if nv is not None else None, 0, 0, -1, keep=(no32, nd, nv))]

    def case(label, col, nbytes):
        m = sum(c.length for c in col)
        base = {"data": label, "rows": m, "bytes": int(nbytes)}
        ms_u = None
        if only & {"uniques", "encode"}:
            lib.set_option("uniques_route", 0)
            r = api.utf8_uniques(col)
            ms_u = timed(lambda: api.utf8_uniques(col))
            rec = dict(op="utf8_uniques", **base, distinct=r.length, route=lib.last_kernel(), kernel_ms=round(ms_u[0], 3))
            put(rec, "hash", ms_u)
            rec["read_floor_ms"] = round(2 * nbytes / read_gbps / 1e6, 3)
            if "uniques" in only:
                emit(rec)
        if not only & {"encode", "groupby", "join"}:
            return
        codes, dic, count = api.utf8_dictionary_encode(col)
        if "encode" in only:
            rec = dict(op="utf8_dictionary_encode", **base, distinct=count)
            for route, key in ((0, "hash"), (1, "exact")):
                lib.set_option("uniques_route", route)
                api.utf8_dictionary_encode(col)
                rec[key + "_route"] = lib.last_kernel()
                ms = timed(lambda: api.utf8_dictionary_encode(col))
                put(rec, key, ms)
                if route == 0:
                    rec["kernel_ms"] = round(ms[0], 3)
                    rec["uniques_ms"] = round(ms_u[0], 3)
                    rec["encode_over_uniques"] = round(ms[0] / ms_u[0], 3)
                    # what encode moves beyond uniques: flags 8 + scan 8 + 8 read back, rep 4 + 4, codes 4 (B per row)
                    rec["extra_traffic_floor_ms"] = round(36 * m / read_gbps / 1e6, 3)
            lib.set_option("uniques_route", 0)
            emit(rec)
        if "groupby" in only:
            ms_k = timed(lambda: api.groupby_agg_keys([col], None, "count", count))
            cap = count + 2
            gouts = ([api._window_out(A.U32, cap, True, True)], api._window_out(A.I64, cap, True, False), api._window_out(A.I64, cap, True, False))
            ms_c = timed(lambda: api.groupby_agg([codes], None, "count", count, outs=gouts))
            rec = dict(op="groupby_agg_keys_count", **base, groups=count, kernel_ms=round(ms_k[0], 3))
            put(rec, "text", ms_k)
            put(rec, "codes", ms_c)
            rec["text_over_codes"] = round(ms_k[0] / ms_c[0], 3)
            emit(rec)
        if "join" in only:
            right = every_10th(col)
            both, _d, _c = api.utf8_dictionary_encode(list(col) + right)
            lcodes, rcodes = both[:len(col)], both[len(col):]
            rows = api.equijoin_indices_keys([col], [right], "inner", count_only=True)
            ol, orr = api._window_out(A.U32, rows, True, True), api._window_out(A.U32, rows, True, True)
            ms_k = timed(lambda: api.equijoin_indices_keys([col], [right], "inner", outs=(ol, orr)))   # one call each: the outputs are there
            ms_c = timed(lambda: api.equijoin_indices(lcodes, rcodes, "inner", outs=(ol, orr)))
            rec = dict(op="equijoin_indices_keys_inner", **base, right_rows=right[0].length, out_rows=rows, kernel_ms=round(ms_k[0], 3))
            put(rec, "text", ms_k)
            put(rec, "codes", ms_c)
            rec["text_over_codes"] = round(ms_k[0] / ms_c[0], 3)
            emit(rec)

    rng = np.random.default_rng(23)
    m = args.utf8_rows
    offs, data, valid = city_like(rng, m)
    case("city_like", dev_chunks(offs, data, valid, 1), offs[-1])
    # the same rows behind a 1 KiB common prefix (built on the device, 8 chunks); only as many rows as keep the dictionary —
    # nearly every row is distinct — below 2^31 bytes
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
    case("city_like_1k_prefix", dev_chunks(offs2, d2, valid, 8), offs2[-1])
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
    case("1000_distinct", dev_chunks(offs3, d3, None, 1), offs3[-1])

    lib.set_stream(0)


if __name__ == "__main__":
    main()
