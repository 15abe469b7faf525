#!/usr/bin/env python3
"""rdf_utf8_parse / rdf_utf8_format on device-resident columns: 1e8 rows in 4 chunks by default.

    python tools/bench_textconv.py --textconv [--rows 100000000] [--chunks 4] [--reps 3] [--out profiles/textconv_bench.jsonl]

Cases: parse of Int64 text (1..18 digits and a sign on half the rows, mean about 10 bytes), of yyyy-MM-dd dates by cast and by pattern, of timestamps with
milliseconds; Int64 -> text, date -> text, date_format with yyyy-MM-dd HH:mm:ss.  The text columns are made on the device by
rdf_utf8_format itself.

Timing: HIP events around the whole call (rdf_kernel_timing_*; for format the call into exactly sized buffers: size pass, scan,
the host's read-back of the totals, write pass), best of --reps after --warmup calls.  Every case is reported against
  * its algorithmic bytes (offsets, text bytes, values, validity bits; each read or written once) over the read (parse) or
    copy (format) rate rdf_probe_stream measures in the same process,
  * parse: rdf_utf8_measure(LENGTH) on the same text column — the project's nearest reader; with rdf_set_option
    ("textconv_stage", 0) the parse kernel is measured again in its fallback form (every lane reads global memory),
  * format: rdf_utf8_trim on the produced column — the project's nearest writer.
One JSON line per case on stdout (and appended to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rust_dataframe_amd import _abi as A  # noqa: E402
from rust_dataframe_amd import lib  # noqa: E402


def timed(args, call):
    for _ in range(args.warmup):
        call()
    ms = []
    for _ in range(args.reps):
        lib.kernel_timing_reset(True)
        call()
        ms.append(lib.kernel_timing_get()[0])
    lib.kernel_timing_reset(False)
    return min(ms), float(np.median(ms))


def textconv_bench(args, api, torch):
    so = lib.load()
    so.rdf_utf8_trim.restype = C.c_int
    n, nch = args.rows, args.chunks
    assert n % nch == 0
    cr = n // nch
    pb = 1 << 31
    p0, p1 = torch.empty(pb, dtype=torch.uint8, device="cuda"), torch.empty(pb, dtype=torch.uint8, device="cuda")
    read_gbps, read_shape = lib.probe_stream(0, p0.data_ptr(), 0, 0, pb, 10)
    copy_gbps, copy_shape = lib.probe_stream(1, p0.data_ptr(), p1.data_ptr(), 0, pb, 10)
    del p0, p1
    g = torch.Generator(device="cuda")
    g.manual_seed(41)
    lines = []

    def values(kind):
        out = []
        for _ in range(nch):
            if kind == "int":      # 1..18 digits, every length as likely: mean about 10 bytes
                digits = torch.randint(1, 19, (cr,), device="cuda", generator=g)
                v = (torch.rand(cr, device="cuda", generator=g, dtype=torch.float64) * torch.pow(10.0, digits.double())).to(torch.int64)
                v = torch.where(torch.rand(cr, device="cuda", generator=g) < 0.5, v, -v)
                dt = A.I64
            elif kind == "date":   # 1970 .. 2050
                v, dt = torch.randint(0, 29220, (cr,), device="cuda", generator=g, dtype=torch.int32), A.I32
            else:                  # milliseconds, 1970 .. 2050
                v, dt = torch.randint(0, 29220 * 86400 * 1000, (cr,), device="cuda", generator=g, dtype=torch.int64), A.I64
            out.append(A.DeviceArray(v.data_ptr(), None, 0, cr, dt, 0, keep=(v, None)))
        torch.cuda.synchronize()   # (the library runs on a stream of its own: the values have to be there before it reads them)
        return out

    def report(name, rows, alg, best, med, rate, rate_name, shape, extra):
        rec = {"op": name, "rows": rows, "chunks": nch, "alg_bytes": alg, "kernel": extra.pop("kernel", None) or lib.last_kernel(), "kernel_ms": round(best, 3), "kernel_ms_median": round(med, 3),
               "GBps": round(alg / best / 1e6, 1), rate_name + "_probe_GBps": round(rate, 1), "frac_of_" + rate_name: round(alg / best / 1e6 / rate, 3),
               "floor_ms": round(alg / rate / 1e6, 3), "probe_shape": shape}
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def format_case(name, vals, kind, unit, pattern, es):
        call, _, nullable = api.utf8_format_call(vals, kind, unit, pattern)
        co, cd, keep = api._utf8_outs(vals, [cr] * nch, nullable, True)
        assert call(co, cd) == A.RDF_MEMORY_ERROR
        caps = [cd[i].length for i in range(nch)]
        co, cd, keep = api._utf8_outs(vals, [cr] * nch, nullable, True, caps)
        torch.cuda.synchronize()
        best, med = timed(args, lambda: api._check(call(co, cd)))
        kernel = lib.last_kernel()
        text_bytes = sum(caps)
        alg = n * es + 4 * (n + nch) + text_bytes
        cols = [A.DeviceUtf8(keep[i][0].data_ptr(), keep[i][1].data_ptr(), caps[i], cr, None, 0, 0, 0, keep=keep[i]) for i in range(nch)]
        # the nearest writer: rdf_utf8_trim of the produced column into buffers of the same size (nothing to trim: as many bytes out)
        carr = (A.rdf_utf8_array * nch)(*[c.c_struct() for c in cols])
        to, td, tkeep = api._utf8_outs(cols, [cr] * nch, [False] * nch, True, caps)
        torch.cuda.synchronize()
        tbest, _ = timed(args, lambda: api._check(so.rdf_utf8_trim(carr, C.c_int64(nch), to, td)))
        report(name, n, alg, best, med, copy_gbps, "copy", copy_shape,
               {"kernel": kernel, "text_bytes": text_bytes, "mean_row_bytes": round(text_bytes / n, 2), "utf8_trim_ms": round(tbest, 3), "vs_utf8_trim": round(best / tbest, 3)})
        del tkeep
        return cols

    def parse_case(name, cols, kind, unit, pattern, es):
        text_bytes = sum(c.data_length for c in cols)
        odt = {"int": A.I64, "date": A.I32, "timestamp": A.I64}[kind]
        outs = [api._window_out(odt, cr, True, True) for _ in range(nch)]
        mo = [api._window_out(A.I32, cr, True, False) for _ in range(nch)]
        torch.cuda.synchronize()
        lbest, _ = timed(args, lambda: api.utf8_measure("length", cols, outs=mo))
        alg = 4 * (n + nch) + text_bytes + n * es + n // 8
        extra = {"text_bytes": text_bytes, "mean_row_bytes": round(text_bytes / n, 2), "utf8_length_ms": round(lbest, 3)}
        for stage in (1, 0):
            api._check(so.rdf_set_option(b"textconv_stage", C.c_int64(stage)))
            best, med = timed(args, lambda: api.utf8_parse(cols, kind, unit, pattern, outs=outs))
            _, failed = api.utf8_parse(cols, kind, unit, pattern, outs=outs)
            assert sum(failed) == 0 and sum(o.null_count for o in outs) == 0
            report(name + ("" if stage else " (fallback form: no LDS staging)"), n, alg, best, med, read_gbps, "read", read_shape,
                   dict(extra, lds_staged=bool(stage), vs_utf8_length=round(best / lbest, 3)))
        api._check(so.rdf_set_option(b"textconv_stage", C.c_int64(1)))

    ints = format_case("format Int64 -> text", values("int"), "int", None, None, 8)
    parse_case("parse Int64 text", ints, "int", None, None, 8)
    del ints
    dates = format_case("format date -> text (cast)", values("date"), "date", A.TIME_DAY, None, 4)
    parse_case("parse yyyy-MM-dd dates by cast", dates, "date", None, None, 4)
    parse_case("parse yyyy-MM-dd dates by pattern", dates, "date", None, "yyyy-MM-dd", 4)
    del dates
    ms = values("timestamp")
    stamps = format_case("format timestamp (ms) -> text (cast)", ms, "timestamp", A.TIME_MILLISECOND, None, 8)
    parse_case("parse timestamps with milliseconds", stamps, "timestamp", A.TIME_MILLISECOND, None, 8)
    del stamps
    format_case("date_format yyyy-MM-dd HH:mm:ss", ms, "timestamp", A.TIME_MILLISECOND, "yyyy-MM-dd HH:mm:ss", 8)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--textconv", action="store_true")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not args.textconv:
        ap.error("--textconv is the one mode of this tool")
    import torch
    if lib.device_count() < 1:
        sys.exit("no GPU visible")
    lib.set_device(0)
    lines = textconv_bench(args, lib.api(), torch)
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
