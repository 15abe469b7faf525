#!/usr/bin/env python3
"""rdf_utf8_parse_float / rdf_utf8_format_float on device-resident columns: 1e8 rows in 4 chunks by default.

    python tools/bench_textfloat.py [--rows 100000000] [--chunks 4] [--reps 3] [--out profiles/textfloat_bench.jsonl]

Columns, for Float64 and Float32 each: prices with 2 decimals (about 7 bytes a row), uniform [0, 1) (17 / 9 digits), uniform
random bit patterns.  The text columns are made on the device by rdf_utf8_format_float itself.  Yardsticks in the same process: rdf_probe_stream's read and copy rates (the floor of the
algorithmic bytes), and rdf_utf8_format(INT) / rdf_utf8_parse(INT) / rdf_utf8_measure(LENGTH) on Int64 text of the same mean
width (at most 18 digits).  Last, a column with 1 % rows the fast path leaves undecided (long-digit ties), with and without
"textfloat_exact".

Timing: HIP events around the whole call (rdf_kernel_timing_*; for format the call into exactly sized buffers), best of --reps
after --warmup calls.  One JSON line per case on stdout (and appended to --out)."""
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


def textfloat_bench(args, api, torch):
    n, nch = args.rows, args.chunks
    assert n % nch == 0
    cr = n // nch
    pb = 1 << 31
    p0, p1 = torch.empty(pb, dtype=torch.uint8, device="cuda"), torch.empty(pb, dtype=torch.uint8, device="cuda")
    read_gbps, read_shape = lib.probe_stream(0, p0.data_ptr(), 0, 0, pb, 10)
    copy_gbps, copy_shape = lib.probe_stream(1, p0.data_ptr(), p1.data_ptr(), 0, pb, 10)
    del p0, p1
    g = torch.Generator(device="cuda")
    g.manual_seed(43)
    lines = []

    def values(kind, f32):
        out = []
        ft, dt = (torch.float32, A.F32) if f32 else (torch.float64, A.F64)
        for _ in range(nch):
            if kind == "prices":     # 0.00 .. 99999.99: exponents cluster
                v = (torch.randint(0, 10_000_000, (cr,), device="cuda", generator=g).double() / 100.0).to(ft)
            elif kind == "uniform":
                v = torch.rand(cr, device="cuda", generator=g, dtype=ft)
            elif kind == "bits":     # every exponent as likely: the table is read all over
                if f32:
                    v = torch.randint(-2 ** 31, 2 ** 31, (cr,), device="cuda", generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
                else:
                    v = torch.randint(-2 ** 63, 2 ** 63 - 1, (cr,), device="cuda", generator=g, dtype=torch.int64).view(torch.float64)
            else:                    # Int64 of exactly `kind` digits
                lo = 10 ** (kind - 1)
                v, dt = torch.randint(lo, 10 * lo, (cr,), device="cuda", generator=g, dtype=torch.int64), A.I64
            out.append(A.DeviceArray(v.data_ptr(), None, 0, cr, dt, 0, keep=(v, None)))
        torch.cuda.synchronize()   # (the library runs on a stream of its own: the values have to be there before it reads them)
        return out

    def report(name, rows, alg, best, med, rate, rate_name, shape, extra):
        rec = {"op": name, "rows": rows, "chunks": nch, "alg_bytes": alg, "kernel": lib.last_kernel(), "kernel_ms": round(best, 3), "kernel_ms_median": round(med, 3),
               "GBps": round(alg / best / 1e6, 1), rate_name + "_probe_GBps": round(rate, 1), "frac_of_" + rate_name: round(alg / best / 1e6 / rate, 3),
               "floor_ms": round(alg / rate / 1e6, 3), "probe_shape": shape}
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        return rec

    def format_case(name, vals, es, call_of):
        call, _, nullable = call_of(vals)
        rows = vals[0].length
        co, cd, keep = api._utf8_outs(vals, [rows] * nch, nullable, True)
        assert call(co, cd) == A.RDF_MEMORY_ERROR
        caps = [cd[i].length for i in range(nch)]
        co, cd, keep = api._utf8_outs(vals, [rows] * nch, nullable, True, caps)
        torch.cuda.synchronize()
        text_bytes = sum(caps)
        alg = rows * nch * es + 4 * (rows * nch + nch) + text_bytes
        best, med = timed(args, lambda: api._check(call(co, cd)))
        rec = report(name, rows * nch, alg, best, med, copy_gbps, "copy", copy_shape, {"text_bytes": text_bytes, "mean_row_bytes": round(text_bytes / (rows * nch), 2)})
        cols = [A.DeviceUtf8(keep[i][0].data_ptr(), keep[i][1].data_ptr(), caps[i], rows, None, 0, 0, 0, keep=keep[i]) for i in range(nch)]
        return cols, rec

    def parse_float_case(name, cols, f32, exacts=(0,)):
        rows = cols[0].length
        text_bytes = sum(c.data_length for c in cols)
        es = 4 if f32 else 8
        outs = [api._window_out(A.F32 if f32 else A.F64, rows, True, True) for _ in range(nch)]
        alg = 4 * (rows * nch + nch) + text_bytes + rows * nch * es + rows * nch // 8
        first = None
        for exact in exacts:
            lib.set_option("textfloat_exact", exact)
            best, med = timed(args, lambda: api.utf8_parse_float(cols, dtype=A.F32 if f32 else A.F64, outs=outs))
            _, failed = api.utf8_parse_float(cols, dtype=A.F32 if f32 else A.F64, outs=outs)
            assert sum(failed) == 0 and sum(o.null_count for o in outs) == 0
            r = report(name, rows * nch, alg, best, med, read_gbps, "read", read_shape,
                       {"text_bytes": text_bytes, "mean_row_bytes": round(text_bytes / (rows * nch), 2), "exact_only": bool(exact)})
            first = first or r
        lib.set_option("textfloat_exact", 0)
        return first

    def int_yardsticks(width, fmt_rec, parse_rec, label):
        digits = int(min(18, max(1, round(width))))
        ints, irec = format_case(f"yardstick: format Int64 -> text, {digits} digits ({label})", values(digits, False), 8,
                                 lambda v: api.utf8_format_call(v, "int", None, None))
        outs = [api._window_out(A.I64, cr, True, True) for _ in range(nch)]
        mo = [api._window_out(A.I32, cr, True, False) for _ in range(nch)]
        torch.cuda.synchronize()
        text_bytes = sum(c.data_length for c in ints)
        alg = 4 * (n + nch) + text_bytes + n * 8 + n // 8
        best, med = timed(args, lambda: api.utf8_parse(ints, "int", None, None, outs=outs))
        prec = report(f"yardstick: parse Int64 text, {digits} digits ({label})", n, alg, best, med, read_gbps, "read", read_shape, {"text_bytes": text_bytes})
        lbest, lmed = timed(args, lambda: api.utf8_measure("length", ints, outs=mo))
        report(f"yardstick: utf8_measure(LENGTH), {digits} digits ({label})", n, 4 * (n + nch) + text_bytes + 4 * n, lbest, lmed, read_gbps, "read", read_shape, {"text_bytes": text_bytes})
        rec = {"op": f"ratio to the integer calls ({label})", "format_float_over_format_int": round(fmt_rec["kernel_ms"] / irec["kernel_ms"], 3),
               "parse_float_over_parse_int": round(parse_rec["kernel_ms"] / prec["kernel_ms"], 3), "parse_float_over_length": round(parse_rec["kernel_ms"] / lbest, 3)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for f32 in (False, True):
        tname = "Float32" if f32 else "Float64"
        for kind in ("prices", "uniform", "bits"):
            label = f"{tname} {kind}"
            cols, frec = format_case(f"format {label} -> text", values(kind, f32), 4 if f32 else 8, api.utf8_format_float_call)
            prec = parse_float_case(f"parse {label} text", cols, f32)
            width = frec["mean_row_bytes"]
            del cols
            int_yardsticks(width, frec, prec, label)

    # ---- 1 % undecided rows: long-digit ties among prices.  10^6 rows are written on the host, uploaded once and repeated on
    # the device to the size of a chunk, so the case runs on the same device-resident rows as every other line
    base = min(cr, 1_000_000)
    assert cr % base == 0
    rng = np.random.default_rng(5)
    cents = rng.integers(0, 10_000_000, size=base)

    def repeated(texts):
        host = A.HostUtf8.from_pylist(texts)
        nbytes = int(host.offsets[base])
        d0 = torch.from_numpy(np.ascontiguousarray(host.data[:nbytes])).cuda()
        o0 = torch.from_numpy(np.ascontiguousarray(host.offsets[:base]).astype(np.int64)).cuda()
        rep = cr // base
        data = torch.cat([d0.repeat(rep), torch.zeros(64, dtype=torch.uint8, device="cuda")])
        offs = (o0.repeat(rep) + torch.arange(rep, device="cuda", dtype=torch.int64).repeat_interleave(base) * nbytes)
        offs = torch.cat([offs, torch.tensor([rep * nbytes], device="cuda", dtype=torch.int64)]).to(torch.int32)
        torch.cuda.synchronize()
        return [A.DeviceUtf8(offs.data_ptr(), data.data_ptr(), rep * nbytes, cr, None, 0, 0, 0, keep=(offs, data)) for _ in range(nch)]

    texts = [f"{c // 100}.{c % 100:02d}" for c in cents]
    clean = repeated(texts)
    parse_float_case("parse Float64 prices, host-written (the 1 % case without its undecided rows)", clean, False)
    del clean
    for i in range(0, base, 100):
        texts[i] = f"{9007199254740993 + 2 * (i % 1000)}.{'0' * 30}1"
    cols = repeated(texts)
    parse_float_case("parse Float64 prices with 1 % undecided rows", cols, False, exacts=(0, 1))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--textfloat", action="store_true", help="accepted for symmetry with tools/bench_textconv.py: the one mode of this tool")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="append the lines to this file")
    ap.add_argument("--build", default=None, help="a label written into every line as \"build\" (which build of the kernels was measured)")
    args = ap.parse_args()
    import torch
    if lib.device_count() < 1:
        sys.exit("no GPU visible")
    lib.set_device(0)
    lines = textfloat_bench(args, lib.api(), torch)
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                if args.build:
                    rec = dict(rec, build=args.build)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
