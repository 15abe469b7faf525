#!/usr/bin/env python3
"""rdf_utf8_replace / _translate / _initcap / _split on device-resident StringArrays, next to the two nearest existing ops on
the same column in the same process: rdf_utf8_lower (it reads and rewrites every byte) and rdf_utf8_substring_index (the
existing search).  Three columns: --rows (1e8) short ASCII rows of ~24 bytes in --chunks chunks, the same with 10 % of the rows
holding 2- to 4-byte characters, and --long-rows rows of 16 KiB.

Timing (the contract of tools/bench_utf8.py --build): each call's kernel time from rdf_kernel_timing_* — HIP events around
size pass + scan(s) + write pass of the call into buffers sized beforehand, the host's read-back of the per-chunk totals
included — after --warmup calls, best of --reps; every op's repetitions ALTERNATE with rdf_utf8_lower's, so both see the same
clocks.  Reported per op: the bytes moved (Int32 offsets in and out, the source bytes once, the output bytes once; split: the
list offsets and the child offsets), their rate, and the ratio of the op's time to rdf_utf8_lower's on that column.  One JSON
line per case on stdout, appended to --out.

    python tools/bench_utf8_rewrite.py [--rows 100000000] [--long-rows 100000] [--out profiles/utf8_rewrite_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rust_dataframe_amd import _abi as A  # noqa: E402
from rust_dataframe_amd import lib  # noqa: E402
from bench_utf8 import device_column, pool  # noqa: E402


class Prepared:
    """One call with its output buffers sized by a sizing call: run() -> kernel ms"""
    def __init__(self, torch, so, call, shape, nullable, split=False):
        self.so, self.call, self.split = so, call, split
        k = len(shape)
        self.rows = sum(c.length for c in shape)
        self.ot = [torch.empty(c.length + 1 + 64, dtype=torch.int32, device="cuda") for c in shape]
        self.vt = [torch.empty((c.length + 63) // 64 * 8 + 8, dtype=torch.uint8, device="cuda") if nl else None for c, nl in zip(shape, nullable)]
        self.oo = (A.rdf_out * k)(*[A.rdf_out(t.data_ptr(), v.data_ptr() if v is not None else None, c.length + 1, 0, 0, A.I32, A.MEM_DEVICE)
                                    for t, v, c in zip(self.ot, self.vt, shape)])
        od = (A.rdf_out * k)(*[A.rdf_out(None, None, 0, 0, 0, A.U8, A.MEM_DEVICE) for _ in shape])
        oe = (A.rdf_out * k)(*[A.rdf_out(None, None, 0, 0, 0, A.I32, A.MEM_DEVICE) for _ in shape])
        st = call(self.oo, oe, od) if split else call(self.oo, od)
        assert st in (A.RDF_OK, A.RDF_MEMORY_ERROR), so.rdf_last_error()
        self.out_bytes = [od[i].length for i in range(k)]
        self.elems = [oe[i].length for i in range(k)] if split else [0] * k
        self.dt = [torch.empty(b + 64, dtype=torch.uint8, device="cuda") for b in self.out_bytes]
        self.et = [torch.empty(e + 64, dtype=torch.int32, device="cuda") for e in self.elems]
        self.od = (A.rdf_out * k)(*[A.rdf_out(t.data_ptr(), None, b, 0, 0, A.U8, A.MEM_DEVICE) for t, b in zip(self.dt, self.out_bytes)])
        self.oe = (A.rdf_out * k)(*[A.rdf_out(t.data_ptr(), None, e, 0, 0, A.I32, A.MEM_DEVICE) for t, e in zip(self.et, self.elems)])

    def run(self):
        lib.kernel_timing_reset(True)
        st = self.call(self.oo, self.oe, self.od) if self.split else self.call(self.oo, self.od)
        assert st == A.RDF_OK, self.so.rdf_last_error()
        ms = lib.kernel_timing_get()[0]
        lib.kernel_timing_reset(False)
        return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--chunks", type=int, default=4, help="the column's chunks (one StringArray holds < 2^31 bytes)")
    ap.add_argument("--long-rows", type=int, default=100_000, help="rows of 16 KiB for the long-row path")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    api = lib.api()
    assert lib.device_count() >= 1, "needs a GPU"
    lib.set_device(0)
    so = lib.load()
    so.rdf_utf8_lower.restype = C.c_int

    def emit(rec):          # a line at a time: a later case that fails loses nothing
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def column_cases(label, chunks, in_bytes, needle_never, delim):
        nch = len(chunks)
        rows = sum(c.length for c in chunks)
        carr = (A.rdf_utf8_array * nch)(*[c.c_struct() for c in chunks])
        nullable = [False] * nch
        lower = Prepared(torch, so, lambda co, cd: so.rdf_utf8_lower(carr, C.c_int64(nch), co, cd), chunks, nullable)
        for _ in range(args.warmup):
            lower.run()
        lower_ms = []

        def case(name, prep, note=None):
            for _ in range(args.warmup):
                prep.run()
            ms = []
            for _ in range(args.reps):      # alternating with lower on the same column
                lower_ms.append(lower.run())
                ms.append(prep.run())
            best, lbest = min(ms), min(lower_ms)
            moved = 4 * (rows + nch) * 2 + in_bytes + sum(prep.out_bytes) + 4 * sum(prep.elems)
            rec = {"op": f"{name}_{label}", "rows": rows, "chunks": nch, "in_bytes": in_bytes, "out_bytes": sum(prep.out_bytes), "elements": sum(prep.elems),
                   "moved_bytes": moved, "kernel": lib.last_kernel(), "kernel_ms": round(best, 3), "kernel_ms_median": round(float(np.median(ms)), 3),
                   "GBps": round(moved / best / 1e6, 1), "lower_ms": round(lbest, 3), "ratio_to_lower": round(best / lbest, 3)}
            if note:
                rec["note"] = note
            emit(rec)
            del prep
            return best

        def two(call_shape):
            call, shape, nl = call_shape
            return Prepared(torch, so, call, shape, nl)

        def three(call_shape):
            call, shape, nl = call_shape
            return Prepared(torch, so, call, shape, nl, split=True)

        case("substring_index_never", two(api.utf8_build_call("substring_index", chunks, needle_never, 1)), "the existing search; the needle never occurs")
        case("replace_never", two(api.utf8_replace_call(chunks, needle_never, "x")), "the needle never occurs: compare with substring_index_never")
        case("replace_delete", two(api.utf8_replace_call(chunks, delim, "")), f"replace({delim!r}, '')")
        case("replace_same_length", two(api.utf8_replace_call(chunks, delim, "_")), "r == m: the size pass reads no row byte")
        case("replace_grow", two(api.utf8_replace_call(chunks, delim, "<sp>")))
        case("translate_ascii", two(api.utf8_translate_call(chunks, "abcdefghijklmnopqrstuvwxyz", "ABCDEFGHIJKLMNOPQRSTUVWXYZ")), "compare with lower")
        case("translate_delete_wide", two(api.utf8_translate_call(chunks, "é中😀 ", "e")))
        case("initcap", two(api.utf8_initcap_call(chunks)))
        case("split", three(api.utf8_split_call(chunks, delim, -1)), "compare with replace_delete")
        case("split_limit_2", three(api.utf8_split_call(chunks, delim, 2)))
        emit({"op": f"utf8_lower_{label}", "rows": rows, "chunks": nch, "in_bytes": in_bytes, "kernel_ms": round(min(lower_ms), 3),
              "kernel_ms_median": round(float(np.median(lower_ms)), 3), "GBps": round((8 * (rows + nch) + 2 * in_bytes) / min(lower_ms) / 1e6, 1)})

    rng = np.random.default_rng(37)
    n, nch = args.rows, args.chunks
    assert n % nch == 0
    cr = n // nch
    ascii_pool = pool(rng, 1 << 20, False)
    x, xb = device_column(torch, ascii_pool, cr)
    torch.cuda.synchronize()
    column_cases("ascii", [x] * nch, xb * nch, "#~", " ")
    del x
    wide_pool = pool(rng, 1 << 20, True)
    mixed = [w if i % 10 == 0 else a for i, (a, w) in enumerate(zip(ascii_pool, wide_pool))]
    y, yb = device_column(torch, mixed, cr)
    torch.cuda.synchronize()
    column_cases("wide10", [y] * nch, yb * nch, "#~", " ")
    del y
    # rows of 16 KiB: an op must cost their bytes, not their count
    lrows = args.long_rows
    long_pool = ["".join(rng.choice(list("abcdefghijklmnop "), size=16384)) for _ in range(64)]
    h = A.HostUtf8.from_pylist(long_pool)
    pd = torch.from_numpy(h.data[:int(h.offsets[-1])].copy()).cuda()
    per = 32768          # 4 x 16 KiB x 32768 rows stay at 2^31 bytes a chunk; replace_grow is what needs the room
    chunks = []
    for c0 in range(0, lrows, per // 2):
        k = min(per // 2, lrows - c0)
        offs = (torch.arange(k + 1, device="cuda", dtype=torch.int64) * 16384).to(torch.int32)
        data = pd.repeat((k + 63) // 64)[:k * 16384].contiguous()
        chunks.append(A.DeviceUtf8(offs.data_ptr(), data.data_ptr(), k * 16384, k, None, 0, 0, 0, keep=(offs, data, None)))
    torch.cuda.synchronize()          # (the library runs on its own stream: torch's fills must have landed before the sizing call reads the offsets)
    column_cases("16KiB_rows", chunks, lrows * 16384, "#~", " ")


if __name__ == "__main__":
    main()
