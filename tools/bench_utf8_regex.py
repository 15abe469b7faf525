#!/usr/bin/env python3
"""rdf_utf8_regexp_match / _replace / _split on device-resident StringArrays, each next to the literal operation it stands in for
on the same column in the same process: rlike('needle') against rdf_utf8_predicate(CONTAINS, 'needle'), regexp_replace(x, ' ',
'') against rdf_utf8_replace(x, ' ', ''), regexp_split(x, ' ') against rdf_utf8_split(x, ' '); regexp_replace(x, '\\s+', ' ')
and regexp_replace(x, '[^0-9]', '') against the same literal replace, and rlike of a pattern near the LDS budget and of one near
the table cap against the same CONTAINS.  Three columns, those of tools/bench_utf8_rewrite.py: --rows (1e8) short ASCII rows of
~24 bytes in --chunks chunks, the same with 10 % of the rows holding 2- to 4-byte characters, and --long-rows rows of 16 KiB.

Timing (the method of tools/bench_utf8_rewrite.py): each call's kernel time from rdf_kernel_timing_* — HIP events around all
the kernels of the call into buffers sized beforehand — after --warmup calls, best of --reps; a case's repetitions ALTERNATE
with its literal operation's, so both see the same clocks.  Reported per case: the regex call's time, the literal call's, and
their ratio, which is the number to write down; the pattern's sizes as rdf_utf8_regexp_info reports them.  One JSON line per
case on stdout, appended to --out.

    python tools/bench_utf8_regex.py [--rows 100000000] [--long-rows 100000] [--out profiles/utf8_regex_bench.jsonl]
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
from bench_utf8 import device_column, pool  # noqa: E402
from bench_utf8_rewrite import Prepared  # noqa: E402


class Mask:
    """One mask call (rlike / CONTAINS) into Boolean outputs made beforehand: run() -> kernel ms"""
    out_bytes, elems = [0], [0]

    def __init__(self, api, chunks, fn):
        self.outs = [api._window_out(A.BOOL, c.length, True, False) for c in chunks]
        self.fn = fn

    def run(self):
        lib.kernel_timing_reset(True)
        self.fn(self.outs)
        ms = lib.kernel_timing_get()[0]
        lib.kernel_timing_reset(False)
        return ms


WIDE_STAR = "(?:" + "|".join("acegikmoqsuwyACEGIKMOQSUWY02468") + ")*a(?:a|c){8}"      # 1540 states of 67 classes


def near_a_cap(api, family, cap_bytes):
    """family % n with the largest n whose tables stay within `cap_bytes`, found by asking rdf_utf8_regexp_info (a refused
    pattern raises) -> (pattern, info)"""
    best = None
    for n in range(1, 600):
        try:
            info = api.utf8_regexp_info(family % n)
        except Exception:
            break
        if info["table_bytes"] > cap_bytes:
            break
        best = (family % n, info)
    return best


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

    def emit(rec):          # a line at a time: a later case that fails loses nothing
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    # 1540 states and a counted run: the largest tables that are still walked out of LDS (32 KiB), and that the library takes (256 KiB)
    lds_pattern, lds_info = near_a_cap(api, "(?:a|b)*a(?:a|b){8}|q{%d}", 32 * 1024)
    hbm_pattern, hbm_info = near_a_cap(api, WIDE_STAR + "|z{%d}", 256 * 1024)

    def column_cases(label, chunks, in_bytes):
        nch = len(chunks)
        rows = sum(c.length for c in chunks)

        def two(call_shape):
            call, shape, nl = call_shape
            return Prepared(torch, so, call, shape, nl)

        def three(call_shape):
            call, shape, nl = call_shape
            return Prepared(torch, so, call, shape, nl, split=True)

        def case(name, pattern, regex, literal, literal_name):
            for _ in range(args.warmup):
                literal.run()
                regex.run()
            ms, lms = [], []
            for _ in range(args.reps):      # alternating with the literal operation on the same column
                lms.append(literal.run())
                ms.append(regex.run())
            best, lbest = min(ms), min(lms)
            info = api.utf8_regexp_info(pattern)
            emit({"op": f"{name}_{label}", "pattern": pattern, "against": literal_name, "rows": rows, "chunks": nch, "in_bytes": in_bytes,
                  "out_bytes": sum(regex.out_bytes), "elements": sum(regex.elems), "kernel": lib.last_kernel(), "kernel_ms": round(best, 3),
                  "kernel_ms_median": round(float(np.median(ms)), 3), "in_GBps": round(in_bytes / best / 1e6, 1), "literal_ms": round(lbest, 3),
                  "ratio_to_literal": round(best / lbest, 3), "forward_states": info["forward_states"], "reverse_states": info["reverse_states"],
                  "table_bytes": info["table_bytes"]})

        contains = Mask(api, chunks, lambda outs: api.utf8_predicate("contains", chunks, "needle", outs=outs))
        case("rlike_needle", "needle", Mask(api, chunks, lambda outs: api.utf8_regexp_match(chunks, "needle", outs=outs)), contains, "contains('needle')")
        case("rlike_near_lds_cap", lds_pattern, Mask(api, chunks, lambda outs: api.utf8_regexp_match(chunks, lds_pattern, outs=outs)), contains, "contains('needle')")
        case("rlike_near_table_cap", hbm_pattern, Mask(api, chunks, lambda outs: api.utf8_regexp_match(chunks, hbm_pattern, outs=outs)), contains, "contains('needle')")
        del contains
        replace = two(api.utf8_replace_call(chunks, " ", ""))
        case("regexp_replace_space", " ", two(api.utf8_regexp_replace_call(chunks, " ", "")), replace, "replace(' ', '')")
        case("regexp_replace_spaces_to_one", "\\s+", two(api.utf8_regexp_replace_call(chunks, "\\s+", " ")), replace, "replace(' ', '')")
        case("regexp_replace_non_digits", "[^0-9]", two(api.utf8_regexp_replace_call(chunks, "[^0-9]", "")), replace, "replace(' ', '')")
        del replace
        torch.cuda.empty_cache()
        case("regexp_split_space", " ", three(api.utf8_regexp_split_call(chunks, " ", -1)), three(api.utf8_split_call(chunks, " ", -1)), "split(' ')")
        torch.cuda.empty_cache()

    emit({"op": "near_lds_cap_pattern", "pattern": lds_pattern, **lds_info})
    emit({"op": "near_table_cap_pattern", "pattern": hbm_pattern, **hbm_info})
    rng = np.random.default_rng(37)
    n, nch = args.rows, args.chunks
    assert n % nch == 0
    cr = n // nch
    ascii_pool = pool(rng, 1 << 20, False)
    if n:
        x, xb = device_column(torch, ascii_pool, cr)
        torch.cuda.synchronize()
        column_cases("ascii", [x] * nch, xb * nch)
        del x
        wide_pool = pool(rng, 1 << 20, True)
        mixed = [w if i % 10 == 0 else a for i, (a, w) in enumerate(zip(ascii_pool, wide_pool))]
        y, yb = device_column(torch, mixed, cr)
        torch.cuda.synchronize()
        column_cases("wide10", [y] * nch, yb * nch)
        del y
    # rows of 16 KiB: a row stays on one lane, so this is the rate of one DFA walk a lane
    lrows = args.long_rows
    if lrows:
        long_pool = ["".join(rng.choice(list("abcdefghijklmnop "), size=16384)) for _ in range(64)]
        h = A.HostUtf8.from_pylist(long_pool)
        pd = torch.from_numpy(h.data[:int(h.offsets[-1])].copy()).cuda()
        per = 32768
        chunks = []
        for c0 in range(0, lrows, per // 2):
            k = min(per // 2, lrows - c0)
            offs = (torch.arange(k + 1, device="cuda", dtype=torch.int64) * 16384).to(torch.int32)
            data = pd.repeat((k + 63) // 64)[:k * 16384].contiguous()
            chunks.append(A.DeviceUtf8(offs.data_ptr(), data.data_ptr(), k * 16384, k, None, 0, 0, 0, keep=(offs, data, None)))
        torch.cuda.synchronize()          # (the library runs on its own stream: torch's fills must have landed before the sizing call reads the offsets)
        column_cases("16KiB_rows", chunks, lrows * 16384)


if __name__ == "__main__":
    main()
