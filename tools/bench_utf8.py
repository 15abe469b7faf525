#!/usr/bin/env python3
"""Utf8 operators on device-resident StringArrays: filter (selectivity 1/2), take (random u32 indices), trim, lower on
ASCII text and on mixed 1-4 byte text.  1e8 rows of ~24 bytes by default, in 4 chunks (Int32 offsets bound a chunk to
2^31 - 1 bytes).

Timing: each call's kernel time from rdf_kernel_timing_* (HIP events around the span -> scan -> write sequence of one
call, the host's read-back of the per-chunk totals in between included), after warm-up calls.  Reported: algorithmic
bytes (offsets read + bytes read + mask / indices read + offsets written + bytes written) per second, and that rate as
a fraction of the library's own rdf_probe_stream copy rate measured in the same process.  For take, the numeric
rdf_take of the same random u32 indices over a Float64 column is measured alongside (micro_take_random_u32).
One JSON line per operator on stdout (and appended to --out).

    python tools/bench_utf8.py [--rows 100000000] [--reps 5] [--out FILE]
"""
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


def pool(rng, n, mixed):
    """n host strings, mean ~24 bytes: ASCII letters / digits / a few spaces, or mixed 1-4 byte characters."""
    if mixed:
        chars = list("abcdefghijKLMNOP ") + ["é", "ß", "Σ", "ж", "中", "文", "😀", "ǅ"]
        k = rng.integers(6, 17, size=n)   # ~1.6 bytes per character
    else:
        chars = list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789   ")
        k = rng.integers(12, 37, size=n)
    idx = rng.integers(0, len(chars), size=int(k.sum()))
    out, p = [], 0
    for m in k:
        out.append("".join(chars[j] for j in idx[p:p + m]))
        p += m
    out[0] = "  " + out[0] + " "
    return out


def device_column(torch, strings, rows):
    """`rows` rows on the device: the host pool tiled over and over (offsets shifted per copy) -> (DeviceUtf8, data bytes)."""
    h = A.HostUtf8.from_pylist(strings)
    po = torch.from_numpy(h.offsets.astype(np.int64)).cuda()
    pbytes = int(h.offsets[-1])
    pd = torch.from_numpy(h.data[:pbytes].copy()).cuda()
    reps = (rows + len(strings) - 1) // len(strings)
    data = pd.repeat(reps)
    offs = (po[:-1].unsqueeze(0) + torch.arange(reps, device="cuda", dtype=torch.int64).unsqueeze(1) * pbytes).reshape(-1)[:rows]
    total = int(offs[-1].item()) + int((po[1:] - po[:-1])[(rows - 1) % len(strings)].item())
    assert total < 2**31, "the column must fit Int32 offsets"
    offs = torch.cat([offs, torch.tensor([total], device="cuda", dtype=torch.int64)]).to(torch.int32)
    data = data[:total].contiguous()
    d = A.DeviceUtf8(offs.data_ptr(), data.data_ptr(), total, rows, None, 0, 0, 0, keep=(offs, data, None))
    return d, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--chunks", type=int, default=4, help="the column's chunks (one StringArray holds < 2^31 bytes)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    api = lib.api()
    assert lib.device_count() >= 1, "needs a GPU"
    lib.set_device(0)
    so = lib.load()
    for n in ("filter", "take", "trim", "lower"):
        getattr(so, "rdf_utf8_" + n).restype = C.c_int
    rng = np.random.default_rng(17)
    n = args.rows

    # the copy rate this process reaches (rdf_probe_stream kind 1: a -> b)
    pb = 1 << 31
    pa_, pb_ = torch.empty(pb, dtype=torch.uint8, device="cuda"), torch.empty(pb, dtype=torch.uint8, device="cuda")
    copy_gbps, copy_shape = lib.probe_stream(1, pa_.data_ptr(), pb_.data_ptr(), 0, pb, 10)
    del pa_, pb_

    # `chunks` chunks of n / chunks rows; they share one set of device buffers (each chunk is far larger than the caches)
    nch = args.chunks
    assert n % nch == 0
    cr = n // nch
    ascii_col, ascii_bytes = device_column(torch, pool(rng, 1 << 20, False), cr)
    mixed_col, mixed_bytes = device_column(torch, pool(rng, 1 << 20, True), cr)
    ascii_bytes *= nch
    mixed_bytes *= nch
    keep = torch.randint(0, 2, (n,), device="cuda", dtype=torch.uint8)
    bits = (keep[: (n // 8) * 8].view(-1, 8).to(torch.int32) << torch.arange(8, device="cuda", dtype=torch.int32)).sum(1).to(torch.uint8)
    mask_buf = torch.zeros((n + 63) // 64 * 8 + 8, dtype=torch.uint8, device="cuda")
    mask_buf[: bits.numel()] = bits
    if n % 8:
        tail = keep[(n // 8) * 8:].cpu().numpy()
        mask_buf[n // 8] = int(sum(int(b) << i for i, b in enumerate(tail)))
    masks = [A.DeviceArray(mask_buf.data_ptr(), None, i * cr, cr, A.BOOL, 0, keep=mask_buf) for i in range(nch)]
    # take gathers n / chunks random rows of all n into ONE chunk (which, too, must stay below 2^31 bytes)
    idx_t = torch.randint(0, n, (cr,), device="cuda", dtype=torch.int32)
    idx = A.DeviceArray(idx_t.data_ptr(), None, 0, cr, A.U32, 0, keep=idx_t)

    marr = (A.rdf_array * nch)(*[m.c_struct() for m in masks])
    iarr = (A.rdf_array * 1)(idx.c_struct())
    lines = []

    def run(name, col, in_bytes, call, extra_in, offs_in=None):
        carr = (A.rdf_utf8_array * nch)(*[col.c_struct()] * nch)
        nout = 1 if name.startswith("utf8_take") else nch
        rows_cap = cr
        ot = [torch.empty(rows_cap + 1 + 64, dtype=torch.int32, device="cuda") for _ in range(nout)]
        oo = (A.rdf_out * nout)(*[A.rdf_out(t.data_ptr(), None, rows_cap + 1, 0, 0, A.I32, A.MEM_DEVICE) for t in ot])
        od = (A.rdf_out * nout)(*[A.rdf_out(None, None, 0, 0, 0, A.U8, A.MEM_DEVICE)] * nout)
        st = call(carr, oo, od)
        assert st in (A.RDF_OK, A.RDF_MEMORY_ERROR), (st, so.rdf_last_error())
        needs = [od[i].length for i in range(nout)]
        dt = [torch.empty(k + 64, dtype=torch.uint8, device="cuda") for k in needs]
        for i in range(nout):
            od[i] = A.rdf_out(dt[i].data_ptr(), None, needs[i], 0, 0, A.U8, A.MEM_DEVICE)
        need = sum(needs)
        for _ in range(args.warmup):
            assert call(carr, oo, od) == A.RDF_OK, so.rdf_last_error()
        ms = []
        for _ in range(args.reps):
            lib.kernel_timing_reset(True)
            assert call(carr, oo, od) == A.RDF_OK, so.rdf_last_error()
            t, _k = lib.kernel_timing_get()
            ms.append(t)
        lib.kernel_timing_reset(False)
        rows_out = sum(oo[i].length - 1 for i in range(nout))
        alg = (4 * (n + nch) if offs_in is None else offs_in) + extra_in + in_bytes + 4 * (rows_out + nout) + need
        best = min(ms)
        gbps = alg / best / 1e6
        rec = {"op": name, "rows": n if nout > 1 else cr, "chunks": nch, "rows_out": rows_out, "bytes_in": in_bytes, "bytes_out": need, "alg_bytes": alg,
               "kernel_ms": round(best, 3), "kernel_ms_median": round(float(np.median(ms)), 3), "GBps": round(gbps, 1),
               "copy_probe_GBps": round(copy_gbps, 1), "frac_of_copy": round(gbps / copy_gbps, 3), "copy_probe_shape": copy_shape}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del dt, ot

    # filter reads the kept rows' bytes (half of them); take the gathered rows' bytes (~ all, at random)
    run("utf8_filter_sel_1_2_ascii", ascii_col, ascii_bytes // 2,
        lambda c, oo, od: so.rdf_utf8_filter(c, marr, C.c_int64(nch), oo, od), (n + 7) // 8)
    run("utf8_take_random_u32_ascii", ascii_col, ascii_bytes // nch,
        lambda c, oo, od: so.rdf_utf8_take(c, C.c_int64(nch), iarr, oo, od), 4 * cr, offs_in=8 * cr)
    run("utf8_trim_ascii", ascii_col, ascii_bytes, lambda c, oo, od: so.rdf_utf8_trim(c, C.c_int64(nch), oo, od), 0)
    run("utf8_lower_ascii", ascii_col, ascii_bytes, lambda c, oo, od: so.rdf_utf8_lower(c, C.c_int64(nch), oo, od), 0)
    run("utf8_lower_mixed", mixed_col, mixed_bytes, lambda c, oo, od: so.rdf_utf8_lower(c, C.c_int64(nch), oo, od), 0)

    # the numeric gather of the same indices, for comparison with take
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    X = A.DeviceArray(x.data_ptr(), None, 0, n, A.F64, 0, keep=x)
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    Y = A.DeviceArray(y.data_ptr(), None, 0, n, A.F64, 0, keep=y)
    for _ in range(args.warmup):
        api.take([X], idx, Y)
    ms = []
    for _ in range(args.reps):
        lib.kernel_timing_reset(True)
        api.take([X], idx, Y)
        ms.append(lib.kernel_timing_get()[0])
    lib.kernel_timing_reset(False)
    alg = (4 + 8 + 8) * cr
    rec = {"op": "micro_take_random_u32", "rows": cr, "alg_bytes": alg, "kernel_ms": round(min(ms), 3),
           "GBps": round(alg / min(ms) / 1e6, 1), "copy_probe_GBps": round(copy_gbps, 1), "frac_of_copy": round(alg / min(ms) / 1e6 / copy_gbps, 3)}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    if args.out:
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
