#!/usr/bin/env python3
"""rdf_filter of ONE column held in ONE chunk — the layout that runs on mask_count_one_kernel / compact_one_kernel (rdf_kernels.hip)
when the LDS-DMA kernel cannot take it: 700 Float64 rows and 2048 Int16 rows in host memory (a call is a handful of launches and two
copies: wall time per call and the time of its kernels) and 1e9 Int16 rows on the device (kernel time).  One JSON line per entry,
`kernel_ms` holding the figure, so that tools/ab_libs.py can alternate builds over it.
Usage: python tools/bench_filter_one_chunk.py [--rows N] [--calls K]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rust_dataframe_amd import _abi as A  # noqa: E402
from rust_dataframe_amd import lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000, help="rows of the long device-resident chunk")
    ap.add_argument("--calls", type=int, default=2000, help="calls per timed batch of the small chunks (7 batches, the median is reported)")
    args = ap.parse_args()
    lib.set_device(0)
    api = lib.api()
    rng = np.random.default_rng(5)
    for n, npdt, name in ((700, np.float64, "f64"), (2048, np.int16, "i16")):
        col = [A.HostArray.from_numpy((rng.uniform(size=n) * 1000).astype(npdt))]
        mask = [A.HostArray.from_numpy(rng.uniform(size=n) < 0.5, dtype=A.BOOL)]
        out = [A.HostArray.empty_out(col[0].dtype, n, False)]
        for _ in range(200):
            api.filter(col, mask, out)
        lib.synchronize()
        lib.kernel_timing_reset(True)
        for _ in range(args.calls):
            api.filter(col, mask, out)
        lib.synchronize()
        kms, _ = lib.kernel_timing_get()
        lib.kernel_timing_reset(False)
        print(json.dumps({"kernel": f"rdf_filter_kernel_time_{n}_rows_{name}_one_chunk_host", "rows": n, "kernel_ms": kms / args.calls, "last_kernel": lib.last_kernel()}), flush=True)
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                api.filter(col, mask, out)
            ts.append((time.perf_counter() - t0) / args.calls * 1e3)
        print(json.dumps({"kernel": f"rdf_filter_wall_{n}_rows_{name}_one_chunk_host", "rows": n, "kernel_ms": statistics.median(ts), "last_kernel": lib.last_kernel()}), flush=True)
    # one long chunk of a 2-byte column on the device (the block-tile kernel of rdf_bfilter.hip takes 8- / 4-byte columns only)
    n = args.rows
    v = torch.randint(-30000, 30000, (n,), dtype=torch.int16, device="cuda")
    mb = torch.randint(0, 256, (n // 8 + 64,), dtype=torch.uint8, device="cuda")
    ob = torch.empty(n, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    X = A.DeviceArray(v.data_ptr(), None, 0, n, A.I16, 0, keep=v)
    M = A.DeviceArray(mb.data_ptr(), None, 0, n, A.BOOL, 0, keep=mb)
    O = A.DeviceArray(ob.data_ptr(), None, 0, n, A.I16, 0, keep=ob)
    for _ in range(2):
        api.filter([X], [M], [O])
    lib.synchronize()
    lib.kernel_timing_reset(True)
    steps = 5
    for _ in range(steps):
        api.filter([X], [M], [O])
    lib.synchronize()
    ms, _ = lib.kernel_timing_get()
    lib.kernel_timing_reset(False)
    print(json.dumps({"kernel": "filter_1col_i16_one_chunk", "rows": n, "kernel_ms": ms / steps, "last_kernel": lib.last_kernel()}), flush=True)


if __name__ == "__main__":
    main()
