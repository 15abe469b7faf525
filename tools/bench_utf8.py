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

--sort measures rdf_lexsort_to_indices instead, on --sort-rows (1e7) device-resident rows: city-like rows (4-40 bytes,
10 % NULL), the same rows behind a 1 KiB common prefix, rows of 1000 distinct values, and [utf8, f64].  Each is timed by
HIP events around the whole call (rdf_kernel_timing_*: the rounds' host read-backs included), next to the floor — the
numeric rdf_sort_to_indices of as many random u64 keys — and to pyarrow.compute.sort_indices of the same rows on the
host.  The rounds each sort took come from rdf_last_kernel.

    python tools/bench_utf8.py [--rows 100000000] [--reps 5] [--out FILE]
    python tools/bench_utf8.py --sort [--sort-rows 10000000] [--reps 3] [--out FILE]
    python tools/bench_utf8.py --pred [--rows 100000000] [--long-rows 100000] [--out profiles/utf8_pred.jsonl]
    python tools/bench_utf8.py --build [--rows 100000000] [--long-rows 100000] [--out profiles/utf8_build.jsonl]
    python tools/bench_utf8.py --digest [--rows 100000000] [--long-rows 100000] [--out profiles/digest_bench.jsonl]
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


def city_like(rng, n, null_frac=0.1, lo=4, hi=40):
    """n rows of lo..hi ASCII bytes (a capital, then lower-case letters, spaces and commas), null_frac of them NULL
    -> (int64 offsets, uint8 bytes, bool valid)."""
    lens = rng.integers(lo, hi + 1, n)
    valid = rng.random(n) >= null_frac
    lens[~valid] = 0
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz  ,", dtype=np.uint8)
    data = alpha[rng.integers(0, len(alpha), int(offs[-1]))]
    data[offs[:-1][lens > 0]] = rng.integers(65, 91, int((lens > 0).sum()))
    return offs, data, valid


def sort_bench(args, api, torch):
    import time
    import pyarrow as pa
    import pyarrow.compute as pc
    rng = np.random.default_rng(23)
    n = args.sort_rows
    lines = []

    def dev_chunks(offs, data, valid, nch):
        """device chunks of n / nch rows each (Int32 offsets per chunk) over one device copy of the bytes"""
        dd = torch.from_numpy(data).cuda() if isinstance(data, np.ndarray) else data
        per = (len(offs) - 1 + nch - 1) // nch
        out = []
        for c in range(nch):
            r0, r1 = c * per, min((c + 1) * per, len(offs) - 1)
            o = offs[r0:r1 + 1] - offs[r0]
            assert o[-1] < 2**31
            ot = torch.from_numpy(o.astype(np.int32)).cuda()
            vt = None
            if valid is not None:
                bits = A.pack_bits(valid[r0:r1])
                vt = torch.from_numpy(bits).cuda()
            out.append(A.DeviceUtf8(ot.data_ptr(), dd.data_ptr() + int(offs[r0]), int(o[-1]), r1 - r0,
                                    vt.data_ptr() if vt is not None else None, 0, 0, -1, keep=(ot, dd, vt)))
        return out

    def host_arrow(offs, data, valid):
        assert offs[-1] < 2**31
        return pa.StringArray.from_buffers(len(offs) - 1, pa.py_buffer(offs.astype(np.int32)), pa.py_buffer(data),
                                           pa.py_buffer(A.pack_bits(valid)) if valid is not None else None)

    def time_device(keys):
        out_t = torch.empty(n + 64, dtype=torch.int32, device="cuda")
        out = A.DeviceArray(out_t.data_ptr(), None, 0, n, A.U32, 0, keep=out_t)
        for _ in range(args.warmup):
            api.lexsort_to_indices(keys, out=out)
        ms, wall = [], []
        for _ in range(args.reps):
            lib.kernel_timing_reset(True)
            t0 = time.perf_counter()
            api.lexsort_to_indices(keys, out=out)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(lib.kernel_timing_get()[0])
        lib.kernel_timing_reset(False)
        k = lib.last_kernel()
        rounds = int(k.split("Utf8 rounds: ")[1].rstrip(")")) if "Utf8 rounds: " in k else 0
        return min(ms), float(np.median(ms)), min(wall), rounds, out_t[:n].cpu().numpy().view(np.uint32)

    def time_arrow(fn):
        if fn is None:
            return None
        fn()
        best = 1e30
        for _ in range(max(1, min(args.reps, 3))):
            t0 = time.perf_counter()
            r = fn()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best, r

    def record(name, keys, arrow_fn, nbytes, note=None):
        best, med, wall, rounds, got = time_device(keys)
        ar = time_arrow(arrow_fn)
        same = None
        if ar is not None:
            same = bool(np.array_equal(got.astype(np.int64), ar[1].to_numpy().astype(np.int64)))
        rec = {"op": name, "rows": n, "bytes": int(nbytes), "rounds": rounds, "device_ms": round(best, 3), "device_ms_median": round(med, 3),
               "call_wall_ms": round(wall, 3), "pyarrow_host_ms": round(ar[0], 1) if ar else None, "same_order_as_pyarrow": same,
               "floor_u64_ms": round(floor_ms, 3)}
        if note:
            rec["note"] = note
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    # the floor: the numeric sort of n random u64 keys
    kt = torch.randint(-2**62, 2**62, (n,), device="cuda", dtype=torch.int64)
    K = A.DeviceArray(kt.data_ptr(), None, 0, n, A.U64, 0, keep=kt)
    ft = torch.empty(n + 64, dtype=torch.int32, device="cuda")
    F = A.DeviceArray(ft.data_ptr(), None, 0, n, A.U32, 0, keep=ft)
    for _ in range(args.warmup):
        api.sort_to_indices([[K]], [False], out=F)
    fl = []
    for _ in range(args.reps):
        lib.kernel_timing_reset(True)
        api.sort_to_indices([[K]], [False], out=F)
        fl.append(lib.kernel_timing_get()[0])
    lib.kernel_timing_reset(False)
    floor_ms = min(fl)
    kh = kt.cpu().numpy().view(np.uint64)
    pa_floor = time_arrow(lambda: pc.sort_indices(pa.array(kh)))
    rec = {"op": "sort_u64_floor", "rows": n, "device_ms": round(floor_ms, 3), "pyarrow_host_ms": round(pa_floor[0], 1)}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    del kt, K, ft, F

    # 1. city-like rows
    offs, data, valid = city_like(rng, n)
    col = dev_chunks(offs, data, valid, 1)
    arr = host_arrow(offs, data, valid)
    record("utf8_sort_city_like", [(col, False)], lambda: pc.sort_indices(arr), offs[-1])

    # 2. the same rows behind a 1 KiB common prefix (built on the device: ~10 GB, 8 chunks)
    P = 1024
    lens = np.diff(offs)
    offs2 = np.zeros(n + 1, dtype=np.int64)
    offs2[1:] = np.cumsum(lens + P)
    d2 = torch.full((int(offs2[-1]) + 64,), ord("p"), dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(data).cuda()
    row_of = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.from_numpy(lens).cuda())
    o1 = torch.from_numpy(offs[:-1]).cuda()
    o2 = torch.from_numpy(offs2[:-1]).cuda()
    pos = torch.arange(int(offs[-1]), device="cuda", dtype=torch.int64)
    d2[o2[row_of] + P + (pos - o1[row_of])] = src
    del row_of, pos, o1, o2, src
    col2 = dev_chunks(offs2, d2, valid, 8)
    record("utf8_sort_city_like_1k_prefix", [(col2, False)], None, offs2[-1],
           note="pyarrow not run: a host sort of 10 GB of strings sharing 1 KiB")
    del col2, d2

    # 3. rows of 1000 distinct values
    woffs, wdata, _v = city_like(rng, 1000, null_frac=0.0)
    pick = rng.integers(0, 1000, n)
    wl = np.diff(woffs)
    lens3 = wl[pick]
    offs3 = np.zeros(n + 1, dtype=np.int64)
    offs3[1:] = np.cumsum(lens3)
    d3 = torch.empty(int(offs3[-1]) + 64, dtype=torch.uint8, device="cuda")
    row_of = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.from_numpy(lens3).cuda())
    pos = torch.arange(int(offs3[-1]), device="cuda", dtype=torch.int64)
    wsrc = torch.from_numpy(wdata).cuda()
    pk = torch.from_numpy(pick).cuda()
    d3[:int(offs3[-1])] = wsrc[torch.from_numpy(woffs[:-1]).cuda()[pk[row_of]] + (pos - torch.from_numpy(offs3[:-1]).cuda()[row_of])]
    del row_of, pos
    data3 = d3[:int(offs3[-1])].cpu().numpy()
    col3 = dev_chunks(offs3, d3, None, 1)
    arr3 = host_arrow(offs3, data3, None)
    record("utf8_sort_1000_distinct", [(col3, False)], lambda: pc.sort_indices(arr3), offs3[-1])
    del col3, d3

    # 4. [utf8, f64]
    fv = rng.random(n)
    fa = torch.from_numpy(fv).cuda()
    FA = A.DeviceArray(fa.data_ptr(), None, 0, n, A.F64, 0, keep=fa)
    tab = pa.table({"s": arr, "f": pa.array(fv)})
    record("utf8_sort_utf8_f64", [(col, False), ([FA], False)],
           lambda: pc.sort_indices(tab, sort_keys=[("s", "ascending"), ("f", "ascending")]), offs[-1] + 8 * n)
    if args.out:
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


def pred_bench(args, api, torch):
    """--pred: rdf_utf8_predicate / rdf_utf8_compare / rdf_utf8_measure on device-resident rows.  Per case: the HIP-event
    kernel time, the algorithmic bytes (Int32 offsets + the data bytes the op must look at + 2 bits, or 4 bytes + 1 bit, per
    row out) and their rate as a fraction of rdf_probe_stream's READ rate in the same process; pyarrow.compute on the host
    over --arrow-rows of the same rows; rdf_utf8_trim on the same column for context."""
    import time
    import pyarrow as pa
    import pyarrow.compute as pc
    so = lib.load()
    so.rdf_utf8_trim.restype = C.c_int
    rng = np.random.default_rng(29)
    n, nch = args.rows, args.chunks
    assert n % nch == 0
    cr = n // nch
    pb = 1 << 31
    probe = torch.empty(pb, dtype=torch.uint8, device="cuda")
    read_gbps, read_shape = lib.probe_stream(0, probe.data_ptr(), 0, 0, pb, 10)
    del probe
    lines = []
    hit = "London, UK"

    def column(strings):
        col, nbytes = device_column(torch, strings, cr)
        reps, rem = divmod(cr, len(strings))
        lens = np.array([len(x.encode()) for x in strings], dtype=np.int64)
        return col, lens, reps, rem

    def looked(lens, reps, rem, f):
        """bytes of the rows an op must look at: f(row lengths) summed over the tiled column"""
        v = f(lens)
        return int(v.sum()) * reps * nch + int(v[:rem].sum()) * nch

    def arrow_time(fn, strings):
        k = min(args.arrow_rows, n)
        arr = pa.array((strings * (k // len(strings) + 1))[:k], type=pa.string())
        fn(arr)
        best = 1e30
        for _ in range(3):
            t0 = time.perf_counter()
            fn(arr)
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return k, best

    def run(name, call, rows, data_bytes, out_bytes_per_row, arrow=None, strings=None, chunks=nch):
        for _ in range(args.warmup):
            call()
        ms = []
        for _ in range(args.reps):
            lib.kernel_timing_reset(True)
            res = call()
            ms.append(lib.kernel_timing_get()[0])
        lib.kernel_timing_reset(False)
        alg = 4 * (rows + chunks) + data_bytes + int(rows * out_bytes_per_row)
        best = min(ms)
        rec = {"op": name, "rows": rows, "chunks": chunks, "bytes_looked_at": data_bytes, "alg_bytes": alg, "kernel": lib.last_kernel(),
               "kernel_ms": round(best, 3), "kernel_ms_median": round(float(np.median(ms)), 3), "GBps": round(alg / best / 1e6, 1),
               "read_probe_GBps": round(read_gbps, 1), "frac_of_read": round(alg / best / 1e6 / read_gbps, 3), "read_probe_shape": read_shape,
               "short_row_bytes": 256}
        if res is not None and hasattr(res[0], "null_count"):
            rec["result_rows"] = sum(r.length for r in res)
        if arrow is not None:
            k, t = arrow_time(arrow, strings)
            rec["pyarrow_rows"], rec["pyarrow_ms"] = k, round(t, 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    BIT2, I32 = 0.25, 4.125
    for label, mixed in (("ascii", False), ("mixed", True)):
        strings = pool(rng, 1 << 20, mixed)
        for i in range(0, len(strings), 16):
            strings[i] = hit
        col, lens, reps, rem = column(strings)
        cols = [col] * nch
        bo = [api._window_out(A.BOOL, cr, True, False) for _ in range(nch)]     # outputs allocated once
        io = [api._window_out(A.I32, cr, True, False) for _ in range(nch)]
        allb = looked(lens, reps, rem, lambda v: v)
        m = len(hit)
        run(f"eq_1_16_{label}", lambda: api.utf8_predicate("eq", cols, hit, outs=bo), n, looked(lens, reps, rem, lambda v: np.where(v == m, v, 0)), BIT2,
            lambda a: pc.equal(a, hit), strings)
        run(f"starts_with_3_{label}", lambda: api.utf8_predicate("starts_with", cols, "Lon", outs=bo), n, looked(lens, reps, rem, lambda v: np.minimum(v, 3)), BIT2,
            lambda a: pc.starts_with(a, "Lon"), strings)
        run(f"contains_3_{label}", lambda: api.utf8_predicate("contains", cols, "don", outs=bo), n, allb, BIT2, lambda a: pc.match_substring(a, "don"), strings)
        run(f"like_ab_cd_{label}", lambda: api.utf8_predicate("like", cols, "%ab%cd%", outs=bo), n, allb, BIT2, lambda a: pc.match_like(a, "%ab%cd%"), strings)
        run(f"length_{label}", lambda: api.utf8_measure("length", cols, outs=io), n, allb, I32, lambda a: pc.utf8_length(a), strings)
        run(f"octet_length_{label}", lambda: api.utf8_measure("octet_length", cols, outs=io), n, 0, I32, lambda a: pc.binary_length(a), strings)
        run(f"locate_3_{label}", lambda: api.utf8_measure("locate", cols, "don", 1, outs=io), n, allb, I32, lambda a: pc.find_substring(a, "don"), strings)
        run(f"compare_eq_columns_{label}", lambda: api.utf8_compare("eq", cols, cols, outs=bo), n, 2 * allb, BIT2, lambda a: pc.equal(a, a), strings)
        run(f"compare_lt_columns_{label}", lambda: api.utf8_compare("lt", cols, cols, outs=bo), n, 2 * allb, BIT2)
        # today's text reader on the same column: rdf_utf8_trim (the span pass + the copy)
        carr = (A.rdf_utf8_array * nch)(*[col.c_struct()] * nch)
        ot = [torch.empty(cr + 1 + 64, dtype=torch.int32, device="cuda") for _ in range(nch)]
        dt = [torch.empty(int(lens.sum()) * (reps + 1) + 64, dtype=torch.uint8, device="cuda") for _ in range(nch)]
        oo = (A.rdf_out * nch)(*[A.rdf_out(t.data_ptr(), None, cr + 1, 0, 0, A.I32, A.MEM_DEVICE) for t in ot])
        od = (A.rdf_out * nch)(*[A.rdf_out(t.data_ptr(), None, t.numel() - 64, 0, 0, A.U8, A.MEM_DEVICE) for t in dt])

        def trim():
            assert so.rdf_utf8_trim(carr, C.c_int64(nch), oo, od) == A.RDF_OK, so.rdf_last_error()
        run(f"utf8_trim_{label}", trim, n, 2 * allb, 4)
        del ot, dt, col, cols, bo, io
    # the long-row path: rows of 16 KiB
    lrows = args.long_rows
    long_pool = ["".join(rng.choice(list("abcdefghijklmnop "), size=16384)) for _ in range(64)]
    h = A.HostUtf8.from_pylist(long_pool)
    po = torch.from_numpy(h.offsets.astype(np.int64)).cuda()
    pd = torch.from_numpy(h.data[:int(h.offsets[-1])].copy()).cuda()
    per = min(lrows, (2**31 - 1) // 16384 // 64 * 64)
    chunks = []
    for c0 in range(0, lrows, per):
        k = min(per, lrows - c0)
        offs = (torch.arange(k + 1, device="cuda", dtype=torch.int64) * 16384).to(torch.int32)
        data = pd.repeat((k + 63) // 64)[:k * 16384].contiguous()
        chunks.append(A.DeviceUtf8(offs.data_ptr(), data.data_ptr(), k * 16384, k, None, 0, 0, 0, keep=(offs, data, None)))
    lb = lrows * 16384
    run("contains_none_16KiB_rows", lambda: api.utf8_predicate("contains", chunks, "zzz"), lrows, lb, BIT2, chunks=len(chunks))
    run("contains_3_16KiB_rows", lambda: api.utf8_predicate("contains", chunks, "abc"), lrows, lb, BIT2, chunks=len(chunks))
    run("length_16KiB_rows", lambda: api.utf8_measure("length", chunks), lrows, lb, I32, chunks=len(chunks))
    if args.out:
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


def build_bench(args, api, torch):
    """--build: rdf_utf8_concat / _pad / _repeat / _reverse / _substring_index on device-resident rows.  Per case: the HIP-event
    kernel time of the call into buffers sized beforehand (size pass + scan + write pass), the bytes moved (Int32 offsets in and
    out, the source bytes once, the output bytes once) and their rate as a fraction of rdf_probe_stream's COPY rate in the same
    process; rdf_utf8_trim on the same column (today's writer: the same passes with one source span) for context."""
    so = lib.load()
    so.rdf_utf8_trim.restype = C.c_int
    rng = np.random.default_rng(31)
    n, nch = args.rows, args.chunks
    assert n % nch == 0
    cr = n // nch
    pb = 1 << 30
    pa_, pb_ = torch.empty(pb, dtype=torch.uint8, device="cuda"), torch.empty(pb, dtype=torch.uint8, device="cuda")
    copy_gbps, copy_shape = lib.probe_stream(1, pa_.data_ptr(), pb_.data_ptr(), 0, pb, 10)
    del pa_, pb_
    def emit(rec):          # a line at a time: a later case that fails loses nothing
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def run(name, op, chunks, *a, rows, in_bytes, note=None):
        """the sizing call, buffers of those sizes, then warm-up and the timed calls"""
        call, shape, nullable = api.utf8_build_call(op, chunks, *a)
        k = len(shape)
        ot = [torch.empty(c.length + 1 + 64, dtype=torch.int32, device="cuda") for c in shape]
        vt = [torch.empty((c.length + 63) // 64 * 8 + 8, dtype=torch.uint8, device="cuda") if nl else None for c, nl in zip(shape, nullable)]
        oo = (A.rdf_out * k)(*[A.rdf_out(t.data_ptr(), v.data_ptr() if v is not None else None, c.length + 1, 0, 0, A.I32, A.MEM_DEVICE) for t, v, c in zip(ot, vt, shape)])
        od = (A.rdf_out * k)(*[A.rdf_out(None, None, 0, 0, 0, A.U8, A.MEM_DEVICE) for _ in shape])
        st = call(oo, od)
        assert st in (A.RDF_OK, A.RDF_MEMORY_ERROR), so.rdf_last_error()
        out_bytes = [od[i].length for i in range(k)]
        dt = [torch.empty(b + 64, dtype=torch.uint8, device="cuda") for b in out_bytes]
        od = (A.rdf_out * k)(*[A.rdf_out(t.data_ptr(), None, b, 0, 0, A.U8, A.MEM_DEVICE) for t, b in zip(dt, out_bytes)])
        for _ in range(args.warmup):
            assert call(oo, od) == A.RDF_OK, so.rdf_last_error()
        ms = []
        for _ in range(3):
            lib.kernel_timing_reset(True)
            assert call(oo, od) == A.RDF_OK, so.rdf_last_error()
            ms.append(lib.kernel_timing_get()[0])
        lib.kernel_timing_reset(False)
        best = min(ms)
        moved = 4 * (rows + k) * 2 + in_bytes + sum(out_bytes)
        rec = {"op": name, "rows": rows, "chunks": k, "in_bytes": in_bytes, "out_bytes": sum(out_bytes), "moved_bytes": moved, "kernel": lib.last_kernel(),
               "kernel_ms": round(best, 3), "kernel_ms_median": round(float(np.median(ms)), 3), "GBps": round(moved / best / 1e6, 1),
               "ns_per_out_byte": round(best * 1e6 / max(1, sum(out_bytes)), 4),
               "copy_probe_GBps": round(copy_gbps, 1), "frac_of_copy": round(moved / best / 1e6 / copy_gbps, 3), "copy_probe_shape": copy_shape}
        if note:
            rec["note"] = note
        emit(rec)
        del ot, vt, dt
        return best

    for label, mixed in (("ascii", False), ("mixed", True)):
        strings = pool(rng, 1 << 20, mixed)
        for i in range(0, len(strings), 16):
            strings[i] = "www.apache.org"
        x, xb = device_column(torch, strings, cr)
        y, yb = device_column(torch, strings[::-1], cr)
        xs, ys = [x] * nch, [y] * nch
        # the same columns with 10 % NULL rows
        vx = torch.zeros((cr + 63) // 64 * 8 + 8, dtype=torch.uint8, device="cuda")
        vy = torch.zeros_like(vx)
        torch.cuda.synchronize()
        lib.fill_validity(vx.data_ptr(), cr, 7, 0, 0, 0.1)
        lib.fill_validity(vy.data_ptr(), cr, 7, 1, 0, 0.1)
        xn = [A.DeviceUtf8(x.offsets_ptr, x.data_ptr, x.data_length, cr, vx.data_ptr(), 0, 0, -1, keep=(x.keep, vx))] * nch
        yn = [A.DeviceUtf8(y.offsets_ptr, y.data_ptr, y.data_length, cr, vy.data_ptr(), 0, 0, -1, keep=(y.keep, vy))] * nch
        # today's writer on the same column: rdf_utf8_trim
        carr = (A.rdf_utf8_array * nch)(*[x.c_struct()] * nch)
        ot = [torch.empty(cr + 1 + 64, dtype=torch.int32, device="cuda") for _ in range(nch)]
        dt = [torch.empty(xb + 64, dtype=torch.uint8, device="cuda") for _ in range(nch)]
        oo = (A.rdf_out * nch)(*[A.rdf_out(t.data_ptr(), None, cr + 1, 0, 0, A.I32, A.MEM_DEVICE) for t in ot])
        od = (A.rdf_out * nch)(*[A.rdf_out(t.data_ptr(), None, xb, 0, 0, A.U8, A.MEM_DEVICE) for t in dt])
        tms = []
        for i in range(args.warmup + 3):
            lib.kernel_timing_reset(True)
            assert so.rdf_utf8_trim(carr, C.c_int64(nch), oo, od) == A.RDF_OK, so.rdf_last_error()
            tms.append(lib.kernel_timing_get()[0])
        lib.kernel_timing_reset(False)
        trim_ms = min(tms[args.warmup:])
        rec = {"op": f"utf8_trim_{label}", "rows": n, "chunks": nch, "in_bytes": xb * nch, "kernel": lib.last_kernel(), "kernel_ms": round(trim_ms, 3)}
        emit(rec)
        del ot, dt
        run(f"concat_x_lit_y_{label}", "concat", None, [xs, ", ", ys], rows=n, in_bytes=(xb + yb) * nch, note="compare with two trims")
        run(f"concat_ws_10pct_nulls_{label}", "concat_ws", None, [xn, yn], ", ", rows=n, in_bytes=(xb + yb) * nch, note="in_bytes counts the NULL rows' bytes too")
        run(f"lpad_32_space_{label}", "lpad", xs, 32, " ", rows=n, in_bytes=xb * nch)
        run(f"repeat_3_{label}", "repeat", xs, 3, rows=n, in_bytes=xb * nch)
        run(f"reverse_{label}", "reverse", xs, rows=n, in_bytes=xb * nch)
        run(f"substring_index_dot_2_{label}", "substring_index", xs, ".", 2, rows=n, in_bytes=xb * nch, note="1 row in 16 holds the delimiter twice; the others are searched to their end")
        run(f"substring_index_space_m1_{label}", "substring_index", xs, " ", -1, rows=n, in_bytes=xb * nch)
        del x, y, xs, ys, xn, yn, vx, vy
    # rows of 16 KiB: the copy must cost their bytes, not their count
    lrows = args.long_rows
    long_pool = ["".join(rng.choice(list("abcdefghijklmnop "), size=16384)) for _ in range(64)]
    h = A.HostUtf8.from_pylist(long_pool)
    pd = torch.from_numpy(h.data[:int(h.offsets[-1])].copy()).cuda()
    per = 32768          # 2 x 16 KiB x 32768 rows stay below 2^31 bytes a chunk
    chunks = []
    for c0 in range(0, lrows, per):
        k = min(per, lrows - c0)
        offs = (torch.arange(k + 1, device="cuda", dtype=torch.int64) * 16384).to(torch.int32)
        data = pd.repeat((k + 63) // 64)[:k * 16384].contiguous()
        chunks.append(A.DeviceUtf8(offs.data_ptr(), data.data_ptr(), k * 16384, k, None, 0, 0, 0, keep=(offs, data, None)))
    lb = lrows * 16384
    torch.cuda.synchronize()          # (the library runs on its own stream: torch's fills must have landed before the sizing call reads the offsets)
    run("reverse_16KiB_rows", "reverse", chunks, rows=lrows, in_bytes=lb)
    run("repeat_2_16KiB_rows", "repeat", chunks, 2, rows=lrows, in_bytes=lb)
    run("lpad_20000_16KiB_rows", "lpad", chunks, 20000, "ab", rows=lrows, in_bytes=lb)
    run("substring_index_16KiB_rows", "substring_index", chunks, "ab", 100, rows=lrows, in_bytes=lb)


def digest_bench(args, api, torch):
    """--digest: rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32 on device-resident rows.  Per case: the HIP-event kernel
    time (best of --reps after warm-up; for the digests the count pass, the scan and the write pass of the call into buffers
    sized beforehand), the bytes the function must read (Int32 offsets + the rows' bytes) and their rate as a fraction of
    rdf_probe_stream's READ rate in the same process, next to rdf_utf8_measure(LENGTH) on the same column as the reader's
    floor.  Then rdf_hash_columns over an Int64 column and over (Int64, Utf8), rows of 16 KiB, a skewed column (1 % of the
    rows 16 KiB, the rest short: a lane per row, the only form there is) and hashlib / zlib on one host thread."""
    import hashlib
    import time
    import zlib
    rng = np.random.default_rng(31)
    n, nch = args.rows, max(args.chunks, 8)      # 8 chunks: 12.5 M rows x 128 hex bytes stay below 2^31 bytes a chunk
    assert n % nch == 0
    cr = n // nch
    pb = 1 << 31
    probe = torch.empty(pb, dtype=torch.uint8, device="cuda")
    read_gbps, read_shape = lib.probe_stream(0, probe.data_ptr(), 0, 0, pb, 10)
    del probe
    lines = []

    def run(name, call, rows, data_bytes, chunks, floor_ms=None, extra_in=0):
        for _ in range(args.warmup):
            call()
        ms = []
        for _ in range(args.reps):
            lib.kernel_timing_reset(True)
            call()
            ms.append(lib.kernel_timing_get()[0])
        lib.kernel_timing_reset(False)
        read = 4 * (rows + chunks) + data_bytes + extra_in
        best = min(ms)
        rec = {"op": name, "rows": rows, "chunks": chunks, "bytes_read": read, "kernel": lib.last_kernel(), "kernel_ms": round(best, 3),
               "kernel_ms_median": round(float(np.median(ms)), 3), "read_GBps": round(read / best / 1e6, 1), "read_probe_GBps": round(read_gbps, 1),
               "frac_of_read": round(read / best / 1e6 / read_gbps, 4), "read_probe_shape": read_shape}
        if floor_ms is not None:
            rec["length_floor_ms"] = round(floor_ms, 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        return best

    def digest_call(fn, cols, rows_per_chunk):
        width = A.DIGEST_HEX_BYTES[A.DIGEST_KINDS[fn]]
        ot = [torch.empty(r + 1 + 64, dtype=torch.int32, device="cuda") for r in rows_per_chunk]
        dt = [torch.empty(r * width + 64, dtype=torch.uint8, device="cuda") for r in rows_per_chunk]
        oo = (A.rdf_out * len(cols))(*[A.rdf_out(t.data_ptr(), None, r + 1, 0, 0, A.I32, A.MEM_DEVICE) for t, r in zip(ot, rows_per_chunk)])
        od = (A.rdf_out * len(cols))(*[A.rdf_out(t.data_ptr(), None, r * width, 0, 0, A.U8, A.MEM_DEVICE) for t, r in zip(dt, rows_per_chunk)])
        call, _, _ = api.utf8_digest_call(fn, cols)

        def go(keep=(ot, dt)):
            st = call(oo, od)
            assert st == A.RDF_OK, st
        return go

    def all_functions(label, cols, rows_per_chunk, data_bytes, digests=A.DIGEST_KINDS):
        rows, k = sum(rows_per_chunk), len(cols)
        io32 = [api._window_out(A.I32, r, True, False) for r in rows_per_chunk]
        io64 = [api._window_out(A.I64, r, True, False) for r in rows_per_chunk]
        floor = run(f"length_{label}", lambda: api.utf8_measure("length", cols, outs=io32), rows, data_bytes, k)
        for fn in digests:
            run(f"{fn}_{label}", digest_call(fn, cols, rows_per_chunk), rows, data_bytes, k, floor)
            torch.cuda.empty_cache()
        run(f"crc32_{label}", lambda: api.utf8_crc32(cols, outs=io64), rows, data_bytes, k, floor)
        run(f"hash_{label}", lambda: api.hash_columns("hash", [cols], outs=io32), rows, data_bytes, k, floor)
        run(f"xxhash64_{label}", lambda: api.hash_columns("xxhash64", [cols], outs=io64), rows, data_bytes, k, floor)
        return io32, io64, floor

    for label, mixed in (("ascii", False), ("mixed", True)):
        strings = pool(rng, 1 << 20, mixed)
        col, nbytes = device_column(torch, strings, cr)
        cols = [col] * nch
        io32, io64, floor = all_functions(label, cols, [cr] * nch, nbytes * nch)
        if not mixed:
            ints = torch.randint(-2**62, 2**62, (cr,), dtype=torch.int64, device="cuda")
            icols = [A.DeviceArray(ints.data_ptr(), None, 0, cr, A.I64, 0, keep=ints)] * nch
            for fn, outs in (("hash", io32), ("xxhash64", io64)):
                run(f"{fn}_int64_column", lambda: api.hash_columns(fn, [icols], outs=outs), n, 0, nch, extra_in=8 * n - 4 * (n + nch))
                run(f"{fn}_int64_and_utf8_{label}", lambda: api.hash_columns(fn, [icols, cols], outs=outs), n, nbytes * nch, nch, floor, extra_in=8 * n)
            del ints, icols
        # hashlib / zlib on one host thread over the pool (2^20 rows), for scale
        raw_rows = [x.encode() for x in strings]
        for name, f in (("md5", lambda b: hashlib.md5(b).hexdigest()), ("sha1", lambda b: hashlib.sha1(b).hexdigest()),
                        ("sha256", lambda b: hashlib.sha256(b).hexdigest()), ("sha512", lambda b: hashlib.sha512(b).hexdigest()), ("crc32", zlib.crc32)):
            t0 = time.perf_counter()
            for b in raw_rows:
                f(b)
            rec = {"op": f"host_{name}_{label}", "rows": len(raw_rows), "host_ms": round((time.perf_counter() - t0) * 1e3, 1), "threads": 1}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del col, cols, io32, io64
        torch.cuda.empty_cache()

    # rows of 16 KiB
    lrows = args.long_rows
    long_pool = ["".join(rng.choice(list("abcdefghijklmnop "), size=16384)) for _ in range(64)]
    h = A.HostUtf8.from_pylist(long_pool)
    pd = torch.from_numpy(h.data[:int(h.offsets[-1])].copy()).cuda()
    per = min(lrows, (2**31 - 1) // 16384 // 64 * 64)
    chunks = []
    for c0 in range(0, lrows, per):
        k = min(per, lrows - c0)
        offs = (torch.arange(k + 1, device="cuda", dtype=torch.int64) * 16384).to(torch.int32)
        data = pd.repeat((k + 63) // 64)[:k * 16384].contiguous()
        chunks.append(A.DeviceUtf8(offs.data_ptr(), data.data_ptr(), k * 16384, k, None, 0, 0, 0, keep=(offs, data, None)))
    all_functions("16KiB_rows", chunks, [c.length for c in chunks], lrows * 16384, digests=("md5", "sha1", "sha256", "sha512"))
    del chunks

    # the skewed column: 1 % of the rows 16 KiB, the rest 12 .. 36 bytes, one chunk
    srows = 4_000_000
    lens = torch.randint(12, 37, (srows,), dtype=torch.int64, device="cuda")
    lens[::100] = 16384
    offs64 = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(lens, 0)])
    total = int(offs64[-1].item())
    assert total < 2**31
    data = torch.randint(97, 123, (total,), dtype=torch.uint8, device="cuda")
    offs = offs64.to(torch.int32)
    skew = [A.DeviceUtf8(offs.data_ptr(), data.data_ptr(), total, srows, None, 0, 0, 0, keep=(offs, data, None))]
    all_functions("skewed_1pct_16KiB", skew, [srows], total, digests=("md5", "sha256"))
    if args.out:
        with open(args.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--chunks", type=int, default=4, help="the column's chunks (one StringArray holds < 2^31 bytes)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sort", action="store_true", help="measure rdf_lexsort_to_indices instead of the other operators")
    ap.add_argument("--sort-rows", type=int, default=10_000_000)
    ap.add_argument("--pred", action="store_true", help="measure rdf_utf8_predicate / _compare / _measure instead (profiles/utf8_pred.jsonl)")
    ap.add_argument("--build", action="store_true", help="measure rdf_utf8_concat / _pad / _repeat / _reverse / _substring_index instead (profiles/utf8_build.jsonl)")
    ap.add_argument("--digest", action="store_true", help="measure rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32 instead (profiles/digest_bench.jsonl)")
    ap.add_argument("--long-rows", type=int, default=100_000, help="--pred / --build / --digest: rows of 16 KiB for the long-row path")
    ap.add_argument("--arrow-rows", type=int, default=10_000_000, help="--pred: rows pyarrow.compute is timed on")
    args = ap.parse_args()
    import torch
    api = lib.api()
    assert lib.device_count() >= 1, "needs a GPU"
    lib.set_device(0)
    if args.sort:
        sort_bench(args, api, torch)
        return
    if args.pred:
        pred_bench(args, api, torch)
        return
    if args.build:
        build_bench(args, api, torch)
        return
    if args.digest:
        digest_bench(args, api, torch)
        return
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
