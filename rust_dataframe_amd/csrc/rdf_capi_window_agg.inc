// rdf_capi_window_agg.inc — host side of rdf_window_agg: sum / min / max / count / avg / first_value / last_value over window
// frames (kernels: rdf_window_agg.hip, argument blocks: rdf_window_agg.h); textually included by rdf_capi.cpp after
// rdf_capi_window.inc, whose front (checks, staging, sort_core, flag pass, scan, start tables) it shares with rdf_window.
//
// After the front: one scan per (value column, payload) a call needs — scans that two calls would build alike are built
// once — and one emit launch that answers every call of the request.

namespace {

int window_agg_out_dtype(int fn, int value_dtype) {
    switch (fn) {
        case RDF_WAGG_COUNT: return RDF_I64;
        case RDF_WAGG_AVG: return RDF_F64;
        case RDF_WAGG_FIRST_VALUE: case RDF_WAGG_LAST_VALUE: return RDF_U32;
        default: return value_dtype;
    }
}

constexpr int64_t kWaggOffsetCap = (int64_t)1 << 32;   // an offset of 2^32 or more is beyond every partition

rdf_status window_agg_check_frame(int c, const rdf_window_frame& f) {
    if (f.unit != RDF_FRAME_ROWS && f.unit != RDF_FRAME_RANGE) return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: unknown frame unit %d", c, f.unit);
    for (int kind : {f.start_kind, f.end_kind})
        if (kind < RDF_BOUND_UNBOUNDED_PRECEDING || kind > RDF_BOUND_UNBOUNDED_FOLLOWING)
            return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: unknown frame bound %d", c, kind);
    if (f.start_kind == RDF_BOUND_UNBOUNDED_FOLLOWING) return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: a frame cannot start at UNBOUNDED FOLLOWING", c);
    if (f.end_kind == RDF_BOUND_UNBOUNDED_PRECEDING) return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: a frame cannot end at UNBOUNDED PRECEDING", c);
    const bool so = f.start_kind == RDF_BOUND_PRECEDING || f.start_kind == RDF_BOUND_FOLLOWING;
    const bool eo = f.end_kind == RDF_BOUND_PRECEDING || f.end_kind == RDF_BOUND_FOLLOWING;
    if ((so && f.start < 0) || (eo && f.end < 0)) return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: a frame offset cannot be negative", c);
    if (f.unit == RDF_FRAME_RANGE && (so || eo)) return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: range offsets are not built", c);
    if (f.start_kind > f.end_kind || (f.start_kind == RDF_BOUND_PRECEDING && f.end_kind == RDF_BOUND_PRECEDING && f.start < f.end) ||
        (f.start_kind == RDF_BOUND_FOLLOWING && f.end_kind == RDF_BOUND_FOLLOWING && f.start > f.end))
        return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: the frame starts after its end", c);
    return RDF_OK;
}

// One scan of the request: what it runs over and where its words live.
struct WaggScan {
    int kind, value, restart, backward, ismax;
    uint32_t w;
    uint64_t* out[4];
};

// The scans the calls of one request need, each built once (rdf_window_agg and rdf_window_range_agg).
struct WaggScans {
    const WinFront& wf;
    const int* vdt;                     // dtype per value column
    std::vector<WaggScan> scans;
    WaggScans(const WinFront& front, const int* value_dtypes) : wf(front), vdt(value_dtypes) { scans.reserve(4 * RDF_WINDOW_MAX_CALLS); }   // (pointers into it are handed out)
    rdf_status get(int kind, int value, int restart, int backward, int ismax, uint32_t w, WaggScan** out) {
        for (WaggScan& sc : scans)
            if (sc.kind == kind && sc.value == value && sc.restart == restart && sc.backward == backward && sc.ismax == ismax && sc.w == w) { *out = &sc; return RDF_OK; }
        const int64_t n = wf.n, nseg = (n + kWaggSeg - 1) / kWaggSeg;
        WaggScan sc{kind, value, restart, backward, ismax, w, {}};
        WaggScanArgs a;
        memset(&a, 0, sizeof a);
        void* p;
        for (int x = 0; x < wagg_words(kind); ++x) {
            RDF_TRY(arena_alloc((size_t)n * 8, &p));
            a.out[x] = sc.out[x] = (uint64_t*)p;
            RDF_TRY(arena_alloc((size_t)nseg * 8, &p));
            a.seg[x] = (uint64_t*)p;
        }
        RDF_TRY(arena_alloc((size_t)nseg * 4, &p));
        a.seg_first = (uint32_t*)p;
        a.scan = wf.scan;
        a.pstart = wf.pstart;
        a.perm = wf.perm;
        a.chunks = wf.d.tb.dev_at<DevChunkCol>(wf.d.o_ch) + (size_t)(wf.nkeys + value) * wf.nch;
        a.row_start = wf.d_row_start;
        a.nchunks = wf.nch;
        a.n = n;
        a.f64 = vdt[value] == RDF_F64;
        a.restart = restart;
        a.backward = backward;
        a.ismax = ismax;
        a.w = w;
        HIP_TRY(launch_wagg_scan(kind, a, g_ctx.stream));
        scans.push_back(sc);
        *out = &scans.back();
        return RDF_OK;
    }
};

// Builds (or finds) the scans call (fn, value) needs over a frame of the given kinds and points `o` at them.  so / eo: the
// signed ROWS offsets of the two ends (read for MIN / MAX over a ROWS frame bounded on both sides only).
rdf_status window_agg_wire_call(WaggScans& S, int fn, int value, int unit, int start_kind, int end_kind, int64_t so, int64_t eo, WaggCallOut& o) {
    WaggScan* sc = nullptr;
    const bool is_ext = fn == RDF_WAGG_MIN || fn == RDF_WAGG_MAX;
    // SUM / COUNT(value) / Int64 MIN, MAX (their NULL rule): the prefix of the column's own dtype.  AVG: the Float64 one.
    if (fn == RDF_WAGG_AVG || (o.f64 && (fn == RDF_WAGG_SUM || (fn == RDF_WAGG_COUNT && value >= 0)))) {
        RDF_TRY(S.get(kWaggSumF, value, kWaggRestartPartition, 0, 0, 0, &sc));
        for (int x = 0; x < 4; ++x) o.sum[x] = sc->out[x];
    } else if (!o.f64 && value >= 0 && (fn == RDF_WAGG_SUM || fn == RDF_WAGG_COUNT || is_ext)) {
        RDF_TRY(S.get(kWaggSumI, value, kWaggRestartPartition, 0, 0, 0, &sc));
        o.sum[0] = sc->out[0];
        o.sum[2] = sc->out[1];
    }
    if (is_ext) {
        const int ismax = fn == RDF_WAGG_MAX;
        const bool ub_start = start_kind == RDF_BOUND_UNBOUNDED_PRECEDING, ub_end = end_kind == RDF_BOUND_UNBOUNDED_FOLLOWING;
        if (ub_start) {                                     // [0, b]: F[b] of a scan that restarts at partition starts only
            o.ext_mode = kWaggExtForward;
            RDF_TRY(S.get(kWaggExt, value, kWaggRestartPartition, 0, ismax, 0, &sc));
            o.fwd = sc->out[0];
        } else if (ub_end) {                                // [a, n - 1]: B[a]
            o.ext_mode = kWaggExtBackward;
            RDF_TRY(S.get(kWaggExt, value, kWaggRestartPartition, 1, ismax, 0, &sc));
            o.bwd = sc->out[0];
        } else if (unit == RDF_FRAME_RANGE) {               // CURRENT ROW .. CURRENT ROW: the peer group, F[l]
            o.ext_mode = kWaggExtForward;
            RDF_TRY(S.get(kWaggExt, value, kWaggRestartPeer, 0, ismax, 0, &sc));
            o.fwd = sc->out[0];
        } else {                                            // both bounds finite: blocks of the unclipped frame length
            const int64_t width = eo - so + 1;              // >= 1: checked by the caller
            o.w = (uint32_t)std::min<int64_t>(width, 0xFFFFFFFFll);   // >= every partition: one block each
            o.ext_mode = kWaggExtBlock;
            RDF_TRY(S.get(kWaggExt, value, kWaggRestartBlock, 0, ismax, o.w, &sc));
            o.fwd = sc->out[0];
            RDF_TRY(S.get(kWaggExt, value, kWaggRestartBlock, 1, ismax, o.w, &sc));
            o.bwd = sc->out[0];
        }
    }
    return RDF_OK;
}

// Where call c's answer is written on the device: the caller's buffers, or arena copies of them for host memory.
rdf_status window_agg_alloc_out(int fn, const rdf_out& out, int32_t mem, int64_t n, WaggCallOut& o, void** dvalid) {
    o.values = out.values;
    if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)n * (size_t)dtype_size(out.dtype), &o.values));
    if (fn != RDF_WAGG_COUNT) {
        void* pv;
        RDF_TRY(arena_alloc((size_t)n, &pv));
        o.vbytes = (uint8_t*)pv;
        *dvalid = out.validity;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)((n + 63) / 64) * 8, dvalid));
    }
    return RDF_OK;
}

// After the emit launch: validity bitmaps, NULL counts (and `extra` more bytes that follow them on the device, copied to
// extra_out), host outputs, lengths.
rdf_status window_agg_finish(WinFront& wf, const WaggEmitArgs& ea, const int* fns, void* const* dvalid, const void* pnulls, size_t extra, void* extra_out, rdf_out* outs) {
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    const int64_t n = wf.n;
    const int32_t mem = wf.mem, ncalls = ea.ncalls;
    for (int c = 0; c < ncalls; ++c)
        if (ea.calls[c].vbytes) HIP_TRY(launch_win_pack(ea.calls[c].vbytes, n, (uint64_t*)dvalid[c], s));
    wf.kt->stop();
    const size_t pin_off = wf.pin_off;
    RDF_TRY(pinned_reserve(pin_off + RDF_WINDOW_MAX_CALLS * 8 + extra));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, pnulls, RDF_WINDOW_MAX_CALLS * 8 + extra, hipMemcpyDeviceToHost, s));
    if (mem == RDF_MEM_HOST)
        for (int c = 0; c < ncalls; ++c) {
            HIP_TRY(hipMemcpyAsync(outs[c].values, ea.calls[c].values, (size_t)n * (size_t)dtype_size(outs[c].dtype), hipMemcpyDeviceToHost, s));
            if (dvalid[c]) HIP_TRY(hipMemcpyAsync(outs[c].validity, dvalid[c], (size_t)((n + 7) / 8), hipMemcpyDeviceToHost, s));
        }
    HIP_TRY(hipStreamSynchronize(s));
    unsigned long long nulls[RDF_WINDOW_MAX_CALLS];
    memcpy(nulls, ctx.pinned + pin_off, sizeof nulls);
    if (extra) memcpy(extra_out, ctx.pinned + pin_off + sizeof nulls, extra);
    for (int c = 0; c < ncalls; ++c) {
        outs[c].length = n;
        outs[c].null_count = (int64_t)nulls[c];
        if (fns[c] == RDF_WAGG_COUNT && outs[c].validity) {   // a bitmap nobody needs was handed in: all valid
            if (mem == RDF_MEM_HOST) memset(outs[c].validity, 0xFF, (size_t)((n + 7) / 8));
            else HIP_TRY(hipMemsetAsync(outs[c].validity, 0xFF, (size_t)((n + 7) / 8), s));
        }
    }
    if (mem == RDF_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(s));
    return RDF_OK;
}

}  // namespace

rdf_status rdf_window_agg(const rdf_sort_key* partition_by, int32_t npartition, const rdf_sort_key* order_by, int32_t norder,
                          const rdf_array* const* values, int32_t nvalues, int64_t nchunks, int64_t nrows_if_no_keys,
                          const rdf_window_agg_call* calls, int32_t ncalls, rdf_out* outs) {
    // ---- everything that can be refused is refused before any device work
    RDF_TRY(window_front_counts("window_agg", calls, outs, ncalls, partition_by, npartition, order_by, norder));
    if (nvalues < 0 || nvalues > RDF_WINDOW_MAX_VALUES) return fail(RDF_INVALID_ARGUMENT, "window_agg: 0 .. %d value columns", RDF_WINDOW_MAX_VALUES);
    if (nvalues > 0 && !values) return fail(RDF_INVALID_ARGUMENT, "window_agg: null value list");
    if (nvalues > 0 && nchunks < 1) return fail(RDF_INVALID_ARGUMENT, "window_agg: bad arguments");
    int vdt[RDF_WINDOW_MAX_VALUES] = {};
    for (int v = 0; v < nvalues; ++v) {
        if (!values[v]) return fail(RDF_INVALID_ARGUMENT, "window_agg: value column %d is null", v);
        vdt[v] = values[v][0].dtype;
        for (int64_t c = 0; c < nchunks; ++c)
            if ((values[v][c].dtype != RDF_I64 && values[v][c].dtype != RDF_F64) || values[v][c].dtype != vdt[v])
                return fail(RDF_INVALID_ARGUMENT, "window_agg: value column %d: Int64 or Float64 chunks of one dtype", v);
    }
    for (int c = 0; c < ncalls; ++c) {
        const rdf_window_agg_call& w = calls[c];
        if (w.fn < RDF_WAGG_SUM || w.fn > RDF_WAGG_LAST_VALUE) return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: unknown function %d", c, w.fn);
        const bool reads = w.fn == RDF_WAGG_SUM || w.fn == RDF_WAGG_MIN || w.fn == RDF_WAGG_MAX || w.fn == RDF_WAGG_AVG;
        if (w.value >= nvalues || w.value < -1 || (w.value == -1 && reads))
            return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: value index %d out of range", c, w.value);
        RDF_TRY(window_agg_check_frame(c, w.frame));
        if (outs[c].dtype != window_agg_out_dtype(w.fn, w.value >= 0 ? vdt[w.value] : RDF_I64)) return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: wrong output dtype", c);
        if (w.fn != RDF_WAGG_COUNT && !outs[c].validity) return fail(RDF_INVALID_ARGUMENT, "window_agg: call %d: the result can be NULL and needs a validity bitmap", c);
    }
    WinFront wf;
    bool done = false;
    RDF_TRY(window_front_check("window_agg", partition_by, npartition, order_by, norder, values, nvalues, nchunks, nrows_if_no_keys, outs, ncalls, wf, &done));
    if (done) return RDF_OK;
    const int64_t n = wf.n;
    const int32_t mem = wf.mem;

    // ---- the order, then partition and peer-group structure: rdf_window's front
    RDF_TRY(window_front_device("window_agg", npartition, wf));
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    void* pnulls;
    RDF_TRY(arena_alloc(RDF_WINDOW_MAX_CALLS * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, RDF_WINDOW_MAX_CALLS * 8, s));

    // ---- the scans the calls need, each built once
    WaggScans S(wf, vdt);
    WaggEmitArgs ea;
    memset(&ea, 0, sizeof ea);
    ea.scan = wf.scan;
    ea.pstart = wf.pstart;
    ea.gstart = wf.gstart;
    ea.perm = wf.perm;
    ea.n = n;
    ea.ncalls = ncalls;
    ea.nulls = (unsigned long long*)pnulls;
    void* dvalid[RDF_WINDOW_MAX_CALLS] = {};
    int fns[RDF_WINDOW_MAX_CALLS] = {};
    for (int c = 0; c < ncalls; ++c) {
        const rdf_window_agg_call& w = calls[c];
        const rdf_window_frame& f = w.frame;
        WaggCallOut& o = ea.calls[c];
        fns[c] = o.fn = w.fn;
        o.f64 = w.value >= 0 && vdt[w.value] == RDF_F64;
        o.unit = f.unit;
        o.start_kind = f.start_kind;
        o.end_kind = f.end_kind;
        o.start = std::min(f.start, kWaggOffsetCap);
        o.end = std::min(f.end, kWaggOffsetCap);
        o.w = 1;
        const int64_t so = f.start_kind == RDF_BOUND_PRECEDING ? -o.start : f.start_kind == RDF_BOUND_FOLLOWING ? o.start : 0;
        const int64_t eo = f.end_kind == RDF_BOUND_PRECEDING ? -o.end : f.end_kind == RDF_BOUND_FOLLOWING ? o.end : 0;
        RDF_TRY(window_agg_wire_call(S, w.fn, w.value, f.unit, f.start_kind, f.end_kind, so, eo, o));
        RDF_TRY(window_agg_alloc_out(w.fn, outs[c], mem, n, o, &dvalid[c]));
    }
    HIP_TRY(launch_wagg_emit(ea, s));
    RDF_TRY(window_agg_finish(wf, ea, fns, dvalid, pnulls, 0, nullptr, outs));
    ctx.last_kernel = wf.sort_kernels + "win_flags_kernel + win_starts_kernel + " + std::to_string(S.scans.size()) + " x wagg_scan + wagg_emit_kernel";
    return RDF_OK;
}
