// rdf_capi_window.inc — host side of rdf_window: the SQL window functions over partitions (kernels: rdf_window.hip,
// argument blocks: rdf_window.h); textually included by rdf_capi.cpp (it uses that file's context, arena and staging
// helpers, sort_core, launch_scan, and lexsort_keys_to_device of rdf_capi_sort_utf8.inc).
//
// One stable sort over (partition keys, order keys) — float keys canonical, so that -0.0 / +0.0 and the NaNs are
// neighbours in row order — then four passes over the permutation: neighbour flags, one scan, the start tables, and one
// emit launch that answers every call of the request.

namespace {

int window_out_dtype(int fn) {
    switch (fn) {
        case RDF_WIN_PERCENT_RANK: case RDF_WIN_CUME_DIST: return RDF_F64;
        case RDF_WIN_LAG: case RDF_WIN_LEAD: return RDF_U32;
        default: return RDF_I64;
    }
}

// ---- the shared front of rdf_window and rdf_window_agg: everything about keys, rows and outputs that can be refused, then
// the sort, the flag pass, the scan and the start tables.  `extra` are nextra more numeric columns (rdf_window_agg's values)
// that are checked and staged like keys but take no part in the order.
struct WinFront {
    int nkeys = 0, nextra = 0;
    int32_t mem = -1;
    int64_t nch = 1, n = 0;
    std::vector<rdf_sort_key> keys;     // partition keys, order keys, then the extra columns
    std::vector<int64_t> row_start;
    size_t pin_off = 0;
    LexKeysOnDevice d;
    const uint32_t* perm = nullptr;     // nullptr: no keys, the rows are in order
    const int64_t* d_row_start = nullptr;
    const int64_t* scan = nullptr;
    const uint32_t* pstart = nullptr;
    const uint32_t* gstart = nullptr;
    std::string sort_kernels;
    std::unique_ptr<KernelTimer> kt;    // started before the flag pass; the caller stops it after its last kernel
};

rdf_status window_front_counts(const char* fn, const void* calls, const rdf_out* outs, int32_t ncalls, const rdf_sort_key* partition_by,
                               int32_t npartition, const rdf_sort_key* order_by, int32_t norder) {
    if (!calls || !outs || ncalls < 1) return fail(RDF_INVALID_ARGUMENT, "%s: no calls", fn);
    if (ncalls > RDF_WINDOW_MAX_CALLS) return fail(RDF_INVALID_ARGUMENT, "%s: at most %d calls", fn, RDF_WINDOW_MAX_CALLS);
    if (npartition < 0 || npartition > RDF_WINDOW_MAX_KEYS || norder < 0 || norder > RDF_WINDOW_MAX_KEYS)
        return fail(RDF_INVALID_ARGUMENT, "%s: 0 .. %d partition keys and 0 .. %d order keys", fn, RDF_WINDOW_MAX_KEYS, RDF_WINDOW_MAX_KEYS);
    if ((npartition > 0 && !partition_by) || (norder > 0 && !order_by)) return fail(RDF_INVALID_ARGUMENT, "%s: null key list", fn);
    return RDF_OK;
}

// *done: the call is answered (zero rows); the status is the call's.
rdf_status window_front_check(const char* fn, const rdf_sort_key* partition_by, int32_t npartition, const rdf_sort_key* order_by, int32_t norder,
                              const rdf_array* const* extra, int32_t nextra, int64_t nchunks, int64_t nrows_if_no_keys, rdf_out* outs,
                              int32_t ncalls, WinFront& w, bool* done) {
    *done = false;
    const int nkeys = npartition + norder, ncols = nkeys + nextra;
    w.nkeys = nkeys;
    w.nextra = nextra;
    w.keys.resize((size_t)ncols);
    for (int k = 0; k < ncols; ++k) {
        if (k >= nkeys) { w.keys[k] = rdf_sort_key{extra[k - nkeys], nullptr, rdf_sort_options{0, 0}}; continue; }
        w.keys[k] = k < npartition ? partition_by[k] : order_by[k - npartition];
        if (k < npartition) w.keys[k].options = rdf_sort_options{0, 0};
    }
    if (ncols > 0 && nchunks < 1) return fail(RDF_INVALID_ARGUMENT, "%s: bad arguments", fn);
    bool any_utf8 = false;
    RDF_TRY(lexsort_check_keys(w.keys.data(), ncols, nchunks, fn, &w.mem, &any_utf8));   // the sort's own rules: the same dtypes are refused
    if (w.mem < 0) {   // no keys: the outputs say where the call lives
        w.mem = outs[0].mem;
        if (w.mem != RDF_MEM_HOST && w.mem != RDF_MEM_DEVICE) return fail(RDF_INVALID_ARGUMENT, "bad mem tag %d", w.mem);
    }
    RDF_TRY(check_out_mem(outs, ncalls, w.mem));
    w.nch = ncols > 0 ? nchunks : 1;
    if (ncols > 0) {
        RDF_TRY(lexsort_row_starts(w.keys.data(), ncols, w.nch, fn, w.row_start));
        if (nrows_if_no_keys != 0 && nrows_if_no_keys != w.row_start[(size_t)w.nch]) return fail(RDF_INVALID_ARGUMENT, "%s: nrows_if_no_keys contradicts the keys' rows", fn);
    } else {
        if (nrows_if_no_keys < 0) return fail(RDF_INVALID_ARGUMENT, "%s: negative row count", fn);
        if (nrows_if_no_keys >= (int64_t)1 << 32) return fail(RDF_INVALID_ARGUMENT, "%s: UInt32 row indices cap a call at 2^32-1 rows", fn);
        w.row_start.assign(2, 0);
        w.row_start[1] = nrows_if_no_keys;
    }
    const int64_t n = w.n = w.row_start[(size_t)w.nch];
    for (int c = 0; c < ncalls; ++c)
        if (n > 0 && outs[c].capacity > 0 && !outs[c].values) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: null output buffer", fn, c);
    bool fits = true;
    for (int c = 0; c < ncalls; ++c) fits &= outs[c].capacity >= n;
    if (!fits) {
        for (int c = 0; c < ncalls; ++c) { outs[c].length = n; outs[c].null_count = 0; }
        return fail(RDF_MEMORY_ERROR, "output capacity too small");
    }
    if (n == 0) {
        for (int c = 0; c < ncalls; ++c) { outs[c].length = 0; outs[c].null_count = 0; }
        *done = true;
    }
    return RDF_OK;
}

// The device half: inputs staged, sort_core over (partition keys, order keys) with float keys canonical, then the partition
// and peer-group structure.  Begins the arena.
rdf_status window_front_device(const char* fn, int npartition, WinFront& w) {
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    arena_begin();
    const int nkeys = w.nkeys, ncols = nkeys + w.nextra;
    const int64_t n = w.n, nch = w.nch;
    LexKeysOnDevice& d = w.d;
    if (ncols > 0) {
        RDF_TRY(lexsort_keys_to_device(w.keys.data(), ncols, nch, w.mem, w.row_start, fn, w.pin_off, d));
        w.d_row_start = d.tb.dev_at<int64_t>(d.o_rs);
    }
    if (nkeys > 0) {
        std::vector<rdf_sort_options> opts((size_t)nkeys);
        for (int k = 0; k < nkeys; ++k) opts[k] = w.keys[k].options;
        RDF_TRY(sort_core(d.tb.dev_at<DevChunkCol>(d.o_ch), w.d_row_start, nch, n, nkeys, d.dts, d.nullable, opts.data(), w.pin_off, &w.perm, d.ucols, true));
        w.sort_kernels = ctx.last_kernel + " + ";
    }
    void *pflags, *pscan, *ppstart, *pgstart;
    RDF_TRY(arena_alloc((size_t)n * 8, &pflags));
    RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &pscan));
    RDF_TRY(arena_alloc((size_t)(n + 1) * 4, &ppstart));
    RDF_TRY(arena_alloc((size_t)(n + 1) * 4, &pgstart));
    WinFlagArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.nkeys = nkeys;
    for (int k = 0; k < nkeys; ++k) {
        fa.keys[k].chunks = w.keys[k].values ? d.tb.dev_at<DevChunkCol>(d.o_ch) + (size_t)k * nch : nullptr;
        fa.keys[k].utf8 = w.keys[k].utf8 ? d.ucols[k].d_chunks : nullptr;
        fa.keys[k].dtype = d.dts[k];
        fa.keys[k].order = k >= npartition ? 1 : 0;
    }
    fa.row_start = nkeys > 0 ? w.d_row_start : nullptr;   // (no keys: nothing is gathered, whatever the extra columns' chunks)
    fa.nchunks = nkeys > 0 ? nch : 1;
    fa.n = n;
    fa.perm = w.perm;
    fa.flags = (int64_t*)pflags;
    w.kt.reset(new KernelTimer());
    HIP_TRY(launch_win_flags(fa, s));
    HIP_TRY(launch_scan((const int64_t*)pflags, (int64_t*)pscan, n, (int64_t*)pscan + n + 1, s));
    WinStartArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.scan = (const int64_t*)pscan;
    sa.n = n;
    sa.pstart = (uint32_t*)ppstart;
    sa.gstart = (uint32_t*)pgstart;
    HIP_TRY(launch_win_starts(sa, s));
    w.scan = sa.scan;
    w.pstart = sa.pstart;
    w.gstart = sa.gstart;
    return RDF_OK;
}

}  // namespace

rdf_status rdf_window(const rdf_sort_key* partition_by, int32_t npartition, const rdf_sort_key* order_by, int32_t norder,
                      int64_t nchunks, int64_t nrows_if_no_keys, const rdf_window_call* calls, int32_t ncalls, rdf_out* outs) {
    // ---- everything that can be refused is refused before any device work
    RDF_TRY(window_front_counts("window", calls, outs, ncalls, partition_by, npartition, order_by, norder));
    for (int c = 0; c < ncalls; ++c) {
        const rdf_window_call& w = calls[c];
        if (w.fn < RDF_WIN_ROW_NUMBER || w.fn > RDF_WIN_LEAD) return fail(RDF_INVALID_ARGUMENT, "window: call %d: unknown function %d", c, w.fn);
        if (w.fn == RDF_WIN_NTILE && w.param < 1) return fail(RDF_INVALID_ARGUMENT, "window: call %d: ntile needs at least 1 bucket", c);
        if (w.fn >= RDF_WIN_LAG && w.param < 0) return fail(RDF_INVALID_ARGUMENT, "window: call %d: a lag / lead offset cannot be negative", c);
        if (outs[c].dtype != window_out_dtype(w.fn)) return fail(RDF_INVALID_ARGUMENT, "window: call %d: wrong output dtype", c);
        if (w.fn >= RDF_WIN_LAG && w.param > 0 && !outs[c].validity) return fail(RDF_INVALID_ARGUMENT, "window: call %d: lag / lead with an offset need a validity bitmap", c);
    }
    WinFront wf;
    bool done = false;
    RDF_TRY(window_front_check("window", partition_by, npartition, order_by, norder, nullptr, 0, nchunks, nrows_if_no_keys, outs, ncalls, wf, &done));
    if (done) return RDF_OK;
    const int64_t n = wf.n;
    const int32_t mem = wf.mem;

    // ---- the order, then partition and peer-group structure
    RDF_TRY(window_front_device("window", npartition, wf));
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    const size_t pin_off = wf.pin_off;
    const uint32_t* perm = wf.perm;
    void* pnulls;
    RDF_TRY(arena_alloc(RDF_WINDOW_MAX_CALLS * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, RDF_WINDOW_MAX_CALLS * 8, s));

    // ---- every call's answer from one launch; host outputs are written on the device and copied back
    WinEmitArgs ea;
    memset(&ea, 0, sizeof ea);
    ea.scan = wf.scan;
    ea.pstart = wf.pstart;
    ea.gstart = wf.gstart;
    ea.perm = perm;
    ea.n = n;
    ea.ncalls = ncalls;
    ea.nulls = (unsigned long long*)pnulls;
    void* dvalid[RDF_WINDOW_MAX_CALLS] = {};
    for (int c = 0; c < ncalls; ++c) {
        WinCallOut& o = ea.calls[c];
        o.fn = calls[c].fn;
        o.param = (uint64_t)calls[c].param;
        o.values = outs[c].values;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)n * (size_t)dtype_size(outs[c].dtype), &o.values));
        if (calls[c].fn >= RDF_WIN_LAG && outs[c].validity) {
            void* pv;
            RDF_TRY(arena_alloc((size_t)n, &pv));
            o.vbytes = (uint8_t*)pv;
            dvalid[c] = outs[c].validity;
            if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)((n + 63) / 64) * 8, &dvalid[c]));
        }
    }
    HIP_TRY(launch_win_emit(ea, s));
    for (int c = 0; c < ncalls; ++c)
        if (ea.calls[c].vbytes) HIP_TRY(launch_win_pack(ea.calls[c].vbytes, n, (uint64_t*)dvalid[c], s));
    wf.kt->stop();
    RDF_TRY(pinned_reserve(pin_off + 64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, pnulls, RDF_WINDOW_MAX_CALLS * 8, hipMemcpyDeviceToHost, s));
    if (mem == RDF_MEM_HOST)
        for (int c = 0; c < ncalls; ++c) {
            HIP_TRY(hipMemcpyAsync(outs[c].values, ea.calls[c].values, (size_t)n * (size_t)dtype_size(outs[c].dtype), hipMemcpyDeviceToHost, s));
            if (dvalid[c]) HIP_TRY(hipMemcpyAsync(outs[c].validity, dvalid[c], (size_t)((n + 7) / 8), hipMemcpyDeviceToHost, s));
        }
    HIP_TRY(hipStreamSynchronize(s));
    unsigned long long nulls[RDF_WINDOW_MAX_CALLS];
    memcpy(nulls, ctx.pinned + pin_off, sizeof nulls);
    for (int c = 0; c < ncalls; ++c) {
        outs[c].length = n;
        outs[c].null_count = calls[c].fn >= RDF_WIN_LAG ? (int64_t)nulls[c] : 0;
        if (calls[c].fn < RDF_WIN_LAG && outs[c].validity) {   // a bitmap nobody needs was handed in: all valid
            if (mem == RDF_MEM_HOST) memset(outs[c].validity, 0xFF, (size_t)((n + 7) / 8));
            else HIP_TRY(hipMemsetAsync(outs[c].validity, 0xFF, (size_t)((n + 7) / 8), s));
        }
    }
    if (mem == RDF_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(s));
    ctx.last_kernel = wf.sort_kernels + "win_flags_kernel + win_starts_kernel + win_emit_kernel";
    return RDF_OK;
}
