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

}  // namespace

rdf_status rdf_window(const rdf_sort_key* partition_by, int32_t npartition, const rdf_sort_key* order_by, int32_t norder,
                      int64_t nchunks, int64_t nrows_if_no_keys, const rdf_window_call* calls, int32_t ncalls, rdf_out* outs) {
    // ---- everything that can be refused is refused before any device work
    if (!calls || !outs || ncalls < 1) return fail(RDF_INVALID_ARGUMENT, "window: no calls");
    if (ncalls > RDF_WINDOW_MAX_CALLS) return fail(RDF_INVALID_ARGUMENT, "window: at most %d calls", RDF_WINDOW_MAX_CALLS);
    if (npartition < 0 || npartition > RDF_WINDOW_MAX_KEYS || norder < 0 || norder > RDF_WINDOW_MAX_KEYS)
        return fail(RDF_INVALID_ARGUMENT, "window: 0 .. %d partition keys and 0 .. %d order keys", RDF_WINDOW_MAX_KEYS, RDF_WINDOW_MAX_KEYS);
    if ((npartition > 0 && !partition_by) || (norder > 0 && !order_by)) return fail(RDF_INVALID_ARGUMENT, "window: null key list");
    for (int c = 0; c < ncalls; ++c) {
        const rdf_window_call& w = calls[c];
        if (w.fn < RDF_WIN_ROW_NUMBER || w.fn > RDF_WIN_LEAD) return fail(RDF_INVALID_ARGUMENT, "window: call %d: unknown function %d", c, w.fn);
        if (w.fn == RDF_WIN_NTILE && w.param < 1) return fail(RDF_INVALID_ARGUMENT, "window: call %d: ntile needs at least 1 bucket", c);
        if (w.fn >= RDF_WIN_LAG && w.param < 0) return fail(RDF_INVALID_ARGUMENT, "window: call %d: a lag / lead offset cannot be negative", c);
        if (outs[c].dtype != window_out_dtype(w.fn)) return fail(RDF_INVALID_ARGUMENT, "window: call %d: wrong output dtype", c);
        if (w.fn >= RDF_WIN_LAG && w.param > 0 && !outs[c].validity) return fail(RDF_INVALID_ARGUMENT, "window: call %d: lag / lead with an offset need a validity bitmap", c);
    }
    const int nkeys = npartition + norder;
    std::vector<rdf_sort_key> keys((size_t)nkeys);
    for (int k = 0; k < nkeys; ++k) {
        keys[k] = k < npartition ? partition_by[k] : order_by[k - npartition];
        if (k < npartition) keys[k].options = rdf_sort_options{0, 0};
    }
    if (nkeys > 0 && nchunks < 1) return fail(RDF_INVALID_ARGUMENT, "window: bad arguments");
    int32_t mem = -1;
    bool any_utf8 = false;
    RDF_TRY(lexsort_check_keys(keys.data(), nkeys, nchunks, "window", &mem, &any_utf8));   // the sort's own rules: the same dtypes are refused
    if (mem < 0) {   // no keys: the outputs say where the call lives
        mem = outs[0].mem;
        if (mem != RDF_MEM_HOST && mem != RDF_MEM_DEVICE) return fail(RDF_INVALID_ARGUMENT, "bad mem tag %d", mem);
    }
    RDF_TRY(check_out_mem(outs, ncalls, mem));
    const int64_t nch = nkeys > 0 ? nchunks : 1;
    std::vector<int64_t> row_start;
    if (nkeys > 0) {
        RDF_TRY(lexsort_row_starts(keys.data(), nkeys, nch, "window", row_start));
        if (nrows_if_no_keys != 0 && nrows_if_no_keys != row_start[(size_t)nch]) return fail(RDF_INVALID_ARGUMENT, "window: nrows_if_no_keys contradicts the keys' rows");
    } else {
        if (nrows_if_no_keys < 0) return fail(RDF_INVALID_ARGUMENT, "window: negative row count");
        if (nrows_if_no_keys >= (int64_t)1 << 32) return fail(RDF_INVALID_ARGUMENT, "window: UInt32 row indices cap a call at 2^32-1 rows");
        row_start.assign(2, 0);
        row_start[1] = nrows_if_no_keys;
    }
    const int64_t n = row_start[(size_t)nch];
    for (int c = 0; c < ncalls; ++c)
        if (n > 0 && outs[c].capacity > 0 && !outs[c].values) return fail(RDF_INVALID_ARGUMENT, "window: call %d: null output buffer", c);
    bool fits = true;
    for (int c = 0; c < ncalls; ++c) fits &= outs[c].capacity >= n;
    if (!fits) {
        for (int c = 0; c < ncalls; ++c) { outs[c].length = n; outs[c].null_count = 0; }
        return fail(RDF_MEMORY_ERROR, "output capacity too small");
    }
    if (n == 0) {
        for (int c = 0; c < ncalls; ++c) { outs[c].length = 0; outs[c].null_count = 0; }
        return RDF_OK;
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    arena_begin();

    // ---- the order: sort_core over (partition keys, order keys), float keys canonical
    size_t pin_off = 0;
    LexKeysOnDevice d;
    const uint32_t* perm = nullptr;
    const int64_t* d_row_start = nullptr;
    if (nkeys > 0) {
        RDF_TRY(lexsort_keys_to_device(keys.data(), nkeys, nch, mem, row_start, "window", pin_off, d));
        std::vector<rdf_sort_options> opts((size_t)nkeys);
        for (int k = 0; k < nkeys; ++k) opts[k] = keys[k].options;
        d_row_start = d.tb.dev_at<int64_t>(d.o_rs);
        RDF_TRY(sort_core(d.tb.dev_at<DevChunkCol>(d.o_ch), d_row_start, nch, n, nkeys, d.dts, d.nullable, opts.data(), pin_off, &perm, d.ucols, true));
    }
    const std::string sort_kernels = nkeys > 0 ? ctx.last_kernel + " + " : std::string();

    // ---- partition and peer-group structure
    void *pflags, *pscan, *ppstart, *pgstart, *pnulls;
    RDF_TRY(arena_alloc((size_t)n * 8, &pflags));
    RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &pscan));
    RDF_TRY(arena_alloc((size_t)(n + 1) * 4, &ppstart));
    RDF_TRY(arena_alloc((size_t)(n + 1) * 4, &pgstart));
    RDF_TRY(arena_alloc(RDF_WINDOW_MAX_CALLS * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, RDF_WINDOW_MAX_CALLS * 8, s));
    KernelTimer kt;
    WinFlagArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.nkeys = nkeys;
    for (int k = 0; k < nkeys; ++k) {
        fa.keys[k].chunks = keys[k].values ? d.tb.dev_at<DevChunkCol>(d.o_ch) + (size_t)k * nch : nullptr;
        fa.keys[k].utf8 = keys[k].utf8 ? d.ucols[k].d_chunks : nullptr;
        fa.keys[k].dtype = d.dts[k];
        fa.keys[k].order = k >= npartition ? 1 : 0;
    }
    fa.row_start = d_row_start;
    fa.nchunks = nch;
    fa.n = n;
    fa.perm = perm;
    fa.flags = (int64_t*)pflags;
    HIP_TRY(launch_win_flags(fa, s));
    HIP_TRY(launch_scan((const int64_t*)pflags, (int64_t*)pscan, n, (int64_t*)pscan + n + 1, s));
    WinStartArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.scan = (const int64_t*)pscan;
    sa.n = n;
    sa.pstart = (uint32_t*)ppstart;
    sa.gstart = (uint32_t*)pgstart;
    HIP_TRY(launch_win_starts(sa, s));

    // ---- every call's answer from one launch; host outputs are written on the device and copied back
    WinEmitArgs ea;
    memset(&ea, 0, sizeof ea);
    ea.scan = sa.scan;
    ea.pstart = sa.pstart;
    ea.gstart = sa.gstart;
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
    kt.stop();
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
    ctx.last_kernel = sort_kernels + "win_flags_kernel + win_starts_kernel + win_emit_kernel";
    return RDF_OK;
}
