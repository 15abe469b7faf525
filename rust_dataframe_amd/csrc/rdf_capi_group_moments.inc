// rdf_capi_group_moments.inc — host side of rdf_groupby_moments: variance, stddev, skewness, kurtosis, covar and corr per
// group (kernels: rdf_group_moments.hip, argument blocks: rdf_group_moments.h); textually included by rdf_capi.cpp after
// rdf_capi_window.inc, whose device front (staging, sort_core, flag pass, scan, start tables) it runs unchanged with the
// grouping columns as partition keys, NO order keys, and x (and y) as passenger columns: the sort is over the keys alone.
//
// After the front: the group count comes back in one 8-byte copy (the outputs are sized by it), level 0 folds the sorted
// rows into piece states, the levels above merge them, the finish kernel reads the statistics off the states, the
// validity bytes are packed, and host outputs are copied back.

rdf_status rdf_groupby_moments(const rdf_sort_key* group_by, int32_t ngroup, const rdf_array* x, const rdf_array* y,
                               int64_t nchunks, const rdf_group_stat_call* calls, int32_t ncalls, rdf_out* out_group_rows,
                               rdf_out* outs, rdf_out* out_counts, void* out_states, int64_t states_capacity,
                               int64_t* out_groups) {
    // ---- everything that can be refused is refused before any device work
    const char* fn = "groupby_moments";
    if (!out_groups) return fail(RDF_INVALID_ARGUMENT, "%s: null out_groups", fn);
    if (ngroup < 0 || ngroup > RDF_MAX_GROUP_KEYS) return fail(RDF_INVALID_ARGUMENT, "%s: 0 .. %d grouping keys", fn, RDF_MAX_GROUP_KEYS);
    if (ngroup > 0 && !group_by) return fail(RDF_INVALID_ARGUMENT, "%s: null key list", fn);
    if (ncalls < 0 || ncalls > RDF_GROUP_MOMENTS_MAX_CALLS) return fail(RDF_INVALID_ARGUMENT, "%s: at most %d calls", fn, RDF_GROUP_MOMENTS_MAX_CALLS);
    if (ncalls > 0 && (!calls || !outs)) return fail(RDF_INVALID_ARGUMENT, "%s: null call list", fn);
    const bool asked = ncalls > 0 || out_counts || out_states;
    if (asked != (x != nullptr) || (y && !x))
        return fail(RDF_INVALID_ARGUMENT, "%s: x is given exactly when there are calls, counts or states (and y only with x)", fn);
    for (int c = 0; c < ncalls; ++c)
        if (calls[c].stat < 0 || calls[c].stat > (y ? (int)RDF_COSTAT_CORR : (int)RDF_STAT_KURTOSIS))
            return fail(RDF_INVALID_ARGUMENT, "%s: call %d: unknown statistic %d of %s", fn, c, calls[c].stat, y ? "a pair" : "one column");
    const int nextra = (x ? 1 : 0) + (y ? 1 : 0), ncols = ngroup + nextra;
    if (ncols > 0 && nchunks < 1) return fail(RDF_INVALID_ARGUMENT, "%s: bad arguments", fn);
    WinFront wf;
    wf.nkeys = ngroup;
    wf.nextra = nextra;
    wf.keys.resize((size_t)ncols);
    for (int k = 0; k < ngroup; ++k) {
        wf.keys[k] = group_by[k];
        wf.keys[k].options = rdf_sort_options{0, 0};
    }
    if (x) wf.keys[(size_t)ngroup] = rdf_sort_key{x, nullptr, rdf_sort_options{0, 0}};
    if (y) wf.keys[(size_t)ngroup + 1] = rdf_sort_key{y, nullptr, rdf_sort_options{0, 0}};
    bool any_utf8 = false;
    RDF_TRY(lexsort_check_keys(wf.keys.data(), ngroup, nchunks, fn, &wf.mem, &any_utf8));
    for (const rdf_array* v : {x, y})
        for (int64_t c = 0; v && c < nchunks; ++c)
            if (!is_numeric(v[c].dtype) || v[c].dtype != v[0].dtype)
                return fail(RDF_INVALID_ARGUMENT, "%s: %s: numeric chunks of one dtype", fn, v == x ? "x" : "y");
    for (int c = 0; c < ncalls; ++c) {
        if (outs[c].dtype != RDF_F64) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: wrong output dtype", fn, c);
    }
    for (int c = 0; c < ncalls; ++c)
        if (!outs[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: every statistic needs a validity bitmap", fn, c);
    if (out_counts && out_counts->dtype != RDF_I64) return fail(RDF_INVALID_ARGUMENT, "%s: counts are Int64", fn);
    if (out_group_rows && out_group_rows->dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "%s: group rows are UInt32", fn);
    if (out_states && states_capacity < 0) return fail(RDF_INVALID_ARGUMENT, "%s: negative states_capacity", fn);
    if (x) RDF_TRY(check_mem(x, nchunks, &wf.mem));
    if (y) RDF_TRY(check_mem(y, nchunks, &wf.mem));
    if (ncols == 0) {   // no keys and no value: no rows
        *out_groups = 0;
        if (out_group_rows) { out_group_rows->length = 0; out_group_rows->null_count = 0; }
        return RDF_OK;
    }
    const int32_t mem = wf.mem;
    if (out_group_rows) RDF_TRY(check_out_mem(out_group_rows, 1, mem));
    if (out_counts) RDF_TRY(check_out_mem(out_counts, 1, mem));
    RDF_TRY(check_out_mem(outs, ncalls, mem));
    wf.nch = nchunks;
    RDF_TRY(lexsort_row_starts(wf.keys.data(), ncols, nchunks, fn, wf.row_start));
    const int64_t n = wf.n = wf.row_start[(size_t)nchunks];
    for (int c = 0; c < ncalls; ++c)
        if (n > 0 && outs[c].capacity > 0 && !outs[c].values) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: null output buffer", fn, c);
    if (out_group_rows && n > 0 && out_group_rows->capacity > 0 && !out_group_rows->values) return fail(RDF_INVALID_ARGUMENT, "%s: null group rows buffer", fn);
    if (out_counts && n > 0 && out_counts->capacity > 0 && !out_counts->values) return fail(RDF_INVALID_ARGUMENT, "%s: null counts buffer", fn);
    auto set_lengths = [&](int64_t g) {
        *out_groups = g;
        if (out_group_rows) { out_group_rows->length = g; out_group_rows->null_count = 0; }
        if (out_counts) { out_counts->length = g; out_counts->null_count = 0; }
        for (int c = 0; c < ncalls; ++c) { outs[c].length = g; outs[c].null_count = 0; }
    };
    if (n == 0) { set_lengths(0); return RDF_OK; }

    // ---- the order and the group structure: rdf_window's front over the keys alone
    RDF_TRY(window_front_device(fn, ngroup, wf));
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    const size_t pin_off = wf.pin_off;
    RDF_TRY(pinned_reserve(pin_off + 64 + RDF_GROUP_MOMENTS_MAX_CALLS * 8));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, wf.scan + n, 8, hipMemcpyDeviceToHost, s));   // the scan's total: groups in the high word
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t total = 0;
    memcpy(&total, ctx.pinned + pin_off, 8);
    const int64_t G = (int64_t)(total >> 32);
    if (G < 1 || G > n) {
        wf.kt->stop();
        return fail(RDF_COMPUTE_ERROR, "internal: %s: %lld groups over %lld rows", fn, (long long)G, (long long)n);
    }
    set_lengths(G);
    bool fits = (!out_group_rows || out_group_rows->capacity >= G) && (!out_counts || out_counts->capacity >= G) && (!out_states || states_capacity >= G);
    for (int c = 0; c < ncalls; ++c) fits &= outs[c].capacity >= G;
    if (!fits) {
        wf.kt->stop();
        return fail(RDF_MEMORY_ERROR, "output capacity too small (the group count is in *out_groups and every length)");
    }
    const std::string front_kernels = wf.sort_kernels + "win_flags_kernel + win_starts_kernel";
    if (!out_group_rows && !asked) {   // the count-only call
        wf.kt->stop();
        ctx.last_kernel = front_kernels;
        return RDF_OK;
    }

    // ---- one state per group: level 0 over the sorted rows, then the levels of partials
    const bool pair = y != nullptr;
    const size_t state_size = pair ? sizeof(rdf_comoments_state) : sizeof(rdf_moments_state);
    const size_t item_size = pair ? sizeof(GmItem2) : sizeof(GmItem1);
    void* d_states = nullptr;
    int levels = 0;
    if (x) {
        d_states = out_states;
        if (!out_states || mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)G * state_size, &d_states));
        GmFoldArgs fa;
        memset(&fa, 0, sizeof fa);
        fa.scan = wf.scan;
        fa.perm = wf.perm;
        fa.x = wf.d.tb.dev_at<DevChunkCol>(wf.d.o_ch) + (size_t)ngroup * nchunks;
        if (pair) fa.y = fa.x + nchunks;
        fa.row_start = wf.d_row_start;
        fa.nchunks = nchunks;
        fa.dt_x = x[0].dtype;
        fa.dt_y = pair ? y[0].dtype : x[0].dtype;
        fa.states = d_states;
        fa.groups = G;
        int64_t m = n;
        for (;; ++levels) {
            fa.m = m;
            fa.part = nullptr;
            const int64_t next = 2 * gm_tiles(m);
            if (m > kGmTile) RDF_TRY(arena_alloc((size_t)next * item_size, &fa.part));
            HIP_TRY(levels == 0 ? launch_gm_level0(fa, s) : launch_gm_fold(fa, pair, s));
            if (!fa.part) break;
            fa.in = fa.part;
            m = next;
        }
    }

    // ---- the statistics, the counts and the first rows: one thread per (group, call)
    void* pnulls;
    RDF_TRY(arena_alloc(RDF_GROUP_MOMENTS_MAX_CALLS * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, RDF_GROUP_MOMENTS_MAX_CALLS * 8, s));
    GmFinishArgs ga;
    memset(&ga, 0, sizeof ga);
    ga.states = d_states;
    ga.pair = pair ? 1 : 0;
    ga.ncalls = ncalls;
    ga.groups = G;
    ga.pstart = wf.pstart;
    ga.perm = wf.perm;
    ga.nulls = (unsigned long long*)pnulls;
    void *d_rows = nullptr, *d_counts = nullptr;
    if (out_group_rows) {
        d_rows = out_group_rows->values;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)G * 4, &d_rows));
        ga.group_rows = (uint32_t*)d_rows;
    }
    if (out_counts) {
        d_counts = out_counts->values;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)G * 8, &d_counts));
        ga.counts = (int64_t*)d_counts;
    }
    void* dwords[RDF_GROUP_MOMENTS_MAX_CALLS] = {};
    const size_t vbytes_len = (size_t)((G + 7) / 8);
    for (int c = 0; c < ncalls; ++c) {
        GmCallOut& o = ga.calls[c];
        o.stat = calls[c].stat;
        void* pv = outs[c].values;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)G * 8, &pv));
        o.values = (double*)pv;
        RDF_TRY(arena_alloc((size_t)G, &pv));
        o.vbytes = (uint8_t*)pv;
        RDF_TRY(arena_alloc((size_t)((G + 63) / 64) * 8, &dwords[c]));   // whole words here, the caller's bitmap gets its bytes
    }
    HIP_TRY(launch_gm_finish(ga, s));
    for (int c = 0; c < ncalls; ++c) HIP_TRY(launch_win_pack(ga.calls[c].vbytes, G, (uint64_t*)dwords[c], s));
    wf.kt->stop();

    // ---- results to the caller
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + 64, pnulls, RDF_GROUP_MOMENTS_MAX_CALLS * 8, hipMemcpyDeviceToHost, s));
    const hipMemcpyKind kind = mem == RDF_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (mem == RDF_MEM_HOST) {
        if (out_group_rows) HIP_TRY(hipMemcpyAsync(out_group_rows->values, d_rows, (size_t)G * 4, kind, s));
        if (out_counts) HIP_TRY(hipMemcpyAsync(out_counts->values, d_counts, (size_t)G * 8, kind, s));
        if (out_states) HIP_TRY(hipMemcpyAsync(out_states, d_states, (size_t)G * state_size, kind, s));
        for (int c = 0; c < ncalls; ++c) HIP_TRY(hipMemcpyAsync(outs[c].values, ga.calls[c].values, (size_t)G * 8, kind, s));
    }
    for (int c = 0; c < ncalls; ++c) HIP_TRY(hipMemcpyAsync(outs[c].validity, dwords[c], vbytes_len, kind, s));
    HIP_TRY(hipStreamSynchronize(s));
    unsigned long long nulls[RDF_GROUP_MOMENTS_MAX_CALLS];
    memcpy(nulls, ctx.pinned + pin_off + 64, sizeof nulls);
    for (int c = 0; c < ncalls; ++c) outs[c].null_count = (int64_t)nulls[c];
    for (rdf_out* o : {out_group_rows, out_counts})
        if (o && o->validity) {   // a bitmap nobody needs was handed in: all valid
            if (mem == RDF_MEM_HOST) memset(o->validity, 0xFF, vbytes_len);
            else HIP_TRY(hipMemsetAsync(o->validity, 0xFF, vbytes_len, s));
        }
    if (mem == RDF_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(s));
    ctx.last_kernel = front_kernels + (x ? std::string(" + gm_level0_kernel") + (levels ? " + " + std::to_string(levels) + " x gm_fold_kernel" : std::string()) : std::string()) +
                      " + gm_finish_kernel";
    return RDF_OK;
}
