// rdf_capi_percentile.inc — host side of rdf_groupby_percentile: percentiles (continuous and discrete) and the median per
// group (kernel: rdf_percentile.hip, the decisions about one group and one call: rdf_percentile.h); textually included by
// rdf_capi.cpp after rdf_capi_group_sorted.inc.  It runs rdf_window's device front unchanged, with the grouping columns as
// partition keys and the value column as the one order key, exactly as rdf_groupby_sorted does.  A whole numeric column
// (no grouping columns) can take the select route instead (percentile_select below): no sort, a radix select whose every
// launch is queued at once.
//
// After the front: the group and pair counts come back in one 8-byte copy (the outputs are sized by them), one launch answers
// every (group, call), the first row of every group is rdf_groupby_sorted's fold over the heads with no calls, the validity
// bytes are packed, and host outputs are copied back.

static_assert(PCT_CONT == RDF_PCT_CONT && PCT_DISC == RDF_PCT_DISC, "rdf_percentile.h restates rdf_percentile_kind");
static_assert(PCT_I8 == RDF_I8 && PCT_I16 == RDF_I16 && PCT_I32 == RDF_I32 && PCT_I64 == RDF_I64 && PCT_U8 == RDF_U8 && PCT_U16 == RDF_U16 &&
              PCT_U32 == RDF_U32 && PCT_U64 == RDF_U64 && PCT_F32 == RDF_F32 && PCT_F64 == RDF_F64, "rdf_percentile.h restates rdf_dtype");

namespace {

// The select route: ngroup == 0, a numeric value column, n > 0 rows, everything already checked.  One group.
rdf_status percentile_select(const char* fn, const rdf_sort_key* value, int64_t nchunks, const std::vector<int64_t>& row_start, int32_t mem,
                             const rdf_percentile_call* calls, int32_t ncalls, rdf_out* out_group_rows, rdf_out* outs, rdf_out* out_counts) {
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    arena_begin();
    const int64_t n = row_start[(size_t)nchunks];
    size_t pin_off = 0;
    LexKeysOnDevice d;
    rdf_sort_key key = *value;
    key.options = rdf_sort_options{0, 0};
    RDF_TRY(lexsort_keys_to_device(&key, 1, nchunks, mem, row_start, fn, pin_off, d));
    void *pstate, *pnulls;
    RDF_TRY(arena_alloc(sizeof(PctSelState), &pstate));
    RDF_TRY(arena_alloc(RDF_PERCENTILE_MAX_CALLS * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pstate, 0, sizeof(PctSelState), s));
    HIP_TRY(hipMemsetAsync(pnulls, 0, RDF_PERCENTILE_MAX_CALLS * 8, s));
    PctSelArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.st = (PctSelState*)pstate;
    sa.vchunks = d.tb.dev_at<DevChunkCol>(d.o_ch);
    sa.row_start = d.tb.dev_at<int64_t>(d.o_rs);
    sa.nchunks = nchunks;
    sa.n = n;
    sa.vdtype = value->values[0].dtype;
    sa.key_bits = pct_key_bits(sa.vdtype);
    sa.ncalls = ncalls;
    sa.nulls = (unsigned long long*)pnulls;
    void *d_counts = nullptr, *d_rows = nullptr;
    if (out_counts) { d_counts = out_counts->values; if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc(8, &d_counts)); sa.counts = (int64_t*)d_counts; }
    if (out_group_rows) { d_rows = out_group_rows->values; if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc(8, &d_rows)); sa.group_rows = (uint32_t*)d_rows; }
    void* dwords[RDF_PERCENTILE_MAX_CALLS] = {};
    bool any_disc = false;
    for (int c = 0; c < ncalls; ++c) {
        PctCallOut& o = sa.calls[c];
        o.kind = calls[c].kind;
        o.p = calls[c].p;
        any_disc |= o.kind == RDF_PCT_DISC;
        o.values = outs[c].values;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc(8, &o.values));
        if (outs[c].validity) {
            void* pv;
            RDF_TRY(arena_alloc(8, &pv));
            o.vbytes = (uint8_t*)pv;
            RDF_TRY(arena_alloc(8, &dwords[c]));
        }
    }
    // every launch of the longest case is queued; a launch whose work the state says is done returns at once, so nothing
    // comes back to the host between the passes
    const int npass = (sa.key_bits + kPctSelBits - 1) / kPctSelBits;
    KernelTimer kt;
    for (int p = 0; p < npass; ++p) {
        sa.pass = p;
        HIP_TRY(launch_pct_sel_hist(sa, s));
        HIP_TRY(launch_pct_sel_plan(sa, s));
    }
    if (npass > 1) {
        HIP_TRY(launch_pct_sel_gather(sa, s));
        HIP_TRY(launch_pct_sel_finish(sa, s));
    }
    if (any_disc) HIP_TRY(launch_pct_sel_rows(sa, s));
    HIP_TRY(launch_pct_sel_emit(sa, s));
    for (int c = 0; c < ncalls; ++c)
        if (sa.calls[c].vbytes) HIP_TRY(launch_win_pack(sa.calls[c].vbytes, 1, (uint64_t*)dwords[c], s));
    kt.stop();

    // ---- results to the caller
    RDF_TRY(pinned_reserve(pin_off + 128 + RDF_PERCENTILE_MAX_CALLS * 8));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, &sa.st->nslots, 24, hipMemcpyDeviceToHost, s));     // nslots, digits_done, phase, passes, cand_count, finished
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + 64, pnulls, RDF_PERCENTILE_MAX_CALLS * 8, hipMemcpyDeviceToHost, s));
    const hipMemcpyKind kind = mem == RDF_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (mem == RDF_MEM_HOST) {
        if (out_group_rows) HIP_TRY(hipMemcpyAsync(out_group_rows->values, d_rows, 4, kind, s));
        if (out_counts) HIP_TRY(hipMemcpyAsync(out_counts->values, d_counts, 8, kind, s));
        for (int c = 0; c < ncalls; ++c) HIP_TRY(hipMemcpyAsync(outs[c].values, sa.calls[c].values, (size_t)dtype_size(outs[c].dtype), kind, s));
    }
    for (int c = 0; c < ncalls; ++c)
        if (dwords[c]) HIP_TRY(hipMemcpyAsync(outs[c].validity, dwords[c], 1, kind, s));
    HIP_TRY(hipStreamSynchronize(s));
    int32_t head[6];
    unsigned long long nulls[RDF_PERCENTILE_MAX_CALLS];
    memcpy(head, ctx.pinned + pin_off, sizeof head);
    memcpy(nulls, ctx.pinned + pin_off + 64, sizeof nulls);
    if (head[2] != PCT_SEL_RESOLVED) return fail(RDF_COMPUTE_ERROR, "internal: %s: the select stopped in phase %d after %d digits", fn, head[2], head[1]);
    for (int c = 0; c < ncalls; ++c) outs[c].null_count = (int64_t)nulls[c];
    for (rdf_out* o : {out_group_rows, out_counts})
        if (o && o->validity) {
            if (mem == RDF_MEM_HOST) memset(o->validity, 0xFF, 1);
            else HIP_TRY(hipMemsetAsync(o->validity, 0xFF, 1, s));
        }
    if (mem == RDF_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(s));
    ctx.last_kernel = "select: " + std::to_string(head[3]) + " x pct_sel_hist_kernel + pct_sel_plan_kernel" +
                      (head[5] ? " + pct_sel_gather_kernel + pct_sel_finish_kernel" : "") + (any_disc ? " + pct_sel_rows_kernel" : "") + " + pct_sel_emit_kernel";
    return RDF_OK;
}

}  // namespace

rdf_status rdf_groupby_percentile(const rdf_sort_key* group_by, int32_t ngroup, const rdf_sort_key* value, int64_t nchunks,
                                  const rdf_percentile_call* calls, int32_t ncalls, rdf_out* out_group_rows, rdf_out* outs,
                                  rdf_out* out_counts, int64_t* out_groups) {
    // ---- everything that can be refused is refused before any device work
    const char* fn = "groupby_percentile";
    if (!out_groups) return fail(RDF_INVALID_ARGUMENT, "%s: null out_groups", fn);
    if (ngroup < 0 || ngroup > RDF_MAX_GROUP_KEYS) return fail(RDF_INVALID_ARGUMENT, "%s: 0 .. %d grouping keys", fn, RDF_MAX_GROUP_KEYS);
    if (ngroup > 0 && !group_by) return fail(RDF_INVALID_ARGUMENT, "%s: null key list", fn);
    if (ncalls < 0 || ncalls > RDF_PERCENTILE_MAX_CALLS) return fail(RDF_INVALID_ARGUMENT, "%s: at most %d calls", fn, RDF_PERCENTILE_MAX_CALLS);
    if (ncalls > 0 && (!calls || !outs)) return fail(RDF_INVALID_ARGUMENT, "%s: null call list", fn);
    if ((ncalls > 0 || out_counts) != (value != nullptr)) return fail(RDF_INVALID_ARGUMENT, "%s: a value column is given exactly when there are calls or counts", fn);
    for (int c = 0; c < ncalls; ++c) {
        if (calls[c].kind != RDF_PCT_CONT && calls[c].kind != RDF_PCT_DISC) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: unknown kind %d", fn, c, calls[c].kind);
        if (!pct_p_ok(calls[c].p)) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: p must lie in [0, 1]", fn, c);
    }
    const bool select_ok = ngroup == 0 && value && value->values && !value->utf8;
    const int route = g_ctx.opt_percentile_route;
    if (route == 2 && !select_ok) return fail(RDF_INVALID_ARGUMENT, "%s: the select route serves a numeric value column without grouping keys", fn);
    const int ncols = ngroup + (value ? 1 : 0);
    if (ncols > 0 && nchunks < 1) return fail(RDF_INVALID_ARGUMENT, "%s: bad arguments", fn);
    WinFront wf;
    wf.nkeys = ncols;
    wf.nextra = 0;
    wf.keys.resize((size_t)ncols);
    for (int k = 0; k < ncols; ++k) {
        wf.keys[k] = k < ngroup ? group_by[k] : *value;
        wf.keys[k].options = rdf_sort_options{0, 0};
    }
    bool any_utf8 = false;
    RDF_TRY(lexsort_check_keys(wf.keys.data(), ncols, nchunks, fn, &wf.mem, &any_utf8));
    const bool value_utf8 = value && value->utf8;
    bool value_nullable = false;
    if (value)
        for (int64_t c = 0; c < nchunks; ++c) value_nullable |= (value->values ? value->values[c].validity : value->utf8[c].offsets.validity) != nullptr;
    for (int c = 0; c < ncalls; ++c) {
        if (calls[c].kind == RDF_PCT_CONT && value_utf8) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: a continuous percentile of a Utf8 column", fn, c);
        if (outs[c].dtype != (calls[c].kind == RDF_PCT_CONT ? RDF_F64 : RDF_U32)) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: wrong output dtype", fn, c);
        if (value_nullable && !outs[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: a nullable value column needs a validity bitmap", fn, c);
    }
    if (out_counts && out_counts->dtype != RDF_I64) return fail(RDF_INVALID_ARGUMENT, "%s: counts are Int64", fn);
    if (out_group_rows && out_group_rows->dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "%s: group rows are UInt32", fn);
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
    // auto, from the measurements of DESIGN §25.4: the select route was faster for every dtype, size and distribution
    // measured (1.75 x at the least), so it takes every call it can serve
    const bool select_auto = select_ok;
    if (route == 2 || (route == 0 && select_auto)) {   // one group: the whole column, without a sort
        set_lengths(1);
        bool fits1 = (!out_group_rows || out_group_rows->capacity >= 1) && (!out_counts || out_counts->capacity >= 1);
        for (int c = 0; c < ncalls; ++c) fits1 &= outs[c].capacity >= 1;
        if (!fits1) return fail(RDF_MEMORY_ERROR, "output capacity too small (the group count is in *out_groups and every length)");
        return percentile_select(fn, value, nchunks, wf.row_start, mem, calls, ncalls, out_group_rows, outs, out_counts);
    }

    // ---- the order, then group and pair structure: rdf_window's front
    RDF_TRY(window_front_device(fn, ngroup, wf));
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    const size_t pin_off = wf.pin_off;
    RDF_TRY(pinned_reserve(pin_off + 64 + RDF_PERCENTILE_MAX_CALLS * 8));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, wf.scan + n, 8, hipMemcpyDeviceToHost, s));   // the scan's total: groups high, pairs low
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t total = 0;
    memcpy(&total, ctx.pinned + pin_off, 8);
    const int64_t G = (int64_t)(total >> 32), D = (int64_t)(uint32_t)total;
    if (G < 1 || D < G || D > n) {
        wf.kt->stop();
        return fail(RDF_COMPUTE_ERROR, "internal: %s: %lld groups of %lld pairs over %lld rows", fn, (long long)G, (long long)D, (long long)n);
    }
    set_lengths(G);
    bool fits = (!out_group_rows || out_group_rows->capacity >= G) && (!out_counts || out_counts->capacity >= G);
    for (int c = 0; c < ncalls; ++c) fits &= outs[c].capacity >= G;
    if (!fits) {
        wf.kt->stop();
        return fail(RDF_MEMORY_ERROR, "output capacity too small (the group count is in *out_groups and every length)");
    }
    const std::string front_kernels = wf.sort_kernels + "win_flags_kernel + win_starts_kernel";
    if (!out_group_rows && !out_counts && ncalls == 0) {   // the count-only call
        wf.kt->stop();
        ctx.last_kernel = "sorted: " + front_kernels;
        return RDF_OK;
    }

    // ---- one thread per (group, call)
    void* pnulls;
    RDF_TRY(arena_alloc(RDF_PERCENTILE_MAX_CALLS * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, RDF_PERCENTILE_MAX_CALLS * 8, s));
    PctPickArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.scan = wf.scan;
    pa.pstart = wf.pstart;
    pa.gstart = wf.gstart;
    pa.perm = wf.perm;
    if (value && value->values) pa.vchunks = wf.d.tb.dev_at<DevChunkCol>(wf.d.o_ch) + (size_t)ngroup * nchunks;
    if (value && value->utf8) pa.vutf8 = wf.d.ucols[ngroup].d_chunks;
    pa.row_start = wf.d_row_start;
    pa.nchunks = nchunks;
    pa.vdtype = value && value->values ? value->values[0].dtype : RDF_U8;
    pa.nullable = value_nullable ? 1 : 0;
    pa.groups = G;
    pa.ncalls = ncalls;
    pa.nulls = (unsigned long long*)pnulls;
    void* d_counts = nullptr;
    if (out_counts) {
        d_counts = out_counts->values;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)G * 8, &d_counts));
        pa.counts = (int64_t*)d_counts;
    }
    void* dwords[RDF_PERCENTILE_MAX_CALLS] = {};
    const size_t vbytes_len = (size_t)((G + 7) / 8);
    for (int c = 0; c < ncalls; ++c) {
        PctCallOut& o = pa.calls[c];
        o.kind = calls[c].kind;
        o.p = calls[c].p;
        o.values = outs[c].values;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)G * (size_t)dtype_size(outs[c].dtype), &o.values));
        if (outs[c].validity) {
            void* pv;
            RDF_TRY(arena_alloc((size_t)G, &pv));
            o.vbytes = (uint8_t*)pv;
            RDF_TRY(arena_alloc((size_t)((G + 63) / 64) * 8, &dwords[c]));   // whole words here, the caller's bitmap gets its bytes
        }
    }
    if (value) HIP_TRY(launch_pct_pick(pa, s));
    for (int c = 0; c < ncalls; ++c)
        if (pa.calls[c].vbytes) HIP_TRY(launch_win_pack(pa.calls[c].vbytes, G, (uint64_t*)dwords[c], s));

    // ---- the first row of every group: rdf_groupby_sorted's fold over the heads, no calls
    void* d_rows = nullptr;
    int levels = 0;
    if (out_group_rows) {
        d_rows = out_group_rows->values;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)G * 4, &d_rows));
        GrpFoldArgs fa;
        memset(&fa, 0, sizeof fa);
        fa.scan = wf.scan;
        fa.gstart = wf.gstart;
        fa.perm = wf.perm;
        fa.row_start = wf.d_row_start;
        fa.nchunks = nchunks;
        fa.vdtype = RDF_U8;
        fa.groups = G;
        fa.group_rows = (uint32_t*)d_rows;
        int64_t m = D;
        const GrpState* in = nullptr;
        for (;; ++levels) {
            fa.level = levels;
            fa.in = in;
            fa.m = m;
            fa.part = nullptr;
            const int64_t next = 2 * grp_tiles(m);
            if (m > kGrpTile) {
                void* pp;
                RDF_TRY(arena_alloc((size_t)next * sizeof(GrpState), &pp));
                fa.part = (GrpState*)pp;
            }
            HIP_TRY(launch_grp_fold(fa, s));
            if (!fa.part) break;
            in = fa.part;
            m = next;
        }
        ++levels;
    }
    wf.kt->stop();

    // ---- results to the caller
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + 64, pnulls, RDF_PERCENTILE_MAX_CALLS * 8, hipMemcpyDeviceToHost, s));
    const hipMemcpyKind kind = mem == RDF_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (mem == RDF_MEM_HOST) {
        if (out_group_rows) HIP_TRY(hipMemcpyAsync(out_group_rows->values, d_rows, (size_t)G * 4, kind, s));
        if (out_counts) HIP_TRY(hipMemcpyAsync(out_counts->values, d_counts, (size_t)G * 8, kind, s));
        for (int c = 0; c < ncalls; ++c)
            HIP_TRY(hipMemcpyAsync(outs[c].values, pa.calls[c].values, (size_t)G * (size_t)dtype_size(outs[c].dtype), kind, s));
    }
    for (int c = 0; c < ncalls; ++c)
        if (dwords[c]) HIP_TRY(hipMemcpyAsync(outs[c].validity, dwords[c], vbytes_len, kind, s));
    HIP_TRY(hipStreamSynchronize(s));
    unsigned long long nulls[RDF_PERCENTILE_MAX_CALLS];
    memcpy(nulls, ctx.pinned + pin_off + 64, sizeof nulls);
    for (int c = 0; c < ncalls; ++c) outs[c].null_count = (int64_t)nulls[c];
    for (rdf_out* o : {out_group_rows, out_counts})
        if (o && o->validity) {   // a bitmap nobody needs was handed in: all valid
            if (mem == RDF_MEM_HOST) memset(o->validity, 0xFF, vbytes_len);
            else HIP_TRY(hipMemsetAsync(o->validity, 0xFF, vbytes_len, s));
        }
    if (mem == RDF_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(s));
    ctx.last_kernel = "sorted: " + front_kernels + (value ? " + pct_pick_kernel" : "") + (levels ? " + " + std::to_string(levels) + " x grp_fold_kernel" : std::string());
    return RDF_OK;
}
