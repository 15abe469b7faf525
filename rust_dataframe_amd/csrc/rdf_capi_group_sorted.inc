// rdf_capi_group_sorted.inc — host side of rdf_groupby_sorted: count_distinct / sum_distinct / first / last per group
// (kernels: rdf_group_sorted.hip, argument blocks: rdf_group_sorted.h); textually included by rdf_capi.cpp after
// rdf_capi_window.inc, whose device front (staging, sort_core, flag pass, scan, start tables) it runs unchanged with the
// grouping columns as partition keys and the value column as the one order key.
//
// After the front: the group and pair counts come back in one 8-byte copy (the outputs are sized by them), then the fold
// walks the head list level by level, the validity bytes are packed, and host outputs are copied back.

namespace {

int group_sorted_out_dtype(int fn, bool value_is_float) {
    switch (fn) {
        case RDF_GRP_COUNT_DISTINCT: return RDF_I64;
        case RDF_GRP_SUM_DISTINCT: return value_is_float ? RDF_F64 : RDF_I64;
        default: return RDF_U32;
    }
}

}  // namespace

rdf_status rdf_groupby_sorted(const rdf_sort_key* group_by, int32_t ngroup, const rdf_sort_key* value, int64_t nchunks,
                              const rdf_group_call* calls, int32_t ncalls, rdf_out* out_group_rows, rdf_out* outs,
                              int64_t* out_groups) {
    // ---- everything that can be refused is refused before any device work
    const char* fn = "groupby_sorted";
    if (!out_groups) return fail(RDF_INVALID_ARGUMENT, "%s: null out_groups", fn);
    if (ngroup < 0 || ngroup > RDF_MAX_GROUP_KEYS) return fail(RDF_INVALID_ARGUMENT, "%s: 0 .. %d grouping keys", fn, RDF_MAX_GROUP_KEYS);
    if (ngroup > 0 && !group_by) return fail(RDF_INVALID_ARGUMENT, "%s: null key list", fn);
    if (ncalls < 0 || ncalls > RDF_GROUP_MAX_CALLS) return fail(RDF_INVALID_ARGUMENT, "%s: at most %d calls", fn, RDF_GROUP_MAX_CALLS);
    if (ncalls > 0 && (!calls || !outs)) return fail(RDF_INVALID_ARGUMENT, "%s: null call list", fn);
    if ((ncalls > 0) != (value != nullptr)) return fail(RDF_INVALID_ARGUMENT, "%s: a value column is given exactly when there are calls", fn);
    for (int c = 0; c < ncalls; ++c)
        if (calls[c].fn < RDF_GRP_COUNT_DISTINCT || calls[c].fn > RDF_GRP_LAST) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: unknown function %d", fn, c, calls[c].fn);
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
    const bool value_float = value && value->values && is_float(value->values[0].dtype);
    bool value_nullable = false;
    if (value)
        for (int64_t c = 0; c < nchunks; ++c) value_nullable |= (value->values ? value->values[c].validity : value->utf8[c].offsets.validity) != nullptr;
    for (int c = 0; c < ncalls; ++c) {
        if (calls[c].fn == RDF_GRP_SUM_DISTINCT && value_utf8) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: sum_distinct of a Utf8 column", fn, c);
        if (outs[c].dtype != group_sorted_out_dtype(calls[c].fn, value_float)) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: wrong output dtype", fn, c);
        if (calls[c].fn >= RDF_GRP_FIRST && calls[c].ignore_nulls && value_nullable && !outs[c].validity)
            return fail(RDF_INVALID_ARGUMENT, "%s: call %d: first / last with ignore_nulls over a nullable column need a validity bitmap", fn, c);
    }
    if (out_group_rows && out_group_rows->dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "%s: group rows are UInt32", fn);
    if (ncols == 0) {   // no keys and no value: no rows
        *out_groups = 0;
        if (out_group_rows) { out_group_rows->length = 0; out_group_rows->null_count = 0; }
        return RDF_OK;
    }
    const int32_t mem = wf.mem;
    if (out_group_rows) RDF_TRY(check_out_mem(out_group_rows, 1, mem));
    RDF_TRY(check_out_mem(outs, ncalls, mem));
    wf.nch = nchunks;
    RDF_TRY(lexsort_row_starts(wf.keys.data(), ncols, nchunks, fn, wf.row_start));
    const int64_t n = wf.n = wf.row_start[(size_t)nchunks];
    for (int c = 0; c < ncalls; ++c)
        if (n > 0 && outs[c].capacity > 0 && !outs[c].values) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: null output buffer", fn, c);
    if (out_group_rows && n > 0 && out_group_rows->capacity > 0 && !out_group_rows->values) return fail(RDF_INVALID_ARGUMENT, "%s: null group rows buffer", fn);
    auto set_lengths = [&](int64_t g) {
        *out_groups = g;
        if (out_group_rows) { out_group_rows->length = g; out_group_rows->null_count = 0; }
        for (int c = 0; c < ncalls; ++c) { outs[c].length = g; outs[c].null_count = 0; }
    };
    if (n == 0) { set_lengths(0); return RDF_OK; }

    // ---- the order, then group and pair structure: rdf_window's front
    RDF_TRY(window_front_device(fn, ngroup, wf));
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    const size_t pin_off = wf.pin_off;
    RDF_TRY(pinned_reserve(pin_off + 64 + RDF_GROUP_MAX_CALLS * 8));
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
    bool fits = !out_group_rows || out_group_rows->capacity >= G;
    for (int c = 0; c < ncalls; ++c) fits &= outs[c].capacity >= G;
    if (!fits) {
        wf.kt->stop();
        return fail(RDF_MEMORY_ERROR, "output capacity too small (the group count is in *out_groups and every length)");
    }
    const std::string front_kernels = wf.sort_kernels + "win_flags_kernel + win_starts_kernel";
    if (!out_group_rows && ncalls == 0) {   // the count-only call
        wf.kt->stop();
        ctx.last_kernel = front_kernels;
        return RDF_OK;
    }

    // ---- the fold over the head list, level by level
    void* pnulls;
    RDF_TRY(arena_alloc(RDF_GROUP_MAX_CALLS * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, RDF_GROUP_MAX_CALLS * 8, s));
    GrpFoldArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.scan = wf.scan;
    fa.gstart = wf.gstart;
    fa.perm = wf.perm;
    if (value && value->values) fa.vchunks = wf.d.tb.dev_at<DevChunkCol>(wf.d.o_ch) + (size_t)ngroup * nchunks;
    if (value && value->utf8) fa.vutf8 = wf.d.ucols[ngroup].d_chunks;
    fa.row_start = wf.d_row_start;
    fa.nchunks = nchunks;
    fa.vdtype = value && value->values ? value->values[0].dtype : RDF_U8;
    fa.groups = G;
    fa.ncalls = ncalls;
    fa.nulls = (unsigned long long*)pnulls;
    void* d_rows = nullptr;
    if (out_group_rows) {
        d_rows = out_group_rows->values;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)G * 4, &d_rows));
        fa.group_rows = (uint32_t*)d_rows;
    }
    void* dwords[RDF_GROUP_MAX_CALLS] = {};
    const size_t vbytes_len = (size_t)((G + 7) / 8);
    for (int c = 0; c < ncalls; ++c) {
        GrpCallOut& o = fa.calls[c];
        o.fn = calls[c].fn;
        o.ignore_nulls = calls[c].fn >= RDF_GRP_FIRST && calls[c].ignore_nulls ? 1 : 0;
        o.values = outs[c].values;
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)G * (size_t)dtype_size(outs[c].dtype), &o.values));
        if (o.ignore_nulls && outs[c].validity) {
            void* pv;
            RDF_TRY(arena_alloc((size_t)G, &pv));
            o.vbytes = (uint8_t*)pv;
            RDF_TRY(arena_alloc((size_t)((G + 63) / 64) * 8, &dwords[c]));   // whole words here, the caller's bitmap gets its bytes
        }
    }
    int levels = 0;
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
    for (int c = 0; c < ncalls; ++c)
        if (fa.calls[c].vbytes) HIP_TRY(launch_win_pack(fa.calls[c].vbytes, G, (uint64_t*)dwords[c], s));
    wf.kt->stop();

    // ---- results to the caller
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + 64, pnulls, RDF_GROUP_MAX_CALLS * 8, hipMemcpyDeviceToHost, s));
    const hipMemcpyKind kind = mem == RDF_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (mem == RDF_MEM_HOST) {
        if (out_group_rows) HIP_TRY(hipMemcpyAsync(out_group_rows->values, d_rows, (size_t)G * 4, kind, s));
        for (int c = 0; c < ncalls; ++c)
            HIP_TRY(hipMemcpyAsync(outs[c].values, fa.calls[c].values, (size_t)G * (size_t)dtype_size(outs[c].dtype), kind, s));
    }
    for (int c = 0; c < ncalls; ++c)
        if (dwords[c]) HIP_TRY(hipMemcpyAsync(outs[c].validity, dwords[c], vbytes_len, kind, s));
    HIP_TRY(hipStreamSynchronize(s));
    unsigned long long nulls[RDF_GROUP_MAX_CALLS];
    memcpy(nulls, ctx.pinned + pin_off + 64, sizeof nulls);
    for (int c = 0; c < ncalls; ++c) {
        outs[c].null_count = dwords[c] ? (int64_t)nulls[c] : 0;
        if (!dwords[c] && outs[c].validity) {   // a bitmap nobody needs was handed in: all valid
            if (mem == RDF_MEM_HOST) memset(outs[c].validity, 0xFF, vbytes_len);
            else HIP_TRY(hipMemsetAsync(outs[c].validity, 0xFF, vbytes_len, s));
        }
    }
    if (out_group_rows && out_group_rows->validity) {
        if (mem == RDF_MEM_HOST) memset(out_group_rows->validity, 0xFF, vbytes_len);
        else HIP_TRY(hipMemsetAsync(out_group_rows->validity, 0xFF, vbytes_len, s));
    }
    if (mem == RDF_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(s));
    ctx.last_kernel = front_kernels + " + " + std::to_string(levels) + " x grp_fold_kernel";
    return RDF_OK;
}
