// rdf_capi_groupby_multi.inc — host side of rdf_groupby_multi (kernels: rdf_groupby_multi.hip; route and LDS layout:
// rdf_groupby_multi_plan.h); textually included by rdf_capi.cpp after rdf_capi_dict.inc (it uses rdf_capi_groupby.inc's key
// packer and copy helpers and rdf_capi_dict.inc's code buffers).
//
//   rdf_groupby_multi   validation -> Utf8 keys to dictionary codes -> several keys packed into one (GbKeyPack) -> ONE pass
//                       over the packed key and the value columns (gbm_stream_kernel while the promised groups fit a block's
//                       LDS table, gbm_table_kernel otherwise) -> gbm_emit_kernel -> gbm_finish_kernel -> copy-out, the
//                       dictionary taken by the group codes.

namespace {

struct GbmCallPlan {
    int op[kGbmMaxCalls];        // AGG_* / GBM_COUNT
    int value[kGbmMaxCalls];     // value column, -1: the call counts rows
    int odt[kGbmMaxCalls];       // dtype of outs[c]
    int vdt[kGbmMaxValues];
    bool vnullable[kGbmMaxValues];
};

// device words of a call: [0] distinct keys of the table proper, [1] flags, [2] emit cursor, then the per-call null counts
constexpr size_t kGbmHeadBytes = 64 + 8 * kGbmMaxCalls;

rdf_status gbm_table_alloc(GbmTable& t, unsigned long long** nulls, int ncalls, int64_t groups, const int* op) {
    int64_t capacity = 1024;
    while (capacity < 2 * groups) capacity <<= 1;
    const int64_t entries = capacity + 2;
    void* p = nullptr;
    RDF_TRY(arena_alloc(kGbmHeadBytes + sizeof(uint64_t) * (size_t)entries * (size_t)(2 + 2 * ncalls) + 64, &p));
    t.head = (unsigned int*)p;
    *nulls = (unsigned long long*)((char*)p + 64);
    t.keys = (unsigned long long*)((char*)p + kGbmHeadBytes);
    t.rows = t.keys + entries;
    t.acc = t.rows + entries;
    t.cnt = t.acc + (size_t)ncalls * (size_t)entries;
    t.capacity = capacity;
    t.entries = entries;
    hipStream_t s = g_ctx.stream;
    HIP_TRY(hipMemsetAsync(p, 0, kGbmHeadBytes, s));
    HIP_TRY(hipMemsetAsync(t.keys, 0xFF, sizeof(uint64_t) * (size_t)entries, s));                       // the free marker
    HIP_TRY(hipMemsetAsync(t.rows, 0, sizeof(uint64_t) * (size_t)entries, s));
    for (int c = 0; c < ncalls; ++c)                                                                     // the identities: ~0 for MIN, 0 otherwise
        HIP_TRY(hipMemsetAsync(t.acc + (size_t)c * (size_t)entries, op[c] == AGG_MIN ? 0xFF : 0, sizeof(uint64_t) * (size_t)entries, s));
    HIP_TRY(hipMemsetAsync(t.cnt, 0, sizeof(uint64_t) * (size_t)ncalls * (size_t)entries, s));
    return RDF_OK;
}

// The checked core over integer key columns (keys[k * nchunks + i]); Utf8 keys arrive as their codes.  slack: as groupby_agg_impl's.
rdf_status groupby_multi_impl(const rdf_array* keys, int32_t nkeys, const rdf_array* const* values, int32_t nvalues, int64_t nchunks,
                              const GbmCallPlan& cp, int32_t ncalls, int64_t max_groups, int32_t mem,
                              rdf_out* out_keys, rdf_out* outs, rdf_out* out_counts, rdf_out* out_group_rows, int64_t slack, int64_t* out_groups) {
    int kdt[kMaxKeyCols];
    bool knullable[kMaxKeyCols];
    int64_t nrows = 0;
    for (int64_t c = 0; c < nchunks; ++c) nrows += keys[c].length;
    for (int k = 0; k < nkeys; ++k) {
        kdt[k] = keys[(int64_t)k * nchunks].dtype;
        knullable[k] = false;
        for (int64_t c = 0; c < nchunks; ++c) knullable[k] |= keys[(int64_t)k * nchunks + c].validity != nullptr;
    }
    auto deliver_empty = [&]() {
        for (int k = 0; k < nkeys; ++k) { out_keys[k].length = 0; out_keys[k].null_count = 0; }
        for (int c = 0; c < ncalls; ++c) { outs[c].length = out_counts[c].length = 0; outs[c].null_count = out_counts[c].null_count = 0; }
        if (out_group_rows) { out_group_rows->length = 0; out_group_rows->null_count = 0; }
        *out_groups = 0;
    };
    if (nrows == 0) { deliver_empty(); return RDF_OK; }

    GbKeyPack pk;
    RDF_TRY(pk.plan(keys, nkeys, nchunks, kdt, knullable, max_groups, nrows));
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();
    size_t pin_off = 0, used = 0;
    InputStager st;
    for (int64_t i = 0; i < (int64_t)nkeys * nchunks; ++i) st.add(&keys[i]);
    for (int v = 0; v < nvalues; ++v) for (int64_t c = 0; c < nchunks; ++c) st.add(&values[v][c]);
    RDF_TRY(st.finish(pin_off, &used));
    pin_off += (used + 255) & ~(size_t)255;
    GbInput in;
    in.clen.resize((size_t)nchunks);
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0), sub_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        in.clen[(size_t)c] = keys[c].length;
        row_start[(size_t)c + 1] = row_start[(size_t)c] + keys[c].length;
        sub_start[(size_t)c + 1] = sub_start[(size_t)c] + (keys[c].length + kGbmSub - 1) / kGbmSub;
    }
    if (nkeys == 1) {
        in.kdt = kdt[0];
        in.keys.assign(st.dev.begin(), st.dev.begin() + (size_t)nchunks);
    } else {
        RDF_TRY(pk.pack(st.dev, kdt, knullable, nkeys, nchunks, nrows, in.clen, row_start, max_groups, pin_off, in));
    }

    // chunk tables of the one pass
    TableBuilder tb;
    const size_t o_k = tb.reserve(sizeof(DevChunkCol) * (size_t)nchunks);
    const size_t o_v = tb.reserve(sizeof(DevChunkCol) * (size_t)std::max(nvalues, 1) * (size_t)nchunks);
    const size_t o_ss = tb.reserve(sizeof(int64_t) * sub_start.size());
    const size_t o_len = tb.reserve(sizeof(int64_t) * in.clen.size());
    RDF_TRY(tb.bind(pin_off));
    memcpy(tb.at<char>(o_k), in.keys.data(), sizeof(DevChunkCol) * (size_t)nchunks);
    if (nvalues > 0) memcpy(tb.at<char>(o_v), st.dev.data() + (size_t)nkeys * (size_t)nchunks, sizeof(DevChunkCol) * (size_t)nvalues * (size_t)nchunks);
    memcpy(tb.at<char>(o_ss), sub_start.data(), sizeof(int64_t) * sub_start.size());
    memcpy(tb.at<char>(o_len), in.clen.data(), sizeof(int64_t) * in.clen.size());
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(pin_off));
    pin_off += (tb.size + 255) & ~(size_t)255;

    GbmArgs a;
    memset(&a, 0, sizeof a);
    a.keys = tb.dev_at<DevChunkCol>(o_k);
    a.values = tb.dev_at<DevChunkCol>(o_v);
    a.chunk_sub_start = tb.dev_at<int64_t>(o_ss);
    a.chunk_len = tb.dev_at<int64_t>(o_len);
    a.nchunks = nchunks;
    a.nsubs = sub_start[(size_t)nchunks];
    if (nchunks == 1) {
        a.key0 = in.keys[0];
        a.len0 = in.clen[0];
        for (int v = 0; v < nvalues; ++v) a.val0[v] = st.dev[(size_t)nkeys + (size_t)v];
    }
    a.key_dtype = in.kdt;
    a.nvalues = nvalues;
    a.ncalls = ncalls;
    uint32_t rows_mask = 0;
    {   // the calls ordered by value column (those that count rows take no part in the pass)
        int slot = 0;
        for (int v = 0; v < nvalues; ++v) {
            a.value_dtype[v] = cp.vdt[v];
            a.first_bits |= (uint64_t)slot << (4 * v);
            for (int c = 0; c < ncalls; ++c)
                if (cp.value[c] == v) { a.order_bits |= (uint64_t)c << (8 * slot); ++slot; }
        }
        a.first_bits |= (uint64_t)slot << (4 * nvalues);
        for (int c = 0; c < ncalls; ++c) {
            const int cls = cp.value[c] >= 0 ? value_class(cp.vdt[cp.value[c]]) : CLS_UNSIGNED;
            a.call_bits |= ((uint32_t)cp.op[c] | (uint32_t)cls << 2) << (4 * c);
            if (cp.value[c] < 0) rows_mask |= 1u << c;
        }
    }
    const GbmPlan plan = gbm_plan(ncalls, max_groups, ctx.opt_gbm_slots, ctx.opt_gbm_route);
    a.slots = plan.slots; a.off_acc = plan.off_acc; a.off_rows = plan.off_rows; a.off_cnt = plan.off_cnt; a.off_tail = plan.off_tail;
    const int rpt = gbm_rows_per_thread(nvalues);
    const int ncu = std::max(1, eval_grid_limit() / 8);
    const int64_t table_groups = std::min<int64_t>(max_groups, nrows) + 2;

    unsigned long long* dnulls = nullptr;
    int route = plan.route;
    unsigned int head[4] = {0, 0, 0, 0};
    unsigned long long srows[2] = {0, 0};
    for (;;) {
        RDF_TRY(gbm_table_alloc(a.t, &dnulls, ncalls, table_groups, cp.op));
        KernelTimer kt;
        if (route == GBM_ROUTE_STREAM) {
            const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((a.nsubs + rpt - 1) / rpt, 2 * (int64_t)ncu));
            HIP_TRY(launch_gbm_stream(a, rpt, grid, (size_t)plan.lds_bytes, ctx.stream));
            ctx.last_kernel = "gbm_stream_kernel";
        } else {
            HIP_TRY(launch_gbm_table(a, rpt, ctx.stream));
            ctx.last_kernel = "gbm_table_kernel";
        }
        kt.stop();
        RDF_TRY(pinned_reserve(pin_off + 64));
        HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, a.t.head, 16, hipMemcpyDeviceToHost, ctx.stream));
        HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + 16, a.t.rows + a.t.capacity, 16, hipMemcpyDeviceToHost, ctx.stream));
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        memcpy(head, ctx.pinned + pin_off, 16);
        memcpy(srows, ctx.pinned + pin_off + 16, 16);
        if ((head[1] & 8u) && route == GBM_ROUTE_STREAM && max_groups > plan.capacity) {
            // the stream route was forced beyond its capacity and a block's table filled up: that proves nothing about the
            // promise, the table route takes any number of groups
            route = GBM_ROUTE_TABLE;
            continue;
        }
        break;
    }
    const int64_t ng_main = (int64_t)head[0];
    const int64_t ng = ng_main + (srows[0] ? 1 : 0) + (srows[1] ? 1 : 0);
    // (a block table holds 2 x capacity keys, and the route is planned for max_groups <= capacity: full means more than promised)
    if ((head[1] & (4u | 8u)) || ng > max_groups + slack) return fail(RDF_MEMORY_ERROR, "groupby_multi: more than max_groups (%lld) distinct keys", (long long)max_groups);

    // dense outputs, sized by the groups that exist
    const int64_t cap_out = std::max<int64_t>(ng, 1);
    const int64_t words = (cap_out + 63) / 64;
    void *dkeys, *dkvalid, *drows, *dacc, *dcnt, *dvalid;
    RDF_TRY(arena_alloc((size_t)cap_out * 8 + 64, &dkeys));
    RDF_TRY(arena_alloc((size_t)words * 8 + 8, &dkvalid));
    RDF_TRY(arena_alloc((size_t)cap_out * 8 + 64, &drows));
    RDF_TRY(arena_alloc((size_t)ncalls * (size_t)cap_out * 8 + 64, &dacc));
    RDF_TRY(arena_alloc((size_t)ncalls * (size_t)cap_out * 8 + 64, &dcnt));
    RDF_TRY(arena_alloc((size_t)ncalls * (size_t)words * 8 + 8, &dvalid));
    HIP_TRY(hipMemsetAsync(dkvalid, 0, (size_t)words * 8 + 8, ctx.stream));
    GbmEmitArgs ea;
    memset(&ea, 0, sizeof ea);
    ea.t = a.t; ea.ncalls = ncalls; ea.key_dtype = in.kdt; ea.rows_mask = rows_mask; ea.ng_main = ng_main; ea.cap_out = cap_out;
    ea.out_keys = dkeys; ea.out_keys_validity = (uint32_t*)dkvalid; ea.out_rows = (int64_t*)drows; ea.out_acc = (uint64_t*)dacc; ea.out_cnt = (int64_t*)dcnt;
    GbmFinishArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.acc = (uint64_t*)dacc; fa.cnt = (const int64_t*)dcnt; fa.validity = (uint64_t*)dvalid; fa.nulls = dnulls;
    fa.n = ng; fa.cap_out = cap_out; fa.words = words; fa.ncalls = ncalls; fa.call_bits = a.call_bits;
    {
        KernelTimer kt;
        HIP_TRY(launch_gbm_emit(ea, ctx.stream));
        HIP_TRY(launch_gbm_finish(fa, ctx.stream));
        kt.stop();
    }
    ctx.last_kernel += " + gbm_emit_kernel + gbm_finish_kernel";
    RDF_TRY(pinned_reserve(pin_off + 128));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, dnulls, 8 * (size_t)ncalls, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    unsigned long long vnulls[kGbmMaxCalls];
    memcpy(vnulls, ctx.pinned + pin_off, 8 * (size_t)ncalls);

    // ---- copy-out
    const size_t bits = (size_t)((ng + 7) / 8);
    if (nkeys == 1) {
        RDF_TRY(gb_copy_out(dkeys, (size_t)ng * (size_t)dtype_size(kdt[0]), out_keys->values, mem));
        if (out_keys->validity) RDF_TRY(gb_copy_out(dkvalid, bits, out_keys->validity, mem));
        out_keys->length = ng;
        out_keys->null_count = srows[1] ? 1 : 0;
    } else {
        void* pkn = nullptr;
        RDF_TRY(arena_alloc(64, &pkn));
        RDF_TRY(pk.unpack(dkeys, ng, kdt, nkeys, (unsigned long long*)pkn, out_keys, mem, pin_off));
    }
    for (int c = 0; c < ncalls; ++c) {
        RDF_TRY(gb_copy_out((const char*)dacc + (size_t)c * (size_t)cap_out * 8, (size_t)ng * 8, outs[c].values, mem));
        RDF_TRY(gb_copy_out((const char*)dcnt + (size_t)c * (size_t)cap_out * 8, (size_t)ng * 8, out_counts[c].values, mem));
        if (outs[c].validity) RDF_TRY(gb_copy_out((const char*)dvalid + (size_t)c * (size_t)words * 8, bits, outs[c].validity, mem));
        RDF_TRY(gb_fill_valid(&out_counts[c], ng, mem));
        outs[c].length = out_counts[c].length = ng;
        outs[c].null_count = (int64_t)vnulls[c];
        out_counts[c].null_count = 0;
    }
    if (out_group_rows) {
        RDF_TRY(gb_copy_out(drows, (size_t)ng * 8, out_group_rows->values, mem));
        RDF_TRY(gb_fill_valid(out_group_rows, ng, mem));
        out_group_rows->length = ng;
        out_group_rows->null_count = 0;
    }
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    *out_groups = ng;
    return RDF_OK;
}

}  // namespace

extern "C" {

int64_t rdf_groupby_multi_capacity(int32_t ncalls) { return gbm_capacity(ncalls); }

rdf_status rdf_groupby_multi(const rdf_sort_key* keys, int32_t nkeys, const rdf_array* const* values, int32_t nvalues, int64_t nchunks,
                             const rdf_multi_agg_call* calls, int32_t ncalls, int64_t max_groups,
                             rdf_key_out* out_keys, rdf_out* outs, rdf_out* out_counts, rdf_out* out_group_rows, int64_t* out_groups) {
    const char* fn = "groupby_multi";
    if (nchunks < 1 || !keys) return fail(RDF_INVALID_ARGUMENT, "%s: a column has at least one chunk", fn);
    if (nkeys < 1 || nkeys > kMaxKeyCols) return fail(RDF_INVALID_ARGUMENT, "%s: 1..%d grouping columns", fn, kMaxKeyCols);
    if (ncalls < 1 || ncalls > RDF_MULTI_MAX_CALLS) return fail(RDF_INVALID_ARGUMENT, "%s: 1..%d aggregate calls", fn, RDF_MULTI_MAX_CALLS);
    if (nvalues < 0 || nvalues > RDF_MULTI_MAX_VALUES) return fail(RDF_INVALID_ARGUMENT, "%s: 0..%d value columns", fn, RDF_MULTI_MAX_VALUES);
    if (!calls || !out_keys || !outs || !out_counts || !out_groups || (nvalues > 0 && !values)) return fail(RDF_INVALID_ARGUMENT, "%s: null argument", fn);
    if (max_groups < 1) return fail(RDF_INVALID_ARGUMENT, "%s: max_groups must be positive", fn);
    GbmCallPlan cp;
    for (int c = 0; c < ncalls; ++c) {
        if (calls[c].agg < RDF_AGG_SUM || calls[c].agg > RDF_AGG_COUNT) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: unknown aggregate %d", fn, c, calls[c].agg);
        if (calls[c].value < -1 || calls[c].value >= nvalues) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: value column %d of %d", fn, c, calls[c].value, nvalues);
        if (calls[c].value == -1 && calls[c].agg != RDF_AGG_COUNT) return fail(RDF_INVALID_ARGUMENT, "%s: call %d: only COUNT takes no value column", fn, c);
        cp.op[c] = calls[c].agg == RDF_AGG_MIN ? AGG_MIN : calls[c].agg == RDF_AGG_MAX ? AGG_MAX : calls[c].agg == RDF_AGG_COUNT ? GBM_COUNT : AGG_SUM;
        cp.value[c] = calls[c].value;
    }
    int32_t mem = -1;
    bool any_utf8 = false;
    RDF_TRY(lexsort_check_keys(keys, nkeys, nchunks, fn, &mem, &any_utf8));
    for (int k = 0; k < nkeys; ++k)
        if (keys[k].values && !(keys[k].values[0].dtype >= RDF_I8 && keys[k].values[0].dtype <= RDF_U64)) return fail(RDF_INVALID_ARGUMENT, "%s: integer or Utf8 key column required", fn);
    for (int v = 0; v < nvalues; ++v) {
        if (!values[v]) return fail(RDF_INVALID_ARGUMENT, "%s: value column %d is null", fn, v);
        RDF_TRY(check_mem(values[v], nchunks, &mem));
        cp.vdt[v] = values[v][0].dtype;
        if (!is_numeric(cp.vdt[v])) return fail(RDF_INVALID_ARGUMENT, "%s: numeric value column required", fn);
        cp.vnullable[v] = false;
        for (int64_t c = 0; c < nchunks; ++c) {
            if (values[v][c].dtype != cp.vdt[v]) return fail(RDF_INVALID_ARGUMENT, "%s: chunks differ in dtype", fn);
            cp.vnullable[v] |= values[v][c].validity != nullptr;
        }
    }
    std::vector<int64_t> row_start;
    RDF_TRY(lexsort_row_starts(keys, nkeys, nchunks, fn, row_start));
    const int64_t nrows = row_start[(size_t)nchunks];
    for (int v = 0; v < nvalues; ++v)
        for (int64_t c = 0; c < nchunks; ++c)
            if (values[v][c].length != row_start[(size_t)c + 1] - row_start[(size_t)c]) return fail(RDF_COMPUTE_ERROR, "%s: key and value chunks differ in length", fn);
    for (int k = 0; k < nkeys; ++k) {
        const rdf_key_out& o = out_keys[k];
        if (keys[k].values) {
            if (!o.values || o.utf8_offsets || o.utf8_data) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d: a numeric key comes back in `values` alone", fn, k);
            RDF_TRY(check_out_mem(o.values, 1, mem));
            if (o.values->dtype != keys[k].values[0].dtype) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d must have the key dtype", fn, k);
            bool kn = false;
            for (int64_t c = 0; c < nchunks; ++c) kn |= keys[k].values[c].validity != nullptr;
            if (kn && !o.values->validity) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d needs a validity buffer", fn, k);
            continue;
        }
        if (o.values || !o.utf8_offsets || !o.utf8_data) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d: a Utf8 key comes back in the (utf8_offsets, utf8_data) pair alone", fn, k);
        if (o.utf8_offsets->dtype != RDF_I32 || o.utf8_data->dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d: (Int32 offsets, UInt8 data)", fn, k);
        RDF_TRY(check_out_mem(o.utf8_offsets, 1, mem));
        RDF_TRY(check_out_mem(o.utf8_data, 1, mem));
        if (!o.utf8_offsets->values || o.utf8_offsets->capacity < 1) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d has no offsets buffer", fn, k);
        if (o.utf8_data->capacity < 0 || (o.utf8_data->capacity > 0 && !o.utf8_data->values)) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d: data capacity without a buffer", fn, k);
        if (utf8_nullable(keys[k].utf8, nchunks) && !o.utf8_offsets->validity) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d needs a validity buffer", fn, k);
    }
    RDF_TRY(check_out_mem(outs, ncalls, mem));
    RDF_TRY(check_out_mem(out_counts, ncalls, mem));
    if (out_group_rows) RDF_TRY(check_out_mem(out_group_rows, 1, mem));
    for (int c = 0; c < ncalls; ++c) {
        const int v = cp.value[c];
        cp.odt[c] = cp.op[c] == GBM_COUNT ? RDF_I64 : gb_acc_dtype(cp.op[c], cp.vdt[v]);
        if (outs[c].dtype != cp.odt[c] || out_counts[c].dtype != RDF_I64)
            return fail(RDF_INVALID_ARGUMENT, "%s: call %d: outputs must be (%s, Int64)", fn, c, cp.odt[c] == RDF_F64 ? "Float64" : cp.odt[c] == RDF_U64 ? "UInt64" : "Int64");
        if ((cp.op[c] == AGG_MIN || cp.op[c] == AGG_MAX) && cp.vnullable[v] && !outs[c].validity)
            return fail(RDF_INVALID_ARGUMENT, "%s: call %d: min / max of a nullable column needs an output validity buffer", fn, c);
    }
    if (out_group_rows && out_group_rows->dtype != RDF_I64) return fail(RDF_INVALID_ARGUMENT, "%s: the group rows are Int64", fn);
    const int64_t cap_needed = std::min<int64_t>(max_groups + 2, nrows + 2);
    for (int c = 0; c < ncalls; ++c)
        if (outs[c].capacity < cap_needed || out_counts[c].capacity < cap_needed) return fail(RDF_MEMORY_ERROR, "output capacity too small (need max_groups + 2)");
    if (out_group_rows && out_group_rows->capacity < cap_needed) return fail(RDF_MEMORY_ERROR, "output capacity too small (need max_groups + 2)");
    for (int k = 0; k < nkeys; ++k)
        if (keys[k].values && out_keys[k].values->capacity < cap_needed) return fail(RDF_MEMORY_ERROR, "output capacity too small (need max_groups + 2)");

    // the integer call's own list: numeric keys as they are, Utf8 keys as their codes
    std::vector<rdf_array> flat((size_t)nkeys * (size_t)nchunks);
    rdf_out ok[kMaxKeyCols];
    if (!any_utf8) {
        for (int k = 0; k < nkeys; ++k) {
            for (int64_t c = 0; c < nchunks; ++c) flat[(size_t)k * nchunks + c] = keys[k].values[c];
            ok[k] = *out_keys[k].values;
        }
        const rdf_status st = groupby_multi_impl(flat.data(), nkeys, values, nvalues, nchunks, cp, ncalls, max_groups, mem, ok, outs, out_counts, out_group_rows, 0, out_groups);
        if (st == RDF_OK) for (int k = 0; k < nkeys; ++k) *out_keys[k].values = ok[k];
        return st;
    }
    RDF_TRY(ensure_ready());

    DictCodes codes[kMaxKeyCols];
    DictBuf doffs[kMaxKeyCols], ddata[kMaxKeyCols], gcodes[kMaxKeyCols], toffs[kMaxKeyCols];
    rdf_utf8_array dict[kMaxKeyCols];
    bool nullable[kMaxKeyCols] = {false, false, false, false};
    const size_t vb = (size_t)cap_needed * 8, vbits = ((size_t)cap_needed + 63) / 64 * 8 + 8;
    // every numeric output goes through a buffer of the call's own: the caller's stay untouched until every Utf8 key fits
    auto shadow = [&](const rdf_out& o, DictBuf& buf, rdf_out* t) -> rdf_status {
        RDF_TRY(buf.alloc(vb + 256 + vbits, mem));
        *t = o;
        t->values = buf.p;
        t->validity = o.validity ? (uint8_t*)buf.p + ((vb + 255) & ~(size_t)255) : nullptr;
        t->capacity = cap_needed;
        return RDF_OK;
    };
    for (int k = 0; k < nkeys; ++k) {
        if (keys[k].values) {
            for (int64_t c = 0; c < nchunks; ++c) flat[(size_t)k * nchunks + c] = keys[k].values[c];
            RDF_TRY(shadow(*out_keys[k].values, gcodes[k], &ok[k]));
            continue;
        }
        const rdf_utf8_array* ch = keys[k].utf8;
        nullable[k] = utf8_nullable(ch, nchunks);
        int64_t bytes = 0;
        for (int64_t c = 0; c < nchunks; ++c) bytes += ch[c].data.length;
        RDF_TRY(codes[k].make(ch, nchunks, mem));
        RDF_TRY(doffs[k].alloc((size_t)(nrows + 1) * 4, mem));
        RDF_TRY(ddata[k].alloc((size_t)bytes + 8, mem));
        rdf_out o_off, o_dat;
        memset(&o_off, 0, sizeof o_off);
        memset(&o_dat, 0, sizeof o_dat);
        o_off.values = doffs[k].p; o_off.capacity = nrows + 1; o_off.dtype = RDF_I32; o_off.mem = mem;
        o_dat.values = ddata[k].p; o_dat.capacity = bytes + 8; o_dat.dtype = RDF_U8; o_dat.mem = mem;
        int64_t count = 0;
        RDF_TRY(rdf_utf8_dictionary_encode(ch, nchunks, codes[k].outs.data(), &o_off, &o_dat, &count));
        codes[k].finish(nullable[k]);
        for (int64_t c = 0; c < nchunks; ++c) flat[(size_t)k * nchunks + c] = codes[k].arrays[c];
        dict[k].offsets = rdf_array{o_off.values, nullptr, 0, o_off.length, 0, RDF_I32, mem};
        dict[k].data = rdf_array{o_dat.values, nullptr, 0, o_dat.length, 0, RDF_U8, mem};
        RDF_TRY(gcodes[k].alloc((size_t)cap_needed * 4 + 256 + vbits, mem));
        memset(&ok[k], 0, sizeof ok[k]);
        ok[k].values = gcodes[k].p;
        ok[k].validity = nullable[k] ? (uint8_t*)gcodes[k].p + (((size_t)cap_needed * 4 + 255) & ~(size_t)255) : nullptr;
        ok[k].capacity = cap_needed; ok[k].dtype = RDF_U32; ok[k].mem = mem;
    }
    DictBuf bvals[kGbmMaxCalls], bcnts[kGbmMaxCalls], brows;
    rdf_out tv[kGbmMaxCalls], tc[kGbmMaxCalls], tr;
    for (int c = 0; c < ncalls; ++c) { RDF_TRY(shadow(outs[c], bvals[c], &tv[c])); RDF_TRY(shadow(out_counts[c], bcnts[c], &tc[c])); }
    if (out_group_rows) RDF_TRY(shadow(*out_group_rows, brows, &tr));
    int64_t groups = 0;
    // (over Utf8 keys the NULL group and the code whose hash is the free marker never counted against max_groups: rdf_groupby_agg_keys' rule)
    RDF_TRY(groupby_multi_impl(flat.data(), nkeys, values, nvalues, nchunks, cp, ncalls, max_groups, mem, ok, tv, tc, out_group_rows ? &tr : nullptr, 2, &groups));
    const std::string gb_kernels = g_ctx.last_kernel;

    // ---- Utf8 key columns: the dictionary taken by the group codes (a NULL code gives a NULL row); sized first
    rdf_array gidx[kMaxKeyCols];
    bool fits = true;
    for (int k = 0; k < nkeys; ++k) {
        if (keys[k].values) continue;
        gidx[k] = rdf_array{ok[k].values, ok[k].validity, 0, groups, ok[k].validity ? ok[k].null_count : 0, RDF_U32, mem};
        RDF_TRY(toffs[k].alloc((size_t)(groups + 1) * 4 + (size_t)((groups + 63) / 64) * 8 + 256 + 8, mem));
        rdf_out to, td;
        memset(&to, 0, sizeof to);
        memset(&td, 0, sizeof td);
        to.values = toffs[k].p; to.validity = (uint8_t*)toffs[k].p + (((size_t)(groups + 1) * 4 + 255) & ~(size_t)255);
        to.capacity = groups + 1; to.dtype = RDF_I32; to.mem = mem;
        td.dtype = RDF_U8; td.mem = mem;
        const rdf_status st = rdf_utf8_take(&dict[k], 1, &gidx[k], &to, &td);
        if (st != RDF_OK && st != RDF_MEMORY_ERROR) return st;
        out_keys[k].utf8_offsets->length = groups + 1;
        out_keys[k].utf8_data->length = td.length;
        if (out_keys[k].utf8_offsets->capacity < groups + 1 || out_keys[k].utf8_data->capacity < td.length) fits = false;
    }
    if (!fits) return fail(RDF_MEMORY_ERROR, "%s: a Utf8 key output is too small (the needed lengths are in its length fields)", fn);
    for (int k = 0; k < nkeys; ++k)
        if (!keys[k].values) RDF_TRY(rdf_utf8_take(&dict[k], 1, &gidx[k], out_keys[k].utf8_offsets, out_keys[k].utf8_data));
    auto deliver = [&](const rdf_out& from, rdf_out* to) -> rdf_status {
        const size_t bytes = (size_t)groups * (size_t)dtype_size(from.dtype), nbits = (size_t)((groups + 7) / 8);
        if (mem == RDF_MEM_HOST) {
            if (bytes) memcpy(to->values, from.values, bytes);
            if (to->validity && from.validity && nbits) memcpy(to->validity, from.validity, nbits);
        } else {
            if (bytes) HIP_TRY(hipMemcpyAsync(to->values, from.values, bytes, hipMemcpyDeviceToDevice, g_ctx.stream));
            if (to->validity && from.validity && nbits) HIP_TRY(hipMemcpyAsync(to->validity, from.validity, nbits, hipMemcpyDeviceToDevice, g_ctx.stream));
        }
        to->length = from.length;
        to->null_count = from.null_count;
        return RDF_OK;
    };
    for (int c = 0; c < ncalls; ++c) { RDF_TRY(deliver(tv[c], &outs[c])); RDF_TRY(deliver(tc[c], &out_counts[c])); }
    if (out_group_rows) RDF_TRY(deliver(tr, out_group_rows));
    for (int k = 0; k < nkeys; ++k)
        if (keys[k].values) RDF_TRY(deliver(ok[k], out_keys[k].values));
    if (mem == RDF_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    *out_groups = groups;
    g_ctx.last_kernel = "cs_dict_codes_kernel + " + gb_kernels + " + utf8_span_kernel + utf8_copy_kernel";
    return RDF_OK;
}

}  // extern "C"
