// rdf_capi_colstats.inc — host side of Column::hist / Column::uniques (kernels: rdf_colstats.hip); textually included by
// rdf_capi.cpp (it uses that file's per-thread context, arena, staging helpers, the column aggregates, the sorts and the
// Utf8 take path).
//
//   rdf_hist          [min / max pass when no range is given] -> one counting pass -> edges computed here (cs_edge)
//   rdf_uniques       hash route: LDS set per block -> insert-only table in HBM -> emit; the table is sized from the rows,
//                     capped by the "uniques_table_bits" budget; when it gives up — or "uniques_route" 1 asks for it — the
//                     sort route: rdf_sort_to_indices' passes, first row of every run of equal keys kept
//   rdf_utf8_uniques  hash route: hash -> (hash, smallest row) table -> verify every row's bytes against its hash's
//                     representative; exact route (table full, a verify mismatch, or forced): rdf_lexsort_to_indices'
//                     order, neighbours compared.  Either way the representatives are gathered by the Utf8 take path.

namespace {

struct CsPoolBuf {   // a device buffer that outlives the arena resets of the entry points called in between
    void* p = nullptr;
    size_t got = 0;
    rdf_status alloc(size_t bytes) { return pool_alloc(bytes, &p, &got); }
    ~CsPoolBuf() { if (p) pool_release(p, got); }
};

// the chunks (and one more array, e.g. a row order) on the device, with the tile tables of rdf_colstats.hip
struct CsStaged {
    InputStager in;
    TableBuilder tb;
    CsCol col;
    const void* extra = nullptr;
};
rdf_status cs_stage(const rdf_array* chunks, int64_t nchunks, const rdf_array* extra, CsStaged& st) {
    for (int64_t c = 0; c < nchunks; ++c) st.in.add(&chunks[c]);
    if (extra) st.in.add(extra);
    size_t pin_off = 0, used = 0;
    RDF_TRY(st.in.finish(pin_off, &used));
    pin_off += (used + 255) & ~(size_t)255;
    const size_t o_ch = st.tb.reserve(sizeof(DevChunkCol) * (size_t)nchunks);
    const size_t o_rs = st.tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_ts = st.tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    RDF_TRY(st.tb.bind(pin_off));
    DevChunkCol* hch = st.tb.at<DevChunkCol>(o_ch);
    int64_t* hrs = st.tb.at<int64_t>(o_rs);
    int64_t* hts = st.tb.at<int64_t>(o_ts);
    hrs[0] = hts[0] = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        hch[c] = st.in.dev[(size_t)c];
        hrs[c + 1] = hrs[c] + chunks[c].length;
        hts[c + 1] = hts[c] + (chunks[c].length + kCsTile - 1) / kCsTile;
    }
    st.col.nchunks = nchunks;
    st.col.n = hrs[nchunks];
    st.col.ntiles = hts[nchunks];
    RDF_TRY(st.tb.alloc());
    RDF_TRY(st.tb.upload(pin_off));
    st.col.chunks = st.tb.dev_at<DevChunkCol>(o_ch);
    st.col.row_start = st.tb.dev_at<int64_t>(o_rs);
    st.col.tile_start = st.tb.dev_at<int64_t>(o_ts);
    if (extra) {
        const DevChunkCol& d = st.in.dev[(size_t)nchunks];
        st.extra = (const char*)d.values + (size_t)d.offset * (size_t)dtype_size(extra->dtype);
    }
    return RDF_OK;
}

// the counters of a distinct pass, zeroed / read back through the pinned buffer's first bytes
rdf_status cs_counters(unsigned long long** g) {
    void* p;
    RDF_TRY(arena_alloc(64, &p));
    HIP_TRY(hipMemsetAsync(p, 0, 64, g_ctx.stream));
    *g = (unsigned long long*)p;
    return RDF_OK;
}
rdf_status cs_read_counters(const unsigned long long* g, uint64_t (&h)[8]) {
    HIP_TRY(hipMemcpyAsync(h, g, 64, hipMemcpyDeviceToHost, g_ctx.stream));
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    return RDF_OK;
}

// slots of the insert-only table for a column of n rows: twice the rows (it is filled to half), within the budget
uint64_t cs_table_slots(int64_t n) {
    int bits = g_ctx.opt_uniques_table_bits;
    bits = bits < 10 ? 10 : (bits > 32 ? 32 : bits);
    uint64_t slots = 1024;
    while (slots < ((uint64_t)1 << bits) && slots < 2 * (uint64_t)n) slots <<= 1;
    return slots;
}

rdf_status cs_finish_values(rdf_out* out, int64_t count, int32_t mem) {
    if (out->validity && count > 0) {
        if (mem == RDF_MEM_HOST) memset(out->validity, 0xFF, (size_t)((count + 7) / 8));
        else HIP_TRY(hipMemsetAsync(out->validity, 0xFF, (size_t)((count + 7) / 8), g_ctx.stream));
    }
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    out->length = count;
    out->null_count = 0;
    return RDF_OK;
}

// the sort route of rdf_uniques
rdf_status cs_uniques_sorted(const rdf_array* chunks, int64_t nchunks, int64_t n, int32_t mem, rdf_out* out_values, int64_t* out_count) {
    Ctx& ctx = g_ctx;
    const bool is_f64 = chunks[0].dtype == RDF_F64;
    std::vector<uint32_t> hperm;
    CsPoolBuf dperm;
    rdf_out idx;
    memset(&idx, 0, sizeof idx);
    idx.capacity = n; idx.dtype = RDF_U32; idx.mem = mem;
    if (mem == RDF_MEM_HOST) { hperm.resize((size_t)n); idx.values = hperm.data(); }
    else { RDF_TRY(dperm.alloc((size_t)(n + 64) * 4)); idx.values = dperm.p; }
    const rdf_sort_options so{0, 0};
    RDF_TRY(rdf_sort_to_indices(chunks, 1, nchunks, &so, &idx));
    arena_begin();
    const rdf_array perm{idx.values, nullptr, 0, n, 0, RDF_U32, mem};
    CsStaged st;
    RDF_TRY(cs_stage(chunks, nchunks, &perm, st));
    CsRunArgs a;
    memset(&a, 0, sizeof a);
    a.col = st.col;
    a.is_f64 = is_f64;
    a.perm = (const uint32_t*)st.extra;
    RDF_TRY(cs_counters(&a.g));
    // a capacity of all rows always fits: one pass writes as it counts; else count first
    const bool direct = out_values && out_values->capacity >= n;
    void* stage_out = nullptr;
    if (direct && mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)(n + 1) * 8, &stage_out));
    a.out64 = direct ? (uint64_t*)(mem == RDF_MEM_HOST ? stage_out : out_values->values) : nullptr;
    ctx.last_kernel = "cs_runs_kernel";
    HIP_TRY(launch_cs_runs(a, ctx.stream));
    uint64_t g[8];
    RDF_TRY(cs_read_counters(a.g, g));
    const int64_t runs = (int64_t)g[CS_G_EMITTED];
    const int64_t count = runs + (g[CS_G_SPECIAL] ? 1 : 0);
    *out_count = count;
    if (!out_values) return RDF_OK;
    if (out_values->capacity < count) {
        out_values->length = count;
        return fail(RDF_MEMORY_ERROR, "uniques: %lld distinct values, capacity %lld", (long long)count, (long long)out_values->capacity);
    }
    if (!direct) {
        if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)(count + 1) * 8, &stage_out));
        a.out64 = (uint64_t*)(mem == RDF_MEM_HOST ? stage_out : out_values->values);
        HIP_TRY(hipMemsetAsync(a.g, 0, 64, ctx.stream));
        HIP_TRY(launch_cs_runs(a, ctx.stream));
    }
    const uint64_t nan = 0x7FF8000000000000ull;
    if (g[CS_G_SPECIAL]) HIP_TRY(hipMemcpyAsync(a.out64 + runs, &nan, 8, hipMemcpyHostToDevice, ctx.stream));
    if (mem == RDF_MEM_HOST && count > 0) HIP_TRY(hipMemcpyAsync(out_values->values, stage_out, (size_t)count * 8, hipMemcpyDeviceToHost, ctx.stream));
    return cs_finish_values(out_values, count, mem);
}

// ---- Utf8: the chunks (and a row order) on the device as a Utf8Chunk table
struct CsUtf8Staged {
    std::vector<rdf_array> views;
    InputStager in;
    const Utf8Chunk* d_chunks = nullptr;
    const void* extra = nullptr;
};
rdf_status cs_utf8_stage(const rdf_utf8_array* chunks, int64_t nchunks, int32_t mem, const rdf_array* extra, CsUtf8Staged& st) {
    Ctx& ctx = g_ctx;
    std::vector<int32_t> lohi;
    RDF_TRY(utf8_value_ranges(chunks, nchunks, mem, lohi, "utf8_uniques"));
    st.views.reserve((size_t)nchunks * 3 + 1);
    std::vector<int> vi((size_t)nchunks * 3, -1);
    for (int64_t i = 0; i < nchunks; ++i) {
        const rdf_utf8_array& c = chunks[i];
        const int64_t rows = c.offsets.length - 1;
        rdf_array offs = c.offsets;
        offs.validity = nullptr; offs.null_count = 0;
        st.views.push_back(offs); vi[3 * i] = (int)st.views.size() - 1;
        if (c.offsets.validity) {
            st.views.push_back(rdf_array{c.offsets.validity, nullptr, c.offsets.offset, rows, 0, RDF_BOOL, c.offsets.mem});
            vi[3 * i + 1] = (int)st.views.size() - 1;
        }
        st.views.push_back(rdf_array{c.data.values, nullptr, c.data.offset + lohi[2 * i], (int64_t)lohi[2 * i + 1] - lohi[2 * i], 0, RDF_U8, c.data.mem});
        vi[3 * i + 2] = (int)st.views.size() - 1;
    }
    int xv = -1;
    if (extra) { st.views.push_back(*extra); xv = (int)st.views.size() - 1; }
    for (const rdf_array& v : st.views) st.in.add(&v);
    size_t used = 0;
    RDF_TRY(st.in.finish(0, &used));
    const size_t pin = (used + 255) & ~(size_t)255;
    const size_t tb = (size_t)nchunks * sizeof(Utf8Chunk);
    RDF_TRY(pinned_reserve(pin + tb + 64));
    Utf8Chunk* hc = (Utf8Chunk*)(ctx.pinned + pin);
    int64_t row_start = 0;
    for (int64_t i = 0; i < nchunks; ++i) {
        Utf8Chunk& u = hc[i];
        memset(&u, 0, sizeof u);
        const DevChunkCol& d_off = st.in.dev[vi[3 * i]];
        u.offs = (const int32_t*)d_off.values + d_off.offset;
        if (vi[3 * i + 1] >= 0) { u.valid = (const uint8_t*)st.in.dev[vi[3 * i + 1]].values; u.valid_off = st.in.dev[vi[3 * i + 1]].offset; }
        const DevChunkCol& d_dat = st.in.dev[vi[3 * i + 2]];
        u.data = (const uint8_t*)d_dat.values + d_dat.offset - lohi[2 * i];
        u.rows = chunks[i].offsets.length - 1;
        u.row_start = row_start;
        row_start += u.rows;
        u.lo = lohi[2 * i]; u.hi = lohi[2 * i + 1];
    }
    void* dtab;
    RDF_TRY(arena_alloc(tb, &dtab));
    HIP_TRY(hipMemcpyAsync(dtab, hc, tb, hipMemcpyHostToDevice, ctx.stream));
    st.d_chunks = (const Utf8Chunk*)dtab;
    if (extra) {
        const DevChunkCol& d = st.in.dev[xv];
        st.extra = (const char*)d.values + (size_t)d.offset * (size_t)dtype_size(extra->dtype);
    }
    return RDF_OK;
}

// an empty result: one offset, no bytes
rdf_status cs_utf8_empty(rdf_out* out_offsets, rdf_out* out_data, int32_t mem) {
    if (mem == RDF_MEM_HOST) *(int32_t*)out_offsets->values = 0;
    else {
        HIP_TRY(hipMemsetAsync(out_offsets->values, 0, 4, g_ctx.stream));
        HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    }
    out_offsets->length = 1; out_offsets->null_count = 0;
    out_data->length = 0; out_data->null_count = 0;
    return RDF_OK;
}

// rows -> their strings, through the take path.  The rows are valid ones: the chunks go in without their validity, so the
// output needs no validity buffer.
rdf_status cs_utf8_gather(const rdf_utf8_array* chunks, int64_t nchunks, int32_t mem, const uint32_t* d_rows, int64_t count,
                          rdf_out* out_offsets, rdf_out* out_data) {
    std::vector<rdf_utf8_array> plain(chunks, chunks + nchunks);
    for (auto& c : plain) { c.offsets.validity = nullptr; c.offsets.null_count = 0; }
    std::vector<uint32_t> hrows;
    rdf_array idx{d_rows, nullptr, 0, count, 0, RDF_U32, mem};
    if (mem == RDF_MEM_HOST) {
        hrows.resize((size_t)count);
        HIP_TRY(hipMemcpyAsync(hrows.data(), d_rows, (size_t)count * 4, hipMemcpyDeviceToHost, g_ctx.stream));
        HIP_TRY(hipStreamSynchronize(g_ctx.stream));
        idx.values = hrows.data();
    }
    return utf8_run(UTF8_TAKE, plain.data(), nchunks, nullptr, &idx, 0, 0, out_offsets, out_data, "utf8_uniques");
}

}  // namespace

extern "C" {

rdf_status rdf_hist(const rdf_array* chunks, int64_t nchunks, int64_t nbins, const double* range, rdf_out* out_counts,
                    rdf_out* out_edges, int64_t* out_counted) {
    if (nchunks < 0 || (nchunks > 0 && !chunks)) return fail(RDF_INVALID_ARGUMENT, "hist: bad chunk list");
    if (!out_counts || !out_edges || !out_counted) return fail(RDF_INVALID_ARGUMENT, "hist: null output");
    for (int64_t c = 0; c < nchunks; ++c)
        if ((chunks[c].dtype != RDF_I64 && chunks[c].dtype != RDF_F64) || chunks[c].dtype != chunks[0].dtype)
            return fail(RDF_INVALID_ARGUMENT, "Unsupported type for histogram (Int64 and Float64 columns only)");   // src/table.rs:288
    if (nbins < 1 || nbins > ((int64_t)1 << 24)) return fail(RDF_INVALID_ARGUMENT, "hist: 1 <= nbins <= 2^24");
    if (range && !(std::isfinite(range[0]) && std::isfinite(range[1]) && range[0] <= range[1]))
        return fail(RDF_INVALID_ARGUMENT, "hist: range must be finite with lo <= hi");
    if (range && !std::isfinite(range[1] - range[0])) return fail(RDF_INVALID_ARGUMENT, "hist: range is wider than a double");
    int32_t mem = -1;
    RDF_TRY(check_mem(chunks, nchunks, &mem));
    if (mem < 0) mem = out_counts->mem;
    RDF_TRY(check_out_mem(out_counts, 1, mem));
    RDF_TRY(check_out_mem(out_edges, 1, mem));
    if (out_counts->dtype != RDF_I64 || out_edges->dtype != RDF_F64) return fail(RDF_INVALID_ARGUMENT, "hist: counts are Int64, edges Float64");
    if (out_counts->capacity < nbins || out_edges->capacity < nbins + 1) {
        out_counts->length = nbins;
        out_edges->length = nbins + 1;
        return fail(RDF_MEMORY_ERROR, "hist: %lld counts and %lld edges needed", (long long)nbins, (long long)nbins + 1);
    }
    if (!out_counts->values || !out_edges->values) return fail(RDF_INVALID_ARGUMENT, "hist: null output buffer");
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    int64_t n = 0;
    for (int64_t c = 0; c < nchunks; ++c) n += chunks[c].length;
    const bool is_int = nchunks > 0 && chunks[0].dtype == RDF_I64;

    double lo = 0.0, hi = 1.0;
    if (range) { lo = range[0]; hi = range[1]; }
    else if (n > 0) {   // the library's own min / max: NaN does not win, NULLs are skipped
        rdf_agg_result r;
        RDF_TRY(agg_column(chunks, nchunks, false, &r));
        if (r.is_some) {
            const double mn = is_int ? (double)r.min_i64 : r.min_f64, mx = is_int ? (double)r.max_i64 : r.max_f64;
            if (mn == mn && mx == mx) {
                if (!std::isfinite(mn) || !std::isfinite(mx)) return fail(RDF_COMPUTE_ERROR, "hist: range is not finite (%g, %g)", mn, mx);
                if (!std::isfinite(mx - mn)) return fail(RDF_COMPUTE_ERROR, "hist: range is wider than a double");
                lo = mn; hi = mx;
            }
        }
    }
    if (lo == hi) { lo -= 0.5; hi += 0.5; }
    const double step = (hi - lo) / (double)nbins;

    arena_begin();
    CsStaged st;
    RDF_TRY(cs_stage(chunks, nchunks, nullptr, st));
    CsHistArgs a;
    memset(&a, 0, sizeof a);
    a.col = st.col;
    a.is_int = is_int;
    a.peels = nbins <= 64 ? 8 : 2;
    a.lo = lo; a.hi = hi; a.step = step;
    a.scale = (double)nbins / (hi - lo);
    a.nbins = nbins;
    void *dcounted, *dcounts = out_counts->values;
    RDF_TRY(arena_alloc(8, &dcounted));
    if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)nbins * 8, &dcounts));
    HIP_TRY(hipMemsetAsync(dcounted, 0, 8, ctx.stream));
    HIP_TRY(hipMemsetAsync(dcounts, 0, (size_t)nbins * 8, ctx.stream));
    a.counts = (unsigned long long*)dcounts;
    a.counted = (unsigned long long*)dcounted;
    KernelTimer kt;
    ctx.last_kernel = "cs_hist_kernel";
    HIP_TRY(launch_cs_hist(a, ctx.stream));
    kt.stop();
    std::vector<double> edges((size_t)nbins + 1);
    for (int64_t i = 0; i <= nbins; ++i) edges[(size_t)i] = cs_edge(lo, hi, step, nbins, i);
    uint64_t counted = 0;
    HIP_TRY(hipMemcpyAsync(&counted, dcounted, 8, hipMemcpyDeviceToHost, ctx.stream));
    if (mem == RDF_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out_counts->values, dcounts, (size_t)nbins * 8, hipMemcpyDeviceToHost, ctx.stream));
        memcpy(out_edges->values, edges.data(), edges.size() * 8);
        if (out_counts->validity) memset(out_counts->validity, 0xFF, (size_t)((nbins + 7) / 8));
        if (out_edges->validity) memset(out_edges->validity, 0xFF, (size_t)((nbins + 8) / 8));
    } else {
        HIP_TRY(hipMemcpyAsync(out_edges->values, edges.data(), edges.size() * 8, hipMemcpyHostToDevice, ctx.stream));
        if (out_counts->validity) HIP_TRY(hipMemsetAsync(out_counts->validity, 0xFF, (size_t)((nbins + 7) / 8), ctx.stream));
        if (out_edges->validity) HIP_TRY(hipMemsetAsync(out_edges->validity, 0xFF, (size_t)((nbins + 8) / 8), ctx.stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    out_counts->length = nbins; out_counts->null_count = 0;
    out_edges->length = nbins + 1; out_edges->null_count = 0;
    *out_counted = (int64_t)counted;
    return RDF_OK;
}

rdf_status rdf_uniques(const rdf_array* chunks, int64_t nchunks, rdf_out* out_values, int64_t* out_count) {
    if (nchunks < 0 || (nchunks > 0 && !chunks)) return fail(RDF_INVALID_ARGUMENT, "uniques: bad chunk list");
    if (!out_count) return fail(RDF_INVALID_ARGUMENT, "uniques: null count pointer");
    *out_count = 0;
    for (int64_t c = 0; c < nchunks; ++c)
        if ((chunks[c].dtype != RDF_I64 && chunks[c].dtype != RDF_U64 && chunks[c].dtype != RDF_F64) || chunks[c].dtype != chunks[0].dtype)
            return fail(RDF_INVALID_ARGUMENT, "Datatype not supported for uniques (Int64, UInt64 and Float64 columns; Utf8: rdf_utf8_uniques)");   // src/table.rs:339
    int32_t mem = -1;
    RDF_TRY(check_mem(chunks, nchunks, &mem));
    if (out_values) {
        if (mem >= 0) RDF_TRY(check_out_mem(out_values, 1, mem));
        else mem = out_values->mem;
        if (nchunks > 0 && out_values->dtype != chunks[0].dtype) return fail(RDF_INVALID_ARGUMENT, "uniques: the output has the input's dtype");
        if (out_values->capacity < 0 || (out_values->capacity > 0 && !out_values->values)) return fail(RDF_INVALID_ARGUMENT, "uniques: capacity without a buffer");
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    int64_t n = 0;
    for (int64_t c = 0; c < nchunks; ++c) n += chunks[c].length;
    if (n == 0) {
        if (out_values) { out_values->length = 0; out_values->null_count = 0; }
        return RDF_OK;
    }
    if (ctx.opt_uniques_route == 1) return cs_uniques_sorted(chunks, nchunks, n, mem, out_values, out_count);

    arena_begin();
    CsStaged st;
    RDF_TRY(cs_stage(chunks, nchunks, nullptr, st));
    const uint64_t slots = cs_table_slots(n);
    CsSetArgs a;
    memset(&a, 0, sizeof a);
    a.col = st.col;
    a.is_f64 = chunks[0].dtype == RDF_F64;
    a.mask = slots - 1;
    a.max_fill = slots / 2;
    void* ptab;
    RDF_TRY(arena_alloc((size_t)slots * 8, &ptab));
    a.table = (uint64_t*)ptab;
    RDF_TRY(cs_counters(&a.g));
    KernelTimer kt;
    ctx.last_kernel = "cs_distinct_kernel";
    HIP_TRY(launch_cs_fill64(a.table, (int64_t)slots, kCsEmpty, ctx.stream));
    HIP_TRY(launch_cs_distinct(a, ctx.stream));
    kt.stop();
    uint64_t g[8];
    RDF_TRY(cs_read_counters(a.g, g));
    if (g[CS_G_OVERFLOW]) return cs_uniques_sorted(chunks, nchunks, n, mem, out_values, out_count);   // more keys than the table was sized for
    const int64_t keys = (int64_t)g[CS_G_COUNT];
    const int64_t count = keys + (g[CS_G_SPECIAL] ? 1 : 0);
    *out_count = count;
    if (!out_values) return RDF_OK;
    if (out_values->capacity < count) {
        out_values->length = count;
        return fail(RDF_MEMORY_ERROR, "uniques: %lld distinct values, capacity %lld", (long long)count, (long long)out_values->capacity);
    }
    void* dout = out_values->values;
    if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)(count + 1) * 8, &dout));
    a.out64 = (uint64_t*)dout;
    HIP_TRY(launch_cs_emit(a, ctx.stream));
    const uint64_t special = kCsEmpty;   // the one key the table cannot hold travels as a flag
    if (g[CS_G_SPECIAL]) HIP_TRY(hipMemcpyAsync(a.out64 + keys, &special, 8, hipMemcpyHostToDevice, ctx.stream));
    if (mem == RDF_MEM_HOST && count > 0) HIP_TRY(hipMemcpyAsync(out_values->values, dout, (size_t)count * 8, hipMemcpyDeviceToHost, ctx.stream));
    return cs_finish_values(out_values, count, mem);
}

rdf_status rdf_utf8_uniques(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data, int64_t* out_count) {
    const char* fn = "utf8_uniques";
    if (nchunks < 0 || (nchunks > 0 && !chunks)) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk list", fn);
    if (!out_count || !out_offsets || !out_data) return fail(RDF_INVALID_ARGUMENT, "%s: null output", fn);
    *out_count = 0;
    int32_t mem = -1;
    int64_t n = 0;
    for (int64_t i = 0; i < nchunks; ++i) {
        const rdf_utf8_array& c = chunks[i];
        if (c.offsets.dtype != RDF_I32 || c.offsets.length < 1)
            return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: offsets must be an Int32 array of rows + 1 entries", fn, (long long)i);
        if (c.data.dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: data must be a UInt8 array", fn, (long long)i);
        RDF_TRY(check_mem(&c.offsets, 1, &mem));
        RDF_TRY(check_mem(&c.data, 1, &mem));
        n += c.offsets.length - 1;
    }
    if (out_offsets->dtype != RDF_I32 || out_data->dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: outputs are (Int32 offsets, UInt8 data)", fn);
    if (mem < 0) mem = out_offsets->mem;
    RDF_TRY(check_out_mem(out_offsets, 1, mem));
    RDF_TRY(check_out_mem(out_data, 1, mem));
    if (!out_offsets->values || out_offsets->capacity < 1) return fail(RDF_INVALID_ARGUMENT, "%s: the output has no offsets buffer", fn);
    if (out_data->capacity < 0 || (out_data->capacity > 0 && !out_data->values)) return fail(RDF_INVALID_ARGUMENT, "%s: data capacity without a buffer", fn);
    if (n >= (int64_t)1 << 32) return fail(RDF_INVALID_ARGUMENT, "%s: a column holds at most 2^32-1 rows (src/table.rs:218)", fn);
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    if (n == 0) return cs_utf8_empty(out_offsets, out_data, mem);

    CsPoolBuf rows;     // the representative row of every distinct value
    int64_t count = -1;
    if (ctx.opt_uniques_route != 1) {
        arena_begin();
        CsUtf8Staged st;
        RDF_TRY(cs_utf8_stage(chunks, nchunks, mem, nullptr, st));
        const uint64_t slots = cs_table_slots(n);
        CsUtf8Args a;
        memset(&a, 0, sizeof a);
        a.chunks = st.d_chunks; a.nchunks = nchunks; a.n = n;
        a.set.mask = slots - 1;
        a.set.max_fill = slots / 2;
        void *ptab, *prep, *phash;
        RDF_TRY(arena_alloc((size_t)slots * 8, &ptab));
        RDF_TRY(arena_alloc((size_t)slots * 4, &prep));
        RDF_TRY(arena_alloc((size_t)n * 8, &phash));
        a.set.table = (uint64_t*)ptab; a.set.rep = (uint32_t*)prep; a.hash = (uint64_t*)phash;
        RDF_TRY(cs_counters(&a.set.g));
        KernelTimer kt;
        ctx.last_kernel = "cs_utf8_hash_kernel + cs_utf8_verify_kernel";
        HIP_TRY(launch_cs_fill64(a.set.table, (int64_t)slots, kCsEmpty, ctx.stream));
        HIP_TRY(hipMemsetAsync(prep, 0xFF, (size_t)slots * 4, ctx.stream));
        HIP_TRY(launch_cs_utf8_hash(a, ctx.stream));
        HIP_TRY(launch_cs_utf8_verify(a, ctx.stream));   // (a table that gave up leaves rows without a slot: a mismatch)
        kt.stop();
        uint64_t g[8];
        RDF_TRY(cs_read_counters(a.set.g, g));
        if (!g[CS_G_OVERFLOW] && !g[CS_G_MISMATCH]) {
            count = (int64_t)g[CS_G_COUNT];
            if (count > 0) {
                RDF_TRY(rows.alloc((size_t)(count + 64) * 4));
                a.set.out32 = (uint32_t*)rows.p;
                HIP_TRY(launch_cs_emit(a.set, ctx.stream));
                HIP_TRY(hipStreamSynchronize(ctx.stream));
            }
        }
    }
    if (count < 0) {   // the exact route: sorted order, neighbours compared
        std::vector<uint32_t> hperm;
        CsPoolBuf dperm;
        rdf_out idx;
        memset(&idx, 0, sizeof idx);
        idx.capacity = n; idx.dtype = RDF_U32; idx.mem = mem;
        if (mem == RDF_MEM_HOST) { hperm.resize((size_t)n); idx.values = hperm.data(); }
        else { RDF_TRY(dperm.alloc((size_t)(n + 64) * 4)); idx.values = dperm.p; }
        rdf_sort_key key;
        memset(&key, 0, sizeof key);
        key.utf8 = chunks;
        RDF_TRY(rdf_lexsort_to_indices(&key, 1, nchunks, &idx));
        arena_begin();
        const rdf_array perm{idx.values, nullptr, 0, n, 0, RDF_U32, mem};
        CsUtf8Staged st;
        RDF_TRY(cs_utf8_stage(chunks, nchunks, mem, &perm, st));
        CsUtf8Args a;
        memset(&a, 0, sizeof a);
        a.chunks = st.d_chunks; a.nchunks = nchunks; a.n = n;
        a.perm = (const uint32_t*)st.extra;
        RDF_TRY(cs_counters(&a.set.g));
        RDF_TRY(rows.alloc((size_t)(n + 64) * 4));
        a.out32 = (uint32_t*)rows.p;
        ctx.last_kernel = "cs_utf8_runs_kernel";
        HIP_TRY(launch_cs_utf8_runs(a, ctx.stream));
        uint64_t g[8];
        RDF_TRY(cs_read_counters(a.set.g, g));
        count = (int64_t)g[CS_G_EMITTED];
    }
    *out_count = count;
    if (count == 0) return cs_utf8_empty(out_offsets, out_data, mem);
    const std::string route = ctx.last_kernel;
    const rdf_status st = cs_utf8_gather(chunks, nchunks, mem, (const uint32_t*)rows.p, count, out_offsets, out_data);
    ctx.last_kernel = route + " + utf8_span_kernel + utf8_copy_kernel";
    return st;
}

}  // extern "C"
