// rdf_capi_sort_utf8.inc — host side of rdf_lexsort_to_indices: DataFrame::sort whose criteria may be Utf8 columns
// (kernels: rdf_utf8_sort.hip); textually included by rdf_capi.cpp (it uses that file's context, arena, staging helpers,
// sort_core and the radix passes of the numeric sort).
//
// A Utf8 criterion takes its place in sort_core's LSD loop over the criteria as a stable refinement of the current order:
// round 0 sorts every row on its first 7 bytes (plus end code), every later round only the rows still tied with a
// neighbour, on the next 7 bytes past the prefix their segment shares.  See rdf_utf8.h for the round's data.

namespace {

rdf_status utf8_sort_column(const Utf8SortCol& col, OsScratch& os, uint64_t* const keys[2], uint32_t* const idxb[2], uint8_t* nullflags,
                            int64_t n, int descending, size_t pin_off, const uint32_t*& idx_cur) {
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    // scratch: a fixed number of words per row, whatever the lengths of the strings
    const int64_t nseg_max = n / 2 + 1;   // a segment of a later round holds >= 2 rows
    void *pperm, *pword, *ptrow, *ptword, *ptseg, *ptnull, *pfu, *pfh, *psu, *psh, *pslcp, *pstats;
    void *pupos[2], *puseg[2], *psdepth[2], *psfirst[2];
    RDF_TRY(arena_alloc((size_t)n * 4, &pperm));
    RDF_TRY(arena_alloc((size_t)n * 8, &pword));
    RDF_TRY(arena_alloc((size_t)n * 4, &ptrow));
    RDF_TRY(arena_alloc((size_t)n * 8, &ptword));
    RDF_TRY(arena_alloc((size_t)n * 4, &ptseg));
    RDF_TRY(arena_alloc((size_t)n, &ptnull));
    RDF_TRY(arena_alloc((size_t)n * 8, &pfu));
    RDF_TRY(arena_alloc((size_t)n * 8, &pfh));
    RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &psu));
    RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &psh));
    RDF_TRY(arena_alloc((size_t)nseg_max * 4, &pslcp));
    RDF_TRY(arena_alloc(64, &pstats));
    for (int i = 0; i < 2; ++i) {
        RDF_TRY(arena_alloc((size_t)n * 4, &pupos[i]));
        RDF_TRY(arena_alloc((size_t)n * 4, &puseg[i]));
        RDF_TRY(arena_alloc((size_t)nseg_max * 4, &psdepth[i]));
        RDF_TRY(arena_alloc((size_t)nseg_max * 4, &psfirst[i]));
    }
    uint64_t* stats = (uint64_t*)pstats;
    Utf8SortArgs a;
    memset(&a, 0, sizeof a);
    a.chunks = col.d_chunks;
    a.nchunks = col.nchunks;
    a.n = n;
    a.descending = descending ? 1 : 0;
    a.perm = (uint32_t*)pperm;
    a.order_in = idx_cur;
    a.word = (uint64_t*)pword;
    a.bit_stats = stats;
    a.trow = (uint32_t*)ptrow; a.tword = (uint64_t*)ptword; a.tseg = (uint32_t*)ptseg; a.tnull = (uint8_t*)ptnull;
    a.fu = (int64_t*)pfu; a.fh = (int64_t*)pfh; a.su = (const int64_t*)psu; a.sh = (const int64_t*)psh;
    a.slcp = (int32_t*)pslcp;
    HIP_TRY(launch_utf8_sort_init(a, s));   // the criterion's order starts as the incoming one

    static const bool dbg = getenv("RDF_DEBUG_SORT") != nullptr;
    const int64_t tiles_full = os.ntiles;
    RDF_TRY(pinned_reserve(pin_off + 64));
    int64_t m = n, nseg = 1;
    int cur = 0;
    for (int round = 0;; ++round) {
        a.round0 = round == 0;
        a.m = m;
        a.nseg = nseg;
        a.upos = round ? (const uint32_t*)pupos[cur] : nullptr;
        a.useg = round ? (const uint32_t*)puseg[cur] : nullptr;
        a.sdepth = (int32_t*)psdepth[cur];
        a.sfirst = (const uint32_t*)psfirst[cur];
        a.nullflags = round == 0 && col.nullable ? nullflags : nullptr;
        a.order = nullptr;
        if (round) HIP_TRY(launch_utf8_sort_lcp(a, s));   // each segment's depth jumps past the prefix its rows share
        RDF_TRY(sort_stats_reset(stats));
        a.keys = keys[0];
        HIP_TRY(launch_utf8_sort_keys(a, s));
        uint64_t bias = 0, kmax = 0;
        int need = 0;
        RDF_TRY(sort_key_range(stats, pin_off, &bias, &need, &kmax));
        // the digit passes over the round's m rows (the scratch was sized for n; seq restarts well before it wraps)
        if (os.state && os.seq > 15000) { HIP_TRY(hipMemsetAsync(os.state, 0, (size_t)tiles_full * 256 * 8, s)); os.seq = 0; }
        os.ntiles = (m + os_tile_items() - 1) / os_tile_items();
        int kc = 0, ic = 1;
        const uint32_t* ord = nullptr;
        rdf_status st = os_column_passes(os, keys, idxb, nullflags, m, bias, need, a.nullflags != nullptr, kc, ic, ord, kmax >= bias ? kmax - bias : ~0ull);
        if (st == RDF_OK && round && nseg > 1) {   // stable by segment over the word order: segments stay where they were
            a.order = ord;
            a.keys = keys[kc];
            if (launch_utf8_sort_seg_keys(a, s) != hipSuccess) st = fail(RDF_DEVICE_ERROR, "utf8 sort: segment keys launch failed");
            int need2 = 0;
            for (uint64_t r = (uint64_t)(nseg - 1); r; r >>= 8) ++need2;
            if (st == RDF_OK) st = os_column_passes(os, keys, idxb, nullptr, m, 0, need2, false, kc, ic, ord, (uint64_t)(nseg - 1));
        }
        os.ntiles = tiles_full;
        RDF_TRY(st);
        a.order = ord;
        HIP_TRY(launch_utf8_sort_mark(a, s));
        HIP_TRY(launch_scan(a.fu, (int64_t*)psu, m, (int64_t*)psu + m + 1, s));
        HIP_TRY(launch_scan(a.fh, (int64_t*)psh, m, (int64_t*)psh + m + 1, s));
        HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + 16, (int64_t*)psu + m, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + 24, (int64_t*)psh + m, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        int64_t m2 = 0, nseg2 = 0;
        memcpy(&m2, ctx.pinned + pin_off + 16, 8);
        memcpy(&nseg2, ctx.pinned + pin_off + 24, 8);
        ++ctx.utf8_sort_rounds;
        if (dbg) fprintf(stderr, "[rdf] utf8 sort: round %d: %lld rows in %lld segments, %d key bytes -> %lld rows in %lld segments go on\n",
                         round, (long long)m, (long long)nseg, need, (long long)m2, (long long)nseg2);
        if (m2 <= 0) break;
        if (m2 > m || nseg2 > nseg_max) return fail(RDF_COMPUTE_ERROR, "internal: utf8 sort rounds do not shrink");
        a.nupos = (uint32_t*)pupos[cur ^ 1];
        a.nuseg = (uint32_t*)puseg[cur ^ 1];
        a.nsdepth = (int32_t*)psdepth[cur ^ 1];
        a.nsfirst = (uint32_t*)psfirst[cur ^ 1];
        HIP_TRY(launch_utf8_sort_next(a, s));
        cur ^= 1;
        m = m2;
        nseg = nseg2;
    }
    idx_cur = a.perm;
    return RDF_OK;
}

// The criteria of a lexsort on the device (host arrays staged, device arrays aliased) and their descriptor tables: d_chunks
// [k * nchunks + c] for the numeric criteria, Utf8Chunk [k * nchunks + c] for the Utf8 ones, the prefix of the batch lengths.
// Shared by rdf_lexsort_to_indices and rdf_window.  pin_off: the first free byte of the pinned staging buffer afterwards.
struct LexKeysOnDevice {
    TableBuilder tb;
    size_t o_ch = 0, o_rs = 0, o_u8 = 0;
    int dts[kMaxFrameCols];
    bool nullable[kMaxFrameCols];
    Utf8SortCol ucols[kMaxFrameCols];
};
rdf_status lexsort_keys_to_device(const rdf_sort_key* keys, int nkeys, int64_t nchunks, int32_t mem, const std::vector<int64_t>& row_start,
                                  const char* fn, size_t& pin_off, LexKeysOnDevice& d) {
    auto rows_of = [&](int k, int64_t c) { return keys[k].values ? keys[k].values[c].length : keys[k].utf8[c].offsets.length - 1; };
    // ---- every Utf8 chunk's value-offset range, checked against its data array before a byte of it is read
    std::vector<std::vector<int32_t>> lohi((size_t)nkeys);
    for (int k = 0; k < nkeys; ++k)
        if (keys[k].utf8) RDF_TRY(utf8_value_ranges(keys[k].utf8, nchunks, mem, lohi[k], fn));

    // ---- inputs on the device (host arrays staged, device arrays aliased): numeric chunks, then per Utf8 chunk its
    // offsets, validity (a bitmap of `rows` bits) and the bytes of its value range
    std::vector<rdf_array> views;
    views.reserve((size_t)nkeys * nchunks * 3);
    std::vector<int> vi((size_t)nkeys * nchunks * 3, -1);
    for (int k = 0; k < nkeys; ++k)
        for (int64_t c = 0; c < nchunks; ++c) {
            const size_t e = ((size_t)k * nchunks + c) * 3;
            if (keys[k].values) { views.push_back(keys[k].values[c]); vi[e] = (int)views.size() - 1; continue; }
            const rdf_utf8_array& u = keys[k].utf8[c];
            const int64_t rows = u.offsets.length - 1;
            rdf_array offs = u.offsets;
            offs.validity = nullptr; offs.null_count = 0;
            views.push_back(offs); vi[e] = (int)views.size() - 1;
            if (u.offsets.validity) {
                views.push_back(rdf_array{u.offsets.validity, nullptr, u.offsets.offset, rows, 0, RDF_BOOL, u.offsets.mem});
                vi[e + 1] = (int)views.size() - 1;
            }
            const int32_t lo = lohi[k][2 * c], hi = lohi[k][2 * c + 1];
            views.push_back(rdf_array{u.data.values, nullptr, u.data.offset + lo, (int64_t)hi - lo, 0, RDF_U8, u.data.mem});
            vi[e + 2] = (int)views.size() - 1;
        }
    InputStager in;
    for (const rdf_array& v : views) in.add(&v);
    size_t used = 0;
    pin_off = 0;
    RDF_TRY(in.finish(pin_off, &used));
    pin_off += (used + 255) & ~(size_t)255;

    TableBuilder& tb = d.tb;
    d.o_ch = tb.reserve(sizeof(DevChunkCol) * (size_t)nkeys * nchunks);
    d.o_rs = tb.reserve(sizeof(int64_t) * row_start.size());
    d.o_u8 = tb.reserve(sizeof(Utf8Chunk) * (size_t)nkeys * nchunks);
    RDF_TRY(tb.bind(pin_off));
    DevChunkCol* hch = tb.at<DevChunkCol>(d.o_ch);
    Utf8Chunk* hu8 = tb.at<Utf8Chunk>(d.o_u8);
    memset(hch, 0, sizeof(DevChunkCol) * (size_t)nkeys * nchunks);
    memset(hu8, 0, sizeof(Utf8Chunk) * (size_t)nkeys * nchunks);
    memcpy(tb.at<char>(d.o_rs), row_start.data(), sizeof(int64_t) * row_start.size());
    for (int k = 0; k < nkeys; ++k) {
        d.dts[k] = keys[k].values ? keys[k].values[0].dtype : RDF_U8;
        d.nullable[k] = false;
        d.ucols[k] = Utf8SortCol{nullptr, nchunks, false};
        for (int64_t c = 0; c < nchunks; ++c) {
            const size_t i = (size_t)k * nchunks + c, e = i * 3;
            if (keys[k].values) {
                hch[i] = in.dev[vi[e]];
                d.nullable[k] |= keys[k].values[c].validity != nullptr;
                continue;
            }
            Utf8Chunk& u = hu8[i];
            const DevChunkCol& d_off = in.dev[vi[e]];
            u.offs = (const int32_t*)d_off.values + d_off.offset;
            if (vi[e + 1] >= 0) { u.valid = (const uint8_t*)in.dev[vi[e + 1]].values; u.valid_off = in.dev[vi[e + 1]].offset; d.ucols[k].nullable = true; }
            const DevChunkCol& d_dat = in.dev[vi[e + 2]];
            u.lo = lohi[k][2 * c];
            u.hi = lohi[k][2 * c + 1];
            u.data = (const uint8_t*)d_dat.values + d_dat.offset - u.lo;   // data[o] = the byte at value offset o
            u.rows = rows_of(k, c);
            u.row_start = row_start[(size_t)c];
        }
    }
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(pin_off));
    for (int k = 0; k < nkeys; ++k)
        if (keys[k].utf8) d.ucols[k].d_chunks = tb.dev_at<Utf8Chunk>(d.o_u8) + (size_t)k * nchunks;
    pin_off += (tb.size + 255) & ~(size_t)255;
    return RDF_OK;
}

// What a list of sort criteria must satisfy, for rdf_lexsort_to_indices and rdf_window alike (`fn` names the caller in the
// message): exactly one of values / utf8 per key, numeric chunks of one dtype, Int32 offsets and UInt8 data, one memory space.
rdf_status lexsort_check_keys(const rdf_sort_key* keys, int nkeys, int64_t nchunks, const char* fn, int32_t* mem, bool* any_utf8) {
    for (int k = 0; k < nkeys; ++k) {
        const rdf_sort_key& key = keys[k];
        if ((key.values != nullptr) == (key.utf8 != nullptr)) return fail(RDF_INVALID_ARGUMENT, "%s: key %d must set exactly one of values / utf8", fn, k);
        if (key.values) {
            RDF_TRY(check_mem(key.values, nchunks, mem));
            for (int64_t c = 0; c < nchunks; ++c)
                if (!is_numeric(key.values[c].dtype) || key.values[c].dtype != key.values[0].dtype)
                    return fail(RDF_INVALID_ARGUMENT, "%s: key %d: numeric chunks of one dtype", fn, k);
        } else {
            *any_utf8 = true;
            for (int64_t c = 0; c < nchunks; ++c) {
                const rdf_utf8_array& u = key.utf8[c];
                if (u.offsets.dtype != RDF_I32 || u.offsets.length < 1)
                    return fail(RDF_INVALID_ARGUMENT, "%s: key %d chunk %lld: offsets must be an Int32 array of rows + 1 entries", fn, k, (long long)c);
                if (u.data.dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: key %d chunk %lld: data must be a UInt8 array", fn, k, (long long)c);
                RDF_TRY(check_mem(&u.offsets, 1, mem));
                RDF_TRY(check_mem(&u.data, 1, mem));
            }
        }
    }
    return RDF_OK;
}
// The prefix of the batch lengths (nchunks + 1 entries) of checked keys: every key has the rows of key 0 in every chunk, and
// UInt32 row numbers must reach every row.
rdf_status lexsort_row_starts(const rdf_sort_key* keys, int nkeys, int64_t nchunks, const char* fn, std::vector<int64_t>& row_start) {
    auto rows_of = [&](int k, int64_t c) { return keys[k].values ? keys[k].values[c].length : keys[k].utf8[c].offsets.length - 1; };
    row_start.assign((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) row_start[(size_t)c + 1] = row_start[(size_t)c] + rows_of(0, c);
    for (int k = 1; k < nkeys; ++k)
        for (int64_t c = 0; c < nchunks; ++c)
            if (rows_of(k, c) != rows_of(0, c)) return fail(RDF_COMPUTE_ERROR, "%s: columns of a batch differ in length", fn);
    if (row_start[(size_t)nchunks] >= (int64_t)1 << 32) return fail(RDF_INVALID_ARGUMENT, "%s: UInt32 indices cap a column at 2^32-1 rows (src/table.rs:218)", fn);
    return RDF_OK;
}

}  // namespace

rdf_status rdf_lexsort_to_indices(const rdf_sort_key* keys, int32_t nkeys, int64_t nchunks, rdf_out* out_indices) {
    if (nkeys < 1 || !keys) return fail(RDF_COMPUTE_ERROR, "Sort criteria cannot be empty");  // src/dataframe.rs:195-199
    if (nchunks < 1 || !out_indices) return fail(RDF_INVALID_ARGUMENT, "lexsort: bad arguments");
    if (nkeys > kMaxFrameCols) return fail(RDF_INVALID_ARGUMENT, "lexsort: at most %d sort criteria", kMaxFrameCols);
    int32_t mem = -1;
    bool any_utf8 = false;
    RDF_TRY(lexsort_check_keys(keys, nkeys, nchunks, "lexsort", &mem, &any_utf8));
    RDF_TRY(check_out_mem(out_indices, 1, mem));
    if (out_indices->dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "lexsort: indices are UInt32");
    std::vector<int64_t> row_start;
    RDF_TRY(lexsort_row_starts(keys, nkeys, nchunks, "lexsort", row_start));
    const int64_t n = row_start[(size_t)nchunks];
    if (out_indices->capacity < n) return fail(RDF_MEMORY_ERROR, "output capacity too small");
    std::vector<rdf_sort_options> opts((size_t)nkeys);
    for (int k = 0; k < nkeys; ++k) opts[k] = keys[k].options;
    if (!any_utf8) {   // numeric criteria only: the numeric sort itself, bit for bit
        std::vector<rdf_array> cols((size_t)nkeys * nchunks);
        for (int k = 0; k < nkeys; ++k)
            for (int64_t c = 0; c < nchunks; ++c) cols[(size_t)k * nchunks + c] = keys[k].values[c];
        return rdf_sort_to_indices(cols.data(), nkeys, nchunks, opts.data(), out_indices);
    }
    if (n == 0) { out_indices->length = 0; out_indices->null_count = 0; return RDF_OK; }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();

    size_t pin_off = 0;
    LexKeysOnDevice d;
    RDF_TRY(lexsort_keys_to_device(keys, nkeys, nchunks, mem, row_start, "lexsort", pin_off, d));
    const TableBuilder& tb = d.tb;
    const size_t o_ch = d.o_ch, o_rs = d.o_rs;
    const int* dts = d.dts;
    const bool* nullable = d.nullable;
    const Utf8SortCol* ucols = d.ucols;

    const uint32_t* idx_cur = nullptr;
    RDF_TRY(sort_core(tb.dev_at<DevChunkCol>(o_ch), tb.dev_at<int64_t>(o_rs), nchunks, n, nkeys, dts, nullable, opts.data(), pin_off, &idx_cur, ucols));
    if (mem == RDF_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out_indices->values, idx_cur, (size_t)n * 4, hipMemcpyDeviceToHost, ctx.stream));
        if (out_indices->validity) memset(out_indices->validity, 0xFF, (size_t)((n + 7) / 8));
    } else {
        HIP_TRY(hipMemcpyAsync(out_indices->values, idx_cur, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx.stream));
        if (out_indices->validity) HIP_TRY(hipMemsetAsync(out_indices->validity, 0xFF, (size_t)((n + 7) / 8), ctx.stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    out_indices->length = n;
    out_indices->null_count = 0;
    return RDF_OK;
}
