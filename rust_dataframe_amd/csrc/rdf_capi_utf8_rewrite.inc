// rdf_capi_utf8_rewrite.inc — host side of rdf_utf8_replace / _translate / _initcap / _split (kernels: rdf_utf8_rewrite.hip,
// what is decided about one row: rdf_utf8_rewrite.h); textually included by rdf_capi.cpp after rdf_capi_utf8_build.inc (it uses
// that file's utf8_build_check_literal and rdf_capi.cpp's per-thread context, arena and staging helpers).
//
// One call = every argument checked in the order include/rdf_mi355x.h lists -> the column staged with the staging of the
// Utf8 sort (device inputs aliased) -> the literals, the compiled translate table and the tile prefix in one upload -> size
// pass -> scan(s) -> per-chunk totals read back -> the sizing rule of the rdf_utf8_filter .. _upper family -> write pass.
// Nothing is written to the caller's buffers before the sizing rule has passed.

namespace {

struct Utf8RewriteCall {
    const char* fn;
    int op;                        // U8R_*
    const rdf_utf8_array* chunks;
    int64_t nchunks;
    const uint8_t* lit;            // search / delimiter / matching
    int64_t lit_bytes;
    const uint8_t* rep;            // replacement / replace
    int64_t rep_bytes;
    int64_t limit;                 // split
    rdf_out* out_list;             // split: the list offsets (and the rows' validity)
    rdf_out* out_offsets;          // the rows' offsets (split: the child's)
    rdf_out* out_data;
    const uint8_t* regex;          // rdf_capi_utf8_regex.inc: a compiled regular expression's image; lit is unused then
    int64_t regex_bytes;
    int regex_op;                  // U8X_EXTRACT / _REPLACE / _SPLIT
};

rdf_status utf8_rewrite_run(const Utf8RewriteCall& q) {
    const char* fn = q.fn;
    const int64_t nchunks = q.nchunks;
    const bool split = q.op == U8R_SPLIT;
    rdf_out* rows_out = split ? q.out_list : q.out_offsets;   // what holds one entry per row, and the rows' validity
    if (nchunks < 0 || (nchunks > 0 && (!q.chunks || !q.out_offsets || !q.out_data || (split && !q.out_list))))
        return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    if (nchunks == 0) return RDF_OK;
    // ---- dtypes, memory kinds, buffers and bitmaps, capacities: in this order, each over the whole call
    for (int64_t c = 0; c < nchunks; ++c) {
        const rdf_utf8_array& u = q.chunks[c];
        if (u.offsets.dtype != RDF_I32 || u.offsets.length < 1)
            return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: offsets must be an Int32 array of rows + 1 entries", fn, (long long)c);
        if (u.data.dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: data must be a UInt8 array", fn, (long long)c);
    }
    for (int64_t c = 0; c < nchunks; ++c)
        if (q.out_offsets[c].dtype != RDF_I32 || q.out_data[c].dtype != RDF_U8 || (split && q.out_list[c].dtype != RDF_I32))
            return fail(RDF_INVALID_ARGUMENT, split ? "%s: outputs are (Int32 list offsets, Int32 offsets, UInt8 data)" : "%s: outputs are (Int32 offsets, UInt8 data)", fn);
    int32_t mem = -1;
    for (int64_t c = 0; c < nchunks; ++c) {
        RDF_TRY(check_mem(&q.chunks[c].offsets, 1, &mem));
        RDF_TRY(check_mem(&q.chunks[c].data, 1, &mem));
    }
    RDF_TRY(check_out_mem(q.out_offsets, nchunks, mem));
    RDF_TRY(check_out_mem(q.out_data, nchunks, mem));
    if (split) RDF_TRY(check_out_mem(q.out_list, nchunks, mem));
    for (int64_t c = 0; c < nchunks; ++c) {
        if (!rows_out[c].values || rows_out[c].capacity < 1) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld has no offsets buffer", fn, (long long)c);
        if (q.out_data[c].capacity < 0 || (split && q.out_offsets[c].capacity < 0))
            return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: a negative capacity", fn, (long long)c);
        if (!split && q.out_data[c].capacity > 0 && !q.out_data[c].values)
            return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: data capacity without a buffer", fn, (long long)c);
        if (q.chunks[c].offsets.validity && !rows_out[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld needs a validity buffer", fn, (long long)c);
    }
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = q.chunks[c].offsets.length - 1;
        row_start[(size_t)c + 1] = row_start[(size_t)c] + rows;
        if (rows_out[c].capacity < rows + 1) {
            rows_out[c].length = rows + 1;
            return fail(RDF_MEMORY_ERROR, "%s: output %lld: offsets need %lld entries", fn, (long long)c, (long long)(rows + 1));
        }
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();
    const int64_t n = row_start[(size_t)nchunks];

    // ---- the column on the device: the value ranges checked, host arrays staged, the Utf8Chunk table built
    rdf_sort_key key;
    memset(&key, 0, sizeof key);
    key.utf8 = q.chunks;
    size_t pin_off = 0;
    LexKeysOnDevice d;
    RDF_TRY(lexsort_keys_to_device(&key, 1, nchunks, mem, row_start, fn, pin_off, d));

    // ---- the tile prefix of both passes, the literals and the compiled table: one upload
    TableBuilder tb;
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_lit = tb.reserve((size_t)q.lit_bytes + 16);
    const size_t o_rep = tb.reserve((size_t)q.rep_bytes + 16);
    const size_t o_tab = tb.reserve(q.op == U8R_TRANSLATE ? sizeof(Utf8TranslateTable) : q.regex ? (size_t)q.regex_bytes : 16);
    RDF_TRY(tb.bind(pin_off));
    RDF_TRY(tb.alloc());
    int64_t* hts = tb.at<int64_t>(o_ts);
    hts[0] = 0;
    for (int64_t c = 0; c < nchunks; ++c) hts[c + 1] = hts[c] + (row_start[(size_t)c + 1] - row_start[(size_t)c] + kUtf8PredThreads - 1) / kUtf8PredThreads;
    if (q.op == U8R_TRANSLATE) utf8_translate_compile(q.lit, q.lit_bytes, q.rep, q.rep_bytes, tb.at<Utf8TranslateTable>(o_tab));
    else {
        if (q.lit_bytes > 0) memcpy(tb.at<uint8_t>(o_lit), q.lit, (size_t)q.lit_bytes);
        if (q.rep_bytes > 0) memcpy(tb.at<uint8_t>(o_rep), q.rep, (size_t)q.rep_bytes);
    }
    if (q.regex) memcpy(tb.at<uint8_t>(o_tab), q.regex, (size_t)q.regex_bytes);
    RDF_TRY(tb.upload(pin_off));
    pin_off += (tb.size + 255) & ~(size_t)255;

    void *pblen, *pelen = nullptr, *pbscan, *pescan = nullptr, *ptot, *pnulls;
    RDF_TRY(arena_alloc((size_t)n * 8, &pblen));
    RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &pbscan));
    if (split) {
        RDF_TRY(arena_alloc((size_t)n * 8, &pelen));
        RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &pescan));
    }
    RDF_TRY(arena_alloc((size_t)nchunks * 24, &ptot));
    RDF_TRY(arena_alloc((size_t)nchunks * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, (size_t)nchunks * 8, ctx.stream));

    Utf8RewriteArgs a;
    memset(&a, 0, sizeof a);
    a.chunks = d.ucols[0].d_chunks;
    a.nchunks = nchunks;
    a.tile_start = tb.dev_at<int64_t>(o_ts);
    a.ntiles = hts[nchunks];
    a.op = q.op;
    a.lit = tb.dev_at<uint8_t>(o_lit);
    a.rep = tb.dev_at<uint8_t>(o_rep);
    a.lit_bytes = q.op == U8R_TRANSLATE ? 0 : (int32_t)q.lit_bytes;
    a.rep_bytes = q.op == U8R_TRANSLATE ? 0 : (int32_t)q.rep_bytes;
    a.table = tb.dev_at<Utf8TranslateTable>(o_tab);
    a.maxhits = split ? utf8_split_max_hits(q.limit) : kUtf8AllHits;
    a.n = n;
    a.blen = (int64_t*)pblen;
    a.elen = (int64_t*)pelen;
    a.bscan = (const int64_t*)pbscan;
    a.escan = (const int64_t*)pescan;
    a.tot = (int64_t*)ptot;
    a.null_counts = (unsigned long long*)pnulls;
    KernelTimer kt;
    a.regex = q.regex ? tb.dev_at<uint8_t>(o_tab) : nullptr;
    a.regex_op = q.regex_op;
    ctx.last_kernel = q.regex ? "utf8_regex_size_kernel + utf8_regex_write_kernel" : "utf8_rewrite_size_kernel + utf8_rewrite_write_kernel";
    if (q.regex) HIP_TRY(launch_utf8_regex_size(a, q.regex_bytes, ctx.stream));
    else HIP_TRY(launch_utf8_rewrite_size(a, ctx.stream));
    HIP_TRY(launch_scan(a.blen, (int64_t*)pbscan, n, (int64_t*)pbscan + n + 1, ctx.stream));
    if (split) HIP_TRY(launch_scan(a.elen, (int64_t*)pescan, n, (int64_t*)pescan + n + 1, ctx.stream));
    HIP_TRY(launch_utf8_rewrite_totals(a, ctx.stream));
    const size_t totb = (size_t)nchunks * 24, nullb = (size_t)nchunks * 8;
    RDF_TRY(pinned_reserve(pin_off + totb + nullb + 64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, ptot, totb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + totb, pnulls, nullb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    std::vector<int64_t> tot((size_t)nchunks * 3), nulls((size_t)nchunks);
    memcpy(tot.data(), ctx.pinned + pin_off, totb);
    memcpy(nulls.data(), ctx.pinned + pin_off + totb, nullb);
    pin_off += (totb + nullb + 64 + 63) & ~(size_t)63;

    // ---- the sizing rule: every length reported, nothing written unless every chunk fits
    for (int64_t o = 0; o < nchunks; ++o)
        if (tot[3 * o] > INT32_MAX || tot[3 * o + 2] >= INT32_MAX) {
            kt.stop();
            return fail(RDF_COMPUTE_ERROR, "%s: output %lld holds %lld bytes and %lld elements, beyond the Int32 offsets", fn, (long long)o, (long long)tot[3 * o],
                        (long long)tot[3 * o + 2]);
        }
    bool fits = true;
    for (int64_t o = 0; o < nchunks; ++o) {
        const int64_t bytes = tot[3 * o], rows = tot[3 * o + 1], elems = tot[3 * o + 2];
        q.out_data[o].length = bytes;
        rows_out[o].length = rows + 1;
        if (q.out_data[o].capacity < bytes || (bytes > 0 && !q.out_data[o].values)) fits = false;
        if (split) {
            q.out_offsets[o].length = elems + 1;
            if (q.out_offsets[o].capacity < elems + 1 || !q.out_offsets[o].values) fits = false;
        }
    }
    if (!fits) {   // (the sizing call: its size pass is timed like any other)
        kt.stop();
        return fail(RDF_MEMORY_ERROR, split ? "%s: output capacity too small (the needed lengths are in out_offsets[i].length and out_data[i].length)"
                                            : "%s: output capacity too small (the needed lengths are in out_data[i].length)", fn);
    }

    // ---- write
    Region outr;
    std::vector<int> oi((size_t)nchunks * 4, -1);
    if (mem == RDF_MEM_HOST) {
        for (int64_t o = 0; o < nchunks; ++o) {
            const int64_t bytes = tot[3 * o], rows = tot[3 * o + 1], elems = tot[3 * o + 2];
            oi[4 * o] = outr.add(rows_out[o].values, (size_t)(rows + 1) * 4);
            if (rows_out[o].validity && rows > 0) oi[4 * o + 1] = outr.add(rows_out[o].validity, (size_t)((rows + 7) / 8));
            if (bytes > 0) oi[4 * o + 2] = outr.add(q.out_data[o].values, (size_t)bytes);
            if (split) oi[4 * o + 3] = outr.add(q.out_offsets[o].values, (size_t)(elems + 1) * 4);
        }
        RDF_TRY(outr.layout());
    }
    TableBuilder to;
    const size_t o_outs = to.reserve(sizeof(Utf8RewriteOut) * (size_t)nchunks);
    RDF_TRY(to.bind(pin_off));
    RDF_TRY(to.alloc());
    Utf8RewriteOut* ho = to.at<Utf8RewriteOut>(o_outs);
    int64_t obyte = 0, oelem = 0;
    for (int64_t o = 0; o < nchunks; ++o) {
        Utf8RewriteOut& u = ho[o];
        memset(&u, 0, sizeof u);
        u.bytes = tot[3 * o];
        u.rows = tot[3 * o + 1];
        u.elems = tot[3 * o + 2];
        int32_t* rows_ptr;
        if (mem == RDF_MEM_HOST) {
            rows_ptr = (int32_t*)outr.ptr(oi[4 * o]);
            u.valid = oi[4 * o + 1] >= 0 ? (uint8_t*)outr.ptr(oi[4 * o + 1]) : nullptr;
            u.data = oi[4 * o + 2] >= 0 ? (uint8_t*)outr.ptr(oi[4 * o + 2]) : nullptr;
            u.offs = split ? (int32_t*)outr.ptr(oi[4 * o + 3]) : rows_ptr;
        } else {
            rows_ptr = (int32_t*)rows_out[o].values;
            u.valid = u.rows > 0 ? rows_out[o].validity : nullptr;
            u.data = (uint8_t*)q.out_data[o].values;
            u.offs = split ? (int32_t*)q.out_offsets[o].values : rows_ptr;
        }
        u.list_offs = split ? rows_ptr : nullptr;
        u.row_start = row_start[(size_t)o];
        u.byte_start = obyte;
        u.elem_start = oelem;
        obyte += u.bytes;
        oelem += u.elems;
    }
    RDF_TRY(to.upload(pin_off));
    a.outs = to.dev_at<Utf8RewriteOut>(o_outs);
    if (q.regex) HIP_TRY(launch_utf8_regex_write(a, q.regex_bytes, ctx.stream));
    else HIP_TRY(launch_utf8_rewrite_write(a, ctx.stream));
    kt.stop();
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(pinned_reserve(outr.small_bytes));   // (inputs copied directly leave the staging buffer smaller than the packed outputs)
        RDF_TRY(outr.download(0));
    }
    for (int64_t o = 0; o < nchunks; ++o) {
        rows_out[o].null_count = nulls[(size_t)o];
        q.out_data[o].null_count = 0;
        if (split) q.out_offsets[o].null_count = 0;
    }
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_utf8_replace(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* search, int64_t search_bytes, const uint8_t* replacement,
                            int64_t replacement_bytes, rdf_out* out_offsets, rdf_out* out_data) {
    const char* fn = "utf8_replace";
    RDF_TRY(utf8_build_check_literal(fn, "the search string", search, search_bytes));
    RDF_TRY(utf8_build_check_literal(fn, "the replacement", replacement, replacement_bytes));
    const Utf8RewriteCall q = {fn, U8R_REPLACE, chunks, nchunks, search, search_bytes, replacement, replacement_bytes, 0, nullptr, out_offsets, out_data};
    return utf8_rewrite_run(q);
}
rdf_status rdf_utf8_translate(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* matching, int64_t matching_bytes, const uint8_t* replace,
                              int64_t replace_bytes, rdf_out* out_offsets, rdf_out* out_data) {
    const char* fn = "utf8_translate";
    RDF_TRY(utf8_build_check_literal(fn, "the matching string", matching, matching_bytes));
    RDF_TRY(utf8_build_check_literal(fn, "the replace string", replace, replace_bytes));
    const Utf8RewriteCall q = {fn, U8R_TRANSLATE, chunks, nchunks, matching, matching_bytes, replace, replace_bytes, 0, nullptr, out_offsets, out_data};
    return utf8_rewrite_run(q);
}
rdf_status rdf_utf8_initcap(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    const Utf8RewriteCall q = {"utf8_initcap", U8R_INITCAP, chunks, nchunks, nullptr, 0, nullptr, 0, 0, nullptr, out_offsets, out_data};
    return utf8_rewrite_run(q);
}
rdf_status rdf_utf8_split(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* delim, int64_t delim_bytes, int64_t limit, rdf_out* out_list_offsets,
                          rdf_out* out_offsets, rdf_out* out_data) {
    const char* fn = "utf8_split";
    RDF_TRY(utf8_build_check_literal(fn, "the delimiter", delim, delim_bytes));
    if (delim_bytes == 0) return fail(RDF_INVALID_ARGUMENT, "%s: an empty delimiter", fn);
    const Utf8RewriteCall q = {fn, U8R_SPLIT, chunks, nchunks, delim, delim_bytes, nullptr, 0, limit, out_list_offsets, out_offsets, out_data};
    return utf8_rewrite_run(q);
}

}  // extern "C"
