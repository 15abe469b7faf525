// rdf_capi_utf8_build.inc — host side of rdf_utf8_concat / _pad / _repeat / _reverse / _substring_index / _coalesce / _case_when (kernels:
// rdf_utf8_build.hip, what is decided about one row: rdf_utf8_build.h); textually included by rdf_capi.cpp (it uses that
// file's per-thread context, arena and staging helpers, utf8_value_ranges and lexsort_keys_to_device).
//
// One call = every argument checked -> the column parts staged with the staging of the Utf8 sort (device inputs aliased) ->
// the parts table, the literals and the tile prefix in one upload into the arena -> size pass -> scan -> per-chunk totals read
// back -> the sizing rule of the rdf_utf8_filter .. _upper family -> write pass.  Nothing is written to the caller's buffers
// before the sizing rule has passed.

namespace {

static_assert(kUtf8PartsMax == RDF_UTF8_PARTS_MAX, "rdf_utf8_build.h restates RDF_UTF8_PARTS_MAX");

struct Utf8BuildCall {
    const char* fn;
    int op;                        // U8B_*
    const rdf_utf8_part* parts;
    int nparts;
    int64_t nchunks;
    const uint8_t* lit;            // separator / pad / delimiter
    int64_t lit_bytes;
    int64_t param;                 // pad: len, repeat: times, substring_index: count
    rdf_out* out_offsets;
    rdf_out* out_data;
    const rdf_array* const* conds = nullptr;   // utf8_case_when: nconds lists of nchunks RDF_BOOL chunks; parts[nconds] is `otherwise`
    int nconds = 0;
};

rdf_status utf8_build_check_literal(const char* fn, const char* what, const uint8_t* p, int64_t bytes) {
    if (bytes < 0) return fail(RDF_INVALID_ARGUMENT, "%s: %s: negative length %lld", fn, what, (long long)bytes);
    if (bytes > RDF_UTF8_PATTERN_MAX) return fail(RDF_INVALID_ARGUMENT, "%s: %s of %lld bytes, at most %d", fn, what, (long long)bytes, RDF_UTF8_PATTERN_MAX);
    if (!p && bytes > 0) return fail(RDF_INVALID_ARGUMENT, "%s: %s: null pointer with %lld bytes", fn, what, (long long)bytes);
    return RDF_OK;
}

// the checks every call shares (dtypes, memory kinds, validity buffers, row counts, offsets capacity), then the device work
rdf_status utf8_build_run(const Utf8BuildCall& q) {
    const char* fn = q.fn;
    const int64_t nchunks = q.nchunks;
    const bool select = q.op == U8B_COALESCE || q.op == U8B_CASE_WHEN;   // (a part with neither pointer is the NULL literal)
    const rdf_utf8_array* cols[kUtf8SelectSlots];
    int col_of[kUtf8SelectSlots];
    int ncols = 0;
    for (int k = 0; k < q.nparts; ++k) {
        col_of[k] = -1;
        if (q.parts[k].utf8) { col_of[k] = ncols; cols[ncols++] = q.parts[k].utf8; }
    }
    if (nchunks < 0 || (nchunks > 0 && (!q.out_offsets || !q.out_data))) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    // ---- dtypes, memory kinds, validity buffers, row counts, capacities: in this order, each over the whole call
    for (int k = 0; k < ncols; ++k)
        for (int64_t c = 0; c < nchunks; ++c) {
            const rdf_utf8_array& u = cols[k][c];
            if (u.offsets.dtype != RDF_I32 || u.offsets.length < 1)
                return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: offsets must be an Int32 array of rows + 1 entries", fn, (long long)c);
            if (u.data.dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: data must be a UInt8 array", fn, (long long)c);
        }
    for (int64_t c = 0; c < nchunks; ++c)
        if (q.out_offsets[c].dtype != RDF_I32 || q.out_data[c].dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: outputs are (Int32 offsets, UInt8 data)", fn);
    int32_t mem = -1;
    for (int k = 0; k < ncols; ++k)
        for (int64_t c = 0; c < nchunks; ++c) {
            RDF_TRY(check_mem(&cols[k][c].offsets, 1, &mem));
            RDF_TRY(check_mem(&cols[k][c].data, 1, &mem));
        }
    for (int k = 0; k < q.nconds; ++k) RDF_TRY(check_mem(q.conds[k], nchunks, &mem));
    if (nchunks > 0) {
        RDF_TRY(check_out_mem(q.out_offsets, nchunks, mem));
        RDF_TRY(check_out_mem(q.out_data, nchunks, mem));
    }
    for (int64_t c = 0; c < nchunks; ++c) {
        if (!q.out_offsets[c].values || q.out_offsets[c].capacity < 1) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld has no offsets buffer", fn, (long long)c);
        if (q.out_data[c].capacity < 0 || (q.out_data[c].capacity > 0 && !q.out_data[c].values))
            return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: data capacity without a buffer", fn, (long long)c);
        bool nullable = false;
        if (select) {   // coalesce: no part is never-NULL in the chunk; case_when: any value (an absent `otherwise` is the NULL literal) can be NULL
            bool any = false, all = true;
            for (int k = 0; k < q.nparts; ++k) {
                const bool n = q.parts[k].utf8 ? q.parts[k].utf8[c].offsets.validity != nullptr : q.parts[k].literal == nullptr;
                any |= n;
                all &= n;
            }
            nullable = q.op == U8B_COALESCE ? all : any;
        } else if (q.op != U8B_CONCAT_WS)
            for (int k = 0; k < ncols; ++k) nullable |= cols[k][c].offsets.validity != nullptr;
        if (nullable && !q.out_offsets[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld needs a validity buffer", fn, (long long)c);
    }
    for (int k = 1; k < ncols; ++k)
        for (int64_t c = 0; c < nchunks; ++c)
            if (cols[k][c].offsets.length != cols[0][c].offsets.length)
                return fail(RDF_COMPUTE_ERROR, "%s: chunk %lld: the parts' chunk lengths differ", fn, (long long)c);
    for (int k = 0; k < q.nconds; ++k)
        for (int64_t c = 0; c < nchunks; ++c)
            if (q.conds[k][c].length != cols[0][c].offsets.length - 1)
                return fail(RDF_COMPUTE_ERROR, "%s: chunk %lld: a condition's row count differs", fn, (long long)c);
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = cols[0][c].offsets.length - 1;
        row_start[(size_t)c + 1] = row_start[(size_t)c] + rows;
        if (q.out_offsets[c].capacity < rows + 1) {
            q.out_offsets[c].length = rows + 1;
            return fail(RDF_MEMORY_ERROR, "%s: output %lld: offsets need %lld entries", fn, (long long)c, (long long)(rows + 1));
        }
    }
    if (nchunks == 0) return RDF_OK;
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();
    const int64_t n = row_start[(size_t)nchunks];

    // ---- the column parts on the device: the value ranges checked, host arrays staged, the Utf8Chunk tables built
    rdf_sort_key keys[kUtf8SelectSlots + kUtf8PartsMax];   // the column parts, then case_when's conditions (Boolean chunks staged alongside)
    memset(keys, 0, sizeof keys);
    for (int k = 0; k < ncols; ++k) keys[k].utf8 = cols[k];
    for (int k = 0; k < q.nconds; ++k) keys[ncols + k].values = q.conds[k];
    size_t pin_off = 0;
    LexKeysOnDevice d;
    RDF_TRY(lexsort_keys_to_device(keys, ncols + q.nconds, nchunks, mem, row_start, fn, pin_off, d));

    // ---- the tile prefix of the size pass, the parts, and every literal's bytes: one upload
    size_t lit_total = (size_t)q.lit_bytes;
    for (int k = 0; k < q.nparts; ++k)
        if (!q.parts[k].utf8 && q.parts[k].literal) lit_total += (size_t)q.parts[k].literal_bytes;
    TableBuilder tb;
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_parts = tb.reserve(sizeof(Utf8BuildPart) * (size_t)q.nparts);
    const size_t o_lit = tb.reserve(lit_total + 16);
    const size_t o_conds = tb.reserve(sizeof(Utf8BuildCond) * (size_t)q.nconds * (size_t)nchunks);
    RDF_TRY(tb.bind(pin_off));
    RDF_TRY(tb.alloc());
    int64_t* hts = tb.at<int64_t>(o_ts);
    hts[0] = 0;
    for (int64_t c = 0; c < nchunks; ++c) hts[c + 1] = hts[c] + (row_start[(size_t)c + 1] - row_start[(size_t)c] + kUtf8PredThreads - 1) / kUtf8PredThreads;
    Utf8BuildPart* hparts = tb.at<Utf8BuildPart>(o_parts);
    uint8_t* hlit = tb.at<uint8_t>(o_lit);
    if (q.lit_bytes > 0) memcpy(hlit, q.lit, (size_t)q.lit_bytes);
    size_t lit_at = (size_t)q.lit_bytes;
    for (int k = 0; k < q.nparts; ++k) {
        memset(&hparts[k], 0, sizeof(Utf8BuildPart));
        if (q.parts[k].utf8) { hparts[k].col = d.ucols[col_of[k]].d_chunks; continue; }
        if (select && !q.parts[k].literal) { hparts[k].lit_bytes = -1; continue; }
        if (q.parts[k].literal_bytes > 0) memcpy(hlit + lit_at, q.parts[k].literal, (size_t)q.parts[k].literal_bytes);
        hparts[k].lit = tb.dev_at<uint8_t>(o_lit) + lit_at;
        hparts[k].lit_bytes = (int32_t)q.parts[k].literal_bytes;
        lit_at += (size_t)q.parts[k].literal_bytes;
    }
    Utf8BuildCond* hconds = tb.at<Utf8BuildCond>(o_conds);
    for (size_t i = 0; i < (size_t)q.nconds * (size_t)nchunks; ++i) {
        const DevChunkCol& cc = d.tb.at<DevChunkCol>(d.o_ch)[(size_t)ncols * (size_t)nchunks + i];
        hconds[i] = Utf8BuildCond{(const uint8_t*)cc.values, cc.validity, cc.offset};
    }
    RDF_TRY(tb.upload(pin_off));
    pin_off += (tb.size + 255) & ~(size_t)255;

    void *pblen, *paux, *pbscan, *ptot, *pnulls;
    RDF_TRY(arena_alloc((size_t)n * 8, &pblen));
    RDF_TRY(arena_alloc((size_t)n * 4, &paux));
    RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &pbscan));
    RDF_TRY(arena_alloc((size_t)nchunks * 16, &ptot));
    RDF_TRY(arena_alloc((size_t)nchunks * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, (size_t)nchunks * 8, ctx.stream));

    Utf8BuildArgs a;
    memset(&a, 0, sizeof a);
    a.parts = tb.dev_at<Utf8BuildPart>(o_parts);
    a.nparts = q.nparts;
    a.op = q.op;
    a.shape = d.ucols[0].d_chunks;
    a.nchunks = nchunks;
    a.tile_start = tb.dev_at<int64_t>(o_ts);
    a.nsize_tiles = hts[nchunks];
    a.lit = tb.dev_at<uint8_t>(o_lit);
    a.lit_bytes = (int32_t)q.lit_bytes;
    a.lit_cp = (int32_t)utf8_count_code_points(q.lit, q.lit_bytes);
    a.param = q.param;
    a.conds = tb.dev_at<Utf8BuildCond>(o_conds);
    a.nconds = q.nconds;
    a.n = n;
    a.blen = (int64_t*)pblen;
    a.aux = (uint32_t*)paux;
    a.bscan = (const int64_t*)pbscan;
    a.tot = (int64_t*)ptot;
    a.null_counts = (unsigned long long*)pnulls;
    KernelTimer kt;
    ctx.last_kernel = "utf8_build_size_kernel + utf8_build_copy_kernel";
    HIP_TRY(launch_utf8_build_size(a, ctx.stream));
    HIP_TRY(launch_scan(a.blen, (int64_t*)pbscan, n, (int64_t*)pbscan + n + 1, ctx.stream));
    HIP_TRY(launch_utf8_build_totals(a, ctx.stream));
    const size_t totb = (size_t)nchunks * 16, nullb = (size_t)nchunks * 8;
    RDF_TRY(pinned_reserve(pin_off + totb + nullb + 64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, ptot, totb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + totb, pnulls, nullb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    std::vector<int64_t> tot((size_t)nchunks * 2), nulls((size_t)nchunks);
    memcpy(tot.data(), ctx.pinned + pin_off, totb);
    memcpy(nulls.data(), ctx.pinned + pin_off + totb, nullb);
    pin_off += (totb + nullb + 64 + 63) & ~(size_t)63;

    // ---- the sizing rule: every length reported, nothing written unless every chunk fits
    for (int64_t o = 0; o < nchunks; ++o)
        if (tot[2 * o] > INT32_MAX) {
            kt.stop();
            return fail(RDF_COMPUTE_ERROR, "%s: output %lld holds %lld bytes or more, beyond the Int32 offsets", fn, (long long)o, (long long)tot[2 * o]);
        }
    bool fits = true;
    for (int64_t o = 0; o < nchunks; ++o) {
        q.out_data[o].length = tot[2 * o];
        q.out_offsets[o].length = tot[2 * o + 1] + 1;
        if (q.out_data[o].capacity < tot[2 * o]) fits = false;
    }
    if (!fits) {   // (the sizing call: its size pass is timed like any other)
        kt.stop();
        return fail(RDF_MEMORY_ERROR, "%s: output capacity too small (the needed lengths are in out_data[i].length)", fn);
    }

    // ---- write
    Region outr;
    std::vector<int> oi((size_t)nchunks * 3, -1);
    if (mem == RDF_MEM_HOST) {
        for (int64_t o = 0; o < nchunks; ++o) {
            const int64_t rows = tot[2 * o + 1], bytes = tot[2 * o];
            oi[3 * o] = outr.add(q.out_offsets[o].values, (size_t)(rows + 1) * 4);
            if (q.out_offsets[o].validity && rows > 0) oi[3 * o + 1] = outr.add(q.out_offsets[o].validity, (size_t)((rows + 7) / 8));
            if (bytes > 0) oi[3 * o + 2] = outr.add(q.out_data[o].values, (size_t)bytes);
        }
        RDF_TRY(outr.layout());
    }
    TableBuilder to;
    const size_t o_outs = to.reserve(sizeof(Utf8OutChunk) * (size_t)nchunks);
    RDF_TRY(to.bind(pin_off));
    RDF_TRY(to.alloc());
    Utf8OutChunk* ho = to.at<Utf8OutChunk>(o_outs);
    int64_t obyte = 0, otile = 0;
    for (int64_t o = 0; o < nchunks; ++o) {
        Utf8OutChunk& u = ho[o];
        memset(&u, 0, sizeof u);
        u.rows = tot[2 * o + 1];
        u.bytes = tot[2 * o];
        if (mem == RDF_MEM_HOST) {
            u.offs = (int32_t*)outr.ptr(oi[3 * o]);
            u.valid = oi[3 * o + 1] >= 0 ? (uint8_t*)outr.ptr(oi[3 * o + 1]) : nullptr;
            u.data = oi[3 * o + 2] >= 0 ? (uint8_t*)outr.ptr(oi[3 * o + 2]) : nullptr;
        } else {
            u.offs = (int32_t*)q.out_offsets[o].values;
            u.valid = u.rows > 0 ? q.out_offsets[o].validity : nullptr;
            u.data = (uint8_t*)q.out_data[o].values;
        }
        u.row_start = row_start[(size_t)o];
        u.byte_start = obyte;
        u.tile_start = otile;
        obyte += u.bytes;
        otile += (u.bytes + kUtf8CopyTile - 1) / kUtf8CopyTile;
    }
    RDF_TRY(to.upload(pin_off));
    void* ptiles;
    RDF_TRY(arena_alloc((size_t)otile * 8 + 8, &ptiles));
    a.outs = to.dev_at<Utf8OutChunk>(o_outs);
    a.ntiles = otile;
    a.tile_row = (int64_t*)ptiles;
    HIP_TRY(launch_utf8_build_write(a, ctx.stream));
    kt.stop();
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(pinned_reserve(outr.small_bytes));   // (inputs copied directly leave the staging buffer smaller than the packed outputs)
        RDF_TRY(outr.download(0));
    }
    for (int64_t o = 0; o < nchunks; ++o) {
        q.out_offsets[o].null_count = q.op == U8B_CONCAT_WS ? 0 : nulls[(size_t)o];
        q.out_data[o].null_count = 0;
    }
    return RDF_OK;
}

// rdf_utf8_pad .. _substring_index: one column, as a one-part call
rdf_status utf8_build_unary(const char* fn, int op, const rdf_utf8_array* chunks, int64_t nchunks, const char* what, const uint8_t* lit, int64_t lit_bytes,
                            int64_t param, rdf_out* out_offsets, rdf_out* out_data) {
    if (what) RDF_TRY(utf8_build_check_literal(fn, what, lit, lit_bytes));
    if (nchunks < 0 || (nchunks > 0 && !chunks)) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk list", fn);
    if (nchunks == 0) return RDF_OK;
    const rdf_utf8_part part = {chunks, nullptr, 0};
    const Utf8BuildCall q = {fn, op, &part, 1, nchunks, lit, lit_bytes, param, out_offsets, out_data};
    return utf8_build_run(q);
}

}  // namespace

extern "C" {

rdf_status rdf_utf8_concat(const rdf_utf8_part* parts, int32_t nparts, int64_t nchunks, int32_t with_separator, const uint8_t* sep, int64_t sep_bytes,
                           rdf_out* out_offsets, rdf_out* out_data) {
    const char* fn = with_separator ? "utf8_concat_ws" : "utf8_concat";
    if (nparts < 1 || nparts > RDF_UTF8_PARTS_MAX || !parts) return fail(RDF_INVALID_ARGUMENT, "%s: %d parts, 1 .. %d are taken", fn, nparts, RDF_UTF8_PARTS_MAX);
    bool any_col = false;
    for (int k = 0; k < nparts; ++k) {
        if ((parts[k].utf8 != nullptr) == (parts[k].literal != nullptr)) return fail(RDF_INVALID_ARGUMENT, "%s: part %d must set exactly one of utf8 / literal", fn, k);
        any_col |= parts[k].utf8 != nullptr;
    }
    if (!any_col) return fail(RDF_INVALID_ARGUMENT, "%s: at least one part must be a column (the row count is its)", fn);
    for (int k = 0; k < nparts; ++k)
        if (parts[k].literal) RDF_TRY(utf8_build_check_literal(fn, "a literal part", parts[k].literal, parts[k].literal_bytes));
    RDF_TRY(utf8_build_check_literal(fn, "the separator", sep, sep_bytes));
    if (!with_separator && sep_bytes != 0) return fail(RDF_INVALID_ARGUMENT, "%s: a separator of %lld bytes without with_separator", fn, (long long)sep_bytes);
    const Utf8BuildCall q = {fn, with_separator ? U8B_CONCAT_WS : U8B_CONCAT, parts, nparts, nchunks, sep, sep_bytes, 0, out_offsets, out_data};
    return utf8_build_run(q);
}

// rdf_utf8_coalesce / rdf_utf8_case_when: the checks of their own in the order the header lists, then the shared run.  slots:
// the value parts in the kernel's order (case_when: the branches' values, then `otherwise`, which absent is the NULL literal).
static rdf_status utf8_select(const char* fn, int op, const rdf_array* const* conds, const rdf_utf8_part* values, int32_t n, int lo, const rdf_utf8_part* otherwise,
                              int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    const bool cw = op == U8B_CASE_WHEN;
    if (n < lo || n > RDF_UTF8_PARTS_MAX) return fail(RDF_INVALID_ARGUMENT, "%s: %d %s, %d .. %d are taken", fn, n, cw ? "branches" : "parts", lo, RDF_UTF8_PARTS_MAX);
    if (nchunks < 0) return fail(RDF_INVALID_ARGUMENT, "%s: negative nchunks", fn);
    if (nchunks == 0) return RDF_OK;
    if (!values || !out_offsets || !out_data || (cw && !conds)) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    rdf_utf8_part slots[kUtf8SelectSlots];
    int ns = 0;
    for (int k = 0; k < n; ++k) {
        if (cw && !conds[k]) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
        slots[ns++] = values[k];
    }
    if (cw) slots[ns++] = otherwise ? *otherwise : rdf_utf8_part{nullptr, nullptr, 0};
    bool any_col = false;
    for (int k = 0; k < ns; ++k) any_col |= slots[k].utf8 != nullptr;
    if (!any_col) return fail(RDF_INVALID_ARGUMENT, "%s: no column part (the row count is its)", fn);
    for (int k = 0; k < ns; ++k)
        if (slots[k].utf8 && slots[k].literal) return fail(RDF_INVALID_ARGUMENT, "%s: part %d sets both utf8 and literal", fn, k);
    for (int k = 0; k < ns; ++k)
        if (slots[k].literal) RDF_TRY(utf8_build_check_literal(fn, "a literal part", slots[k].literal, slots[k].literal_bytes));
    for (int k = 0; cw && k < n; ++k)
        for (int64_t c = 0; c < nchunks; ++c)
            if (conds[k][c].dtype != RDF_BOOL) return fail(RDF_INVALID_ARGUMENT, "%s: condition %d is not RDF_BOOL", fn, k);
    Utf8BuildCall q = {fn, op, slots, ns, nchunks, nullptr, 0, 0, out_offsets, out_data};
    q.conds = conds;
    q.nconds = cw ? n : 0;
    return utf8_build_run(q);
}

rdf_status rdf_utf8_coalesce(const rdf_utf8_part* parts, int32_t nparts, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_select("utf8_coalesce", U8B_COALESCE, nullptr, parts, nparts, 1, nullptr, nchunks, out_offsets, out_data);
}
rdf_status rdf_utf8_case_when(const rdf_array* const* conds, const rdf_utf8_part* values, int32_t nbranches, const rdf_utf8_part* otherwise, int64_t nchunks,
                              rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_select("utf8_case_when", U8B_CASE_WHEN, conds, values, nbranches, 1, otherwise, nchunks, out_offsets, out_data);
}

rdf_status rdf_utf8_pad(int32_t side, const rdf_utf8_array* chunks, int64_t nchunks, int64_t len, const uint8_t* pad, int64_t pad_bytes,
                        rdf_out* out_offsets, rdf_out* out_data) {
    if (side != 0 && side != 1) return fail(RDF_INVALID_ARGUMENT, "utf8_pad: side %d, 0 (lpad) or 1 (rpad)", side);
    return utf8_build_unary(side ? "utf8_rpad" : "utf8_lpad", side ? U8B_RPAD : U8B_LPAD, chunks, nchunks, "the pad", pad, pad_bytes, utf8_build_clamp(len),
                            out_offsets, out_data);
}
rdf_status rdf_utf8_repeat(const rdf_utf8_array* chunks, int64_t nchunks, int64_t times, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_build_unary("utf8_repeat", U8B_REPEAT, chunks, nchunks, nullptr, nullptr, 0, utf8_build_clamp(times), out_offsets, out_data);
}
rdf_status rdf_utf8_reverse(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_build_unary("utf8_reverse", U8B_REVERSE, chunks, nchunks, nullptr, nullptr, 0, 0, out_offsets, out_data);
}
rdf_status rdf_utf8_substring_index(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* delim, int64_t delim_bytes, int64_t count,
                                    rdf_out* out_offsets, rdf_out* out_data) {
    // a row has fewer than 2^31 occurrences: beyond that every count means "the whole row"
    const int64_t cnt = count < 0 ? -utf8_build_clamp(count == INT64_MIN ? INT64_MAX : -count) : utf8_build_clamp(count);
    return utf8_build_unary("utf8_substring_index", U8B_SUBSTRING_INDEX, chunks, nchunks, "the delimiter", delim, delim_bytes, cnt, out_offsets, out_data);
}

}  // extern "C"
