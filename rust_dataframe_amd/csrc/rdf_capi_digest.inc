// rdf_capi_digest.inc — host side of rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32 (kernels: rdf_digest.hip, what is
// computed about one row: rdf_digest.h); textually included by rdf_capi.cpp (it uses that file's per-thread context, arena
// and staging helpers, utf8_value_ranges and lexsort_keys_to_device).
//
// One call = every argument checked -> the columns staged with the staging of the Utf8 sort (device inputs aliased) -> the
// tile prefix and the descriptors in one upload into the arena -> the kernel(s) -> host outputs copied back.  rdf_utf8_digest
// counts the non-NULL rows per tile first and applies the sizing rule of the rdf_utf8_filter .. _upper family before anything
// is written to the caller's buffers.

namespace {

static_assert(DGH_MURMUR3_32 == RDF_HASH_MURMUR3_32 && DGH_XXHASH64 == RDF_HASH_XXHASH64, "rdf_digest.h restates rdf_hash_kind");
static_assert(DG_MD5 == RDF_DIGEST_MD5 && DG_SHA1 == RDF_DIGEST_SHA1 && DG_SHA224 == RDF_DIGEST_SHA224 && DG_SHA256 == RDF_DIGEST_SHA256 &&
              DG_SHA384 == RDF_DIGEST_SHA384 && DG_SHA512 == RDF_DIGEST_SHA512, "rdf_digest.h restates rdf_digest_kind");
static_assert(DGT_I8 == RDF_I8 && DGT_I64 == RDF_I64 && DGT_U8 == RDF_U8 && DGT_U64 == RDF_U64 && DGT_F32 == RDF_F32 && DGT_F64 == RDF_F64 &&
              DGT_BOOL == RDF_BOOL, "rdf_digest.h restates rdf_dtype");
static_assert(kHashColsMax == RDF_HASH_COLS_MAX && kHashColsMax <= kMaxFrameCols, "rdf_digest.h restates RDF_HASH_COLS_MAX");

rdf_status digest_check_utf8_chunks(const char* fn, const rdf_utf8_array* chunks, int64_t nchunks) {
    for (int64_t c = 0; c < nchunks; ++c) {
        const rdf_utf8_array& u = chunks[c];
        if (u.offsets.dtype != RDF_I32 || u.offsets.length < 1)
            return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: offsets must be an Int32 array of rows + 1 entries", fn, (long long)c);
        if (u.data.dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: data must be a UInt8 array", fn, (long long)c);
    }
    return RDF_OK;
}

// the tile prefix of a call: tiles of kUtf8PredThreads rows that never straddle a chunk
void digest_tile_prefix(const std::vector<int64_t>& row_start, int64_t* hts) {
    hts[0] = 0;
    for (size_t c = 0; c + 1 < row_start.size(); ++c) hts[c + 1] = hts[c] + (row_start[c + 1] - row_start[c] + kUtf8PredThreads - 1) / kUtf8PredThreads;
}

// outputs of one fixed-width value a row (rdf_hash_columns, rdf_utf8_crc32): staging space for host outputs, descriptors
struct RowOuts {
    Region outr;
    std::vector<int> oi;
    rdf_status plan(const rdf_out* outs, const std::vector<int64_t>& row_start, int32_t mem, size_t es) {
        const int64_t nchunks = (int64_t)row_start.size() - 1;
        oi.assign((size_t)nchunks * 2, -1);
        if (mem != RDF_MEM_HOST) return RDF_OK;
        for (int64_t c = 0; c < nchunks; ++c) {
            const int64_t rows = row_start[(size_t)c + 1] - row_start[(size_t)c];
            if (rows == 0) continue;
            oi[2 * c] = outr.add(outs[c].values, (size_t)rows * es);
            if (outs[c].validity) oi[2 * c + 1] = outr.add(outs[c].validity, (size_t)((rows + 7) / 8));
        }
        return outr.layout();
    }
    void fill(const rdf_out* outs, int32_t mem, Utf8PredOut* hout) const {
        for (size_t c = 0; c < oi.size() / 2; ++c) {
            if (mem == RDF_MEM_HOST) {
                hout[c].values = oi[2 * c] >= 0 ? outr.ptr(oi[2 * c]) : nullptr;
                hout[c].valid = oi[2 * c + 1] >= 0 ? (uint8_t*)outr.ptr(oi[2 * c + 1]) : nullptr;
            } else {
                hout[c].values = outs[c].values;
                hout[c].valid = outs[c].validity;
            }
        }
    }
    rdf_status download(int32_t mem) {
        if (mem != RDF_MEM_HOST) return RDF_OK;
        RDF_TRY(pinned_reserve(outr.small_bytes));
        return outr.download(0);
    }
};

// capacity of one value a row, per chunk
rdf_status digest_check_row_capacity(const char* fn, rdf_out* outs, const std::vector<int64_t>& row_start) {
    for (size_t c = 0; c + 1 < row_start.size(); ++c) {
        const int64_t rows = row_start[c + 1] - row_start[c];
        if (outs[c].capacity < rows) {
            outs[c].length = rows;
            return fail(RDF_MEMORY_ERROR, "%s: output %lld: capacity %lld below the %lld rows", fn, (long long)c, (long long)outs[c].capacity, (long long)rows);
        }
        if (rows > 0 && !outs[c].values) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: null values pointer", fn, (long long)c);
    }
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_hash_columns(int32_t kind, const rdf_sort_key* cols, int32_t ncols, int64_t nchunks, int64_t seed, rdf_out* out) {
    const char* fn = "hash_columns";
    if (kind != RDF_HASH_MURMUR3_32 && kind != RDF_HASH_XXHASH64) return fail(RDF_INVALID_ARGUMENT, "%s: unknown hash %d", fn, kind);
    if (ncols < 1 || ncols > RDF_HASH_COLS_MAX || !cols) return fail(RDF_INVALID_ARGUMENT, "%s: %d columns, 1 .. %d are taken", fn, ncols, RDF_HASH_COLS_MAX);
    for (int k = 0; k < ncols; ++k)
        if ((cols[k].values != nullptr) == (cols[k].utf8 != nullptr)) return fail(RDF_INVALID_ARGUMENT, "%s: column %d must set exactly one of values / utf8", fn, k);
    if (kind == RDF_HASH_MURMUR3_32 && (seed < INT32_MIN || seed > INT32_MAX))
        return fail(RDF_INVALID_ARGUMENT, "%s: seed %lld does not fit the Int32 of Murmur3_x86_32", fn, (long long)seed);
    if (nchunks < 0 || (nchunks > 0 && !out)) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    if (nchunks == 0) return RDF_OK;
    // ---- dtypes, memory kinds, row counts, capacities: in this order, each over the whole call
    for (int k = 0; k < ncols; ++k) {
        if (cols[k].utf8) { RDF_TRY(digest_check_utf8_chunks(fn, cols[k].utf8, nchunks)); continue; }
        for (int64_t c = 0; c < nchunks; ++c) {
            const int dt = cols[k].values[c].dtype;
            if (dt < RDF_I8 || dt > RDF_BOOL || dt != cols[k].values[0].dtype)
                return fail(RDF_INVALID_ARGUMENT, "%s: column %d: chunks of one numeric or Boolean dtype", fn, k);
        }
    }
    const int out_dt = kind == RDF_HASH_MURMUR3_32 ? RDF_I32 : RDF_I64;
    for (int64_t c = 0; c < nchunks; ++c)
        if (out[c].dtype != out_dt) return fail(RDF_INVALID_ARGUMENT, "%s: output dtype %d, expected %d", fn, out[c].dtype, out_dt);
    int32_t mem = -1;
    for (int k = 0; k < ncols; ++k) {
        if (cols[k].values) { RDF_TRY(check_mem(cols[k].values, nchunks, &mem)); continue; }
        for (int64_t c = 0; c < nchunks; ++c) {
            RDF_TRY(check_mem(&cols[k].utf8[c].offsets, 1, &mem));
            RDF_TRY(check_mem(&cols[k].utf8[c].data, 1, &mem));
        }
    }
    RDF_TRY(check_out_mem(out, nchunks, mem));
    auto rows_of = [&](int k, int64_t c) { return cols[k].values ? cols[k].values[c].length : cols[k].utf8[c].offsets.length - 1; };
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        row_start[(size_t)c + 1] = row_start[(size_t)c] + rows_of(0, c);
        for (int k = 1; k < ncols; ++k)
            if (rows_of(k, c) != rows_of(0, c)) return fail(RDF_COMPUTE_ERROR, "%s: chunk %lld: the columns' chunk lengths differ", fn, (long long)c);
    }
    RDF_TRY(digest_check_row_capacity(fn, out, row_start));
    const int64_t n = row_start[(size_t)nchunks];
    if (n == 0) {
        for (int64_t c = 0; c < nchunks; ++c) { out[c].length = 0; out[c].null_count = 0; }
        return RDF_OK;
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();

    size_t pin_off = 0;
    LexKeysOnDevice d;
    RDF_TRY(lexsort_keys_to_device(cols, ncols, nchunks, mem, row_start, fn, pin_off, d));
    RowOuts ro;
    RDF_TRY(ro.plan(out, row_start, mem, kind == RDF_HASH_MURMUR3_32 ? 4 : 8));
    TableBuilder tb;
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_out = tb.reserve(sizeof(Utf8PredOut) * (size_t)nchunks);
    const size_t o_cols = tb.reserve(sizeof(HashCol) * (size_t)ncols);
    RDF_TRY(tb.bind(pin_off));
    digest_tile_prefix(row_start, tb.at<int64_t>(o_ts));
    ro.fill(out, mem, tb.at<Utf8PredOut>(o_out));
    HashCol* hc = tb.at<HashCol>(o_cols);
    for (int k = 0; k < ncols; ++k) {
        memset(&hc[k], 0, sizeof(HashCol));
        if (cols[k].utf8) hc[k].utf8 = d.ucols[k].d_chunks;
        else { hc[k].num = d.tb.dev_at<DevChunkCol>(d.o_ch) + (size_t)k * nchunks; hc[k].dtype = d.dts[k]; }
    }
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(pin_off));

    HashColsArgs a;
    memset(&a, 0, sizeof a);
    a.cols = tb.dev_at<HashCol>(o_cols);
    a.ncols = ncols;
    a.kind = kind;
    a.seed = seed;
    a.row_start = d.tb.dev_at<int64_t>(d.o_rs);
    a.nchunks = nchunks;
    a.tile_start = tb.dev_at<int64_t>(o_ts);
    a.ntiles = tb.at<int64_t>(o_ts)[nchunks];
    a.outs = tb.dev_at<Utf8PredOut>(o_out);
    KernelTimer kt;
    ctx.last_kernel = "hash_columns_kernel";
    HIP_TRY(launch_hash_columns(a, ctx.stream));
    kt.stop();
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    RDF_TRY(ro.download(mem));
    for (int64_t c = 0; c < nchunks; ++c) {
        out[c].length = row_start[(size_t)c + 1] - row_start[(size_t)c];
        out[c].null_count = 0;
    }
    return RDF_OK;
}

rdf_status rdf_utf8_crc32(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out) {
    const char* fn = "utf8_crc32";
    if (nchunks < 0 || (nchunks > 0 && (!chunks || !out))) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    if (nchunks == 0) return RDF_OK;
    RDF_TRY(digest_check_utf8_chunks(fn, chunks, nchunks));
    for (int64_t c = 0; c < nchunks; ++c)
        if (out[c].dtype != RDF_I64) return fail(RDF_INVALID_ARGUMENT, "%s: output dtype %d, expected %d", fn, out[c].dtype, RDF_I64);
    int32_t mem = -1;
    for (int64_t c = 0; c < nchunks; ++c) {
        RDF_TRY(check_mem(&chunks[c].offsets, 1, &mem));
        RDF_TRY(check_mem(&chunks[c].data, 1, &mem));
    }
    RDF_TRY(check_out_mem(out, nchunks, mem));
    for (int64_t c = 0; c < nchunks; ++c)
        if (chunks[c].offsets.validity && !out[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld needs a validity buffer", fn, (long long)c);
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) row_start[(size_t)c + 1] = row_start[(size_t)c] + chunks[c].offsets.length - 1;
    RDF_TRY(digest_check_row_capacity(fn, out, row_start));
    const int64_t n = row_start[(size_t)nchunks];
    if (n == 0) {
        for (int64_t c = 0; c < nchunks; ++c) { out[c].length = 0; out[c].null_count = 0; }
        return RDF_OK;
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();

    rdf_sort_key key;
    memset(&key, 0, sizeof key);
    key.utf8 = chunks;
    size_t pin_off = 0;
    LexKeysOnDevice d;
    RDF_TRY(lexsort_keys_to_device(&key, 1, nchunks, mem, row_start, fn, pin_off, d));

    // ---- NULL rows per chunk: known from the input's null_count where that is given, counted by the kernel otherwise
    std::vector<int64_t> nulls((size_t)nchunks, -1);
    bool counting = false;
    for (int64_t c = 0; c < nchunks; ++c) {
        if (!chunks[c].offsets.validity) nulls[(size_t)c] = 0;
        else if (chunks[c].offsets.null_count >= 0) nulls[(size_t)c] = chunks[c].offsets.null_count;
        else counting = true;
    }
    RowOuts ro;
    RDF_TRY(ro.plan(out, row_start, mem, 8));
    TableBuilder tb;
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_out = tb.reserve(sizeof(Utf8PredOut) * (size_t)nchunks);
    const size_t o_nulls = tb.reserve(sizeof(unsigned long long) * (size_t)nchunks);
    RDF_TRY(tb.bind(pin_off));
    digest_tile_prefix(row_start, tb.at<int64_t>(o_ts));
    ro.fill(out, mem, tb.at<Utf8PredOut>(o_out));
    memset(tb.at<char>(o_nulls), 0, sizeof(unsigned long long) * (size_t)nchunks);
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(pin_off));

    Utf8Crc32Args a;
    memset(&a, 0, sizeof a);
    a.chunks = d.ucols[0].d_chunks;
    a.nchunks = nchunks;
    a.tile_start = tb.dev_at<int64_t>(o_ts);
    a.ntiles = tb.at<int64_t>(o_ts)[nchunks];
    a.outs = tb.dev_at<Utf8PredOut>(o_out);
    a.nulls = counting ? tb.dev_at<unsigned long long>(o_nulls) : nullptr;
    KernelTimer kt;
    ctx.last_kernel = "utf8_crc32_kernel";
    HIP_TRY(launch_utf8_crc32(a, ctx.stream));
    kt.stop();
    if (counting) HIP_TRY(hipMemcpyAsync(tb.at<char>(o_nulls), a.nulls, sizeof(unsigned long long) * (size_t)nchunks, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    for (int64_t c = 0; c < nchunks; ++c)
        if (nulls[(size_t)c] < 0) nulls[(size_t)c] = (int64_t)tb.at<unsigned long long>(o_nulls)[c];
    RDF_TRY(ro.download(mem));
    for (int64_t c = 0; c < nchunks; ++c) {
        out[c].length = row_start[(size_t)c + 1] - row_start[(size_t)c];
        out[c].null_count = nulls[(size_t)c];
    }
    return RDF_OK;
}

rdf_status rdf_utf8_digest(int32_t kind, const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    const char* fn = "utf8_digest";
    if (kind < RDF_DIGEST_MD5 || kind > RDF_DIGEST_SHA512) return fail(RDF_INVALID_ARGUMENT, "%s: unknown digest %d", fn, kind);
    if (nchunks < 0 || (nchunks > 0 && (!chunks || !out_offsets || !out_data))) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    if (nchunks == 0) return RDF_OK;
    const int64_t width = digest_hex_bytes(kind);
    RDF_TRY(digest_check_utf8_chunks(fn, chunks, nchunks));
    for (int64_t c = 0; c < nchunks; ++c)
        if (out_offsets[c].dtype != RDF_I32 || out_data[c].dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: outputs are (Int32 offsets, UInt8 data)", fn);
    int32_t mem = -1;
    for (int64_t c = 0; c < nchunks; ++c) {
        RDF_TRY(check_mem(&chunks[c].offsets, 1, &mem));
        RDF_TRY(check_mem(&chunks[c].data, 1, &mem));
    }
    RDF_TRY(check_out_mem(out_offsets, nchunks, mem));
    RDF_TRY(check_out_mem(out_data, nchunks, mem));
    for (int64_t c = 0; c < nchunks; ++c) {
        if (!out_offsets[c].values || out_offsets[c].capacity < 1) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld has no offsets buffer", fn, (long long)c);
        if (out_data[c].capacity < 0 || (out_data[c].capacity > 0 && !out_data[c].values))
            return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: data capacity without a buffer", fn, (long long)c);
        if (chunks[c].offsets.validity && !out_offsets[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld needs a validity buffer", fn, (long long)c);
    }
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = chunks[c].offsets.length - 1;
        row_start[(size_t)c + 1] = row_start[(size_t)c] + rows;
        if (out_offsets[c].capacity < rows + 1) {
            out_offsets[c].length = rows + 1;
            return fail(RDF_MEMORY_ERROR, "%s: output %lld: offsets need %lld entries", fn, (long long)c, (long long)(rows + 1));
        }
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();

    rdf_sort_key key;
    memset(&key, 0, sizeof key);
    key.utf8 = chunks;
    size_t pin_off = 0;
    LexKeysOnDevice d;
    RDF_TRY(lexsort_keys_to_device(&key, 1, nchunks, mem, row_start, fn, pin_off, d));

    // ---- the size pass: non-NULL rows per tile, scanned; per chunk totals read back
    TableBuilder tb;
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    RDF_TRY(tb.bind(pin_off));
    digest_tile_prefix(row_start, tb.at<int64_t>(o_ts));
    const int64_t ntiles = tb.at<int64_t>(o_ts)[nchunks];
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(pin_off));
    pin_off += (tb.size + 255) & ~(size_t)255;
    void *pcount, *pscan, *ptot;
    RDF_TRY(arena_alloc((size_t)(ntiles + 1) * 8, &pcount));
    RDF_TRY(arena_alloc((size_t)(ntiles + 2 + scan_scratch_words(ntiles)) * 8, &pscan));
    RDF_TRY(arena_alloc((size_t)nchunks * 8, &ptot));

    Utf8DigestArgs a;
    memset(&a, 0, sizeof a);
    a.chunks = d.ucols[0].d_chunks;
    a.nchunks = nchunks;
    a.tile_start = tb.dev_at<int64_t>(o_ts);
    a.ntiles = ntiles;
    a.kind = kind;
    a.tile_count = (int64_t*)pcount;
    a.tile_scan = (const int64_t*)pscan;
    a.tot = (int64_t*)ptot;
    KernelTimer kt;
    ctx.last_kernel = "utf8_digest_count_kernel + utf8_digest_kernel";
    if (ntiles > 0) {
        HIP_TRY(launch_utf8_digest_count(a, ctx.stream));
        HIP_TRY(launch_scan(a.tile_count, (int64_t*)pscan, ntiles, (int64_t*)pscan + ntiles + 1, ctx.stream));
    }
    HIP_TRY(launch_utf8_digest_totals(a, ctx.stream));
    const size_t totb = (size_t)nchunks * 8;
    RDF_TRY(pinned_reserve(pin_off + totb + 64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, ptot, totb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    std::vector<int64_t> tot((size_t)nchunks);
    memcpy(tot.data(), ctx.pinned + pin_off, totb);
    pin_off += (totb + 64 + 63) & ~(size_t)63;

    // ---- the sizing rule: every length reported, nothing written unless every chunk fits
    for (int64_t o = 0; o < nchunks; ++o)
        if (tot[(size_t)o] * width > INT32_MAX) {
            kt.stop();
            return fail(RDF_COMPUTE_ERROR, "%s: output %lld holds %lld bytes, beyond the Int32 offsets", fn, (long long)o, (long long)(tot[(size_t)o] * width));
        }
    bool fits = true;
    for (int64_t o = 0; o < nchunks; ++o) {
        out_data[o].length = tot[(size_t)o] * width;
        out_offsets[o].length = row_start[(size_t)o + 1] - row_start[(size_t)o] + 1;
        if (out_data[o].capacity < out_data[o].length) fits = false;
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
            const int64_t rows = row_start[(size_t)o + 1] - row_start[(size_t)o], bytes = tot[(size_t)o] * width;
            oi[3 * o] = outr.add(out_offsets[o].values, (size_t)(rows + 1) * 4);
            if (out_offsets[o].validity && rows > 0) oi[3 * o + 1] = outr.add(out_offsets[o].validity, (size_t)((rows + 7) / 8));
            if (bytes > 0) oi[3 * o + 2] = outr.add(out_data[o].values, (size_t)bytes);
        }
        RDF_TRY(outr.layout());
    }
    TableBuilder to;
    const size_t o_outs = to.reserve(sizeof(Utf8OutChunk) * (size_t)nchunks);
    RDF_TRY(to.bind(pin_off));
    RDF_TRY(to.alloc());
    Utf8OutChunk* ho = to.at<Utf8OutChunk>(o_outs);
    for (int64_t o = 0; o < nchunks; ++o) {
        Utf8OutChunk& u = ho[o];
        memset(&u, 0, sizeof u);
        u.rows = row_start[(size_t)o + 1] - row_start[(size_t)o];
        u.bytes = tot[(size_t)o] * width;
        if (mem == RDF_MEM_HOST) {
            u.offs = (int32_t*)outr.ptr(oi[3 * o]);
            u.valid = oi[3 * o + 1] >= 0 ? (uint8_t*)outr.ptr(oi[3 * o + 1]) : nullptr;
            u.data = oi[3 * o + 2] >= 0 ? (uint8_t*)outr.ptr(oi[3 * o + 2]) : nullptr;
        } else {
            u.offs = (int32_t*)out_offsets[o].values;
            u.valid = u.rows > 0 ? out_offsets[o].validity : nullptr;
            u.data = (uint8_t*)out_data[o].values;
        }
        u.row_start = row_start[(size_t)o];
    }
    RDF_TRY(to.upload(pin_off));
    a.outs = to.dev_at<Utf8OutChunk>(o_outs);
    HIP_TRY(launch_utf8_digest_write(a, ctx.stream));
    kt.stop();
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(pinned_reserve(outr.small_bytes));
        RDF_TRY(outr.download(0));
    }
    for (int64_t o = 0; o < nchunks; ++o) {
        out_offsets[o].null_count = row_start[(size_t)o + 1] - row_start[(size_t)o] - tot[(size_t)o];
        out_data[o].null_count = 0;
    }
    return RDF_OK;
}

}  // extern "C"
