// rdf_capi_textconv.inc — host side of rdf_utf8_parse / rdf_utf8_format (kernels: rdf_textconv.hip, the pattern compiler and
// what is decided about one row: rdf_textconv.h); textually included by rdf_capi.cpp (it uses that file's per-thread context,
// arena and staging helpers, utf8_value_ranges and lexsort_keys_to_device).
//
// parse    every argument checked, the pattern compiled -> the text staged with the staging of the Utf8 sort (device inputs
//          aliased) -> tile prefix, output descriptors, the compiled pattern and the counters in one upload -> ONE kernel ->
//          host outputs copied back.
// format   every argument checked, the pattern compiled -> the values staged -> tile prefix and pattern in one upload -> size
//          pass -> scan -> per-chunk totals read back -> the sizing rule of rdf_utf8_trim -> write pass.
// Nothing is written to the caller's buffers by a call that is refused, except the lengths a too small output needs.

namespace {

static_assert(TC_BOOL == RDF_TEXT_BOOL && TC_INT == RDF_TEXT_INT && TC_DATE == RDF_TEXT_DATE && TC_TIMESTAMP == RDF_TEXT_TIMESTAMP,
              "rdf_textconv.h restates rdf_text_kind");
static_assert(TC_DT_I8 == RDF_I8 && TC_DT_I64 == RDF_I64 && TC_DT_U8 == RDF_U8 && TC_DT_U64 == RDF_U64 && TC_DT_BOOL == RDF_BOOL, "rdf_textconv.h restates rdf_dtype");
static_assert(sizeof(TcPattern) % 4 == 0, "the kernels copy the pattern word by word");

bool tc_is_int_dtype(int dt) { return dt >= RDF_I8 && dt <= RDF_U64; }

// kind, unit and pattern of a call: the checks both entry points share.  *pt is filled when a pattern is given.
rdf_status textconv_check_call(const char* fn, int32_t kind, int32_t unit, bool for_parse, const uint8_t* pattern, int64_t pattern_bytes, TcPattern* pt) {
    if (kind < RDF_TEXT_BOOL || kind > RDF_TEXT_TIMESTAMP) return fail(RDF_INVALID_ARGUMENT, "%s: unknown kind %d", fn, kind);
    const bool temporal = kind == RDF_TEXT_DATE || kind == RDF_TEXT_TIMESTAMP;
    if (for_parse) {
        if (kind == RDF_TEXT_TIMESTAMP && (unit < RDF_TIME_SECOND || unit > RDF_TIME_NANOSECOND))
            return fail(RDF_INVALID_ARGUMENT, "%s: unknown time unit %d (a timestamp is parsed into seconds .. nanoseconds)", fn, unit);
    } else if (temporal && (unit < RDF_TIME_SECOND || unit > RDF_TIME_DAY)) {
        return fail(RDF_INVALID_ARGUMENT, "%s: unknown time unit %d", fn, unit);
    }
    if (!pattern) {
        if (pattern_bytes != 0) return fail(RDF_INVALID_ARGUMENT, "%s: null pattern with %lld bytes", fn, (long long)pattern_bytes);
        return RDF_OK;
    }
    if (!temporal) return fail(RDF_INVALID_ARGUMENT, "%s: a pattern is taken by RDF_TEXT_DATE and RDF_TEXT_TIMESTAMP only", fn);
    if (pattern_bytes < 0) return fail(RDF_INVALID_ARGUMENT, "%s: negative pattern length %lld", fn, (long long)pattern_bytes);
    int64_t pos = 0;
    const int err = textconv_compile(pattern, pattern_bytes, for_parse, pt, &pos);
    if (err != TC_OK) return fail(RDF_INVALID_ARGUMENT, "%s: the pattern does not compile: %s at position %lld", fn, textconv_compile_message(err), (long long)pos);
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_utf8_parse(const rdf_utf8_array* chunks, int64_t nchunks, int32_t kind, int32_t unit, const uint8_t* pattern, int64_t pattern_bytes,
                          rdf_out* out, int64_t* failed) {
    const char* fn = "utf8_parse";
    TcPattern pt;
    RDF_TRY(textconv_check_call(fn, kind, unit, true, pattern, pattern_bytes, &pt));
    if (nchunks < 0 || (nchunks > 0 && (!chunks || !out))) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    if (nchunks == 0) return RDF_OK;
    // ---- dtypes, memory kinds, validity buffers, capacities: in this order, each over the whole call
    for (int64_t c = 0; c < nchunks; ++c) {
        const rdf_utf8_array& u = chunks[c];
        if (u.offsets.dtype != RDF_I32 || u.offsets.length < 1)
            return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: offsets must be an Int32 array of rows + 1 entries", fn, (long long)c);
        if (u.data.dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: data must be a UInt8 array", fn, (long long)c);
    }
    const int out_dt = kind == RDF_TEXT_BOOL ? RDF_BOOL : kind == RDF_TEXT_DATE ? RDF_I32 : kind == RDF_TEXT_TIMESTAMP ? RDF_I64 : out[0].dtype;
    for (int64_t c = 0; c < nchunks; ++c) {
        if (kind == RDF_TEXT_INT && (out[c].dtype == RDF_F32 || out[c].dtype == RDF_F64)) return fail(RDF_COMPUTE_ERROR, "%s does not support type %d", fn, out[c].dtype);
        if (kind == RDF_TEXT_INT && !tc_is_int_dtype(out[c].dtype)) return fail(RDF_INVALID_ARGUMENT, "%s: output dtype %d is no integer type", fn, out[c].dtype);
        if (out[c].dtype != out_dt) return fail(RDF_INVALID_ARGUMENT, "%s: output dtype %d, expected %d", fn, out[c].dtype, out_dt);
    }
    int32_t mem = -1;
    for (int64_t c = 0; c < nchunks; ++c) {
        RDF_TRY(check_mem(&chunks[c].offsets, 1, &mem));
        RDF_TRY(check_mem(&chunks[c].data, 1, &mem));
    }
    RDF_TRY(check_out_mem(out, nchunks, mem));
    for (int64_t c = 0; c < nchunks; ++c)
        if (!out[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld needs a validity buffer (a row that does not parse is NULL)", fn, (long long)c);
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = chunks[c].offsets.length - 1;
        row_start[(size_t)c + 1] = row_start[(size_t)c] + rows;
        if (out[c].capacity < rows) {
            out[c].length = rows;
            return fail(RDF_MEMORY_ERROR, "%s: output %lld: capacity %lld below the %lld rows", fn, (long long)c, (long long)out[c].capacity, (long long)rows);
        }
        if (rows > 0 && !out[c].values) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: null values pointer", fn, (long long)c);
    }
    const int64_t n = row_start[(size_t)nchunks];
    if (n == 0) {
        for (int64_t c = 0; c < nchunks; ++c) { out[c].length = 0; out[c].null_count = 0; if (failed) failed[c] = 0; }
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

    const size_t es = out_dt == RDF_BOOL ? 0 : (size_t)dtype_size(out_dt);
    Region outr;
    std::vector<int> oi((size_t)nchunks * 2, -1);
    if (mem == RDF_MEM_HOST) {
        for (int64_t c = 0; c < nchunks; ++c) {
            const int64_t rows = chunks[c].offsets.length - 1;
            if (rows == 0) continue;
            oi[2 * c] = outr.add(out[c].values, es ? (size_t)rows * es : (size_t)((rows + 7) / 8));
            oi[2 * c + 1] = outr.add(out[c].validity, (size_t)((rows + 7) / 8));
        }
        RDF_TRY(outr.layout());
    }
    TableBuilder tb;
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_out = tb.reserve(sizeof(TcParseOut) * (size_t)nchunks);
    const size_t o_cnt = tb.reserve(sizeof(unsigned long long) * (size_t)nchunks * 2);
    const size_t o_pat = tb.reserve(pattern ? sizeof(TcPattern) : 0);
    RDF_TRY(tb.bind(pin_off));
    int64_t* hts = tb.at<int64_t>(o_ts);
    TcParseOut* hout = tb.at<TcParseOut>(o_out);
    hts[0] = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = chunks[c].offsets.length - 1;
        hts[c + 1] = hts[c] + (rows + kTcTile - 1) / kTcTile;
        if (mem == RDF_MEM_HOST) {
            hout[c].values = oi[2 * c] >= 0 ? outr.ptr(oi[2 * c]) : nullptr;
            hout[c].valid = oi[2 * c + 1] >= 0 ? (uint8_t*)outr.ptr(oi[2 * c + 1]) : nullptr;
        } else {
            hout[c].values = out[c].values;
            hout[c].valid = out[c].validity;
        }
    }
    memset(tb.at<char>(o_cnt), 0, sizeof(unsigned long long) * (size_t)nchunks * 2);
    if (pattern) memcpy(tb.at<char>(o_pat), &pt, sizeof(TcPattern));
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(pin_off));

    TcParseArgs a;
    memset(&a, 0, sizeof a);
    a.chunks = d.ucols[0].d_chunks;
    a.nchunks = nchunks;
    a.tile_start = tb.dev_at<int64_t>(o_ts);
    a.ntiles = hts[nchunks];
    a.outs = tb.dev_at<TcParseOut>(o_out);
    a.pattern = pattern ? tb.dev_at<TcPattern>(o_pat) : nullptr;
    a.kind = kind; a.unit = unit; a.dtype = out_dt;
    a.stage = ctx.opt_textconv_stage;
    a.nulls = tb.dev_at<unsigned long long>(o_cnt);
    a.failed = a.nulls + nchunks;
    KernelTimer kt;
    ctx.last_kernel = "textconv_parse_kernel";
    HIP_TRY(launch_textconv_parse(a, ctx.stream));
    kt.stop();
    HIP_TRY(hipMemcpyAsync(tb.at<char>(o_cnt), a.nulls, sizeof(unsigned long long) * (size_t)nchunks * 2, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    std::vector<unsigned long long> cnt((size_t)nchunks * 2);
    memcpy(cnt.data(), tb.at<char>(o_cnt), sizeof(unsigned long long) * (size_t)nchunks * 2);   // (the download below reuses the staging buffer)
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(pinned_reserve(outr.small_bytes));
        RDF_TRY(outr.download(0));
    }
    for (int64_t c = 0; c < nchunks; ++c) {
        out[c].length = chunks[c].offsets.length - 1;
        out[c].null_count = (int64_t)cnt[(size_t)c];
        if (failed) failed[c] = (int64_t)cnt[(size_t)(nchunks + c)];
    }
    return RDF_OK;
}

rdf_status rdf_utf8_format(const rdf_array* arr, int64_t nchunks, int32_t kind, int32_t unit, const uint8_t* pattern, int64_t pattern_bytes,
                           rdf_out* out_offsets, rdf_out* out_data) {
    const char* fn = "utf8_format";
    TcPattern pt;
    RDF_TRY(textconv_check_call(fn, kind, unit, false, pattern, pattern_bytes, &pt));
    if (nchunks < 0 || (nchunks > 0 && (!arr || !out_offsets || !out_data))) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    if (nchunks == 0) return RDF_OK;
    // ---- dtypes, memory kinds, validity buffers, capacities: in this order, each over the whole call
    const bool temporal = kind == RDF_TEXT_DATE || kind == RDF_TEXT_TIMESTAMP;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int dt = arr[c].dtype;
        if (dt == RDF_F32 || dt == RDF_F64) return fail(RDF_COMPUTE_ERROR, "%s does not support type %d", fn, dt);
        if (temporal && dt != RDF_I32 && dt != RDF_I64) return fail(RDF_COMPUTE_ERROR, "%s does not support type %d", fn, dt);
        if (kind == RDF_TEXT_BOOL && dt != RDF_BOOL) return fail(RDF_INVALID_ARGUMENT, "%s: RDF_TEXT_BOOL takes RDF_BOOL chunks, not dtype %d", fn, dt);
        if (kind == RDF_TEXT_INT && !tc_is_int_dtype(dt)) return fail(RDF_INVALID_ARGUMENT, "%s: RDF_TEXT_INT takes an integer dtype, not %d", fn, dt);
        if (dt != arr[0].dtype) return fail(RDF_INVALID_ARGUMENT, "%s: the chunks of a column share one storage type", fn);
    }
    if (temporal && unit == RDF_TIME_DAY && arr[0].dtype != RDF_I32) return fail(RDF_INVALID_ARGUMENT, "%s: RDF_TIME_DAY values are Int32 day numbers", fn);
    for (int64_t c = 0; c < nchunks; ++c)
        if (out_offsets[c].dtype != RDF_I32 || out_data[c].dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: outputs are (Int32 offsets, UInt8 data)", fn);
    int32_t mem = -1;
    RDF_TRY(check_mem(arr, nchunks, &mem));
    RDF_TRY(check_out_mem(out_offsets, nchunks, mem));
    RDF_TRY(check_out_mem(out_data, nchunks, mem));
    for (int64_t c = 0; c < nchunks; ++c) {
        if (!out_offsets[c].values || out_offsets[c].capacity < 1) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld has no offsets buffer", fn, (long long)c);
        if (out_data[c].capacity < 0 || (out_data[c].capacity > 0 && !out_data[c].values))
            return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: data capacity without a buffer", fn, (long long)c);
        if (arr[c].validity && !out_offsets[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld needs a validity buffer", fn, (long long)c);
    }
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = arr[c].length;
        row_start[(size_t)c + 1] = row_start[(size_t)c] + rows;
        if (out_offsets[c].capacity < rows + 1) {
            out_offsets[c].length = rows + 1;
            return fail(RDF_MEMORY_ERROR, "%s: output %lld: offsets need %lld entries", fn, (long long)c, (long long)(rows + 1));
        }
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();
    const int64_t n = row_start[(size_t)nchunks];

    rdf_sort_key key;
    memset(&key, 0, sizeof key);
    key.values = arr;
    size_t pin_off = 0;
    LexKeysOnDevice d;
    RDF_TRY(lexsort_keys_to_device(&key, 1, nchunks, mem, row_start, fn, pin_off, d));

    TableBuilder tb;
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_pat = tb.reserve(pattern ? sizeof(TcPattern) : 0);
    RDF_TRY(tb.bind(pin_off));
    RDF_TRY(tb.alloc());
    int64_t* hts = tb.at<int64_t>(o_ts);
    hts[0] = 0;
    for (int64_t c = 0; c < nchunks; ++c) hts[c + 1] = hts[c] + (arr[c].length + kTcTile - 1) / kTcTile;
    const int64_t ntiles = hts[nchunks];
    const std::vector<int64_t> tile_start(hts, hts + nchunks + 1);   // (the staging buffer may move when it grows)
    if (pattern) memcpy(tb.at<char>(o_pat), &pt, sizeof(TcPattern));
    RDF_TRY(tb.upload(pin_off));
    pin_off += (tb.size + 255) & ~(size_t)255;

    void *pblen, *pbscan, *ptot, *pnulls;
    RDF_TRY(arena_alloc((size_t)(n + 1) * 8, &pblen));
    RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &pbscan));
    RDF_TRY(arena_alloc((size_t)nchunks * 8, &ptot));
    RDF_TRY(arena_alloc((size_t)nchunks * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, (size_t)nchunks * 8, ctx.stream));

    TcFormatArgs a;
    memset(&a, 0, sizeof a);
    a.chunks = d.tb.dev_at<DevChunkCol>(d.o_ch);
    a.row_start = d.tb.dev_at<int64_t>(d.o_rs);
    a.tile_start = tb.dev_at<int64_t>(o_ts);
    a.nchunks = nchunks;
    a.ntiles = ntiles;
    a.n = n;
    a.pattern = pattern ? tb.dev_at<TcPattern>(o_pat) : nullptr;
    a.kind = kind; a.unit = unit; a.dtype = arr[0].dtype;
    a.max_row = textconv_max_row_bytes(kind, unit, pattern ? &pt : nullptr);
    a.blen = (int64_t*)pblen;
    a.bscan = (const int64_t*)pbscan;
    a.nulls = (unsigned long long*)pnulls;
    a.tot = (int64_t*)ptot;
    KernelTimer kt;
    ctx.last_kernel = "textconv_size_kernel + textconv_write_kernel";
    HIP_TRY(launch_textconv_size(a, ctx.stream));
    HIP_TRY(launch_scan(a.blen, (int64_t*)pbscan, n, (int64_t*)pbscan + n + 1, ctx.stream));
    HIP_TRY(launch_textconv_totals(a, ctx.stream));
    const size_t totb = (size_t)nchunks * 8;
    RDF_TRY(pinned_reserve(pin_off + 2 * totb + 64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, ptot, totb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + totb, pnulls, totb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    std::vector<int64_t> tot((size_t)nchunks), nulls((size_t)nchunks);
    memcpy(tot.data(), ctx.pinned + pin_off, totb);
    memcpy(nulls.data(), ctx.pinned + pin_off + totb, totb);
    pin_off += (2 * totb + 64 + 63) & ~(size_t)63;

    // ---- the sizing rule: every length reported, nothing written unless every chunk fits
    for (int64_t o = 0; o < nchunks; ++o)
        if (tot[(size_t)o] > INT32_MAX) {
            kt.stop();
            return fail(RDF_COMPUTE_ERROR, "%s: output %lld holds %lld bytes, beyond the Int32 offsets", fn, (long long)o, (long long)tot[(size_t)o]);
        }
    bool fits = true;
    for (int64_t o = 0; o < nchunks; ++o) {
        out_data[o].length = tot[(size_t)o];
        out_offsets[o].length = arr[o].length + 1;
        if (out_data[o].capacity < tot[(size_t)o]) fits = false;
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
            const int64_t rows = arr[o].length, bytes = tot[(size_t)o];
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
    int64_t obyte = 0;
    for (int64_t o = 0; o < nchunks; ++o) {
        Utf8OutChunk& u = ho[o];
        memset(&u, 0, sizeof u);
        u.rows = arr[o].length;
        u.bytes = tot[(size_t)o];
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
        u.byte_start = obyte;
        u.tile_start = tile_start[(size_t)o];
        obyte += u.bytes;
    }
    RDF_TRY(to.upload(pin_off));
    a.outs = to.dev_at<Utf8OutChunk>(o_outs);
    HIP_TRY(launch_textconv_write(a, ctx.stream));
    kt.stop();
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(pinned_reserve(outr.small_bytes));
        RDF_TRY(outr.download(0));
    }
    for (int64_t o = 0; o < nchunks; ++o) {
        out_offsets[o].null_count = nulls[(size_t)o];
        out_data[o].null_count = 0;
    }
    return RDF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// rdf_utf8_parse_float / rdf_utf8_format_float (kernels: rdf_textfloat.hip, per-row decisions: rdf_textfloat.h).  The checks,
// their order and their messages are those of the two calls above.
//   parse    ... -> ONE kernel -> the counters read back -> only when some chunk has undecided rows: the resolve kernel
//   format   size pass -> scan -> totals -> the sizing rule -> write pass
rdf_status rdf_utf8_parse_float(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out, int64_t* failed) {
    const char* fn = "utf8_parse_float";
    if (nchunks < 0 || (nchunks > 0 && (!chunks || !out))) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    if (nchunks == 0) return RDF_OK;
    for (int64_t c = 0; c < nchunks; ++c) {
        const rdf_utf8_array& u = chunks[c];
        if (u.offsets.dtype != RDF_I32 || u.offsets.length < 1)
            return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: offsets must be an Int32 array of rows + 1 entries", fn, (long long)c);
        if (u.data.dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: data must be a UInt8 array", fn, (long long)c);
    }
    const int out_dt = out[0].dtype;
    for (int64_t c = 0; c < nchunks; ++c) {
        if (out[c].dtype != RDF_F32 && out[c].dtype != RDF_F64) return fail(RDF_COMPUTE_ERROR, "%s does not support type %d", fn, out[c].dtype);
        if (out[c].dtype != out_dt) return fail(RDF_INVALID_ARGUMENT, "%s: output dtype %d, expected %d", fn, out[c].dtype, out_dt);
    }
    int32_t mem = -1;
    for (int64_t c = 0; c < nchunks; ++c) {
        RDF_TRY(check_mem(&chunks[c].offsets, 1, &mem));
        RDF_TRY(check_mem(&chunks[c].data, 1, &mem));
    }
    RDF_TRY(check_out_mem(out, nchunks, mem));
    for (int64_t c = 0; c < nchunks; ++c)
        if (!out[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld needs a validity buffer (a row that does not parse is NULL)", fn, (long long)c);
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = chunks[c].offsets.length - 1;
        row_start[(size_t)c + 1] = row_start[(size_t)c] + rows;
        if (out[c].capacity < rows) {
            out[c].length = rows;
            return fail(RDF_MEMORY_ERROR, "%s: output %lld: capacity %lld below the %lld rows", fn, (long long)c, (long long)out[c].capacity, (long long)rows);
        }
        if (rows > 0 && !out[c].values) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: null values pointer", fn, (long long)c);
    }
    const int64_t n = row_start[(size_t)nchunks];
    if (n == 0) {
        for (int64_t c = 0; c < nchunks; ++c) { out[c].length = 0; out[c].null_count = 0; if (failed) failed[c] = 0; }
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

    const size_t es = (size_t)dtype_size(out_dt);
    Region outr;
    std::vector<int> oi((size_t)nchunks * 2, -1);
    if (mem == RDF_MEM_HOST) {
        for (int64_t c = 0; c < nchunks; ++c) {
            const int64_t rows = chunks[c].offsets.length - 1;
            if (rows == 0) continue;
            oi[2 * c] = outr.add(out[c].values, (size_t)rows * es);
            oi[2 * c + 1] = outr.add(out[c].validity, (size_t)((rows + 7) / 8));
        }
        RDF_TRY(outr.layout());
    }
    TableBuilder tb;
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_out = tb.reserve(sizeof(TcParseOut) * (size_t)nchunks);
    const size_t o_cnt = tb.reserve(sizeof(unsigned long long) * (size_t)nchunks * 3);
    RDF_TRY(tb.bind(pin_off));
    int64_t* hts = tb.at<int64_t>(o_ts);
    TcParseOut* hout = tb.at<TcParseOut>(o_out);
    hts[0] = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = chunks[c].offsets.length - 1;
        hts[c + 1] = hts[c] + (rows + kTcTile - 1) / kTcTile;
        if (mem == RDF_MEM_HOST) {
            hout[c].values = oi[2 * c] >= 0 ? outr.ptr(oi[2 * c]) : nullptr;
            hout[c].valid = oi[2 * c + 1] >= 0 ? (uint8_t*)outr.ptr(oi[2 * c + 1]) : nullptr;
        } else {
            hout[c].values = out[c].values;
            hout[c].valid = out[c].validity;
        }
    }
    const int64_t ntiles = hts[nchunks];
    memset(tb.at<char>(o_cnt), 0, sizeof(unsigned long long) * (size_t)nchunks * 3);
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(pin_off));
    void* pflags;
    RDF_TRY(arena_alloc((size_t)ntiles * (kTcTile / 64) * sizeof(uint64_t), &pflags));

    TfParseArgs a;
    memset(&a, 0, sizeof a);
    a.chunks = d.ucols[0].d_chunks;
    a.nchunks = nchunks;
    a.tile_start = tb.dev_at<int64_t>(o_ts);
    a.ntiles = ntiles;
    a.outs = tb.dev_at<TcParseOut>(o_out);
    a.f32 = out_dt == RDF_F32;
    a.stage = ctx.opt_textconv_stage;
    a.exact = ctx.opt_textfloat_exact;
    a.nulls = tb.dev_at<unsigned long long>(o_cnt);
    a.failed = a.nulls + nchunks;
    a.undecided = a.nulls + 2 * nchunks;
    a.flags = (uint64_t*)pflags;
    KernelTimer kt;
    ctx.last_kernel = "textfloat_parse_kernel";
    HIP_TRY(launch_textfloat_parse(a, ctx.stream));
    HIP_TRY(hipMemcpyAsync(tb.at<char>(o_cnt), a.nulls, sizeof(unsigned long long) * (size_t)nchunks * 3, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    std::vector<unsigned long long> cnt((size_t)nchunks * 3);
    memcpy(cnt.data(), tb.at<char>(o_cnt), sizeof(unsigned long long) * (size_t)nchunks * 3);   // (the download below reuses the staging buffer)
    unsigned long long undecided = 0;
    for (int64_t c = 0; c < nchunks; ++c) undecided += cnt[(size_t)(2 * nchunks + c)];
    if (undecided) {
        ctx.last_kernel = "textfloat_parse_kernel + textfloat_resolve_kernel";
        HIP_TRY(launch_textfloat_resolve(a, ctx.stream));
    }
    kt.stop();
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(pinned_reserve(outr.small_bytes));
        RDF_TRY(outr.download(0));
    }
    for (int64_t c = 0; c < nchunks; ++c) {
        out[c].length = chunks[c].offsets.length - 1;
        out[c].null_count = (int64_t)cnt[(size_t)c];
        if (failed) failed[c] = (int64_t)cnt[(size_t)(nchunks + c)];
    }
    return RDF_OK;
}

rdf_status rdf_utf8_format_float(const rdf_array* arr, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    const char* fn = "utf8_format_float";
    if (nchunks < 0 || (nchunks > 0 && (!arr || !out_offsets || !out_data))) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    if (nchunks == 0) return RDF_OK;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int dt = arr[c].dtype;
        if (dt != RDF_F32 && dt != RDF_F64) return fail(RDF_COMPUTE_ERROR, "%s does not support type %d", fn, dt);
        if (dt != arr[0].dtype) return fail(RDF_INVALID_ARGUMENT, "%s: the chunks of a column share one storage type", fn);
    }
    for (int64_t c = 0; c < nchunks; ++c)
        if (out_offsets[c].dtype != RDF_I32 || out_data[c].dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: outputs are (Int32 offsets, UInt8 data)", fn);
    int32_t mem = -1;
    RDF_TRY(check_mem(arr, nchunks, &mem));
    RDF_TRY(check_out_mem(out_offsets, nchunks, mem));
    RDF_TRY(check_out_mem(out_data, nchunks, mem));
    for (int64_t c = 0; c < nchunks; ++c) {
        if (!out_offsets[c].values || out_offsets[c].capacity < 1) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld has no offsets buffer", fn, (long long)c);
        if (out_data[c].capacity < 0 || (out_data[c].capacity > 0 && !out_data[c].values))
            return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: data capacity without a buffer", fn, (long long)c);
        if (arr[c].validity && !out_offsets[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld needs a validity buffer", fn, (long long)c);
    }
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = arr[c].length;
        row_start[(size_t)c + 1] = row_start[(size_t)c] + rows;
        if (out_offsets[c].capacity < rows + 1) {
            out_offsets[c].length = rows + 1;
            return fail(RDF_MEMORY_ERROR, "%s: output %lld: offsets need %lld entries", fn, (long long)c, (long long)(rows + 1));
        }
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();
    const int64_t n = row_start[(size_t)nchunks];

    rdf_sort_key key;
    memset(&key, 0, sizeof key);
    key.values = arr;
    size_t pin_off = 0;
    LexKeysOnDevice d;
    RDF_TRY(lexsort_keys_to_device(&key, 1, nchunks, mem, row_start, fn, pin_off, d));

    TableBuilder tb;
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    RDF_TRY(tb.bind(pin_off));
    RDF_TRY(tb.alloc());
    int64_t* hts = tb.at<int64_t>(o_ts);
    hts[0] = 0;
    for (int64_t c = 0; c < nchunks; ++c) hts[c + 1] = hts[c] + (arr[c].length + kTcTile - 1) / kTcTile;
    const int64_t ntiles = hts[nchunks];
    const std::vector<int64_t> tile_start(hts, hts + nchunks + 1);   // (the staging buffer may move when it grows)
    RDF_TRY(tb.upload(pin_off));
    pin_off += (tb.size + 255) & ~(size_t)255;

    void *pblen, *pbscan, *ptot, *pnulls;
    RDF_TRY(arena_alloc((size_t)(n + 1) * 8, &pblen));
    RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &pbscan));
    RDF_TRY(arena_alloc((size_t)nchunks * 8, &ptot));
    RDF_TRY(arena_alloc((size_t)nchunks * 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, (size_t)nchunks * 8, ctx.stream));

    TcFormatArgs a;
    memset(&a, 0, sizeof a);
    a.chunks = d.tb.dev_at<DevChunkCol>(d.o_ch);
    a.row_start = d.tb.dev_at<int64_t>(d.o_rs);
    a.tile_start = tb.dev_at<int64_t>(o_ts);
    a.nchunks = nchunks;
    a.ntiles = ntiles;
    a.n = n;
    a.dtype = arr[0].dtype;
    a.max_row = a.dtype == RDF_F32 ? kTfMaxRowF32 : kTfMaxRowF64;
    a.blen = (int64_t*)pblen;
    a.bscan = (const int64_t*)pbscan;
    a.nulls = (unsigned long long*)pnulls;
    a.tot = (int64_t*)ptot;
    KernelTimer kt;
    ctx.last_kernel = "textfloat_size_kernel + textfloat_write_kernel";
    HIP_TRY(launch_textfloat_size(a, ctx.stream));
    HIP_TRY(launch_scan(a.blen, (int64_t*)pbscan, n, (int64_t*)pbscan + n + 1, ctx.stream));
    HIP_TRY(launch_textconv_totals(a, ctx.stream));
    const size_t totb = (size_t)nchunks * 8;
    RDF_TRY(pinned_reserve(pin_off + 2 * totb + 64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, ptot, totb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + totb, pnulls, totb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    std::vector<int64_t> tot((size_t)nchunks), nulls((size_t)nchunks);
    memcpy(tot.data(), ctx.pinned + pin_off, totb);
    memcpy(nulls.data(), ctx.pinned + pin_off + totb, totb);
    pin_off += (2 * totb + 64 + 63) & ~(size_t)63;

    // ---- the sizing rule: every length reported, nothing written unless every chunk fits
    for (int64_t o = 0; o < nchunks; ++o)
        if (tot[(size_t)o] > INT32_MAX) {
            kt.stop();
            return fail(RDF_COMPUTE_ERROR, "%s: output %lld holds %lld bytes, beyond the Int32 offsets", fn, (long long)o, (long long)tot[(size_t)o]);
        }
    bool fits = true;
    for (int64_t o = 0; o < nchunks; ++o) {
        out_data[o].length = tot[(size_t)o];
        out_offsets[o].length = arr[o].length + 1;
        if (out_data[o].capacity < tot[(size_t)o]) fits = false;
    }
    if (!fits) {
        kt.stop();
        return fail(RDF_MEMORY_ERROR, "%s: output capacity too small (the needed lengths are in out_data[i].length)", fn);
    }

    // ---- write
    Region outr;
    std::vector<int> oi((size_t)nchunks * 3, -1);
    if (mem == RDF_MEM_HOST) {
        for (int64_t o = 0; o < nchunks; ++o) {
            const int64_t rows = arr[o].length, bytes = tot[(size_t)o];
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
    int64_t obyte = 0;
    for (int64_t o = 0; o < nchunks; ++o) {
        Utf8OutChunk& u = ho[o];
        memset(&u, 0, sizeof u);
        u.rows = arr[o].length;
        u.bytes = tot[(size_t)o];
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
        u.byte_start = obyte;
        u.tile_start = tile_start[(size_t)o];
        obyte += u.bytes;
    }
    RDF_TRY(to.upload(pin_off));
    a.outs = to.dev_at<Utf8OutChunk>(o_outs);
    HIP_TRY(launch_textfloat_write(a, ctx.stream));
    kt.stop();
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(pinned_reserve(outr.small_bytes));
        RDF_TRY(outr.download(0));
    }
    for (int64_t o = 0; o < nchunks; ++o) {
        out_offsets[o].null_count = nulls[(size_t)o];
        out_data[o].null_count = 0;
    }
    return RDF_OK;
}

}  // extern "C"
