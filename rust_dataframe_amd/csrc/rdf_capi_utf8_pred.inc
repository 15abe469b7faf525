// rdf_capi_utf8_pred.inc — host side of rdf_utf8_predicate / rdf_utf8_compare / rdf_utf8_measure (kernel: rdf_utf8_pred.hip,
// the pattern compiler and the per-row functions: rdf_utf8_pattern.h); textually included by rdf_capi.cpp (it uses that
// file's per-thread context, arena and staging helpers, utf8_value_ranges and lexsort_keys_to_device).
//
// One call = every argument checked, the pattern compiled -> host inputs staged (device inputs aliased) with the staging of
// the Utf8 sort -> tile prefix, output descriptors, the compiled pattern and the NULL counters in one upload into the arena
// -> ONE kernel -> host outputs copied back.  Nothing is written to the caller's buffers by a call that is refused, except
// the `length` a too small output needs.

namespace {

static_assert(U8P_EQ == RDF_UTF8_EQ && U8P_GE == RDF_UTF8_GE && U8P_STARTS_WITH == RDF_UTF8_STARTS_WITH && U8P_ENDS_WITH == RDF_UTF8_ENDS_WITH &&
              U8P_CONTAINS == RDF_UTF8_CONTAINS && U8P_LIKE == RDF_UTF8_LIKE && U8P_NOPS == RDF_UTF8_LIKE + 1, "rdf_utf8_pattern.h restates rdf_utf8_pred_op");
static_assert(U8M_LENGTH == RDF_UTF8_LENGTH && U8M_OCTET_LENGTH == RDF_UTF8_OCTET_LENGTH && U8M_LOCATE == RDF_UTF8_LOCATE, "rdf_utf8_pattern.h restates rdf_utf8_measure_op");
static_assert(kUtf8PatternMax == RDF_UTF8_PATTERN_MAX, "rdf_utf8_pattern.h restates RDF_UTF8_PATTERN_MAX");

struct Utf8PredCall {
    const char* fn;
    int32_t family, measure, op, pos;
    const rdf_utf8_array* a;
    const rdf_utf8_array* b;      // compare
    int64_t nchunks;
    const Utf8Pattern* pattern;   // compiled, or nullptr
    rdf_out* outs;
    const uint8_t* regex;         // rdf_capi_utf8_regex.inc: a compiled regular expression's image instead of a pattern
    int64_t regex_bytes;
};

// the literal / pattern of a call, checked and compiled
rdf_status utf8_pred_compile(const char* fn, int op, const uint8_t* pattern, int64_t pattern_bytes, int32_t escape, Utf8Pattern* out) {
    if (pattern_bytes < 0) return fail(RDF_INVALID_ARGUMENT, "%s: negative pattern length %lld", fn, (long long)pattern_bytes);
    if (pattern_bytes > RDF_UTF8_PATTERN_MAX) return fail(RDF_INVALID_ARGUMENT, "%s: a pattern of %lld bytes, at most %d", fn, (long long)pattern_bytes, RDF_UTF8_PATTERN_MAX);
    if (!pattern && pattern_bytes > 0) return fail(RDF_INVALID_ARGUMENT, "%s: null pattern", fn);
    switch (utf8_pattern_compile(op, pattern, pattern_bytes, escape, out)) {
        case U8P_OK: return RDF_OK;
        case U8P_BAD_ESCAPE: return fail(RDF_INVALID_ARGUMENT, "%s: escape %d: -1, or one ASCII byte 1..127 other than '%%' and '_'", fn, escape);
        case U8P_LONE_ESCAPE: return fail(RDF_INVALID_ARGUMENT, "%s: the pattern ends in a lone escape", fn);
        case U8P_TOO_MANY_SEGMENTS: return fail(RDF_INVALID_ARGUMENT, "%s: more than %d segments between '%%'", fn, kUtf8PatternSegs);
        default: return fail(RDF_INVALID_ARGUMENT, "%s: the pattern does not compile", fn);
    }
}

rdf_status utf8_pred_run(const Utf8PredCall& q) {
    const char* fn = q.fn;
    const int64_t nchunks = q.nchunks;
    const bool two = q.family == UTF8_FAM_COMPARE;
    if (nchunks < 0 || (nchunks > 0 && (!q.a || !q.outs || (two && !q.b)))) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    if (nchunks == 0) return RDF_OK;
    const int out_dt = q.measure ? RDF_I32 : RDF_BOOL;
    const int ncols = two ? 2 : 1;
    const rdf_utf8_array* cols[2] = {q.a, q.b};
    // ---- dtypes, memory kinds, validity buffers, row counts, capacities: in this order, each over the whole call
    for (int k = 0; k < ncols; ++k)
        for (int64_t c = 0; c < nchunks; ++c) {
            const rdf_utf8_array& u = cols[k][c];
            if (u.offsets.dtype != RDF_I32 || u.offsets.length < 1)
                return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: offsets must be an Int32 array of rows + 1 entries", fn, (long long)c);
            if (u.data.dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: data must be a UInt8 array", fn, (long long)c);
        }
    for (int64_t c = 0; c < nchunks; ++c)
        if (q.outs[c].dtype != out_dt) return fail(RDF_INVALID_ARGUMENT, "%s: output dtype %d, expected %d", fn, q.outs[c].dtype, out_dt);
    int32_t mem = -1;
    for (int k = 0; k < ncols; ++k)
        for (int64_t c = 0; c < nchunks; ++c) {
            RDF_TRY(check_mem(&cols[k][c].offsets, 1, &mem));
            RDF_TRY(check_mem(&cols[k][c].data, 1, &mem));
        }
    RDF_TRY(check_out_mem(q.outs, nchunks, mem));
    for (int64_t c = 0; c < nchunks; ++c) {
        const bool nullable = q.a[c].offsets.validity || (two && q.b[c].offsets.validity);
        if (nullable && !q.outs[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld needs a validity buffer", fn, (long long)c);
    }
    if (two)
        for (int64_t c = 0; c < nchunks; ++c)
            if (q.a[c].offsets.length != q.b[c].offsets.length)
                return fail(RDF_COMPUTE_ERROR, "%s: chunk %lld: the columns' chunk lengths differ", fn, (long long)c);
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = q.a[c].offsets.length - 1;
        row_start[(size_t)c + 1] = row_start[(size_t)c] + rows;
        if (q.outs[c].capacity < rows) {
            q.outs[c].length = rows;
            return fail(RDF_MEMORY_ERROR, "%s: output %lld: capacity %lld below the %lld rows", fn, (long long)c, (long long)q.outs[c].capacity, (long long)rows);
        }
        if (rows > 0 && !q.outs[c].values) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: null values pointer", fn, (long long)c);
    }
    const int64_t n = row_start[(size_t)nchunks];
    if (n == 0) {
        for (int64_t c = 0; c < nchunks; ++c) { q.outs[c].length = 0; q.outs[c].null_count = 0; }
        return RDF_OK;
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();

    // ---- inputs on the device: the value ranges checked, host arrays staged, the Utf8Chunk tables built
    rdf_sort_key keys[2];
    memset(keys, 0, sizeof keys);
    keys[0].utf8 = q.a;
    keys[1].utf8 = q.b;
    size_t pin_off = 0;
    LexKeysOnDevice d;
    RDF_TRY(lexsort_keys_to_device(keys, ncols, nchunks, mem, row_start, fn, pin_off, d));

    // ---- NULL rows per chunk: known from the inputs' null_count where that is given, counted by the kernel otherwise
    std::vector<int64_t> nulls((size_t)nchunks, -1);
    bool counting = false;
    for (int64_t c = 0; c < nchunks; ++c) {
        const rdf_array& oa = q.a[c].offsets;
        const rdf_array* ob = two ? &q.b[c].offsets : nullptr;
        const bool va = oa.validity != nullptr, vb = ob && ob->validity;
        if (!va && !vb) nulls[(size_t)c] = 0;
        else if (va && !vb && oa.null_count >= 0) nulls[(size_t)c] = oa.null_count;
        else if (vb && !va && ob->null_count >= 0) nulls[(size_t)c] = ob->null_count;
        else counting = true;
    }

    Region outr;
    std::vector<int> oi((size_t)nchunks * 2, -1);
    if (mem == RDF_MEM_HOST) {
        for (int64_t c = 0; c < nchunks; ++c) {
            const int64_t rows = q.a[c].offsets.length - 1;
            if (rows == 0) continue;
            oi[2 * c] = outr.add(q.outs[c].values, q.measure ? (size_t)rows * 4 : (size_t)((rows + 7) / 8));
            if (q.outs[c].validity) oi[2 * c + 1] = outr.add(q.outs[c].validity, (size_t)((rows + 7) / 8));
        }
        RDF_TRY(outr.layout());
    }
    TableBuilder tb;
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_out = tb.reserve(sizeof(Utf8PredOut) * (size_t)nchunks);
    const size_t o_nulls = tb.reserve(sizeof(unsigned long long) * (size_t)nchunks);
    const size_t o_pat = tb.reserve(q.pattern ? sizeof(Utf8Pattern) : q.regex ? (size_t)q.regex_bytes : 0);
    RDF_TRY(tb.bind(pin_off));
    int64_t* hts = tb.at<int64_t>(o_ts);
    Utf8PredOut* hout = tb.at<Utf8PredOut>(o_out);
    hts[0] = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t rows = q.a[c].offsets.length - 1;
        hts[c + 1] = hts[c] + (rows + kUtf8PredThreads - 1) / kUtf8PredThreads;
        if (mem == RDF_MEM_HOST) {
            hout[c].values = oi[2 * c] >= 0 ? outr.ptr(oi[2 * c]) : nullptr;
            hout[c].valid = oi[2 * c + 1] >= 0 ? (uint8_t*)outr.ptr(oi[2 * c + 1]) : nullptr;
        } else {
            hout[c].values = q.outs[c].values;
            hout[c].valid = q.outs[c].validity;
        }
    }
    memset(tb.at<char>(o_nulls), 0, sizeof(unsigned long long) * (size_t)nchunks);
    if (q.pattern) memcpy(tb.at<char>(o_pat), q.pattern, sizeof(Utf8Pattern));
    if (q.regex) memcpy(tb.at<char>(o_pat), q.regex, (size_t)q.regex_bytes);
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(pin_off));

    Utf8PredArgs a;
    memset(&a, 0, sizeof a);
    a.a = d.ucols[0].d_chunks;
    a.b = two ? d.ucols[1].d_chunks : nullptr;
    a.nchunks = nchunks;
    a.tile_start = tb.dev_at<int64_t>(o_ts);
    a.ntiles = hts[nchunks];
    a.outs = tb.dev_at<Utf8PredOut>(o_out);
    a.pattern = q.pattern ? tb.dev_at<Utf8Pattern>(o_pat) : nullptr;
    a.family = q.family; a.measure = q.measure; a.op = q.op; a.pos = q.pos;
    a.nulls = counting ? tb.dev_at<unsigned long long>(o_nulls) : nullptr;
    KernelTimer kt;
    a.regex = q.regex ? tb.dev_at<uint8_t>(o_pat) : nullptr;
    ctx.last_kernel = q.regex ? "utf8_regex_measure_kernel" : "utf8_pred_kernel";
    if (q.regex) HIP_TRY(launch_utf8_regex_measure(a, q.regex_bytes, ctx.stream));
    else HIP_TRY(launch_utf8_pred(a, ctx.stream));
    kt.stop();
    if (counting) HIP_TRY(hipMemcpyAsync(tb.at<char>(o_nulls), a.nulls, sizeof(unsigned long long) * (size_t)nchunks, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    for (int64_t c = 0; c < nchunks; ++c)
        if (nulls[(size_t)c] < 0) nulls[(size_t)c] = (int64_t)tb.at<unsigned long long>(o_nulls)[c];
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(pinned_reserve(outr.small_bytes));
        RDF_TRY(outr.download(0));
    }
    for (int64_t c = 0; c < nchunks; ++c) {
        q.outs[c].length = q.a[c].offsets.length - 1;
        q.outs[c].null_count = nulls[(size_t)c];
    }
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_utf8_predicate(int32_t op, const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes,
                              int32_t escape, rdf_out* mask) {
    if (op < RDF_UTF8_EQ || op > RDF_UTF8_LIKE) return fail(RDF_INVALID_ARGUMENT, "utf8_predicate: unknown operation %d", op);
    Utf8Pattern pt;
    RDF_TRY(utf8_pred_compile("utf8_predicate", op, pattern, pattern_bytes, escape, &pt));
    const bool scans = pt.kind == U8P_CONTAINS || pt.kind == U8P_LIKE;
    Utf8PredCall q = {"utf8_predicate", scans ? UTF8_FAM_SCAN : UTF8_FAM_LITERAL, 0, pt.kind, 0, chunks, nullptr, nchunks, &pt, mask};
    return utf8_pred_run(q);
}

rdf_status rdf_utf8_compare(int32_t op, const rdf_utf8_array* a, const rdf_utf8_array* b, int64_t nchunks, rdf_out* mask) {
    if (op < RDF_UTF8_EQ || op > RDF_UTF8_GE) return fail(RDF_INVALID_ARGUMENT, "utf8_compare: operation %d is not one of the six comparisons", op);
    Utf8PredCall q = {"utf8_compare", UTF8_FAM_COMPARE, 0, op, 0, a, b, nchunks, nullptr, mask};
    return utf8_pred_run(q);
}

rdf_status rdf_utf8_measure(int32_t what, const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes,
                            int64_t pos, rdf_out* out) {
    if (what < RDF_UTF8_LENGTH || what > RDF_UTF8_LOCATE) return fail(RDF_INVALID_ARGUMENT, "utf8_measure: unknown operation %d", what);
    Utf8Pattern pt;
    const bool locate = what == RDF_UTF8_LOCATE;
    if (locate) RDF_TRY(utf8_pred_compile("utf8_measure", U8P_CONTAINS, pattern, pattern_bytes, -1, &pt));
    // a position beyond Int32 is beyond every row (a chunk's bytes are Int32 offsets): 0 for every row, like pos < 1
    const int32_t p32 = pos > INT32_MAX ? 0 : (int32_t)std::max<int64_t>(0, pos);
    Utf8PredCall q = {"utf8_measure", what == RDF_UTF8_OCTET_LENGTH ? UTF8_FAM_LITERAL : UTF8_FAM_SCAN, 1, what, locate ? p32 : 0, chunks, nullptr,
                      nchunks, locate ? &pt : nullptr, out};
    return utf8_pred_run(q);
}

}  // extern "C"
