// rdf_capi_select.inc — host side of rdf_null_test / rdf_coalesce / rdf_case_when / rdf_extremum / rdf_nanvl (kernels:
// rdf_select.hip, what is decided about a row: rdf_select.h); textually included by rdf_capi.cpp (it uses that file's
// per-thread context, arena and staging helpers).
//
// One call = every argument checked, in the order the header lists -> host inputs staged (device inputs aliased) -> chunk,
// tile and output tables in one upload -> ONE kernel (+ the NULL counts per chunk when anything can be NULL) -> host outputs
// copied back.  A refused call writes nothing to the caller's buffers; the one exception the header names is a capacity
// below the rows, which sets every chunk's `length` to the rows it needs.

namespace {

static_assert(SEL_IS_NULL == RDF_IS_NULL && SEL_IS_NOT_NULL == RDF_IS_NOT_NULL && SEL_IS_NAN == RDF_IS_NAN && SEL_NTESTS == RDF_IS_NAN + 1,
              "rdf_select.h restates rdf_null_test_op");
static_assert(kSelMaxParts == RDF_SELECT_PARTS_MAX, "rdf_select.h restates RDF_SELECT_PARTS_MAX");

struct SelCall {
    const char* fn;
    SelKind kind;
    int32_t op;                         // null_test: the test; extremum: greatest != 0
    const rdf_array* a;                 // null_test: the column
    const rdf_value_part* parts;        // [nparts] coalesce / extremum; case_when: the branches' values
    int32_t nparts;
    const rdf_array* const* conds;      // case_when: [nparts]
    const rdf_value_part* otherwise;    // case_when, may be nullptr
    const rdf_value_part* pair[2];      // nanvl: a, b
    int64_t nchunks;
    rdf_out* out;
};

// the value slots of a call in the kernel's order: parts, then (case_when) `otherwise`; an absent `otherwise` is the NULL literal
struct SelSlots {
    rdf_value_part v[kSelSlots];
    int n = 0;
};

bool sel_never_null(const rdf_value_part& p, int64_t c) { return p.column ? p.column[c].validity == nullptr : p.literal_is_null == 0; }

rdf_status sel_run(const SelCall& q) {
    const char* fn = q.fn;
    const int64_t nchunks = q.nchunks;
    const bool test = q.kind == SEL_K_NULL_TEST, cw = q.kind == SEL_K_CASE_WHEN;
    // 3. lists
    if (nchunks < 0) return fail(RDF_INVALID_ARGUMENT, "%s: negative nchunks", fn);
    if (nchunks == 0) return RDF_OK;
    if (!q.out) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    SelSlots sl;
    if (test) {
        if (!q.a) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    } else if (q.kind == SEL_K_NANVL) {
        if (!q.pair[0] || !q.pair[1]) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
        sl.v[0] = *q.pair[0]; sl.v[1] = *q.pair[1]; sl.n = 2;
    } else {
        if (!q.parts || (cw && !q.conds)) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
        for (int k = 0; k < q.nparts; ++k) {
            if (cw && !q.conds[k]) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
            sl.v[sl.n++] = q.parts[k];
        }
        if (cw) {
            if (q.otherwise) sl.v[sl.n++] = *q.otherwise;
            else sl.v[sl.n++] = rdf_value_part{nullptr, 0, 1};
        }
    }
    // 4. / 5. parts
    const rdf_array* first = test ? q.a : nullptr;
    for (int k = 0; k < sl.n && !first; ++k) first = sl.v[k].column;
    if (!first) return fail(RDF_INVALID_ARGUMENT, "%s: no column part", fn);
    for (int k = 0; k < sl.n; ++k)
        if (sl.v[k].column && sl.v[k].literal_is_null != 0) return fail(RDF_INVALID_ARGUMENT, "%s: part %d is a column and a NULL literal", fn, k);
    // 8. conditions
    if (cw)
        for (int k = 0; k < q.nparts; ++k)
            for (int64_t c = 0; c < nchunks; ++c)
                if (q.conds[k][c].dtype != RDF_BOOL) return fail(RDF_INVALID_ARGUMENT, "%s: condition %d is not RDF_BOOL", fn, k);
    // 9. one dtype
    const int dt = first[0].dtype, out_dt = test ? (int)RDF_BOOL : dt;
    for (int k = 0; k < (test ? 1 : sl.n); ++k) {
        const rdf_array* col = test ? q.a : sl.v[k].column;
        if (!col) continue;
        for (int64_t c = 0; c < nchunks; ++c)
            if (col[c].dtype != dt) return fail(RDF_INVALID_ARGUMENT, "%s: the value dtypes differ (%d, %d)", fn, col[c].dtype, dt);
    }
    for (int64_t c = 0; c < nchunks; ++c)
        if (q.out[c].dtype != out_dt) return fail(RDF_INVALID_ARGUMENT, "%s: output dtype %d, expected %d", fn, q.out[c].dtype, out_dt);
    // 10. one memory kind
    int32_t mem = -1;
    if (test) {   // (values are never read by IS_NULL / IS_NOT_NULL and may be NULL)
        for (int64_t c = 0; c < nchunks; ++c) {
            const rdf_array& x = q.a[c];
            if (x.mem != RDF_MEM_HOST && x.mem != RDF_MEM_DEVICE) return fail(RDF_INVALID_ARGUMENT, "bad mem tag %d", x.mem);
            if (mem < 0) mem = x.mem;
            else if (mem != x.mem) return fail(RDF_INVALID_ARGUMENT, "all arrays of one call must share one memory space");
            if (x.length < 0 || x.offset < 0) return fail(RDF_INVALID_ARGUMENT, "negative length/offset");
            if (q.op == RDF_IS_NAN && x.length > 0 && !x.values) return fail(RDF_INVALID_ARGUMENT, "null values pointer");
        }
    } else {
        for (int k = 0; k < sl.n; ++k)
            if (sl.v[k].column) RDF_TRY(check_mem(sl.v[k].column, nchunks, &mem));
        if (cw)
            for (int k = 0; k < q.nparts; ++k) RDF_TRY(check_mem(q.conds[k], nchunks, &mem));
    }
    RDF_TRY(check_out_mem(q.out, nchunks, mem));
    // 11. the bitmap, where the arguments say a row can be NULL
    std::vector<char> nullable((size_t)nchunks, 0);
    bool counting = false;
    for (int64_t c = 0; c < nchunks && !test; ++c) {
        bool n;
        if (q.kind == SEL_K_COALESCE || q.kind == SEL_K_EXTREMUM) {
            n = true;
            for (int k = 0; k < sl.n; ++k) n = n && !sel_never_null(sl.v[k], c);
        } else {   // case_when (an absent `otherwise` is the NULL literal of the last slot), nanvl
            n = false;
            for (int k = 0; k < sl.n; ++k) n = n || !sel_never_null(sl.v[k], c);
        }
        nullable[(size_t)c] = n;
        counting |= n;
        if (n && !q.out[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output validity buffer required", fn);
    }
    // 12. the dtype
    const bool dtype_ok = test ? (q.op == RDF_IS_NAN ? is_float(dt) : (dt >= RDF_I8 && dt <= RDF_BOOL))
                               : (q.kind == SEL_K_NANVL ? is_float(dt) : is_numeric(dt));
    if (!dtype_ok) return fail(RDF_COMPUTE_ERROR, "%s does not support type %d", fn, dt);
    // 13. the row counts
    int64_t rows = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t len = first[c].length;
        rows += len;
        for (int k = 0; k < sl.n; ++k)
            if (sl.v[k].column && sl.v[k].column[c].length != len) return fail(RDF_COMPUTE_ERROR, "%s: chunk %lld: the parts' row counts differ", fn, (long long)c);
        if (cw)
            for (int k = 0; k < q.nparts; ++k)
                if (q.conds[k][c].length != len) return fail(RDF_COMPUTE_ERROR, "%s: chunk %lld: a condition's row count differs", fn, (long long)c);
    }
    for (int64_t c = 0; c < nchunks; ++c)
        if (first[c].length > 0 && !q.out[c].values) return fail(RDF_INVALID_ARGUMENT, "%s: null output values pointer", fn);
    // 14. the capacity
    for (int64_t c = 0; c < nchunks; ++c)
        if (q.out[c].capacity < first[c].length) {
            for (int64_t i = 0; i < nchunks; ++i) q.out[i].length = first[i].length;
            return fail(RDF_MEMORY_ERROR, "%s: output capacity too small", fn);
        }
    if (rows == 0) {
        for (int64_t c = 0; c < nchunks; ++c) { q.out[c].length = 0; q.out[c].null_count = 0; }
        return RDF_OK;
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();

    // ---- inputs on the device (host arrays staged, device arrays aliased), outputs of a host call in the arena
    // IS_NULL / IS_NOT_NULL read a column's bitmap only: it is staged as the values of a Boolean array
    InputStager in;
    std::vector<rdf_array> bitmaps;
    const bool bits_only = test && q.op != RDF_IS_NAN;
    if (bits_only) {
        bitmaps.assign(q.a, q.a + nchunks);
        for (auto& x : bitmaps) {
            x.values = x.validity;
            if (!x.validity) x.length = 0;
            x.validity = nullptr;
            x.dtype = RDF_BOOL;
        }
        for (auto& x : bitmaps) in.add(&x);
    } else if (test) {
        for (int64_t c = 0; c < nchunks; ++c) in.add(&q.a[c]);
    } else {
        for (int k = 0; k < sl.n; ++k)
            if (sl.v[k].column) for (int64_t c = 0; c < nchunks; ++c) in.add(&sl.v[k].column[c]);
        if (cw)
            for (int k = 0; k < q.nparts; ++k) for (int64_t c = 0; c < nchunks; ++c) in.add(&q.conds[k][c]);
    }
    const size_t ncols = in.arrays.size() / (size_t)nchunks;
    size_t pin_off = 0, used = 0;
    RDF_TRY(in.finish(pin_off, &used));
    pin_off += (used + 255) & ~(size_t)255;
    const size_t es_out = (size_t)dtype_size(out_dt);
    Region outr;
    std::vector<int> oi((size_t)nchunks * 2, -1);
    if (mem == RDF_MEM_HOST) {
        for (int64_t c = 0; c < nchunks; ++c) {
            const int64_t len = first[c].length;
            if (len == 0) continue;
            oi[2 * c] = outr.add(q.out[c].values, test ? (size_t)((len + 7) / 8) : (size_t)len * es_out);   // (an item is padded by 16 bytes: the last 64-bit word fits)
            if (q.out[c].validity) oi[2 * c + 1] = outr.add(q.out[c].validity, (size_t)((len + 7) / 8));
        }
        RDF_TRY(outr.layout());
    }

    // ---- tables: chunk descriptors, row and tile prefixes, output descriptors; the NULL counts come back into the same place
    TableBuilder tb;
    const size_t o_ch = tb.reserve(sizeof(DevChunkCol) * (size_t)nchunks * ncols);
    const size_t o_rs = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_out = tb.reserve(sizeof(DtOut) * (size_t)nchunks);
    const size_t o_slots = tb.reserve(sizeof(SelSlotDesc) * (size_t)kSelSlots);
    int64_t longest = 0;
    for (int64_t c = 0; c < nchunks; ++c) longest = std::max(longest, first[c].length);
    int64_t split = std::min<int64_t>(kDtMaxNullSplit, std::max<int64_t>(1, longest / (8 * kCsTile)));
    while (split > 1 && nchunks * split > std::max<int64_t>(nchunks, 1 << 16)) split /= 2;
    const size_t o_nulls = tb.reserve(sizeof(int64_t) * (size_t)(nchunks * split));
    RDF_TRY(tb.bind(pin_off));
    DevChunkCol* hch = tb.at<DevChunkCol>(o_ch);
    int64_t* hrs = tb.at<int64_t>(o_rs);
    int64_t* hts = tb.at<int64_t>(o_ts);
    DtOut* hout = tb.at<DtOut>(o_out);
    hrs[0] = hts[0] = 0;
    for (size_t i = 0; i < (size_t)nchunks * ncols; ++i) hch[i] = in.dev[i];
    if (bits_only)
        for (int64_t c = 0; c < nchunks; ++c)
            hch[c] = q.a[c].validity ? DevChunkCol{nullptr, (const uint8_t*)in.dev[(size_t)c].values, in.dev[(size_t)c].offset} : DevChunkCol{nullptr, nullptr, 0};
    for (int64_t c = 0; c < nchunks; ++c) {
        hrs[c + 1] = hrs[c] + first[c].length;
        hts[c + 1] = hts[c] + (first[c].length + kCsTile - 1) / kCsTile;
        if (mem == RDF_MEM_HOST) {
            hout[c].values = oi[2 * c] >= 0 ? outr.ptr(oi[2 * c]) : nullptr;
            hout[c].validity = oi[2 * c + 1] >= 0 ? (uint8_t*)outr.ptr(oi[2 * c + 1]) : nullptr;
        } else {
            hout[c].values = q.out[c].values;
            hout[c].validity = q.out[c].validity;
        }
    }
    memset(tb.at<int64_t>(o_nulls), 0, sizeof(int64_t) * (size_t)(nchunks * split));
    SelArgs a;
    memset(&a, 0, sizeof a);
    a.col.nchunks = nchunks;
    a.col.n = hrs[nchunks];
    a.col.ntiles = hts[nchunks];
    RDF_TRY(tb.alloc());
    const DevChunkCol* dch = tb.dev_at<DevChunkCol>(o_ch);
    a.es = dtype_size(dt);
    SelSlotDesc* hsl = tb.at<SelSlotDesc>(o_slots);
    memset(hsl, 0, sizeof(SelSlotDesc) * (size_t)kSelSlots);
    if (!test) {
        size_t at = 0;
        a.nparts = sl.n;
        const uint64_t keep = a.es == 8 ? ~0ull : ((1ull << (8 * a.es)) - 1);
        for (int k = 0; k < sl.n; ++k) {
            if (sl.v[k].column) { hsl[k].col = dch + at; at += (size_t)nchunks; }
            else if (sl.v[k].literal_is_null) hsl[k].lit_null = 1;
            else hsl[k].lit = sl.v[k].literal_bits & keep;
        }
        if (cw) {
            a.nconds = q.nparts;
            for (int k = 0; k < q.nparts; ++k) { hsl[k].cond = dch + at; at += (size_t)nchunks; }
        }
    }
    RDF_TRY(tb.upload(pin_off));
    if (test) a.col.chunks = dch;
    a.slots = tb.dev_at<SelSlotDesc>(o_slots);
    a.col.row_start = tb.dev_at<int64_t>(o_rs);
    a.col.tile_start = tb.dev_at<int64_t>(o_ts);
    a.outs = tb.dev_at<DtOut>(o_out);
    a.kind = q.kind;
    a.op = q.op;
    a.cls = is_float(dt) ? SEL_FLOAT : is_signed_int(dt) ? SEL_SIGNED : SEL_UNSIGNED;
    if (counting) {
        void* wn = nullptr;
        RDF_TRY(arena_alloc(sizeof(uint32_t) * (size_t)a.col.ntiles * (kCsThreads / 64), &wn));
        a.wave_nulls = (uint32_t*)wn;
        a.chunk_nulls = tb.dev_at<int64_t>(o_nulls);
        a.null_split = split;
    }
    KernelTimer kt;
    ctx.last_kernel = test ? "sel_null_test_kernel" : q.kind == SEL_K_EXTREMUM ? "sel_extremum_kernel" : q.kind == SEL_K_NANVL ? "sel_nanvl_kernel" : "sel_choose_kernel";
    HIP_TRY(launch_select(a, ctx.stream));
    kt.stop();
    if (counting) HIP_TRY(hipMemcpyAsync(tb.at<int64_t>(o_nulls), a.chunk_nulls, sizeof(int64_t) * (size_t)(nchunks * split), hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    std::vector<int64_t> nulls((size_t)nchunks, 0);
    for (int64_t c = 0; c < nchunks; ++c)
        for (int64_t k = 0; k < split; ++k) nulls[(size_t)c] += tb.at<int64_t>(o_nulls)[c * split + k];
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(pinned_reserve(outr.small_bytes));
        RDF_TRY(outr.download(0));
    }
    for (int64_t c = 0; c < nchunks; ++c) {
        q.out[c].length = first[c].length;
        q.out[c].null_count = nulls[(size_t)c];
    }
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_null_test(int32_t op, const rdf_array* a, int64_t nchunks, rdf_out* mask) {
    if (op < RDF_IS_NULL || op > RDF_IS_NAN) return fail(RDF_INVALID_ARGUMENT, "null_test: unknown test %d", op);
    SelCall q = {"null_test", SEL_K_NULL_TEST, op, a, nullptr, 0, nullptr, nullptr, {nullptr, nullptr}, nchunks, mask};
    return sel_run(q);
}

rdf_status rdf_coalesce(const rdf_value_part* parts, int32_t nparts, int64_t nchunks, rdf_out* out) {
    if (nparts < 1 || nparts > RDF_SELECT_PARTS_MAX) return fail(RDF_INVALID_ARGUMENT, "coalesce: 1 to %d parts", RDF_SELECT_PARTS_MAX);
    SelCall q = {"coalesce", SEL_K_COALESCE, 0, nullptr, parts, nparts, nullptr, nullptr, {nullptr, nullptr}, nchunks, out};
    return sel_run(q);
}

rdf_status rdf_case_when(const rdf_array* const* conds, const rdf_value_part* values, int32_t nbranches, const rdf_value_part* otherwise, int64_t nchunks, rdf_out* out) {
    if (nbranches < 1 || nbranches > RDF_SELECT_PARTS_MAX) return fail(RDF_INVALID_ARGUMENT, "case_when: 1 to %d branches", RDF_SELECT_PARTS_MAX);
    SelCall q = {"case_when", SEL_K_CASE_WHEN, 0, nullptr, values, nbranches, conds, otherwise, {nullptr, nullptr}, nchunks, out};
    return sel_run(q);
}

rdf_status rdf_extremum(int32_t greatest, const rdf_value_part* parts, int32_t nparts, int64_t nchunks, rdf_out* out) {
    if (nparts < 2 || nparts > RDF_SELECT_PARTS_MAX) return fail(RDF_INVALID_ARGUMENT, "extremum: 2 to %d parts", RDF_SELECT_PARTS_MAX);
    SelCall q = {greatest ? "greatest" : "least", SEL_K_EXTREMUM, greatest != 0, nullptr, parts, nparts, nullptr, nullptr, {nullptr, nullptr}, nchunks, out};
    return sel_run(q);
}

rdf_status rdf_nanvl(const rdf_value_part* a, const rdf_value_part* b, int64_t nchunks, rdf_out* out) {
    SelCall q = {"nanvl", SEL_K_NANVL, 0, nullptr, nullptr, 2, nullptr, nullptr, {a, b}, nchunks, out};
    return sel_run(q);
}

}  // extern "C"
