// rdf_capi_datetime.inc — host side of rdf_datetime_fields / rdf_datetime_trunc / rdf_date_shift / rdf_date_diff (kernels:
// rdf_datetime.hip, calendar arithmetic: rdf_datetime.h); textually included by rdf_capi.cpp (it uses that file's per-thread
// context, arena and staging helpers).
//
// One call = every argument checked -> host inputs staged (device inputs aliased) -> chunk, tile and output tables in one
// upload -> ONE kernel (+ the NULL counts per chunk when anything can be NULL) -> host outputs copied back.  Nothing is
// written to the caller's buffers, lengths and NULL counts included, by a call that is refused.

namespace {

static_assert(DT_UNIT_S == RDF_TIME_SECOND && DT_UNIT_MS == RDF_TIME_MILLISECOND && DT_UNIT_US == RDF_TIME_MICROSECOND &&
              DT_UNIT_NS == RDF_TIME_NANOSECOND && DT_UNIT_DAY == RDF_TIME_DAY, "rdf_datetime.h restates rdf_time_unit");
static_assert(DT_YEAR == RDF_DT_YEAR && DT_WEEK_OF_YEAR == RDF_DT_WEEK_OF_YEAR && DT_HOUR == RDF_DT_HOUR && DT_DATE == RDF_DT_DATE &&
              DT_NFIELDS == RDF_DT_DATE + 1, "rdf_datetime.h restates rdf_datetime_field");
static_assert(DT_TRUNC_YEAR == RDF_TRUNC_YEAR && DT_TRUNC_WEEK == RDF_TRUNC_WEEK && DT_TRUNC_DAY == RDF_TRUNC_DAY &&
              DT_TRUNC_SECOND == RDF_TRUNC_SECOND && DT_NLEVELS == RDF_TRUNC_SECOND + 1, "rdf_datetime.h restates rdf_trunc_level");
static_assert(DT_SHIFT_DAYS == RDF_SHIFT_DAYS && DT_SHIFT_MONTHS == RDF_SHIFT_MONTHS && DT_SHIFT_LAST_DAY == RDF_SHIFT_LAST_DAY &&
              DT_SHIFT_NEXT_DAY == RDF_SHIFT_NEXT_DAY && DT_NSHIFTS == RDF_SHIFT_NEXT_DAY + 1, "rdf_datetime.h restates rdf_date_shift_op");

enum DtKind { DT_K_FIELDS, DT_K_TRUNC, DT_K_SHIFT, DT_K_DIFF };

struct DtCall {
    const char* fn;
    DtKind kind;
    const rdf_array* a;      // the column
    const rdf_array* b;      // amounts (shift, optional) / start (diff)
    int64_t nchunks;
    int32_t unit, unit_b, op, amount, nfields;
    const int32_t* fields;
    rdf_out* outs;           // [nout * nchunks]
    int nout;
};

bool dt_unit_ok(int32_t unit) { return unit >= RDF_TIME_SECOND && unit <= RDF_TIME_DAY; }

// a temporal column's storage: Int32 or Int64, one dtype for the list; RDF_TIME_DAY (Date32) is Int32
rdf_status dt_check_storage(const DtCall& q, const rdf_array* col, int32_t unit) {
    for (int64_t c = 0; c < q.nchunks; ++c) {
        if (col[c].dtype != RDF_I32 && col[c].dtype != RDF_I64) return fail(RDF_COMPUTE_ERROR, "%s does not support type %d", q.fn, col[c].dtype);
        if (col[c].dtype != col[0].dtype) return fail(RDF_INVALID_ARGUMENT, "%s: the chunks of a column share one storage type", q.fn);
    }
    if (unit == RDF_TIME_DAY && col[0].dtype != RDF_I32) return fail(RDF_INVALID_ARGUMENT, "%s: RDF_TIME_DAY values are Int32 day numbers", q.fn);
    return RDF_OK;
}

rdf_status dt_run(const DtCall& q) {
    const char* fn = q.fn;
    const int64_t nchunks = q.nchunks;
    const bool need_b = q.kind == DT_K_DIFF;
    if (nchunks < 0 || (nchunks > 0 && (!q.a || !q.outs || (need_b && !q.b)))) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk lists", fn);
    if (nchunks == 0) return RDF_OK;
    RDF_TRY(dt_check_storage(q, q.a, q.unit));
    if (q.kind == DT_K_DIFF) RDF_TRY(dt_check_storage(q, q.b, q.unit_b));
    if (q.kind == DT_K_SHIFT && q.b)
        for (int64_t c = 0; c < nchunks; ++c)
            if (q.b[c].dtype != RDF_I32) return fail(RDF_INVALID_ARGUMENT, "%s: the amounts are an Int32 column", fn);
    if (q.b)
        for (int64_t c = 0; c < nchunks; ++c)
            if (q.b[c].length != q.a[c].length) return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: the columns' chunk lengths differ", fn, (long long)c);
    int32_t mem = -1;
    RDF_TRY(check_mem(q.a, nchunks, &mem));
    if (q.b) RDF_TRY(check_mem(q.b, nchunks, &mem));
    const int out_dt = q.kind == DT_K_TRUNC ? q.a[0].dtype : RDF_I32;
    const bool rows_can_fail = q.kind == DT_K_SHIFT && q.op == RDF_SHIFT_NEXT_DAY && q.b;   // a weekday outside 1..7 is a NULL row
    bool counting = rows_can_fail;
    int64_t rows = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        const bool nullable = q.a[c].validity || (q.b && q.b[c].validity) || rows_can_fail;
        counting |= nullable;
        rows += q.a[c].length;
        for (int f = 0; f < q.nout; ++f) {
            const rdf_out& o = q.outs[(int64_t)f * nchunks + c];
            if (o.dtype != out_dt) return fail(RDF_INVALID_ARGUMENT, "%s: output dtype %d, expected %d", fn, o.dtype, out_dt);
            RDF_TRY(check_out_mem(&o, 1, mem));
            if (nullable && !o.validity) return fail(RDF_INVALID_ARGUMENT, "%s: output validity buffer required", fn);
            if (o.capacity < q.a[c].length) return fail(RDF_MEMORY_ERROR, "%s: output capacity too small", fn);
            if (q.a[c].length > 0 && !o.values) return fail(RDF_INVALID_ARGUMENT, "%s: null output values pointer", fn);
        }
    }
    if (rows == 0) {
        for (int64_t i = 0; i < (int64_t)q.nout * nchunks; ++i) { q.outs[i].length = 0; q.outs[i].null_count = 0; }
        return RDF_OK;
    }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();

    // ---- inputs on the device (host arrays staged, device arrays aliased), outputs of a host call in the arena
    InputStager in;
    const int ncols = q.b ? 2 : 1;
    for (int64_t c = 0; c < nchunks; ++c) in.add(&q.a[c]);
    if (q.b) for (int64_t c = 0; c < nchunks; ++c) in.add(&q.b[c]);
    size_t pin_off = 0, used = 0;
    RDF_TRY(in.finish(pin_off, &used));
    pin_off += (used + 255) & ~(size_t)255;
    const size_t es_out = (size_t)dtype_size(out_dt);
    const size_t nouts = (size_t)q.nout * (size_t)nchunks;
    Region outr;
    std::vector<int> oi(nouts * 2, -1);
    if (mem == RDF_MEM_HOST) {
        for (size_t i = 0; i < nouts; ++i) {
            const int64_t len = q.a[i % (size_t)nchunks].length;
            if (len == 0) continue;
            oi[2 * i] = outr.add(q.outs[i].values, (size_t)len * es_out);
            if (q.outs[i].validity) oi[2 * i + 1] = outr.add(q.outs[i].validity, (size_t)((len + 7) / 8));   // (an item is padded by 16 bytes: the last 64-bit word fits)
        }
        RDF_TRY(outr.layout());
    }

    // ---- tables: chunk descriptors, row and tile prefixes, output descriptors; the NULL counts come back into the same place
    TableBuilder tb;
    const size_t o_ch = tb.reserve(sizeof(DevChunkCol) * (size_t)nchunks * (size_t)ncols);
    const size_t o_rs = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_out = tb.reserve(sizeof(DtOut) * nouts);
    // the NULL counts of a chunk are added up in `split` slices (a long chunk has thousands of wave counts), as long as the
    // partial sums of all chunks stay a small table
    int64_t longest = 0;
    for (int64_t c = 0; c < nchunks; ++c) longest = std::max(longest, q.a[c].length);
    int64_t split = std::min<int64_t>(kDtMaxNullSplit, std::max<int64_t>(1, longest / (8 * kCsTile)));
    while (split > 1 && nchunks * split > std::max<int64_t>(nchunks, 1 << 16)) split /= 2;
    const size_t o_nulls = tb.reserve(sizeof(int64_t) * (size_t)(nchunks * split));
    RDF_TRY(tb.bind(pin_off));
    DevChunkCol* hch = tb.at<DevChunkCol>(o_ch);
    int64_t* hrs = tb.at<int64_t>(o_rs);
    int64_t* hts = tb.at<int64_t>(o_ts);
    DtOut* hout = tb.at<DtOut>(o_out);
    hrs[0] = hts[0] = 0;
    for (size_t i = 0; i < (size_t)nchunks * (size_t)ncols; ++i) hch[i] = in.dev[i];
    for (int64_t c = 0; c < nchunks; ++c) {
        hrs[c + 1] = hrs[c] + q.a[c].length;
        hts[c + 1] = hts[c] + (q.a[c].length + kCsTile - 1) / kCsTile;
    }
    for (size_t i = 0; i < nouts; ++i) {
        if (mem == RDF_MEM_HOST) {
            hout[i].values = oi[2 * i] >= 0 ? outr.ptr(oi[2 * i]) : nullptr;
            hout[i].validity = oi[2 * i + 1] >= 0 ? (uint8_t*)outr.ptr(oi[2 * i + 1]) : nullptr;
        } else {
            hout[i].values = q.outs[i].values;
            hout[i].validity = q.outs[i].validity;
        }
    }
    memset(tb.at<int64_t>(o_nulls), 0, sizeof(int64_t) * (size_t)(nchunks * split));
    DtArgs a;
    memset(&a, 0, sizeof a);
    a.col.nchunks = nchunks;
    a.col.n = hrs[nchunks];
    a.col.ntiles = hts[nchunks];
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(pin_off));
    const DevChunkCol* dch = tb.dev_at<DevChunkCol>(o_ch);
    a.col.chunks = dch;
    a.col.row_start = tb.dev_at<int64_t>(o_rs);
    a.col.tile_start = tb.dev_at<int64_t>(o_ts);
    if (q.b) a.b = dch + nchunks;
    a.outs = tb.dev_at<DtOut>(o_out);
    a.es = dtype_size(q.a[0].dtype);
    a.es_b = q.b ? dtype_size(q.b[0].dtype) : 0;
    a.unit = q.unit; a.unit_b = q.unit_b; a.op = q.op; a.amount = q.amount;
    a.nfields = q.nfields;
    for (int f = 0; f < q.nfields; ++f) {
        a.fields[f] = q.fields[f];
        if (dt_field_is_civil(q.fields[f])) a.need |= DT_NEED_CIVIL;
        if (dt_field_is_time(q.fields[f])) a.need |= DT_NEED_TIME;
    }
    if (counting) {
        void* wn = nullptr;
        RDF_TRY(arena_alloc(sizeof(uint32_t) * (size_t)a.col.ntiles * (kCsThreads / 64), &wn));
        a.wave_nulls = (uint32_t*)wn;
        a.chunk_nulls = tb.dev_at<int64_t>(o_nulls);
        a.null_split = split;
    }
    KernelTimer kt;
    switch (q.kind) {
        case DT_K_FIELDS: ctx.last_kernel = "dt_fields_kernel"; HIP_TRY(launch_dt_fields(a, ctx.stream)); break;
        case DT_K_TRUNC: ctx.last_kernel = "dt_trunc_kernel"; HIP_TRY(launch_dt_trunc(a, ctx.stream)); break;
        case DT_K_SHIFT: ctx.last_kernel = "dt_shift_kernel"; HIP_TRY(launch_dt_shift(a, ctx.stream)); break;
        default: ctx.last_kernel = "dt_diff_kernel"; HIP_TRY(launch_dt_diff(a, ctx.stream)); break;
    }
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
    for (int f = 0; f < q.nout; ++f)
        for (int64_t c = 0; c < nchunks; ++c) {
            rdf_out& o = q.outs[(int64_t)f * nchunks + c];
            o.length = q.a[c].length;
            o.null_count = nulls[(size_t)c];
        }
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_datetime_fields(const rdf_array* a, int64_t nchunks, int32_t unit, const int32_t* fields, int32_t nfields, rdf_out* outs) {
    if (!dt_unit_ok(unit)) return fail(RDF_INVALID_ARGUMENT, "datetime_fields: unknown time unit %d", unit);
    if (nfields < 1 || nfields > kDtMaxFields || !fields) return fail(RDF_INVALID_ARGUMENT, "datetime_fields: 1 to %d fields", kDtMaxFields);
    uint32_t seen = 0;
    for (int f = 0; f < nfields; ++f) {
        if (fields[f] < RDF_DT_YEAR || fields[f] > RDF_DT_DATE) return fail(RDF_INVALID_ARGUMENT, "datetime_fields: unknown field %d", fields[f]);
        if (seen & (1u << fields[f])) return fail(RDF_INVALID_ARGUMENT, "datetime_fields: field %d repeats", fields[f]);
        seen |= 1u << fields[f];
    }
    DtCall q = {"datetime_fields", DT_K_FIELDS, a, nullptr, nchunks, unit, 0, 0, 0, nfields, fields, outs, nfields};
    return dt_run(q);
}

rdf_status rdf_datetime_trunc(const rdf_array* a, int64_t nchunks, int32_t unit, int32_t level, rdf_out* out) {
    if (!dt_unit_ok(unit)) return fail(RDF_INVALID_ARGUMENT, "datetime_trunc: unknown time unit %d", unit);
    if (level < RDF_TRUNC_YEAR || level > RDF_TRUNC_SECOND) return fail(RDF_INVALID_ARGUMENT, "datetime_trunc: unknown level %d", level);
    if (!dt_trunc_level_ok(unit, level)) return fail(RDF_INVALID_ARGUMENT, "datetime_trunc: level %d is finer than the unit of RDF_TIME_DAY values", level);
    DtCall q = {"datetime_trunc", DT_K_TRUNC, a, nullptr, nchunks, unit, 0, level, 0, 0, nullptr, out, 1};
    return dt_run(q);
}

rdf_status rdf_date_shift(const rdf_array* a, int64_t nchunks, int32_t unit, int32_t op, const rdf_array* amounts, int32_t amount, rdf_out* out) {
    if (!dt_unit_ok(unit)) return fail(RDF_INVALID_ARGUMENT, "date_shift: unknown time unit %d", unit);
    if (op < RDF_SHIFT_DAYS || op > RDF_SHIFT_NEXT_DAY) return fail(RDF_INVALID_ARGUMENT, "date_shift: unknown operation %d", op);
    if (op == RDF_SHIFT_LAST_DAY && amounts) return fail(RDF_INVALID_ARGUMENT, "date_shift: last_day takes no amounts");
    if (op == RDF_SHIFT_NEXT_DAY && !amounts && (amount < 1 || amount > 7)) return fail(RDF_INVALID_ARGUMENT, "date_shift: next_day: weekday %d outside 1 (Sunday) .. 7 (Saturday)", amount);
    DtCall q = {"date_shift", DT_K_SHIFT, a, amounts, nchunks, unit, 0, op, amount, 0, nullptr, out, 1};
    return dt_run(q);
}

rdf_status rdf_date_diff(const rdf_array* end, int32_t end_unit, const rdf_array* start, int32_t start_unit, int64_t nchunks, rdf_out* out) {
    if (!dt_unit_ok(end_unit) || !dt_unit_ok(start_unit)) return fail(RDF_INVALID_ARGUMENT, "date_diff: unknown time unit %d / %d", end_unit, start_unit);
    DtCall q = {"date_diff", DT_K_DIFF, end, start, nchunks, end_unit, start_unit, 0, 0, 0, nullptr, out, 1};
    return dt_run(q);
}

}  // extern "C"
