// rdf_capi_moments.inc — host side of rdf_moments / rdf_comoments (kernels: rdf_moments.hip, merge formulas:
// rdf_moments.h); textually included by rdf_capi.cpp (it uses that file's per-thread context, arena and staging helpers).
//
//   rdf_moments / rdf_comoments   arguments checked -> chunks (and y, and the mask) staged with one tile table -> ONE kernel,
//                                 a state per block -> the states copied back and folded in block order with mo_merge
//   rdf_*_merge / rdf_*_stat      host only: they never touch the device

namespace {

rdf_status mo_check(const char* fn, bool pair, const rdf_array* x, const rdf_array* y, const rdf_array* mask, int64_t nchunks, const void* out, int64_t* rows) {
    if (!out) return fail(RDF_INVALID_ARGUMENT, "%s: null output state", fn);
    if (nchunks < 0 || (nchunks > 0 && (!x || (pair && !y)))) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk list", fn);
    int64_t n = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        if (!is_numeric(x[c].dtype) || x[c].dtype != x[0].dtype || (y && (!is_numeric(y[c].dtype) || y[c].dtype != y[0].dtype)))
            return fail(RDF_INVALID_ARGUMENT, "%s: numeric columns of one dtype each required", fn);
        if (mask && mask[c].dtype != RDF_BOOL) return fail(RDF_INVALID_ARGUMENT, "%s: the mask is a Boolean column", fn);
        if ((y && y[c].length != x[c].length) || (mask && mask[c].length != x[c].length))
            return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: the columns' chunk lengths differ", fn, (long long)c);
        n += x[c].length > 0 ? x[c].length : 0;
    }
    int32_t mem = -1;
    RDF_TRY(check_mem(x, nchunks, &mem));
    if (y) RDF_TRY(check_mem(y, nchunks, &mem));
    if (mask) RDF_TRY(check_mem(mask, nchunks, &mem));
    *rows = n;
    return RDF_OK;
}

// x (and y, and the mask) on the device with CsCol's tables, the kernel, the blocks' states on the host
template <class State>
rdf_status mo_run(const rdf_array* x, const rdf_array* y, const rdf_array* mask, int64_t nchunks, std::vector<State>& states) {
    Ctx& ctx = g_ctx;
    arena_begin();
    InputStager in;
    TableBuilder tb;
    const int ncols = 1 + (y ? 1 : 0) + (mask ? 1 : 0);
    for (int64_t c = 0; c < nchunks; ++c) in.add(&x[c]);
    if (y) for (int64_t c = 0; c < nchunks; ++c) in.add(&y[c]);
    if (mask) for (int64_t c = 0; c < nchunks; ++c) in.add(&mask[c]);
    size_t pin_off = 0, used = 0;
    RDF_TRY(in.finish(pin_off, &used));
    pin_off += (used + 255) & ~(size_t)255;
    const size_t o_ch = tb.reserve(sizeof(DevChunkCol) * (size_t)nchunks * (size_t)ncols);
    const size_t o_rs = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    const size_t o_ts = tb.reserve(sizeof(int64_t) * ((size_t)nchunks + 1));
    RDF_TRY(tb.bind(pin_off));
    DevChunkCol* hch = tb.at<DevChunkCol>(o_ch);
    int64_t* hrs = tb.at<int64_t>(o_rs);
    int64_t* hts = tb.at<int64_t>(o_ts);
    hrs[0] = hts[0] = 0;
    for (size_t i = 0; i < (size_t)nchunks * (size_t)ncols; ++i) hch[i] = in.dev[i];
    for (int64_t c = 0; c < nchunks; ++c) {
        hrs[c + 1] = hrs[c] + x[c].length;
        hts[c + 1] = hts[c] + (x[c].length + kCsTile - 1) / kCsTile;
    }
    MoArgs a;
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
    if (y) a.y = dch + nchunks;
    if (mask) a.mask = dch + (size_t)nchunks * (size_t)(ncols - 1);
    a.dt_x = x[0].dtype;
    a.dt_y = y ? y[0].dtype : x[0].dtype;
    const int grid = mo_grid(a.col.ntiles);
    RDF_TRY(arena_alloc(sizeof(State) * (size_t)grid, &a.out));
    KernelTimer kt;
    ctx.last_kernel = y ? "mo_comoments_kernel" : "mo_moments_kernel";
    HIP_TRY(y ? launch_mo_comoments(a, grid, ctx.stream) : launch_mo_moments(a, grid, ctx.stream));
    kt.stop();
    states.resize((size_t)grid);
    HIP_TRY(hipMemcpyAsync(states.data(), a.out, sizeof(State) * (size_t)grid, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_moments(const rdf_array* a, const rdf_array* mask, int64_t nchunks, rdf_moments_state* out) {
    int64_t rows = 0;
    RDF_TRY(mo_check("moments", false, a, nullptr, mask, nchunks, out, &rows));
    memset(out, 0, sizeof *out);
    if (rows == 0) return RDF_OK;
    RDF_TRY(ensure_ready());
    std::vector<rdf_moments_state> states;
    RDF_TRY(mo_run(a, nullptr, mask, nchunks, states));
    for (const rdf_moments_state& s : states) mo_merge(*out, s);
    return RDF_OK;
}

rdf_status rdf_comoments(const rdf_array* x, const rdf_array* y, const rdf_array* mask, int64_t nchunks, rdf_comoments_state* out) {
    int64_t rows = 0;
    RDF_TRY(mo_check("comoments", true, x, y, mask, nchunks, out, &rows));
    memset(out, 0, sizeof *out);
    if (rows == 0) return RDF_OK;
    RDF_TRY(ensure_ready());
    std::vector<rdf_comoments_state> states;
    RDF_TRY(mo_run(x, y, mask, nchunks, states));
    for (const rdf_comoments_state& s : states) mo_comerge(*out, s);
    return RDF_OK;
}

rdf_status rdf_moments_merge(rdf_moments_state* into, const rdf_moments_state* other) {
    if (!into || !other) return fail(RDF_INVALID_ARGUMENT, "moments_merge: null state");
    if (into->count < 0 || other->count < 0) return fail(RDF_INVALID_ARGUMENT, "moments_merge: negative count");
    mo_merge(*into, *other);
    return RDF_OK;
}

rdf_status rdf_comoments_merge(rdf_comoments_state* into, const rdf_comoments_state* other) {
    if (!into || !other) return fail(RDF_INVALID_ARGUMENT, "comoments_merge: null state");
    if (into->count < 0 || other->count < 0) return fail(RDF_INVALID_ARGUMENT, "comoments_merge: negative count");
    mo_comerge(*into, *other);
    return RDF_OK;
}

rdf_status rdf_moments_stat(const rdf_moments_state* s, int32_t stat, double* out, int32_t* out_is_some) {
    if (!s || !out || !out_is_some) return fail(RDF_INVALID_ARGUMENT, "moments_stat: null pointer");
    if (stat < RDF_STAT_MEAN || stat > RDF_STAT_KURTOSIS) return fail(RDF_INVALID_ARGUMENT, "moments_stat: unknown statistic %d", stat);
    *out_is_some = mo_stat(*s, stat, out) ? 1 : 0;
    return RDF_OK;
}

rdf_status rdf_comoments_stat(const rdf_comoments_state* s, int32_t stat, double* out, int32_t* out_is_some) {
    if (!s || !out || !out_is_some) return fail(RDF_INVALID_ARGUMENT, "comoments_stat: null pointer");
    if (stat < RDF_COSTAT_COVAR_POP || stat > RDF_COSTAT_CORR) return fail(RDF_INVALID_ARGUMENT, "comoments_stat: unknown statistic %d", stat);
    *out_is_some = mo_costat(*s, stat, out) ? 1 : 0;
    return RDF_OK;
}

}  // extern "C"
