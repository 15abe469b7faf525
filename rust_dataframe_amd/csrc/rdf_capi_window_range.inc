// rdf_capi_window_range.inc — host side of rdf_window_range_agg: the aggregates of rdf_window_agg over RANGE frames whose
// offsets are in the order key's units (kernels: rdf_window_range.hip, rules and sizes: rdf_window_range.h); textually
// included by rdf_capi.cpp after rdf_capi_window_agg.inc, whose front, scans, output handling and emit it shares.
//
// After the front: one gather of the order key into a sorted array, one bounds array per DISTINCT offset bound of the
// request (calls that share a bound share the array), then rdf_window_agg's scans and its emit in the form that reads the
// frame's ends from those arrays.

namespace {

static_assert(WR_UNBOUNDED_PRECEDING == RDF_BOUND_UNBOUNDED_PRECEDING && WR_PRECEDING == RDF_BOUND_PRECEDING && WR_CURRENT_ROW == RDF_BOUND_CURRENT_ROW &&
              WR_FOLLOWING == RDF_BOUND_FOLLOWING && WR_UNBOUNDED_FOLLOWING == RDF_BOUND_UNBOUNDED_FOLLOWING, "rdf_window_range.h restates rdf_frame_bound");
static_assert(sizeof(rdf_window_range_frame) == 40 && sizeof(rdf_window_range_call) == 48, "rdf_window_range_frame / _call layout");
static_assert(2 * RDF_WINDOW_MAX_CALLS == kWRangeMaxBounds, "two ends per call");

}  // namespace

rdf_status rdf_window_range_agg(const rdf_sort_key* partition_by, int32_t npartition, const rdf_sort_key* order_by, int32_t norder,
                                const rdf_array* const* values, int32_t nvalues, int64_t nchunks,
                                const rdf_window_range_call* calls, int32_t ncalls, rdf_out* outs) {
    // ---- everything that can be refused is refused before any device work
    RDF_TRY(window_front_counts("window_range_agg", calls, outs, ncalls, partition_by, npartition, order_by, norder));
    if (norder != 1) return fail(RDF_INVALID_ARGUMENT, "window_range_agg: a range offset needs exactly one order key");
    if (nchunks < 1) return fail(RDF_INVALID_ARGUMENT, "window_range_agg: bad arguments");
    if (!order_by[0].values || order_by[0].utf8) return fail(RDF_INVALID_ARGUMENT, "window_range_agg: the order key must be a numeric column");
    const int kdt = order_by[0].values[0].dtype;
    for (int64_t c = 0; c < nchunks; ++c)
        if ((kdt != RDF_I32 && kdt != RDF_I64 && kdt != RDF_F64) || order_by[0].values[c].dtype != kdt)
            return fail(RDF_INVALID_ARGUMENT, "window_range_agg: the order key must be Int32, Int64 or Float64");
    const bool kf64 = kdt == RDF_F64, desc = order_by[0].options.descending != 0;
    if (nvalues < 0 || nvalues > RDF_WINDOW_MAX_VALUES) return fail(RDF_INVALID_ARGUMENT, "window_range_agg: 0 .. %d value columns", RDF_WINDOW_MAX_VALUES);
    if (nvalues > 0 && !values) return fail(RDF_INVALID_ARGUMENT, "window_range_agg: null value list");
    int vdt[RDF_WINDOW_MAX_VALUES] = {};
    for (int v = 0; v < nvalues; ++v) {
        if (!values[v]) return fail(RDF_INVALID_ARGUMENT, "window_range_agg: value column %d is null", v);
        vdt[v] = values[v][0].dtype;
        for (int64_t c = 0; c < nchunks; ++c)
            if ((values[v][c].dtype != RDF_I64 && values[v][c].dtype != RDF_F64) || values[v][c].dtype != vdt[v])
                return fail(RDF_INVALID_ARGUMENT, "window_range_agg: value column %d: Int64 or Float64 chunks of one dtype", v);
    }
    for (int c = 0; c < ncalls; ++c) {
        const rdf_window_range_call& w = calls[c];
        const rdf_window_range_frame& f = w.frame;
        if (w.fn < RDF_WAGG_SUM || w.fn > RDF_WAGG_LAST_VALUE) return fail(RDF_INVALID_ARGUMENT, "window_range_agg: call %d: unknown function %d", c, w.fn);
        const bool reads = w.fn == RDF_WAGG_SUM || w.fn == RDF_WAGG_MIN || w.fn == RDF_WAGG_MAX || w.fn == RDF_WAGG_AVG;
        if (w.value >= nvalues || w.value < -1 || (w.value == -1 && reads))
            return fail(RDF_INVALID_ARGUMENT, "window_range_agg: call %d: value index %d out of range", c, w.value);
        const int bad = wr_check_frame(f.start_kind, f.end_kind, f.start_i, f.end_i, f.start_f, f.end_f, kf64);
        if (bad != WR_FRAME_OK) return fail(RDF_INVALID_ARGUMENT, "window_range_agg: call %d: %s", c, wr_frame_error(bad));
        if ((w.fn == RDF_WAGG_MIN || w.fn == RDF_WAGG_MAX) && f.start_kind != RDF_BOUND_UNBOUNDED_PRECEDING && f.end_kind != RDF_BOUND_UNBOUNDED_FOLLOWING)
            return fail(RDF_INVALID_ARGUMENT, "window_range_agg: call %d: min / max over a range frame bounded on both sides is not built", c);
        if (outs[c].dtype != window_agg_out_dtype(w.fn, w.value >= 0 ? vdt[w.value] : RDF_I64)) return fail(RDF_INVALID_ARGUMENT, "window_range_agg: call %d: wrong output dtype", c);
        if (w.fn != RDF_WAGG_COUNT && !outs[c].validity) return fail(RDF_INVALID_ARGUMENT, "window_range_agg: call %d: the result can be NULL and needs a validity bitmap", c);
    }
    WinFront wf;
    bool done = false;
    RDF_TRY(window_front_check("window_range_agg", partition_by, npartition, order_by, norder, values, nvalues, nchunks, 0, outs, ncalls, wf, &done));
    if (done) return RDF_OK;
    const int64_t n = wf.n, nch = wf.nch;
    const int32_t mem = wf.mem;
    const int route = g_ctx.opt_window_range_route;

    // ---- the distinct offset bounds.  An offset of zero is CURRENT ROW: the bound value is the row's own key, so a start
    // resolves to its first peer and an end to its last, for NULL / NaN rows by rule.
    WRangeBoundsArgs ba;
    memset(&ba, 0, sizeof ba);
    int bstart[RDF_WINDOW_MAX_CALLS], bend[RDF_WINDOW_MAX_CALLS];
    auto bound_of = [&](int is_end, int kind, int64_t si, double sf) -> int {
        if (!wr_is_offset(kind) || (kf64 ? sf == 0.0 : si == 0)) return -1;
        const WRBound b{is_end, kind == RDF_BOUND_FOLLOWING, kf64 ? 0 : (uint64_t)si, kf64 ? sf : 0.0};
        for (int i = 0; i < ba.nbounds; ++i)
            if (ba.bounds[i].is_end == b.is_end && ba.bounds[i].following == b.following && ba.bounds[i].s_i == b.s_i && ba.bounds[i].s_f == b.s_f) return i;
        ba.bounds[ba.nbounds] = b;
        return ba.nbounds++;
    };
    for (int c = 0; c < ncalls; ++c) {
        const rdf_window_range_frame& f = calls[c].frame;
        bstart[c] = bound_of(0, f.start_kind, f.start_i, f.start_f);
        bend[c] = bound_of(1, f.end_kind, f.end_i, f.end_f);
    }

    // ---- the order, then partition and peer-group structure: rdf_window's front
    RDF_TRY(window_front_device("window_range_agg", npartition, wf));
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    void* pnulls;                                               // the calls' NULL counts, then the two route words
    RDF_TRY(arena_alloc(RDF_WINDOW_MAX_CALLS * 8 + 8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, RDF_WINDOW_MAX_CALLS * 8 + 8, s));

    // ---- the sorted keys and the bounds
    if (ba.nbounds > 0) {
        void *pk, *pc, *pw, *pb;
        RDF_TRY(arena_alloc((size_t)n * 8, &pk));
        RDF_TRY(arena_alloc((size_t)n, &pc));
        RDF_TRY(arena_alloc((size_t)((n + kWRangeTile - 1) / kWRangeTile) * sizeof(uint2), &pw));
        WRangeKeyArgs ka;
        memset(&ka, 0, sizeof ka);
        ka.perm = wf.perm;
        ka.chunks = wf.d.tb.dev_at<DevChunkCol>(wf.d.o_ch) + (size_t)npartition * nch;
        ka.row_start = wf.d_row_start;
        ka.nchunks = nch;
        ka.n = n;
        ka.dtype = kdt;
        ka.desc = desc;
        ka.skey = (uint64_t*)pk;
        ka.scls = (uint8_t*)pc;
        HIP_TRY(launch_wrange_keys(ka, s));
        ba.scan = wf.scan;
        ba.pstart = wf.pstart;
        ba.gstart = wf.gstart;
        ba.skey = ka.skey;
        ba.scls = ka.scls;
        ba.n = n;
        ba.f64 = kf64;
        ba.desc = desc;
        ba.route = route;
        ba.window = (uint2*)pw;
        ba.used = (uint32_t*)((char*)pnulls + RDF_WINDOW_MAX_CALLS * 8);
        for (int b = 0; b < ba.nbounds; ++b) {
            RDF_TRY(arena_alloc((size_t)n * 4, &pb));
            ba.out[b] = (uint32_t*)pb;
        }
        HIP_TRY(launch_wrange_bounds(ba, s));
    }

    // ---- rdf_window_agg's scans, and its emit over the resolved ends
    WaggScans S(wf, vdt);
    WaggEmitArgs ea;
    memset(&ea, 0, sizeof ea);
    ea.scan = wf.scan;
    ea.pstart = wf.pstart;
    ea.gstart = wf.gstart;
    ea.perm = wf.perm;
    ea.n = n;
    ea.ncalls = ncalls;
    ea.nulls = (unsigned long long*)pnulls;
    WaggRangeBounds rb;
    memset(&rb, 0, sizeof rb);
    void* dvalid[RDF_WINDOW_MAX_CALLS] = {};
    int fns[RDF_WINDOW_MAX_CALLS] = {};
    for (int c = 0; c < ncalls; ++c) {
        const rdf_window_range_call& w = calls[c];
        WaggCallOut& o = ea.calls[c];
        fns[c] = o.fn = w.fn;
        o.f64 = w.value >= 0 && vdt[w.value] == RDF_F64;
        o.unit = RDF_FRAME_RANGE;
        o.start_kind = w.frame.start_kind;
        o.end_kind = w.frame.end_kind;
        o.w = 1;
        if (bstart[c] >= 0) rb.start[c] = ba.out[bstart[c]];
        if (bend[c] >= 0) rb.endx[c] = ba.out[bend[c]];
        RDF_TRY(window_agg_wire_call(S, w.fn, w.value, RDF_FRAME_RANGE, o.start_kind, o.end_kind, 0, 0, o));   // (MIN / MAX: one side is unbounded)
        RDF_TRY(window_agg_alloc_out(w.fn, outs[c], mem, n, o, &dvalid[c]));
    }
    HIP_TRY(launch_wagg_emit_range(ea, rb, s));
    uint32_t used[2] = {0, 0};
    RDF_TRY(window_agg_finish(wf, ea, fns, dvalid, pnulls, sizeof used, used, outs));
    std::string bounds;
    if (ba.nbounds > 0) {
        bounds = "wrange_keys_kernel + wrange_window_kernel + ";
        if (used[0]) bounds += "wrange_bounds_lds_kernel + ";
        if (used[1]) bounds += "wrange_bounds_global_kernel + ";
    }
    ctx.last_kernel = wf.sort_kernels + "win_flags_kernel + win_starts_kernel + " + bounds + std::to_string(S.scans.size()) + " x wagg_scan + wagg_emit_range_kernel";
    return RDF_OK;
}
