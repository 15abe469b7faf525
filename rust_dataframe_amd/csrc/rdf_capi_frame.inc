// rdf_capi_frame.inc — frame-level operators; textually included by rdf_capi.cpp (per-thread context, arena, pool, run_program,
// sort_core, gb_engine).
//
// The reference's DataFrame holds its RecordBatches for its lifetime (src/dataframe.rs:30-48) and every operator walks them:
// DataFrame::filter evaluates the BooleanFilter per batch and calls Column::filter per column (src/dataframe.rs:178-189),
// DataFrame::take / sort / join call Column::take per column (:216-222, :194-214, :705-711).  Over the readers' 1024-row batches
// (:352) a 1e9-row frame is a million chunks, and an entry point that takes `rdf_array[nchunks]` / `rdf_out[nchunks]` lists pays
// O(chunks) host work per call — 8 to 60 times the kernels (round-2 review).  The operators here take a pinned frame and RETURN
// a frame: descriptor tables are built by kernels, outputs live in buffers the new frame owns, and nothing per batch ever
// crosses to the host.  Batch boundaries are kept where the reference keeps them (ChunkedArray::filter, src/table.rs:97-107);
// take / sort return one batch per column (Column::take, src/table.rs:218-241, SURVEY.md B4).

namespace {

rdf_status frame_check(rdf_frame* f, const char* fn) {
    if (!f) return fail(RDF_INVALID_ARGUMENT, "%s: null frame", fn);
    RDF_TRY(ensure_ready());
    if (f->device != g_ctx.device) return fail(RDF_INVALID_ARGUMENT, "%s: the frame was pinned on device %d", fn, f->device);
    return RDF_OK;
}

// Host mirrors of a frame an operator built on the device (batch lengths, descriptors): fetched on first need, once.
rdf_status frame_host(rdf_frame& f) {
    if (f.host_valid) return RDF_OK;
    Ctx& ctx = g_ctx;
    f.clen.assign((size_t)f.nchunks, 0);
    f.dev.resize((size_t)f.ncols * (size_t)f.nchunks);
    HIP_TRY(hipMemcpyAsync(f.clen.data(), f.d_clen, sizeof(int64_t) * f.clen.size(), hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(f.dev.data(), f.d_cols, sizeof(DevChunkCol) * f.dev.size(), hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    bool any = false;
    for (int k = 0; k < f.ncols; ++k) any |= f.col_nullable[k];
    f.chunk_nullable.assign((size_t)f.nchunks, any ? 1 : 0);
    f.uniform_len = f.nchunks > 1 ? f.clen[0] : 0;
    for (int64_t c = 0; c + 1 < f.nchunks && f.uniform_len > 0; ++c) if (f.clen[(size_t)c] != f.uniform_len) f.uniform_len = 0;
    if (f.uniform_len > 0 && f.clen[(size_t)f.nchunks - 1] > f.uniform_len) f.uniform_len = 0;
    f.host_valid = true;
    return RDF_OK;
}

rdf_status frame_pool(rdf_frame& f, size_t bytes, void** out) {
    size_t got = 0;
    RDF_TRY(pool_alloc(bytes, out, &got));
    f.pooled.emplace_back(*out, got);
    return RDF_OK;
}

// The columns `cols[0..n)` of `f` as a frame of their own (n <= kMaxCols): what a fused program over a WIDE frame runs on — a
// predicate over lineitem's sixteen columns reads one or two of them.  Shares f's buffers and batch-length table.
rdf_status frame_projection(rdf_frame& f, const std::vector<int>& cols, rdf_frame** out) {
    auto it = f.projections.find(cols);
    if (it != f.projections.end()) { *out = it->second; return RDF_OK; }
    RDF_TRY(frame_host(f));
    std::unique_ptr<rdf_frame> p(new rdf_frame());
    p->device = f.device;
    p->ncols = (int)cols.size();
    p->nchunks = f.nchunks;
    p->total_rows = f.total_rows;
    p->uniform_len = f.uniform_len;
    p->clen = f.clen;
    p->chunk_nullable.assign((size_t)f.nchunks, 0);
    p->dev.resize(cols.size() * (size_t)f.nchunks);
    for (size_t k = 0; k < cols.size(); ++k) {
        const int c = cols[k];
        p->col_dtype[k] = f.col_dtype[c]; p->col_aligned16[k] = f.col_aligned16[c]; p->col_nullable[k] = f.col_nullable[c]; p->col_contig[k] = f.col_contig[c];
        memcpy(p->dev.data() + k * (size_t)f.nchunks, f.dev.data() + (size_t)c * (size_t)f.nchunks, sizeof(DevChunkCol) * (size_t)f.nchunks);
        for (int64_t i = 0; i < f.nchunks; ++i) if (p->dev[k * (size_t)f.nchunks + (size_t)i].validity) p->chunk_nullable[(size_t)i] = 1;
    }
    void* q = nullptr;
    RDF_TRY(frame_table_alloc(*p, p->dev.size() * sizeof(DevChunkCol) + 64, &q));
    p->d_cols = (DevChunkCol*)q;
    hipError_t e = hipMemcpy(q, p->dev.data(), p->dev.size() * sizeof(DevChunkCol), hipMemcpyHostToDevice);
    if (e != hipSuccess) { for (auto& pb : p->pooled) pool_release(pb.first, pb.second); p->pooled.clear(); return fail(RDF_DEVICE_ERROR, "frame projection: %s", hipGetErrorString(e)); }
    p->d_clen = f.d_clen;     // shared with the parent (not in `allocs`)
    *out = p.get();
    f.projections.emplace(cols, p.release());
    return RDF_OK;
}

// prefix of the batch lengths (row -> chunk lookups of take / sort), built on the device from d_clen
rdf_status frame_row_start(rdf_frame& f) {
    if (f.d_row_start) return RDF_OK;
    Ctx& ctx = g_ctx;
    void* p = nullptr;
    RDF_TRY(frame_pool(f, sizeof(int64_t) * ((size_t)f.nchunks + 2 + (size_t)scan_scratch_words(f.nchunks)), &p));
    HIP_TRY(launch_scan(f.d_clen, (int64_t*)p, f.nchunks, (int64_t*)p + f.nchunks + 1, ctx.stream));
    f.d_row_start = (int64_t*)p;
    return RDF_OK;
}

// A new frame whose column buffers it owns.  Tables are allocated here, filled by the caller's kernels.
struct NewFrame {
    std::unique_ptr<rdf_frame> f;
    char* values[kMaxFrameCols];
    uint8_t* validity[kMaxFrameCols];
    ~NewFrame() { if (f) (void)rdf_frame_release(f.release()); }   // an error path: the buffers go back to the pool
};
rdf_status frame_new(NewFrame& nf, int ncols, int64_t nchunks, const int* dtypes, const bool* nullable) {
    nf.f.reset(new rdf_frame());
    rdf_frame& f = *nf.f;
    f.device = g_ctx.device;
    f.ncols = ncols;
    f.nchunks = nchunks;
    f.owned = true;
    f.host_valid = false;
    for (int k = 0; k < ncols; ++k) { f.col_dtype[k] = dtypes[k]; f.col_nullable[k] = nullable[k]; f.col_contig[k] = nchunks == 1; f.col_aligned16[k] = dtypes[k] != RDF_BOOL; nf.values[k] = nullptr; nf.validity[k] = nullptr; }
    void* p = nullptr;
    RDF_TRY(frame_pool(f, sizeof(DevChunkCol) * (size_t)ncols * (size_t)nchunks + 64, &p));
    f.d_cols = (DevChunkCol*)p;
    RDF_TRY(frame_pool(f, sizeof(int64_t) * (size_t)nchunks + 64, &p));
    f.d_clen = (int64_t*)p;
    return RDF_OK;
}
// buffers of `rows` elements per column (+ bitmaps for the nullable ones, zeroed: kernels OR their words in)
rdf_status frame_new_buffers(NewFrame& nf, int64_t rows, bool zero_bitmaps) {
    rdf_frame& f = *nf.f;
    for (int k = 0; k < f.ncols; ++k) {
        void* p = nullptr;
        const size_t es = (size_t)dtype_size(f.col_dtype[k]);
        RDF_TRY(frame_pool(f, (size_t)rows * es + 256, &p));
        nf.values[k] = (char*)p;
        if (f.col_nullable[k]) {
            const size_t bb = (size_t)((rows + 63) / 64 * 8) + 64;
            RDF_TRY(frame_pool(f, bb, &p));
            nf.validity[k] = (uint8_t*)p;
            if (zero_bitmaps) HIP_TRY(hipMemsetAsync(p, 0, bb, g_ctx.stream));
        }
    }
    return RDF_OK;
}
// a one-batch frame: descriptors and length known on the host
rdf_status frame_finish_one_chunk(NewFrame& nf, int64_t rows) {
    rdf_frame& f = *nf.f;
    Ctx& ctx = g_ctx;
    f.total_rows = rows;
    f.clen.assign(1, rows);
    f.dev.resize((size_t)f.ncols);
    bool any = false;
    for (int k = 0; k < f.ncols; ++k) { f.dev[(size_t)k] = DevChunkCol{nf.values[k], nf.validity[k], 0}; any |= f.col_nullable[k]; }
    f.chunk_nullable.assign(1, any ? 1 : 0);
    f.uniform_len = 0;
    RDF_TRY(pinned_reserve(sizeof(DevChunkCol) * (size_t)f.ncols + 64));
    memcpy(ctx.pinned, f.dev.data(), sizeof(DevChunkCol) * (size_t)f.ncols);
    memcpy(ctx.pinned + sizeof(DevChunkCol) * (size_t)f.ncols, &rows, 8);
    HIP_TRY(hipMemcpyAsync(f.d_cols, ctx.pinned, sizeof(DevChunkCol) * (size_t)f.ncols, hipMemcpyHostToDevice, ctx.stream));
    HIP_TRY(hipMemcpyAsync(f.d_clen, ctx.pinned + sizeof(DevChunkCol) * (size_t)f.ncols, 8, hipMemcpyHostToDevice, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    f.host_valid = true;
    return RDF_OK;
}

// The frame's mask buffers for rdf_filter_frame (kept for the frame's lifetime: the same frame is filtered again and again).
rdf_status frame_mask_setup(rdf_frame& f) {
    if (f.mask_values) return RDF_OK;
    Ctx& ctx = g_ctx;
    RDF_TRY(frame_host(f));
    // batch c at bit pos[c] = sum of the 64-rounded lengths before it: every batch's bitmap starts on an 8-byte boundary
    std::vector<int64_t> pos((size_t)f.nchunks + 1, 0);
    for (int64_t c = 0; c < f.nchunks; ++c) pos[(size_t)c + 1] = pos[(size_t)c] + ((f.clen[(size_t)c] + 63) & ~(int64_t)63);
    const size_t bytes = (size_t)(pos[(size_t)f.nchunks] / 8) + 256;
    void *pv = nullptr, *pb = nullptr, *po = nullptr, *pc = nullptr, *pp = nullptr;
    RDF_TRY(frame_pool(f, bytes, &pv));
    RDF_TRY(frame_pool(f, bytes, &pb));
    RDF_TRY(frame_pool(f, sizeof(DevOutChunk) * (size_t)f.nchunks + 64, &po));
    RDF_TRY(frame_pool(f, sizeof(DevChunkCol) * (size_t)f.nchunks + 64, &pc));
    RDF_TRY(frame_pool(f, sizeof(int64_t) * pos.size() + 64, &pp));
    RDF_TRY(pinned_reserve(sizeof(int64_t) * pos.size() + 64));
    memcpy(ctx.pinned, pos.data(), sizeof(int64_t) * pos.size());
    HIP_TRY(hipMemcpyAsync(pp, ctx.pinned, sizeof(int64_t) * pos.size(), hipMemcpyHostToDevice, ctx.stream));
    HIP_TRY(launch_frame_mask_tables((const int64_t*)pp, f.nchunks, (uint8_t*)pv, (uint8_t*)pb, (DevOutChunk*)po, (DevChunkCol*)pc, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    f.mask_values = (uint8_t*)pv;
    f.mask_validity = (uint8_t*)pb;
    f.d_mask_outs = (DevOutChunk*)po;
    f.d_mask_cols = (DevChunkCol*)pc;
    f.d_mask_pos = (int64_t*)pp;
    f.mask_out0 = DevOutChunk{pv, (uint8_t*)pb};
    f.mask_padded_rows = pos[(size_t)f.nchunks];
    f.max_clen = 0;
    for (int64_t c = 0; c < f.nchunks; ++c) f.max_clen = std::max(f.max_clen, f.clen[(size_t)c]);
    return RDF_OK;
}

// `column CMP literal` as the one-pass filter kernel wants it (BooleanFilter::{Gt, GtEq, Eq, NotEq, Lt, LtEq} over
// BooleanInput::{Column, Scalar}, src/expression.rs:752-763; both sides compared as f64, :844-845)
bool fused_term(const rdf_expr_node* nodes, int32_t nnodes, int32_t idx, const rdf_frame& f, FusedTerm* t) {
    if (idx < 0 || idx >= nnodes) return false;
    const rdf_expr_node& n = nodes[idx];
    if (n.kind != RDF_NODE_OP || n.op < RDF_OP_GT || n.op > RDF_OP_LE) return false;
    if (n.lhs < 0 || n.lhs >= nnodes || n.rhs < 0 || n.rhs >= nnodes) return false;
    const rdf_expr_node *L = &nodes[n.lhs], *R = &nodes[n.rhs];
    int op = n.op;
    if (L->kind == RDF_NODE_SCALAR && R->kind == RDF_NODE_COLUMN) {           // c CMP x  ==  x CMP' c
        std::swap(L, R);
        op = op == RDF_OP_GT ? RDF_OP_LT : op == RDF_OP_GE ? RDF_OP_LE : op == RDF_OP_LT ? RDF_OP_GT : op == RDF_OP_LE ? RDF_OP_GE : op;
    }
    if (L->kind != RDF_NODE_COLUMN || R->kind != RDF_NODE_SCALAR) return false;
    if (L->column < 0 || L->column >= f.ncols) return false;
    const int cdt = f.col_dtype[L->column], lt = R->dtype;
    if (cdt != RDF_F64 && cdt != RDF_I64 && cdt != RDF_U64 && cdt != RDF_F32 && cdt != RDF_I32 && cdt != RDF_U32) return false;
    if (!(is_numeric(lt) || lt == RDF_BOOL)) return false;                    // (Scalar::Null compares to NULL everywhere: the general path)
    double lit;
    if (is_float(lt)) lit = lt == RDF_F32 ? (double)(float)R->f64 : R->f64;
    else {
        const uint64_t iv = lt == RDF_BOOL ? (uint64_t)(R->i64 != 0) : h_normalize_int(lt, (uint64_t)R->i64);
        lit = is_signed_int(lt) ? (double)(int64_t)iv : (double)iv;
    }
    t->col = L->column; t->op = op; t->dtype = cdt; t->pad = 0; t->lit = lit;
    return true;
}

// `column CMP literal` for the block kernel (rdf_bfilter.hip).  Float columns keep the comparison.  For an integer column the
// comparison is between (double)x and the literal (src/expression.rs:844-845) and x -> (double)x is monotone, so the rows that pass
// are those of ONE interval of x (its complement for `!=`), found here by bisection with the very conversion the reference does:
// the kernel then compares integers and never converts (bit-exact with the f64 comparison by construction, NaN literal included).
BfTerm bf_term(const FusedTerm& t) {
    BfTerm b;
    memset(&b, 0, sizeof b);
    b.col = t.col; b.op = t.op; b.lit = t.lit;
    if (t.dtype == RDF_F64 || t.dtype == RDF_F32) return b;
    b.kind = 1;
    const bool wide = t.dtype == RDF_I64 || t.dtype == RDF_U64, sgn = t.dtype == RDF_I64 || t.dtype == RDF_I32;
    const uint64_t umax = wide ? ~0ull : 0xFFFFFFFFull;
    b.bias = sgn ? (wide ? 0x8000000000000000ull : 0x80000000ull) : 0;
    auto as_double = [&](uint64_t u) -> double {          // the value whose biased bits are u
        const uint64_t x = u ^ b.bias;
        if (wide) return sgn ? (double)(int64_t)x : (double)x;
        return sgn ? (double)(int32_t)(uint32_t)x : (double)(uint32_t)x;
    };
    // the smallest u with p(u), p monotone (false ... false true ... true); umax + 1 if none: as 128-bit so that it is representable
    auto first_true = [&](auto p) -> unsigned __int128 {
        unsigned __int128 lo = 0, hi = (unsigned __int128)umax + 1;
        while (lo < hi) { const unsigned __int128 mid = lo + (hi - lo) / 2; if (p((uint64_t)mid)) hi = mid; else lo = mid + 1; }
        return lo;
    };
    const double c = t.lit;
    unsigned __int128 lo = 1, hi1 = 0;                    // the interval [lo, hi1): empty
    if (c == c) {                                         // (a NaN literal: every comparison but != is false)
        const unsigned __int128 ge = first_true([&](uint64_t u) { return as_double(u) >= c; });
        const unsigned __int128 gt = first_true([&](uint64_t u) { return as_double(u) > c; });
        const unsigned __int128 end = (unsigned __int128)umax + 1;
        switch (t.op) {
            case RDF_OP_GT: lo = gt; hi1 = end; break;
            case RDF_OP_GE: lo = ge; hi1 = end; break;
            case RDF_OP_LT: lo = 0; hi1 = ge; break;
            case RDF_OP_LE: lo = 0; hi1 = gt; break;
            default: lo = ge; hi1 = gt; break;            // == (and !=, inverted below)
        }
    }
    b.inv = t.op == RDF_OP_NE ? 1 : 0;
    if (lo < hi1) { b.lo = (uint64_t)lo; b.hi = (uint64_t)(hi1 - 1); }
    else { b.lo = 1; b.hi = 0; }
    return b;
}

// rdf_filter_frame in one pass (rdf_filter.hip: ffilter_dma_kernel).  *handled = false: the predicate or the frame is not of
// the shape the kernel takes, nothing was done.
rdf_status filter_frame_fused(rdf_frame& f, const rdf_expr_node* nodes, int32_t nnodes, int32_t root, rdf_frame** out, bool* handled) {
    *handled = false;
    Ctx& ctx = g_ctx;
    if (!ctx.opt_filter_fused || f.ncols > kMaxFilterCols || f.total_rows <= 0) return RDF_OK;
    for (int k = 0; k < f.ncols; ++k) { const int es = dtype_size(f.col_dtype[k]); if (es != 8 && es != 4) return RDF_OK; }
    if (f.total_rows < f.nchunks * (int64_t)(kWDmaTile * 3 / 4)) return RDF_OK;      // short batches: mostly partial tiles
    // A batch of up to 64 tiles finds its offsets with ONE 64-wide read of its predecessors' counts (65 536-row batches: 2.78 ms
    // per 1e9 rows against 4.6 through the mask).  Longer batches add the look-back over super-tile totals, whose words lie a
    // cache line apart: 64 more line fetches per tile, as much traffic as the tile's data — 262 144-row batches 4.0 ms (three
    // passes 4.6; four columns 9.7 against 10.7), 1 048 576-row batches 4.5 = 4.5 (10.7 against 11.6), 16 M rows 5.2 against
    // 4.5, ONE batch of 1e9 rows 4.95 against 4.1: up to 1024 tiles the one pass, beyond it the three passes
    // (rdf_set_option("filter_fused", 2) forces the one-pass kernel: tests, A/B).  Tried and measured slower: the totals packed
    // into consecutive words (6.4 ms at 262 144 rows), every tile adding its count to its super-tile's total with an atomic and
    // nobody gathering (3.9 / 6.7 ms at 262 144 / 1e9 rows), both look-backs requested together with every tile leaving the
    // offset it found (13 ms).
    if (f.max_clen == 0) { RDF_TRY(frame_host(f)); for (int64_t c = 0; c < f.nchunks; ++c) f.max_clen = std::max(f.max_clen, f.clen[(size_t)c]); }
    // Round 5: what a tile of a long batch waits for is a chain of memory round trips (its neighbours' counts -> the super-tile's
    // total -> the walk over the totals), and a wave holds one tile at a time, so every hop of that chain is time the wave moves no
    // data.  Now the walk is done once per super-tile, by its first tile, which leaves the rows in front of the super-tile in a word
    // of its own (ffilter_dma_kernel); the other 63 tiles read that word with lane 63 of the same 64-wide read that
    // brings their neighbours' counts; and the first tile adds up the nearest 8 super-tiles from their tiles' counts instead of
    // waiting for their totals.  1e9 rows, kernels, one pass against three: 262 144-row batches 3.57
    // against 4.07 ms (four columns 9.06 / 10.17), 1 048 576 rows 3.82 / 4.06 (9.30 / 10.3), 16 M rows 3.99 / 3.98 (9.64 / 10.1),
    // ONE batch of 1e9 rows 3.78 / 4.09 (9.60 / 10.2) — the one pass is taken for batches of any length.  (The two older walks, by
    // every tile and over totals only, are measured in profiles/r05_filter_frame_lookback_ab_box8.jsonl / _box9.jsonl.)
    FusedFilterArgs fa;
    memset(&fa, 0, sizeof fa);
    const rdf_expr_node& rn = nodes[root];
    if (rn.kind == RDF_NODE_OP && (rn.op == RDF_OP_AND || rn.op == RDF_OP_OR)) {
        if (!fused_term(nodes, nnodes, rn.lhs, f, &fa.term[0]) || !fused_term(nodes, nnodes, rn.rhs, f, &fa.term[1])) return RDF_OK;
        fa.nterms = 2; fa.combine = rn.op;
    } else {
        if (!fused_term(nodes, nnodes, root, f, &fa.term[0])) return RDF_OK;
        fa.nterms = 1;
    }
    RDF_TRY(frame_mask_setup(f));          // the batches' 64-row rounded positions (and, for the general path, the mask itself)
    *handled = true;
    arena_begin();
    NewFrame nf;
    RDF_TRY(frame_new(nf, f.ncols, f.nchunks, f.col_dtype, f.col_nullable));
    rdf_frame& o = *nf.f;
    // Long batches of equally wide columns: block tiles in registers, counts published ahead of their prefixes, one scanner wave
    // (rdf_bfilter.hip).  The wave-tile kernel below keeps the readers' short batches, where a batch is a tile.
    // Frames of TWO column widths (8- and 4-byte columns side by side: a lineitem-shaped frame) stay on the wave-tile kernel too.  The
    // block kernel twice — the predicate's width first, writing the kept rows into the frame's mask, then the other width by that mask —
    // was built, measured 5 - 20 % behind it and removed: profiles/r06_filter_frame_mixed_widths.jsonl.
    int es0 = dtype_size(f.col_dtype[0]);
    for (int k = 1; k < f.ncols; ++k) if (dtype_size(f.col_dtype[k]) != es0) es0 = 0;
    BFilterArgs block_args;
    memset(&block_args, 0, sizeof block_args);
    // Which form (round 6, measured by batch length: profiles/r06_filter_frame_ragged_batches.jsonl).  The block kernel's time goes with the
    // SLOTS it walks, not with the rows in them: short batches that fill their slots (>= 0.9: the readers' 1024-row batches, batches
    // of 1000 rows) take the short form; batches that average at least half a tile and fill their tiles to 0.5 (one column) / 0.65
    // (several) the long forms — 5000-row batches of one column 2.65 ms per 1e9 rows there against 3.6 on eight-wave slots and 3.4 on
    // the wave-tile kernel —; half-full slots the short form again; everything else the wave-tile kernel.
    struct Form { bool long_tiles = false; int short_shift = -1; const rdf_frame::Tiles* tiles = nullptr; int64_t tile_rows = 0; bool block() const { return long_tiles || short_shift >= 0; } };
    const int64_t mean_len = (f.total_rows + f.nchunks - 1) / f.nchunks;      // (rounded up: a frame of 8192-row batches ends in a short one)
    auto pick_form = [&](int es, int nc, Form& fm) -> rdf_status {
        fm = Form();
        if (!ctx.opt_filter_block || es == 0) return RDF_OK;
        fm.tile_rows = bfilter_tile_rows(es, nc);
        fm.long_tiles = mean_len >= (int64_t)ctx.opt_filter_block_rows;
        double short_fill = 0.0;
        if (!fm.long_tiles && ctx.opt_filter_short) {
            fm.short_shift = bfilter_short_shift(es, nc, f.max_clen);
            if (fm.short_shift >= 0) short_fill = (double)f.total_rows / ((double)f.nchunks * (double)((fm.tile_rows / 8) << fm.short_shift));
            if (short_fill < 0.5) fm.short_shift = -1;
        }
        if (!fm.long_tiles && short_fill < 0.9 && mean_len * 2 >= fm.tile_rows) {
            const rdf_frame::Tiles* lt = nullptr;
            RDF_TRY(frame_tiles(f, (int)fm.tile_rows, &lt));
            const double fill = (double)f.total_rows / ((double)lt->ntiles * (double)fm.tile_rows);
            if (fill >= (nc == 1 ? 0.5 : 0.65)) { fm.long_tiles = true; fm.short_shift = -1; }
        }
        if (fm.long_tiles) RDF_TRY(frame_tiles(f, (int)fm.tile_rows, &fm.tiles));
        return RDF_OK;
    };
    Form form;
    RDF_TRY(pick_form(es0, f.ncols, form));
    const bool block_tiles = form.long_tiles;
    const int short_shift = form.short_shift;
    const bool block_short = short_shift >= 0;
    const rdf_frame::Tiles* tiles = form.tiles;
    if (!form.block()) RDF_TRY(frame_tiles(f, kWDmaTile, &tiles));
    RDF_TRY(frame_new_buffers(nf, f.mask_padded_rows + 64, true));
    void* pouts = nullptr;
    RDF_TRY(arena_alloc(sizeof(DevOutChunk) * (size_t)f.ncols * (size_t)f.nchunks + 64, &pouts));
    void* pnc = nullptr;
    RDF_TRY(arena_alloc(sizeof(int64_t) * (size_t)f.ncols * (size_t)f.nchunks + 64, &pnc));
    HIP_TRY(hipMemsetAsync(pnc, 0, sizeof(int64_t) * (size_t)f.ncols * (size_t)f.nchunks, ctx.stream));
    HIP_TRY(hipMemsetAsync(o.d_clen, 0, sizeof(int64_t) * (size_t)f.nchunks, ctx.stream));
    KernelTimer kt;
    FrameTabArgs ta;
    memset(&ta, 0, sizeof ta);
    ta.pos = f.d_mask_pos; ta.nchunks = f.nchunks; ta.ncols = f.ncols;
    for (int k = 0; k < f.ncols; ++k) { ta.values[k] = nf.values[k]; ta.validity[k] = nf.validity[k]; ta.esize[k] = dtype_size(f.col_dtype[k]); }
    ta.outs = (DevOutChunk*)pouts;
    ta.cols = o.d_cols;
    HIP_TRY(launch_frame_tables(ta, ctx.stream));
    FilterWArgs& wa = fa.w;
    wa.t.chunk_tile_start = block_short ? nullptr : tiles->d_start;
    wa.t.chunk_len = f.d_clen;
    wa.t.nchunks = f.nchunks;
    wa.t.ntiles = block_short ? (f.nchunks + (8 >> short_shift) - 1) / (8 >> short_shift) : tiles->ntiles;
    wa.tile_inv = block_short ? 0 : tiles->tile_inv;
    wa.cols = f.d_cols;
    wa.outs = (DevOutChunk*)pouts;
    wa.out_null_counts = (int64_t*)pnc;
    wa.ncols = f.ncols;
    if (f.nchunks == 1) wa.len0 = f.clen[0];
    for (int k = 0; k < f.ncols; ++k) {
        wa.esize[k] = dtype_size(f.col_dtype[k]);
        if (f.nchunks == 1) { wa.cols0[k] = f.dev[(size_t)k]; wa.outs0[k] = DevOutChunk{nf.values[k], nf.validity[k]}; }
    }
    fa.out_len = o.d_clen;
    if (block_tiles || block_short) {
        BFilterArgs ba;
        memset(&ba, 0, sizeof ba);
        ba.w = wa;
        if (block_short) { ba.short_mode = 1; ba.short_shift = short_shift; }
        else if (bfilter_owned_ok(f.nchunks, f.max_clen, f.total_rows)) ba.short_mode = 2;
        for (int i = 0; i < fa.nterms; ++i) ba.bterm[i] = bf_term(fa.term[i]);
        ba.nterms = fa.nterms; ba.combine = fa.combine;
        ba.out_len = o.d_clen;
        RDF_TRY(bfilter_scratch(ba));
        bool nulls = false;
        for (int k = 0; k < f.ncols; ++k) nulls |= f.col_nullable[k];
        HIP_TRY(launch_bfilter(ba, es0, nulls, ctx.stream));
        block_args = ba;
    } else {
        fa.lookback = f.max_clen > kWDmaTile;
        // tiles at the end of their batch through the DMA path as well, when there is more than the odd one of them (more than 1 % of the
        // tiles' rows do not exist): 1000-row batches of an f64 + i32 frame 8.4 -> 4.3 ms per 1e9 rows; frames of full tiles keep the
        // instantiation without that code (it costs them 15 - 20 % when compiled in)
        fa.ends = ctx.opt_filter_ends && (double)f.total_rows < 0.99 * (double)tiles->ntiles * (double)kWDmaTile ? 1 : 0;
        if (fa.lookback) {
            void* ps = nullptr;
            // [ntiles] tile states, 8 spare words, [ntiles] super-tile states (at the index of a super-tile's first tile), 8 spare words,
            // [ntiles] rows in front of a super-tile (same index), then the 64 ticket counters, 128 bytes apart
            const size_t words = 3 * (size_t)tiles->ntiles + 32 + 64 * 16;
            RDF_TRY(arena_alloc(sizeof(unsigned long long) * words, &ps));
            HIP_TRY(hipMemsetAsync(ps, 0, sizeof(unsigned long long) * words, ctx.stream));
            fa.tile_state = (unsigned long long*)ps;
            fa.ticket = (unsigned int*)((unsigned long long*)ps + 3 * (size_t)tiles->ntiles + 32);
        }
        HIP_TRY(launch_ffilter(fa, ctx.stream));
    }
    // rows of the new frame: the sum of its batch lengths
    void* psum = nullptr;
    RDF_TRY(arena_alloc(sizeof(int64_t) * ((size_t)f.nchunks + 2 + (size_t)scan_scratch_words(f.nchunks)), &psum));
    HIP_TRY(launch_scan(o.d_clen, (int64_t*)psum, f.nchunks, (int64_t*)psum + f.nchunks + 1, ctx.stream));
    kt.stop();
    RDF_TRY(pinned_reserve(64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned, (int64_t*)psum + f.nchunks, 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    int64_t kept = 0;
    memcpy(&kept, ctx.pinned, 8);
    if (block_tiles) RDF_TRY(bfilter_check(block_args));
    ctx.last_kernel = block_tiles ? (block_args.short_mode == 2 ? "bfilter_kernel (a block per batch)" : "bfilter_kernel") : block_short ? "bfilter_kernel (short batches)" : "ffilter_dma_kernel";
    o.total_rows = kept;
    *out = nf.f.release();
    return RDF_OK;
}

// One gather pass over columns [g, g + m) of `src` by `indices` into one-batch outputs.
rdf_status take_cols_launch(rdf_frame& src, int g, int m, const DevChunkCol& indices, bool idx64, int64_t n, char* const* values, uint8_t* const* validity,
                            int64_t* d_nullc, uint32_t* d_flags) {
    Ctx& ctx = g_ctx;
    TakeColsArgs ta;
    memset(&ta, 0, sizeof ta);
    ta.cols_tab = src.d_cols + (size_t)g * (size_t)src.nchunks;
    ta.chunk_row_start = src.d_row_start;
    ta.nchunks = src.nchunks;
    ta.total_rows = src.total_rows;
    ta.uniform_len = src.uniform_len;
    ta.indices = indices;
    ta.n = n;
    ta.out_null_counts = d_nullc + g;
    ta.flags = d_flags;
    ta.ncols = m;
    ta.idx64 = idx64 ? 1 : 0;
    for (int k = 0; k < m; ++k) {
        ta.esize[k] = dtype_size(src.col_dtype[g + k]);
        ta.col_nullable[k] = src.col_nullable[g + k] ? 1 : 0;
        ta.contig[k] = (src.nchunks == 1 || src.col_contig[g + k]) ? 1 : 0;
        if (ta.contig[k]) ta.cols0[k] = src.dev[(size_t)((int64_t)(g + k) * src.nchunks)];
        ta.outs[k] = DevOutChunk{values[g + k], validity[g + k]};
    }
    for (int k = 0; k < m; ++k) if (!ta.contig[k]) ta.need_lookup = 1;
    HIP_TRY(launch_take_cols(ta, ctx.stream));
    return RDF_OK;
}

// indices (ONE u32 / u64 array, host or device) -> a device view
rdf_status stage_indices(const rdf_array* indices, const char* fn, InputStager& st, size_t& pin_off, DevChunkCol* view) {
    if (!indices) return fail(RDF_INVALID_ARGUMENT, "%s: null indices", fn);
    if (indices->dtype != RDF_U32 && indices->dtype != RDF_U64) return fail(RDF_INVALID_ARGUMENT, "%s: indices must be UInt32/UInt64", fn);
    if (indices->mem == RDF_MEM_DEVICE) { *view = DevChunkCol{indices->values, indices->validity, indices->offset}; return RDF_OK; }
    size_t used = 0;
    st.add(indices);
    RDF_TRY(st.finish(pin_off, &used));
    pin_off += (used + 255) & ~(size_t)255;
    *view = st.dev[0];
    return RDF_OK;
}

// Column::take over every column of the frame in one pass -> a one-batch frame of n rows.
rdf_status take_frame_core(rdf_frame& f, const DevChunkCol& idx, bool idx64, bool idx_nullable, int64_t n, rdf_frame** out) {
    Ctx& ctx = g_ctx;
    RDF_TRY(frame_host(f));
    RDF_TRY(frame_row_start(f));
    NewFrame nf;
    bool nullable[kMaxFrameCols];
    for (int k = 0; k < f.ncols; ++k) nullable[k] = f.col_nullable[k] || idx_nullable;
    RDF_TRY(frame_new(nf, f.ncols, 1, f.col_dtype, nullable));
    RDF_TRY(frame_new_buffers(nf, n, false));
    void* p = nullptr;
    RDF_TRY(arena_alloc(16 + 8 * (size_t)f.ncols, &p));
    HIP_TRY(hipMemsetAsync(p, 0, 16 + 8 * (size_t)f.ncols, ctx.stream));
    uint32_t* d_flags = (uint32_t*)p;
    int64_t* d_nullc = (int64_t*)((char*)p + 16);
    {
        // Few columns, or a short index list: gather column by column (take_cols_kernel).  Many columns taken by a list about
        // as long as the frame (sort, join): interleave the columns into row records once and gather records — one memory
        // transaction per row instead of one per row and column.  Modelled on transactions: a gathered element costs a
        // 128-byte line whatever its width.
        bool any_null = false;
        double sum_es = 0;
        for (int k = 0; k < f.ncols; ++k) { any_null |= f.col_nullable[k]; sum_es += dtype_size(f.col_dtype[k]); }
        const int per_group = any_null ? kMaxRowSlots - 1 : kMaxRowSlots;
        const int m0 = std::min(f.ncols, per_group);
        int nslot = 2;
        while (nslot < m0 + (any_null ? 1 : 0)) nslot *= 2;
        const double cost_rows = (double)f.total_rows * (sum_es + 8.0 * nslot * ((f.ncols + per_group - 1) / per_group)) + (double)n * 128.0 * ((f.ncols + per_group - 1) / per_group);
        const double cost_cols = (double)n * 128.0 * f.ncols;
        const bool fits = (double)f.total_rows * 8.0 * nslot <= 64e9;
        bool rows_path = ctx.opt_take_rows == 2 || (ctx.opt_take_rows == 1 && f.ncols >= 3 && fits && cost_rows < 0.85 * cost_cols);
        if (rows_path && ctx.opt_take_rows == 1 && n > 8192) {
            // the model prices a gathered element at a whole line: true for a random list, wrong for a sorted / sequential one,
            // which gathers at streaming speed column by column (4 columns of 2.5e8 sequential rows: 5.8 ms against 16 ms through
            // records).  4096 sampled neighbour pairs tell the two apart.
            void* pn = nullptr;
            RDF_TRY(arena_alloc(16, &pn));
            HIP_TRY(hipMemsetAsync(pn, 0, 16, ctx.stream));
            HIP_TRY(launch_idx_locality(idx, n, idx64, (unsigned int*)pn, ctx.stream));
            RDF_TRY(pinned_reserve(64));
            HIP_TRY(hipMemcpyAsync(ctx.pinned, pn, 4, hipMemcpyDeviceToHost, ctx.stream));
            HIP_TRY(hipStreamSynchronize(ctx.stream));
            unsigned int near = 0;
            memcpy(&near, ctx.pinned, 4);
            if (near > 2048) rows_path = false;
        }
        KernelTimer kt;
        if (rows_path) {
            void* precs = nullptr;
            RDF_TRY(arena_alloc((size_t)f.total_rows * 8 * (size_t)nslot + 256, &precs));
            for (int g = 0; g < f.ncols; g += per_group) {
                const int m = std::min(per_group, f.ncols - g);
                TakeRowsArgs ra;
                memset(&ra, 0, sizeof ra);
                ra.cols_tab = f.d_cols + (size_t)g * (size_t)f.nchunks;
                ra.chunk_row_start = f.d_row_start;
                ra.nchunks = f.nchunks; ra.total_rows = f.total_rows; ra.uniform_len = f.uniform_len;
                ra.indices = idx; ra.n = n;
                ra.recs = (uint64_t*)precs;
                ra.out_null_counts = d_nullc + g;
                ra.flags = d_flags;
                ra.ncols = m; ra.idx64 = idx64 ? 1 : 0; ra.nslot = nslot;
                ra.flag_slot = any_null ? m : -1;
                for (int k = 0; k < m; ++k) {
                    ra.esize[k] = dtype_size(f.col_dtype[g + k]);
                    ra.contig[k] = (f.nchunks == 1 || f.col_contig[g + k]) ? 1 : 0;
                    if (ra.contig[k]) ra.cols0[k] = f.dev[(size_t)((int64_t)(g + k) * f.nchunks)];
                    else ra.need_lookup = 1;
                    ra.outs[k] = DevOutChunk{nf.values[g + k], nf.validity[g + k]};
                }
                HIP_TRY(launch_take_rows(ra, ctx.stream));
            }
            ctx.last_kernel = "rows_pack_kernel + rows_gather_kernel";
        } else {
            for (int g = 0; g < f.ncols; g += kMaxFilterCols)
                RDF_TRY(take_cols_launch(f, g, std::min(kMaxFilterCols, f.ncols - g), idx, idx64, n, nf.values, nf.validity, d_nullc, d_flags));
            ctx.last_kernel = "take_cols_kernel";
        }
        kt.stop();
    }
    RDF_TRY(pinned_reserve(64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned, d_flags, 4, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    uint32_t flags;
    memcpy(&flags, ctx.pinned, 4);
    if (flags & 2u) { rdf_frame* dead = nf.f.release(); (void)rdf_frame_release(dead); return fail(RDF_COMPUTE_ERROR, "take index out of bounds (len %lld)", (long long)f.total_rows); }
    RDF_TRY(frame_finish_one_chunk(nf, n));
    *out = nf.f.release();
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_frame_info(rdf_frame* frame, int32_t* ncols, int64_t* nchunks, int64_t* rows) {
    if (!frame) return fail(RDF_INVALID_ARGUMENT, "frame_info: null frame");
    if (ncols) *ncols = frame->ncols;
    if (nchunks) *nchunks = frame->nchunks;
    if (rows) *rows = frame->total_rows;
    return RDF_OK;
}

rdf_status rdf_frame_column(rdf_frame* frame, int32_t col, rdf_array* chunks) {
    RDF_TRY(frame_check(frame, "frame_column"));
    if (col < 0 || col >= frame->ncols || !chunks) return fail(RDF_INVALID_ARGUMENT, "frame_column: bad column / null output");
    RDF_TRY(frame_host(*frame));
    for (int64_t c = 0; c < frame->nchunks; ++c) {
        const DevChunkCol& d = frame->dev[(size_t)((int64_t)col * frame->nchunks + c)];
        chunks[c].values = d.values; chunks[c].validity = d.validity; chunks[c].offset = d.offset;
        chunks[c].length = frame->clen[(size_t)c]; chunks[c].null_count = d.validity ? -1 : 0;
        chunks[c].dtype = frame->col_dtype[col]; chunks[c].mem = RDF_MEM_DEVICE;
    }
    return RDF_OK;
}

rdf_status rdf_filter_frame(rdf_frame* frame, const rdf_expr_node* nodes, int32_t nnodes, int32_t root, rdf_frame** out) {
    if (!out) return fail(RDF_INVALID_ARGUMENT, "filter_frame: null output pointer");
    *out = nullptr;
    RDF_TRY(frame_check(frame, "filter_frame"));
    if (!nodes || nnodes <= 0 || root < 0 || root >= nnodes) return fail(RDF_INVALID_ARGUMENT, "filter_frame: empty expression");
    rdf_frame& f = *frame;
    Ctx& ctx = g_ctx;
    for (int k = 0; k < f.ncols; ++k) if (!is_numeric(f.col_dtype[k])) return fail(RDF_INVALID_ARGUMENT, "filter: unsupported dtype %d", f.col_dtype[k]);
    {
        RDF_TRY(frame_host(f));
        bool handled = false;
        RDF_TRY(filter_frame_fused(f, nodes, nnodes, root, out, &handled));
        if (handled) return RDF_OK;
    }
    RDF_TRY(frame_mask_setup(f));
    // 1. BooleanFilter::eval_to_array over every batch, into the frame's own mask.  A frame wider than a fused program's 8
    // columns is projected onto the columns the predicate reads.
    std::vector<rdf_expr_node> remapped;
    rdf_frame* pframe = frame;
    if (f.ncols > kMaxCols) {
        std::vector<int> used;
        for (int32_t i = 0; i < nnodes; ++i)
            if (nodes[i].kind == RDF_NODE_COLUMN) {
                if (nodes[i].column < 0 || nodes[i].column >= f.ncols) return fail(RDF_COMPUTE_ERROR, "Cannot find column %d", nodes[i].column);
                if (std::find(used.begin(), used.end(), nodes[i].column) == used.end()) used.push_back(nodes[i].column);
            }
        std::sort(used.begin(), used.end());
        if (used.empty()) used.push_back(0);
        if ((int)used.size() > kMaxCols) return fail(RDF_INVALID_ARGUMENT, "a predicate reads at most %d columns", kMaxCols);
        RDF_TRY(frame_projection(f, used, &pframe));
        remapped.assign(nodes, nodes + nnodes);
        for (auto& nd : remapped) if (nd.kind == RDF_NODE_COLUMN) nd.column = (int32_t)(std::find(used.begin(), used.end(), nd.column) - used.begin());
        nodes = remapped.data();
    }
    if (f.total_rows > 0) {
        ProgramSpec ps;
        ps.nodes = nodes; ps.nnodes = nnodes; ps.filter_root = -1; ps.nvalues = 1; ps.sink = RDF_SINK_STORE;
        for (int v = 0; v < kMaxGroupValues; ++v) ps.value_roots[v] = 0;
        ps.value_roots[0] = root;
        ps.frame_outs = f.d_mask_outs;
        ps.frame_out0[0] = f.mask_out0;
        ps.frame_out_dtype[0] = RDF_BOOL;
        const rdf_status st = run_program(ps, nullptr, pframe->ncols, f.nchunks, nullptr, nullptr, "columns of a batch differ in length", pframe);
        if (st == RDF_INVALID_ARGUMENT && g_ctx.err.find("output dtype") != std::string::npos) return fail(RDF_INVALID_ARGUMENT, "predicate root must be boolean");
        RDF_TRY(st);
    }
    const std::string pred_kernel = ctx.last_kernel;
    arena_begin();
    NewFrame nf;
    RDF_TRY(frame_new(nf, f.ncols, f.nchunks, f.col_dtype, f.col_nullable));
    rdf_frame& o = *nf.f;
    if (f.total_rows == 0) {
        HIP_TRY(hipMemsetAsync(o.d_clen, 0, sizeof(int64_t) * (size_t)f.nchunks, ctx.stream));
        RDF_TRY(frame_new_buffers(nf, 64, true));
        FrameTabArgs fa;
        memset(&fa, 0, sizeof fa);
        fa.pos = o.d_clen; fa.nchunks = f.nchunks;
        for (int g = 0; g < f.ncols; g += kMaxFilterCols) {
            fa.ncols = std::min(kMaxFilterCols, f.ncols - g);
            for (int k = 0; k < fa.ncols; ++k) { fa.values[k] = nf.values[g + k]; fa.validity[k] = nf.validity[g + k]; fa.esize[k] = dtype_size(f.col_dtype[g + k]); }
            fa.cols = o.d_cols + (size_t)g * (size_t)f.nchunks;
            HIP_TRY(launch_frame_tables(fa, ctx.stream));
        }
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        o.total_rows = 0;
        *out = nf.f.release();
        return RDF_OK;
    }
    // 2. keep counts per tile (one wave's rows), their scan
    bool all_wide = true;
    for (int k = 0; k < f.ncols; ++k) { const int es = dtype_size(f.col_dtype[k]); all_wide &= es == 8 || es == 4; }
    const int64_t mean_len = f.total_rows / f.nchunks;
    const bool dma_ok = all_wide && f.total_rows >= f.nchunks * (int64_t)(kWDmaTile * 3 / 4);
    int tile_rows = dma_ok ? kWDmaTile : mean_len <= 256 ? kWTileSmall : kWTile;
    FilterWArgs wa;
    int64_t* d_scan = nullptr;
    const rdf_frame::Tiles* tiles = nullptr;
    auto count_and_scan = [&]() -> rdf_status {
        RDF_TRY(frame_tiles(f, tile_rows, &tiles));
        memset(&wa, 0, sizeof wa);
        wa.t.mask = f.d_mask_cols;
        wa.t.chunk_tile_start = tiles->d_start;
        wa.t.chunk_len = f.d_clen;
        wa.t.nchunks = f.nchunks;
        wa.t.ntiles = tiles->ntiles;
        wa.tile_inv = tiles->tile_inv;
        if (f.nchunks == 1) { wa.mask0 = DevChunkCol{f.mask_values, nullptr, 0}; wa.len0 = f.clen[0]; }
        void* p = nullptr;
        RDF_TRY(arena_alloc(sizeof(int64_t) * (2 * (size_t)tiles->ntiles + 2 + (size_t)scan_scratch_words(tiles->ntiles)), &p));
        int64_t* d_counts = (int64_t*)p;
        d_scan = d_counts + tiles->ntiles;
        // the frame's own mask: one thread per tile reads the tile's words (launch_fcount is the general, descriptor-driven form)
        HIP_TRY(launch_frame_mask_count((const uint64_t*)f.mask_values, f.d_mask_pos, tiles->d_start, f.d_clen, f.nchunks, tiles->ntiles, tile_rows, tiles->tile_inv,
                                        d_counts, ctx.stream));
        HIP_TRY(launch_scan(d_counts, d_scan, tiles->ntiles, d_scan + tiles->ntiles + 1, ctx.stream));
        return RDF_OK;
    };
    KernelTimer kt;
    RDF_TRY(count_and_scan());
    // 3. kept rows per batch -> the new frame's batch lengths; batches start on 64-row boundaries of the column buffers
    void* p = nullptr;
    RDF_TRY(arena_alloc(sizeof(int64_t) * (2 * (size_t)f.nchunks + 2 + (size_t)scan_scratch_words(f.nchunks)), &p));
    int64_t* d_padded = (int64_t*)p;
    int64_t* d_pos = d_padded + f.nchunks;
    HIP_TRY(launch_frame_totals(d_scan, tiles->d_start, f.nchunks, o.d_clen, d_padded, ctx.stream));
    HIP_TRY(launch_scan(d_padded, d_pos, f.nchunks, d_pos + f.nchunks + 1, ctx.stream));
    RDF_TRY(pinned_reserve(64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned, d_scan + tiles->ntiles, 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + 8, d_pos + f.nchunks, 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    int64_t kept = 0, padded_rows = 0;
    memcpy(&kept, ctx.pinned, 8);
    memcpy(&padded_rows, ctx.pinned + 8, 8);
    // the LDS-DMA kernel fetches every sector of a tile: a selective filter (< 1/8 kept) goes to the register-staged wave tiles
    if (tile_rows == kWDmaTile && kept * 8 < f.total_rows) { tile_rows = kWTile; RDF_TRY(count_and_scan()); }
    // 4. the new frame's buffers and descriptor tables (device-built)
    RDF_TRY(frame_new_buffers(nf, padded_rows + 64, true));
    void* pouts = nullptr;
    RDF_TRY(arena_alloc(sizeof(DevOutChunk) * (size_t)f.ncols * (size_t)f.nchunks + 64, &pouts));
    void* pnc = nullptr;
    RDF_TRY(arena_alloc(sizeof(int64_t) * (size_t)f.ncols * (size_t)f.nchunks + 64, &pnc));
    HIP_TRY(hipMemsetAsync(pnc, 0, sizeof(int64_t) * (size_t)f.ncols * (size_t)f.nchunks, ctx.stream));
    FrameTabArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.pos = d_pos; fa.nchunks = f.nchunks;
    for (int g = 0; g < f.ncols; g += kMaxFilterCols) {
        fa.ncols = std::min(kMaxFilterCols, f.ncols - g);
        for (int k = 0; k < fa.ncols; ++k) { fa.values[k] = nf.values[g + k]; fa.validity[k] = nf.validity[g + k]; fa.esize[k] = dtype_size(f.col_dtype[g + k]); }
        fa.outs = (DevOutChunk*)pouts + (size_t)g * (size_t)f.nchunks;
        fa.cols = o.d_cols + (size_t)g * (size_t)f.nchunks;
        HIP_TRY(launch_frame_tables(fa, ctx.stream));
    }
    // 5. one compaction pass per group of columns, ranks shared
    for (int g = 0; g < f.ncols; g += kMaxFilterCols) {
        wa.cols = f.d_cols + (size_t)g * (size_t)f.nchunks;
        wa.outs = (DevOutChunk*)pouts + (size_t)g * (size_t)f.nchunks;
        wa.out_null_counts = (int64_t*)pnc + (size_t)g * (size_t)f.nchunks;
        wa.tile_scan = d_scan;
        wa.ncols = std::min(kMaxFilterCols, f.ncols - g);
        for (int k = 0; k < wa.ncols; ++k) {
            wa.esize[k] = dtype_size(f.col_dtype[g + k]);
            if (f.nchunks == 1) { wa.cols0[k] = f.dev[(size_t)(g + k)]; wa.outs0[k] = DevOutChunk{nf.values[g + k], nf.validity[g + k]}; }
        }
        wa.ends = ctx.opt_filter_ends && tile_rows == kWDmaTile && (double)f.total_rows < 0.99 * (double)tiles->ntiles * (double)kWDmaTile ? 1 : 0;
        HIP_TRY(launch_fcompact(wa, tile_rows, ctx.stream));
    }
    kt.stop();
    ctx.last_kernel = pred_kernel + " + fcount/fcompact";
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    o.total_rows = kept;
    *out = nf.f.release();
    return RDF_OK;
}

rdf_status rdf_take_columns(const rdf_array* cols, int32_t ncols, int64_t nchunks, const rdf_array* indices, rdf_out* outs) {
    if (!cols || !outs || ncols < 1 || ncols > kMaxFrameCols || nchunks < 1) return fail(RDF_INVALID_ARGUMENT, "take_columns: 1..%d columns of at least one chunk", kMaxFrameCols);
    if (!indices) return fail(RDF_INVALID_ARGUMENT, "take: null argument");
    if (indices->dtype != RDF_U32 && indices->dtype != RDF_U64) return fail(RDF_INVALID_ARGUMENT, "take: indices must be UInt32/UInt64");
    int32_t mem = -1;
    RDF_TRY(check_mem(cols, (int64_t)ncols * nchunks, &mem));
    RDF_TRY(check_mem(indices, 1, &mem));
    RDF_TRY(check_out_mem(outs, ncols, mem));
    const int64_t n = indices->length;
    std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) row_start[(size_t)c + 1] = row_start[(size_t)c] + cols[c].length;
    bool nullable[kMaxFrameCols];
    for (int k = 0; k < ncols; ++k) {
        const int dt = cols[(int64_t)k * nchunks].dtype;
        if (!is_numeric(dt) || outs[k].dtype != dt) return fail(RDF_INVALID_ARGUMENT, "take: unsupported or mismatched dtype");
        nullable[k] = false;
        for (int64_t c = 0; c < nchunks; ++c) {
            const rdf_array& a = cols[(int64_t)k * nchunks + c];
            if (a.dtype != dt) return fail(RDF_INVALID_ARGUMENT, "take: chunks differ in dtype");
            if (a.length != cols[c].length) return fail(RDF_COMPUTE_ERROR, "take: columns of a batch differ in length");
            nullable[k] |= a.validity != nullptr;
        }
        if (outs[k].capacity < n) return fail(RDF_MEMORY_ERROR, "output capacity too small");
        if ((nullable[k] || indices->validity) && !outs[k].validity) return fail(RDF_INVALID_ARGUMENT, "output validity buffer required");
    }
    if (n == 0) { for (int k = 0; k < ncols; ++k) { outs[k].length = 0; outs[k].null_count = 0; } return RDF_OK; }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();
    size_t pin_off = 0, used = 0;
    InputStager in;
    in.add(indices);
    for (int64_t i = 0; i < (int64_t)ncols * nchunks; ++i) in.add(&cols[i]);
    RDF_TRY(in.finish(pin_off, &used));
    pin_off += (used + 255) & ~(size_t)255;
    TableBuilder tb;
    const size_t o_ch = tb.reserve(sizeof(DevChunkCol) * (size_t)ncols * (size_t)nchunks);
    const size_t o_rs = tb.reserve(sizeof(int64_t) * row_start.size());
    RDF_TRY(tb.bind(pin_off));
    memcpy(tb.at<char>(o_ch), in.dev.data() + 1, sizeof(DevChunkCol) * (size_t)ncols * (size_t)nchunks);
    memcpy(tb.at<char>(o_rs), row_start.data(), sizeof(int64_t) * row_start.size());
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(pin_off));
    pin_off += (tb.size + 255) & ~(size_t)255;
    // outputs
    Region outr;
    std::vector<int> vi((size_t)ncols, -1), bi((size_t)ncols, -1);
    std::vector<DevOutChunk> docs((size_t)ncols);
    if (mem == RDF_MEM_HOST) {
        for (int k = 0; k < ncols; ++k) {
            vi[(size_t)k] = outr.add(outs[k].values, (size_t)n * (size_t)dtype_size(outs[k].dtype));
            if (outs[k].validity) bi[(size_t)k] = outr.add(outs[k].validity, (size_t)((n + 7) / 8));
        }
        RDF_TRY(outr.layout());
        for (int k = 0; k < ncols; ++k) docs[(size_t)k] = DevOutChunk{outr.ptr(vi[(size_t)k]), bi[(size_t)k] >= 0 ? (uint8_t*)outr.ptr(bi[(size_t)k]) : nullptr};
    } else for (int k = 0; k < ncols; ++k) docs[(size_t)k] = DevOutChunk{outs[k].values, outs[k].validity};
    void* p = nullptr;
    RDF_TRY(arena_alloc(16 + 8 * (size_t)ncols, &p));
    HIP_TRY(hipMemsetAsync(p, 0, 16 + 8 * (size_t)ncols, ctx.stream));
    int64_t uniform = nchunks > 1 ? cols[0].length : 0;
    for (int64_t c = 0; c + 1 < nchunks && uniform > 0; ++c) if (cols[c].length != uniform) uniform = 0;
    if (uniform > 0 && cols[nchunks - 1].length > uniform) uniform = 0;
    {
        KernelTimer kt;
        for (int g = 0; g < ncols; g += kMaxFilterCols) {
            TakeColsArgs ta;
            memset(&ta, 0, sizeof ta);
            ta.cols_tab = tb.dev_at<DevChunkCol>(o_ch) + (size_t)g * (size_t)nchunks;
            ta.chunk_row_start = tb.dev_at<int64_t>(o_rs);
            ta.nchunks = nchunks;
            ta.total_rows = row_start[(size_t)nchunks];
            ta.uniform_len = uniform;
            ta.indices = in.dev[0];
            ta.n = n;
            ta.out_null_counts = (int64_t*)((char*)p + 16) + g;
            ta.flags = (uint32_t*)p;
            ta.ncols = std::min(kMaxFilterCols, ncols - g);
            ta.idx64 = indices->dtype == RDF_U64;
            for (int k = 0; k < ta.ncols; ++k) {
                ta.esize[k] = dtype_size(outs[g + k].dtype);
                ta.col_nullable[k] = nullable[g + k] ? 1 : 0;
                ta.contig[k] = nchunks == 1 ? 1 : 0;
                if (nchunks == 1) ta.cols0[k] = in.dev[(size_t)(1 + g + k)];
                ta.outs[k] = docs[(size_t)(g + k)];
            }
            ta.need_lookup = nchunks > 1 ? 1 : 0;
            HIP_TRY(launch_take_cols(ta, ctx.stream));
        }
        kt.stop();
        ctx.last_kernel = "take_cols_kernel";
    }
    RDF_TRY(pinned_reserve(pin_off + 256 + 8 * (size_t)ncols + outr.small_bytes + 256));
    char* pin = ctx.pinned + pin_off;
    HIP_TRY(hipMemcpyAsync(pin, p, 16 + 8 * (size_t)ncols, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    uint32_t flags;
    memcpy(&flags, pin, 4);
    if (flags & 2u) return fail(RDF_COMPUTE_ERROR, "take index out of bounds (len %lld)", (long long)row_start[(size_t)nchunks]);
    if (mem == RDF_MEM_HOST) RDF_TRY(outr.download(pin_off + ((16 + 8 * (size_t)ncols + 255) & ~(size_t)255)));
    for (int k = 0; k < ncols; ++k) {
        outs[k].length = n;
        memcpy(&outs[k].null_count, pin + 16 + 8 * (size_t)k, 8);
        if (!outs[k].validity) outs[k].null_count = 0;
    }
    return RDF_OK;
}

rdf_status rdf_take_frame(rdf_frame* frame, const rdf_array* indices, rdf_frame** out) {
    if (!out) return fail(RDF_INVALID_ARGUMENT, "take_frame: null output pointer");
    *out = nullptr;
    RDF_TRY(frame_check(frame, "take_frame"));
    for (int k = 0; k < frame->ncols; ++k) if (!is_numeric(frame->col_dtype[k])) return fail(RDF_INVALID_ARGUMENT, "take: unsupported dtype %d", frame->col_dtype[k]);
    arena_begin();
    size_t pin_off = 0;
    InputStager st;
    DevChunkCol idx;
    RDF_TRY(stage_indices(indices, "take_frame", st, pin_off, &idx));
    return take_frame_core(*frame, idx, indices->dtype == RDF_U64, indices->validity != nullptr, indices->length, out);
}

rdf_status rdf_sort_frame(rdf_frame* frame, const int32_t* sort_cols, int32_t nsort, const rdf_sort_options* opts, rdf_out* out_indices, rdf_frame** out) {
    if (out) *out = nullptr;
    RDF_TRY(frame_check(frame, "sort_frame"));
    if (nsort < 1 || !sort_cols) return fail(RDF_COMPUTE_ERROR, "Sort criteria cannot be empty");   // src/dataframe.rs:195-199
    if (nsort > kMaxFrameCols) return fail(RDF_INVALID_ARGUMENT, "sort: at most %d sort columns", kMaxFrameCols);
    if (!out && !out_indices) return fail(RDF_INVALID_ARGUMENT, "sort_frame: nothing to return");
    rdf_frame& f = *frame;
    Ctx& ctx = g_ctx;
    const int64_t n = f.total_rows;
    int dts[kMaxFrameCols];
    bool nullable[kMaxFrameCols];
    std::vector<int> key;
    for (int k = 0; k < nsort; ++k) {
        if (sort_cols[k] < 0 || sort_cols[k] >= f.ncols) return fail(RDF_INVALID_ARGUMENT, "sort_frame: sort column %d out of range", sort_cols[k]);
        dts[k] = f.col_dtype[sort_cols[k]];
        if (!is_numeric(dts[k])) return fail(RDF_INVALID_ARGUMENT, "sort: numeric columns of one dtype per column");
        nullable[k] = f.col_nullable[sort_cols[k]];
        key.push_back(sort_cols[k]);
    }
    if (n >= (int64_t)1 << 32) return fail(RDF_INVALID_ARGUMENT, "sort: UInt32 indices cap a column at 2^32-1 rows (src/table.rs:218)");
    if (out_indices) {
        if (out_indices->dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "sort: indices are UInt32");
        if (out_indices->mem != RDF_MEM_DEVICE) return fail(RDF_INVALID_ARGUMENT, "sort_frame: device-resident outputs only");
        if (out_indices->capacity < n) return fail(RDF_MEMORY_ERROR, "output capacity too small");
    }
    RDF_TRY(frame_host(f));
    RDF_TRY(frame_row_start(f));
    for (int k = 0; k < f.ncols && out; ++k) if (!is_numeric(f.col_dtype[k])) return fail(RDF_INVALID_ARGUMENT, "take: unsupported dtype %d", f.col_dtype[k]);
    if (n == 0) {
        if (out_indices) { out_indices->length = 0; out_indices->null_count = 0; }
        if (out) {
            NewFrame nf;
            RDF_TRY(frame_new(nf, f.ncols, 1, f.col_dtype, f.col_nullable));
            RDF_TRY(frame_new_buffers(nf, 64, true));
            RDF_TRY(frame_finish_one_chunk(nf, 0));
            *out = nf.f.release();
        }
        return RDF_OK;
    }
    arena_begin();
    // the sort columns' descriptor table in criteria order (cached in the frame like a program's column order)
    DevChunkCol* tab = nullptr;
    const int64_t* rs = f.d_row_start;
    int64_t sort_chunks = f.nchunks;
    size_t pin_off = 0;
    bool all_contig = f.nchunks > 1;
    for (int k = 0; k < nsort; ++k) all_contig &= f.col_contig[sort_cols[k]];
    if (all_contig) {   // batches that are consecutive slices of one buffer: the key extraction reads each sort column as ONE chunk
        void* p = nullptr;
        const size_t tb = sizeof(DevChunkCol) * (size_t)nsort;
        RDF_TRY(arena_alloc(tb + 16, &p));
        RDF_TRY(pinned_reserve(tb + 16 + 256));
        for (int k = 0; k < nsort; ++k) memcpy(ctx.pinned + sizeof(DevChunkCol) * (size_t)k, &f.dev[(size_t)((int64_t)sort_cols[k] * f.nchunks)], sizeof(DevChunkCol));
        const int64_t two[2] = {0, n};
        memcpy(ctx.pinned + tb, two, 16);
        HIP_TRY(hipMemcpyAsync(p, ctx.pinned, tb + 16, hipMemcpyHostToDevice, ctx.stream));
        tab = (DevChunkCol*)p;
        rs = (const int64_t*)((char*)p + tb);
        sort_chunks = 1;
        pin_off = (tb + 16 + 255) & ~(size_t)255;
    } else RDF_TRY(frame_col_tab(f, key.data(), nsort, &tab));
    const uint32_t* idx = nullptr;
    RDF_TRY(sort_core(tab, rs, sort_chunks, n, nsort, dts, nullable, opts, pin_off, &idx));
    if (out_indices) {
        HIP_TRY(hipMemcpyAsync(out_indices->values, idx, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx.stream));
        if (out_indices->validity) HIP_TRY(hipMemsetAsync(out_indices->validity, 0xFF, (size_t)((n + 7) / 8), ctx.stream));
        out_indices->length = n;
        out_indices->null_count = 0;
    }
    if (!out) { HIP_TRY(hipStreamSynchronize(ctx.stream)); return RDF_OK; }
    // DataFrame::sort's take of every column by the sorted order (src/dataframe.rs:216-222), one gather pass
    return take_frame_core(f, DevChunkCol{idx, nullptr, 0}, false, false, n, out);
}

rdf_status rdf_groupby_agg_frame(rdf_frame* frame, const int32_t* key_cols, int32_t nkeys, int32_t value_col, int32_t agg, int64_t max_groups,
                                 rdf_frame** out) {
    if (!out) return fail(RDF_INVALID_ARGUMENT, "groupby_agg_frame: null output pointer");
    *out = nullptr;
    RDF_TRY(frame_check(frame, "groupby_agg_frame"));
    if (!key_cols || nkeys < 1 || nkeys > kMaxKeyCols) return fail(RDF_INVALID_ARGUMENT, "groupby: 1..%d grouping columns", kMaxKeyCols);
    if (agg < RDF_AGG_SUM || agg > RDF_AGG_COUNT) return fail(RDF_INVALID_ARGUMENT, "groupby: unknown aggregate %d", agg);
    if (max_groups < 1) return fail(RDF_INVALID_ARGUMENT, "groupby: max_groups must be positive");
    rdf_frame& f = *frame;
    Ctx& ctx = g_ctx;
    if (agg == RDF_AGG_COUNT) value_col = -1;
    else if (value_col < 0 || value_col >= f.ncols) return fail(RDF_INVALID_ARGUMENT, "groupby: %s needs a value column", agg == RDF_AGG_SUM ? "sum" : "min / max");
    int kdt[kMaxKeyCols];
    for (int k = 0; k < nkeys; ++k) {
        if (key_cols[k] < 0 || key_cols[k] >= f.ncols) return fail(RDF_INVALID_ARGUMENT, "groupby: grouping column %d out of range", key_cols[k]);
        kdt[k] = f.col_dtype[key_cols[k]];
        if (!(kdt[k] >= RDF_I8 && kdt[k] <= RDF_U64)) return fail(RDF_INVALID_ARGUMENT, "groupby: grouping columns must be integer-typed (dtype %d)", kdt[k]);
    }
    const int vdt = value_col >= 0 ? f.col_dtype[value_col] : -1;
    if (value_col >= 0 && !is_numeric(vdt)) return fail(RDF_INVALID_ARGUMENT, "groupby: value column must be numeric");
    const int op = agg == RDF_AGG_MIN ? AGG_MIN : agg == RDF_AGG_MAX ? AGG_MAX : AGG_SUM;
    const int odt = gb_acc_dtype(op, vdt);
    RDF_TRY(frame_host(f));
    const int64_t nrows = f.total_rows;
    const int64_t cap = std::min<int64_t>(max_groups, std::max<int64_t>(nrows, 0)) + 2;
    int odts[kMaxKeyCols + 2];
    bool onull[kMaxKeyCols + 2];
    for (int k = 0; k < nkeys; ++k) { odts[k] = kdt[k]; onull[k] = f.col_nullable[key_cols[k]]; }
    odts[nkeys] = odt; onull[nkeys] = op != AGG_SUM && value_col >= 0 && f.col_nullable[value_col];
    odts[nkeys + 1] = RDF_I64; onull[nkeys + 1] = false;
    NewFrame nf;
    RDF_TRY(frame_new(nf, nkeys + 2, 1, odts, onull));
    RDF_TRY(frame_new_buffers(nf, cap + 64, true));

    if (nkeys > 1 || nrows == 0) {
        // several grouping columns: the tuple packing of rdf_groupby_agg walks the batch list (one-time host descriptors)
        std::vector<rdf_array> keys((size_t)nkeys * (size_t)f.nchunks), vals;
        for (int k = 0; k < nkeys; ++k) RDF_TRY(rdf_frame_column(frame, key_cols[k], keys.data() + (size_t)k * (size_t)f.nchunks));
        if (value_col >= 0) { vals.resize((size_t)f.nchunks); RDF_TRY(rdf_frame_column(frame, value_col, vals.data())); }
        rdf_out ok[kMaxKeyCols], ov, oc;
        for (int k = 0; k < nkeys; ++k) ok[k] = rdf_out{nf.values[k], nf.validity[k], cap, 0, 0, kdt[k], RDF_MEM_DEVICE};
        ov = rdf_out{nf.values[nkeys], nf.validity[nkeys], cap, 0, 0, odt, RDF_MEM_DEVICE};
        oc = rdf_out{nf.values[nkeys + 1], nullptr, cap, 0, 0, RDF_I64, RDF_MEM_DEVICE};
        RDF_TRY(rdf_groupby_agg(keys.data(), nkeys, value_col >= 0 ? vals.data() : nullptr, f.nchunks, agg, max_groups, ok, &ov, &oc));
        RDF_TRY(frame_finish_one_chunk(nf, ok[0].length));
        *out = nf.f.release();
        return RDF_OK;
    }

    // one grouping column: the engine runs on the frame's own tables
    const rdf_frame::Tiles* tiles = nullptr;
    RDF_TRY(frame_tiles(f, kEvalTile, &tiles));
    int kmap[2] = {key_cols[0], value_col};
    DevChunkCol* tab = nullptr;
    RDF_TRY(frame_col_tab(f, kmap, value_col >= 0 ? 2 : 1, &tab));
    for (int attempt = 0; attempt < 2; ++attempt) {
        arena_begin();
        size_t pin_off = 0;
        GbInput in;
        in.kdt = kdt[0]; in.vdt = vdt;
        in.keys.assign(1, f.dev[(size_t)((int64_t)key_cols[0] * f.nchunks)]);
        if (value_col >= 0) in.values.assign(1, f.dev[(size_t)((int64_t)value_col * f.nchunks)]);
        if (f.nchunks > 1 && f.col_contig[key_cols[0]] && (value_col < 0 || f.col_contig[value_col])) {
            // batches that are consecutive slices of one buffer (DataFrame::from_csv's): the engine reads the columns as ONE
            // chunk — no tile -> batch lookup (2.75 against 5.2 ms per 1e9 rows at 1000 groups)
            in.clen.assign(1, nrows);
        } else {
            in.d_keys = tab;
            in.d_values = value_col >= 0 ? tab + f.nchunks : tab;
            in.d_tile_start = tiles->d_start;
            in.d_len = f.d_clen;
            in.f_nchunks = f.nchunks; in.f_ntiles = tiles->ntiles; in.f_nrows = nrows;
            in.f_fast = !f.col_nullable[key_cols[0]] && f.col_aligned16[key_cols[0]] && (value_col < 0 || (!f.col_nullable[value_col] && f.col_aligned16[value_col]));
            in.clen.assign(1, f.clen[0]);
        }
        GbScratch sc;
        GbDense d;
        bool skewed = false, lds_full = false;
        int force = ctx.opt_gb_partition == 0 ? 0 : -1;
        if (ctx.opt_gb_partition == 4) force = 1;
        if (attempt == 1) force = 0;     // the partition path gave up (skewed keys, or too many groups in one partition): one table in HBM
        RDF_TRY(gb_engine(in, op, max_groups, force, sc, d, pin_off, &skewed, &lds_full));
        if (skewed) continue;
        const int64_t ng = d.ng;
        if (ng > cap) return fail(RDF_MEMORY_ERROR, "groupby: more than max_groups (%lld) distinct keys", (long long)max_groups);
        HIP_TRY(hipMemcpyAsync(nf.values[0], d.keys, (size_t)ng * (size_t)dtype_size(kdt[0]), hipMemcpyDeviceToDevice, ctx.stream));
        if (nf.validity[0]) HIP_TRY(hipMemcpyAsync(nf.validity[0], d.kvalid, (size_t)((ng + 7) / 8), hipMemcpyDeviceToDevice, ctx.stream));
        HIP_TRY(hipMemcpyAsync(nf.values[1], d.acc, (size_t)ng * 8, hipMemcpyDeviceToDevice, ctx.stream));
        if (nf.validity[1]) HIP_TRY(hipMemcpyAsync(nf.validity[1], d.vvalid, (size_t)((ng + 7) / 8), hipMemcpyDeviceToDevice, ctx.stream));
        HIP_TRY(hipMemcpyAsync(nf.values[2], d.counts, (size_t)ng * 8, hipMemcpyDeviceToDevice, ctx.stream));
        RDF_TRY(frame_finish_one_chunk(nf, ng));
        *out = nf.f.release();
        return RDF_OK;
    }
    return fail(RDF_COMPUTE_ERROR, "groupby: no path completed");
}

}  // extern "C"
