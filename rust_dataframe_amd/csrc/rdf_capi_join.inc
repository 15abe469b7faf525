// rdf_capi_join.inc — the equi-join's host side (calc_equijoin_indices, src/functions/join.rs:19-137; kernels: rdf_join.hip);
// textually included by rdf_capi.cpp behind the sort (it uses that file's per-thread context, arena, staging helpers, table builder
// and the sort's key and radix passes).  The build side is sorted, every probe row finds the range of its partners among the sorted
// rows, and the pairs are written at offsets from a scan of the per-row counts.
//
//   rdf_equijoin_indices_multi    join_check, then join_run once — or twice: a table whose placement overflowed hands the call
//                                 to the bucket index, which sorts the build side by key and so starts over
//   join_run                      the driver over the steps below, one JoinState on the caller's stack:
//     join_stage                    inputs and chunk tables in HBM, sort buffers, counters
//     join_side_keys                key bits of one side (2..4 columns: the tuple's hash, and every column's bits for the verify)
//     join_sort_build               build side: key bits, NULL count, radix sort (NULL keys last)
//     join_probe_keys               probe side: key bits; the wait that tells how many build keys are not NULL
//     join_build_table / _buckets   the lookup: the table of distinct keys (one key column, < 2^31 - 1 build rows) or the bucket index
//     join_count                    count -> scan -> (FULL) append count; the wait that tells the output's length
//     join_write / join_deliver     the pairs, then the caller's buffers and null counts
//
// How large the table and the bucket index are made is rdf_join_place.h (join_table_plan, join_bucket_plan), with a CPU test.

namespace {
// Radix-sort (key bits, row) pairs already produced by sort_keys_kernel: `width` key bytes, then the nulls-last pass.
struct SortBuffers { uint64_t* keys[2]; uint32_t* idx[2]; void* nullflags; };
rdf_status sort_buffers_alloc(int64_t n, SortBuffers& b) {
    void* p;
    for (int i = 0; i < 2; ++i) { RDF_TRY(arena_alloc((size_t)n * 8 + 8, &p)); b.keys[i] = (uint64_t*)p; }
    for (int i = 0; i < 2; ++i) { RDF_TRY(arena_alloc((size_t)n * 4 + 8, &p)); b.idx[i] = (uint32_t*)p; }
    RDF_TRY(arena_alloc((size_t)n + 8, &b.nullflags));
    return RDF_OK;
}
// keys[0] holds the unsorted key bits (identity order).  On return keys[*kcur] / idx[*icur] are sorted.
rdf_status radix_sort_rows(const SortBuffers& b, int64_t n, int width, bool has_nulls, int* kcur_out, int* icur_out, const uint64_t* d_stats, size_t pin_off,
                           uint64_t* kmin_out, uint64_t* kmax_out) {
    int kcur = 0, icur = 1;
    const uint32_t* idx_cur = nullptr;
    uint64_t bias = 0;
    int need = 0;
    uint64_t kmax = 0;
    RDF_TRY(sort_key_range(d_stats, pin_off, &bias, &need, &kmax));
    if (kmax_out) *kmax_out = kmax;
    *kmin_out = bias;
    if (need == 0 && !has_nulls) need = 1;   // all keys equal: one pass still writes the identity order
    OsScratch os;
    RDF_TRY(os_scratch_alloc(n, os));
    RDF_TRY(os_column_passes(os, b.keys, b.idx, (const uint8_t*)b.nullflags, n, bias, std::min(need, width), has_nulls, kcur, icur, idx_cur, kmax >= bias ? kmax - bias : ~0ull));
    *kcur_out = kcur;
    *icur_out = icur;
    return RDF_OK;
}

// How a probe row finds its partners.  Table: one key column -> the build side is sorted by key * golden ratio and the table of its
// distinct keys is laid out by a scan (JoinPlaceArgs): one random transaction per probe row, where the bucket index costs three
// (bucket, sorted keys, build row).  Equal keys stay adjacent and in row order (the sort is stable), so the pairs come out the same
// either way.  Joins on 2..4 key columns and build sides of 2^31 - 1 rows or more take the bucket index whatever the route says.
enum JoinRoute { kJoinTableWhenEligible, kJoinBucketIndex };

struct JoinState {
    // the call (join_check): probe = left, build = right, unless `swap`
    int nkeys, kdt[4];
    int32_t mem;
    bool swap, outer, full, pnulls, bnulls;
    const rdf_array *pk, *bk;
    int64_t pnc, bnc, np, nb;
    rdf_out *out_probe, *out_build;     // both or neither (count only)
    // one run
    bool hashed;                        // the build side is sorted by key * golden ratio (the table's order), not by key
    size_t pin_off;
    const DevChunkCol* d_chunks;        // probe key 0 chunks, probe key 1 chunks, ..., then the build side the same way
    const int64_t *d_prs, *d_brs;       // first row of every chunk, per side
    SortBuffers sb;
    int kcur, icur;                     // sb.keys[kcur] / sb.idx[icur]: the sorted build side
    unsigned long long* d_cnt;          // [0] build NULLs, [1] append cursor, [2] probe rows without a partner, [3] distinct keys, then the placement's overflow flag
    uint64_t *d_bstats, *d_pstats, *d_ostats;   // [min, max] of the build side's sort keys, the probe keys, (hashed) the build keys themselves
    uint64_t bkmin, bkmax;              // key range of the non-NULL build keys ([1, 0] = none)
    int64_t nrv;                        // build rows whose key is not NULL
    const uint64_t *pbits[4], *bbits[4];
    void *ppk, *ppn, *pcounts, *poffs;
    JoinProbeArgs ja;
    JoinAppendArgs aa;
    int64_t probe_rows, total;
    unsigned long long appended, unmatched;
    void *dop, *dob, *dvp, *dvb;        // device outputs
};

rdf_status join_check(const rdf_array* left_keys, int64_t left_nchunks, const rdf_array* right_keys, int64_t right_nchunks, int32_t nkeys, int32_t join_type,
                      rdf_out* out_left, rdf_out* out_right, int64_t* out_rows, JoinState& j) {
    if (!left_keys || !right_keys || left_nchunks < 1 || right_nchunks < 1 || !out_rows) return fail(RDF_INVALID_ARGUMENT, "join: bad arguments");
    if (nkeys < 1 || nkeys > 4) return fail(RDF_INVALID_ARGUMENT, "join: 1 to 4 key columns per side");
    if (join_type < RDF_JOIN_LEFT || join_type > RDF_JOIN_FULL) return fail(RDF_INVALID_ARGUMENT, "join: bad join type");
    if ((out_left == nullptr) != (out_right == nullptr)) return fail(RDF_INVALID_ARGUMENT, "join: give both outputs or neither (count only)");
    j.mem = -1;
    RDF_TRY(check_mem(left_keys, (int64_t)nkeys * left_nchunks, &j.mem));
    RDF_TRY(check_mem(right_keys, (int64_t)nkeys * right_nchunks, &j.mem));
    if (out_left) { RDF_TRY(check_out_mem(out_left, 1, j.mem)); RDF_TRY(check_out_mem(out_right, 1, j.mem)); }
    j.nkeys = nkeys;
    int64_t nleft = 0, nright = 0;
    bool lnulls = false, rnulls = false;
    for (int k = 0; k < 4; ++k) j.kdt[k] = 0;
    for (int k = 0; k < nkeys; ++k) {   // key pair k: left_keys[k * left_nchunks + c] against right_keys[k * right_nchunks + c]
        j.kdt[k] = left_keys[(int64_t)k * left_nchunks].dtype;
        if (!is_numeric(j.kdt[k])) return fail(RDF_INVALID_ARGUMENT, "join: numeric key columns only");
        int64_t nl = 0, nr = 0;
        for (int64_t c = 0; c < left_nchunks; ++c) { const rdf_array& a = left_keys[(int64_t)k * left_nchunks + c]; if (a.dtype != j.kdt[k]) return fail(RDF_INVALID_ARGUMENT, "join: key columns must share one dtype (cast first)"); nl += a.length; lnulls |= a.validity != nullptr; }
        for (int64_t c = 0; c < right_nchunks; ++c) { const rdf_array& a = right_keys[(int64_t)k * right_nchunks + c]; if (a.dtype != j.kdt[k]) return fail(RDF_INVALID_ARGUMENT, "join: key columns must share one dtype (cast first)"); nr += a.length; rnulls |= a.validity != nullptr; }
        if (k == 0) { nleft = nl; nright = nr; }
        else if (nl != nleft || nr != nright) return fail(RDF_COMPUTE_ERROR, "join: key columns of one side differ in length");
    }
    if (nleft >= (int64_t)1 << 32 || nright >= (int64_t)1 << 32) return fail(RDF_INVALID_ARGUMENT, "join: UInt32 indices cap a side at 2^32-1 rows");
    if (out_left && (out_left->dtype != RDF_U32 || out_right->dtype != RDF_U32)) return fail(RDF_INVALID_ARGUMENT, "join: indices are UInt32");
    j.swap = join_type == RDF_JOIN_RIGHT;  // probe = right, build = left
    j.pk = j.swap ? right_keys : left_keys;
    j.bk = j.swap ? left_keys : right_keys;
    j.pnc = j.swap ? right_nchunks : left_nchunks; j.bnc = j.swap ? left_nchunks : right_nchunks;
    j.np = j.swap ? nright : nleft; j.nb = j.swap ? nleft : nright;
    j.pnulls = j.swap ? rnulls : lnulls; j.bnulls = j.swap ? lnulls : rnulls;
    j.outer = join_type != RDF_JOIN_INNER;
    j.full = join_type == RDF_JOIN_FULL;
    j.out_probe = j.swap ? out_right : out_left;
    j.out_build = j.swap ? out_left : out_right;
    return RDF_OK;
}

rdf_status join_stage(JoinState& j) {
    Ctx& ctx = g_ctx;
    size_t used = 0;
    j.pin_off = 0;
    InputStager in;   // staged order: probe key 0 chunks, probe key 1 chunks, ..., then the build side the same way
    for (int64_t c = 0; c < (int64_t)j.nkeys * j.pnc; ++c) in.add(&j.pk[c]);
    for (int64_t c = 0; c < (int64_t)j.nkeys * j.bnc; ++c) in.add(&j.bk[c]);
    RDF_TRY(in.finish(j.pin_off, &used));
    j.pin_off += (used + 255) & ~(size_t)255;
    std::vector<int64_t> prs((size_t)j.pnc + 1, 0), brs((size_t)j.bnc + 1, 0);
    for (int64_t c = 0; c < j.pnc; ++c) prs[(size_t)c + 1] = prs[(size_t)c] + j.pk[c].length;
    for (int64_t c = 0; c < j.bnc; ++c) brs[(size_t)c + 1] = brs[(size_t)c] + j.bk[c].length;
    TableBuilder tb;
    const size_t o_ch = tb.reserve(sizeof(DevChunkCol) * in.dev.size());
    const size_t o_prs = tb.reserve(sizeof(int64_t) * prs.size());
    const size_t o_brs = tb.reserve(sizeof(int64_t) * brs.size());
    RDF_TRY(tb.bind(j.pin_off));
    memcpy(tb.at<char>(o_ch), in.dev.data(), sizeof(DevChunkCol) * in.dev.size());
    memcpy(tb.at<char>(o_prs), prs.data(), sizeof(int64_t) * prs.size());
    memcpy(tb.at<char>(o_brs), brs.data(), sizeof(int64_t) * brs.size());
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(j.pin_off));
    j.pin_off += (tb.size + 255) & ~(size_t)255;
    j.d_chunks = tb.dev_at<DevChunkCol>(o_ch);
    j.d_prs = tb.dev_at<int64_t>(o_prs);
    j.d_brs = tb.dev_at<int64_t>(o_brs);

    RDF_TRY(sort_buffers_alloc(j.nb > 0 ? j.nb : 1, j.sb));
    void* p;
    RDF_TRY(arena_alloc(64, &p));
    j.d_cnt = (unsigned long long*)p;
    HIP_TRY(hipMemsetAsync(j.d_cnt, 0, 64, ctx.stream));
    RDF_TRY(arena_alloc(128, &p));
    j.d_bstats = (uint64_t*)p;
    j.d_pstats = j.d_bstats + 4;
    j.d_ostats = j.d_bstats + 8;
    for (int k = 0; k < 4; ++k) j.pbits[k] = j.bbits[k] = nullptr;
    memset(&j.ja, 0, sizeof j.ja);      // (the lookup step sets its own fields, join_count the rest)
    return RDF_OK;
}

// One column per side: the order-preserving key bits ARE the join key.  Several: the key is a 64-bit hash of the
// tuple's key bits (candidates are verified column by column in the probe kernels), NULL in any column = NULL key.
rdf_status join_side_keys(JoinState& j, bool build, uint64_t* out_keys, uint8_t* nullflags) {
    Ctx& ctx = g_ctx;
    const int64_t n = build ? j.nb : j.np, nch = build ? j.bnc : j.pnc;
    const bool has_nulls = build ? j.bnulls : j.pnulls;
    const size_t chunk0 = build ? (size_t)j.nkeys * (size_t)j.pnc : 0;
    uint64_t* d_stats = build ? j.d_bstats : j.d_pstats;
    const uint64_t** bits_out = build ? j.bbits : j.pbits;
    if (j.nkeys > 1 && has_nulls) HIP_TRY(hipMemsetAsync(nullflags, 0, (size_t)n, ctx.stream));
    JoinCombineArgs ca;
    memset(&ca, 0, sizeof ca);
    for (int k = 0; k < j.nkeys; ++k) {
        SortKeyArgs ka;
        memset(&ka, 0, sizeof ka);
        ka.chunks = j.d_chunks + chunk0 + (size_t)k * (size_t)nch;
        ka.chunk_row_start = build ? j.d_brs : j.d_prs;
        ka.nchunks = nch;
        ka.n = n;
        ka.nullflags = has_nulls ? nullflags : nullptr;
        ka.dtype = j.kdt[k];
        if (j.nkeys == 1) { ka.keys = out_keys; ka.bit_stats = d_stats; if (build && j.hashed) { ka.hash_mul = 0x9E3779B97F4A7C15ull; ka.raw_stats = j.d_ostats; } }   // (the key range stays what the probe's early-out compares against; the sort sees the hashed keys' range)
        else {
            void* pb;
            RDF_TRY(arena_alloc((size_t)n * 8 + 8, &pb));
            ka.keys = (uint64_t*)pb;
            ka.null_or = 1;
            bits_out[k] = ca.bits[k] = (const uint64_t*)pb;
        }
        HIP_TRY(launch_sort_keys(ka, ctx.stream));
    }
    if (j.nkeys > 1) {
        ca.nkeys = j.nkeys; ca.n = n; ca.nullflags = has_nulls ? nullflags : nullptr; ca.out = out_keys; ca.bit_stats = d_stats;
        HIP_TRY(launch_join_combine(ca, ctx.stream));
    }
    return RDF_OK;
}

// build side: key bits + null flags, sorted (NULL keys last)
rdf_status join_sort_build(JoinState& j) {
    Ctx& ctx = g_ctx;
    j.kcur = j.icur = 0;
    j.bkmin = 1; j.bkmax = 0;
    RDF_TRY(sort_stats_reset(j.d_bstats));
    RDF_TRY(sort_stats_reset(j.d_pstats));
    RDF_TRY(sort_stats_reset(j.d_ostats));
    if (j.nb == 0) return RDF_OK;
    RDF_TRY(join_side_keys(j, true, j.sb.keys[0], (uint8_t*)j.sb.nullflags));
    if (j.bnulls) HIP_TRY(launch_count_bytes((const uint8_t*)j.sb.nullflags, j.nb, j.d_cnt, ctx.stream));
    return radix_sort_rows(j.sb, j.nb, j.nkeys == 1 && !j.hashed ? dtype_size(j.kdt[0]) : 8, j.bnulls, &j.kcur, &j.icur, j.d_bstats, j.pin_off, &j.bkmin, &j.bkmax);
}

// probe side: key bits + null flags in row order; then the build side's NULL count and (hashed) its keys' own range
rdf_status join_probe_keys(JoinState& j) {
    Ctx& ctx = g_ctx;
    const int64_t np = j.np;
    RDF_TRY(arena_alloc((size_t)(np > 0 ? np : 1) * 8, &j.ppk));
    RDF_TRY(arena_alloc((size_t)(np > 0 ? np : 1) + 8, &j.ppn));
    RDF_TRY(arena_alloc((size_t)(np + 1) * 8, &j.pcounts));
    RDF_TRY(arena_alloc((size_t)(np + 2 + scan_scratch_words(np)) * 8, &j.poffs));
    if (np > 0) RDF_TRY(join_side_keys(j, false, (uint64_t*)j.ppk, (uint8_t*)j.ppn));
    RDF_TRY(pinned_reserve(j.pin_off + 256));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + j.pin_off, j.d_cnt, 8, hipMemcpyDeviceToHost, ctx.stream));
    if (j.hashed) HIP_TRY(hipMemcpyAsync(ctx.pinned + j.pin_off + 8, j.d_ostats, 16, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    unsigned long long bnull_count = 0;
    memcpy(&bnull_count, ctx.pinned + j.pin_off, 8);
    if (j.hashed) {
        uint64_t st[2];
        memcpy(st, ctx.pinned + j.pin_off + 8, 16);
        if (st[0] > st[1]) { j.bkmin = 1; j.bkmax = 0; } else { j.bkmin = st[0]; j.bkmax = st[1]; }
    }
    j.nrv = j.nb - (int64_t)bnull_count;
    return RDF_OK;
}

// the table of the distinct build keys at load <= 0.5, over a build side sorted by hash
rdf_status join_build_table(JoinState& j, bool* overflowed) {
    Ctx& ctx = g_ctx;
    unsigned long long* d_word = j.d_cnt + 3;      // the distinct count, then the placement's overflow flag
    unsigned long long distinct = 0;
    if (join_table_counts_keys(j.nrv, j.bkmin, j.bkmax)) {     // 8 B/row at the read rate, 0.1 ms per 1e8 rows, and a wait
        HIP_TRY(hipMemsetAsync(d_word, 0, 8, ctx.stream));
        HIP_TRY(launch_join_distinct(j.sb.keys[j.kcur], j.nrv, d_word, ctx.stream));
        HIP_TRY(hipMemcpyAsync(ctx.pinned + j.pin_off, d_word, 8, hipMemcpyDeviceToHost, ctx.stream));
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        memcpy(&distinct, ctx.pinned + j.pin_off, 8);
        HIP_TRY(hipMemsetAsync(d_word, 0, 8, ctx.stream));
    }
    const JoinTablePlan tp = join_table_plan(j.nrv, j.bkmin, j.bkmax, distinct);
    void* ptable;
    RDF_TRY(arena_alloc((size_t)tp.cap * 16 + 64, &ptable));      // (not cleared: the placement writes every slot, the empty ones included)
    JoinPlaceArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.rkeys = j.sb.keys[j.kcur]; pa.ridx = j.sb.idx[j.icur]; pa.nrv = j.nrv; pa.table = (uint64_t*)ptable; pa.cap = tp.cap; pa.tshift = 64 - tp.tbits;
    pa.ntiles = (j.nrv + kJoinPlaceTile - 1) / kJoinPlaceTile;
    void* ptiles;
    RDF_TRY(arena_alloc((size_t)pa.ntiles * 16 + 16, &ptiles));
    pa.tiles = (int64_t*)ptiles;
    pa.flags = d_word;
    HIP_TRY(launch_join_place(pa, ctx.stream));
    // The table is not cleared: a placement that overflowed (a cluster ran past the margin) leaves the slots behind the last
    // key it placed unwritten, and a probe would walk them.  Look at the flag BEFORE anything probes (one 8-byte copy and a wait:
    // microseconds against the milliseconds of a join this size); the caller hands the call to the bucket index if it is set.
    unsigned long long overflow = 0;
    HIP_TRY(hipMemcpyAsync(ctx.pinned + j.pin_off, d_word, 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    memcpy(&overflow, ctx.pinned + j.pin_off, 8);
    *overflowed = overflow != 0;
    j.ja.table = (const uint64_t*)ptable;
    j.ja.tshift = 64 - tp.tbits;
    return RDF_OK;
}

// bucket index over the sorted build keys: about one bucket per build row, on the top bits of (key - min)
rdf_status join_build_buckets(JoinState& j) {
    Ctx& ctx = g_ctx;
    const JoinBucketPlan bp = join_bucket_plan(j.nrv, j.bkmin, j.bkmax);
    void* pbuckets;
    RDF_TRY(arena_alloc((size_t)bp.nbuckets * 8, &pbuckets));
    HIP_TRY(hipMemsetAsync(pbuckets, 0, (size_t)bp.nbuckets * 8, ctx.stream));
    JoinBucketArgs ba;
    memset(&ba, 0, sizeof ba);
    ba.rkeys = j.sb.keys[j.kcur]; ba.nrv = j.nrv; ba.buckets = (uint32_t*)pbuckets; ba.kmin = j.bkmin; ba.bucket_shift = bp.shift;
    HIP_TRY(launch_join_buckets(ba, ctx.stream));
    j.ja.buckets = (const uint32_t*)pbuckets;
    j.ja.bucket_shift = bp.shift;
    return RDF_OK;
}

// count -> scan -> (FULL) how many build rows nobody matched; leaves the output's length in j.total
rdf_status join_count(JoinState& j) {
    Ctx& ctx = g_ctx;
    const int64_t np = j.np, nb = j.nb;
    void *pmatched = nullptr, *pfirst;
    if (j.full) { RDF_TRY(arena_alloc((size_t)((nb + 31) / 32 + 1) * 4, &pmatched)); HIP_TRY(hipMemsetAsync(pmatched, 0, (size_t)((nb + 31) / 32 + 1) * 4, ctx.stream)); }
    RDF_TRY(arena_alloc((size_t)(np > 0 ? np : 1) * 4, &pfirst));
    JoinProbeArgs& ja = j.ja;
    ja.kmin = j.bkmin; ja.kmax = j.bkmax;
    ja.first = (uint32_t*)pfirst;
    ja.nkeys = j.nkeys;
    for (int k = 0; k < 4; ++k) { ja.pbits[k] = j.pbits[k]; ja.bbits[k] = j.bbits[k]; }
    ja.lkeys = (const uint64_t*)j.ppk;
    ja.lnull = j.pnulls ? (const uint8_t*)j.ppn : nullptr;
    ja.rkeys = j.sb.keys[j.kcur];
    ja.ridx = j.sb.idx[j.icur];
    ja.nl = np;
    ja.nrv = j.nrv;
    ja.outer = j.outer;
    ja.counts = (int64_t*)j.pcounts;
    ja.matched = (uint32_t*)pmatched;
    ja.unmatched = j.d_cnt + 2;
    HIP_TRY(launch_join_count(ja, ctx.stream));
    HIP_TRY(launch_scan((const int64_t*)j.pcounts, (int64_t*)j.poffs, np, (int64_t*)j.poffs + np + 1, ctx.stream));
    JoinAppendArgs& aa = j.aa;
    memset(&aa, 0, sizeof aa);
    if (j.full) {
        aa.ridx = j.sb.idx[j.icur];
        aa.matched = (const uint32_t*)pmatched;
        aa.nr = nb;
        aa.nrv = j.nrv;
        aa.cursor = j.d_cnt + 1;
        aa.count_only = 1;
        HIP_TRY(launch_join_append(aa, ctx.stream));
    }
    HIP_TRY(hipMemcpyAsync(ctx.pinned + j.pin_off, (int64_t*)j.poffs + np, 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + j.pin_off + 8, j.d_cnt + 1, 16, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    memcpy(&j.probe_rows, ctx.pinned + j.pin_off, 8);
    memcpy(&j.appended, ctx.pinned + j.pin_off + 8, 8);
    memcpy(&j.unmatched, ctx.pinned + j.pin_off + 16, 8);
    j.total = j.probe_rows + (int64_t)j.appended;
    return RDF_OK;
}

rdf_status join_write(JoinState& j) {
    Ctx& ctx = g_ctx;
    const int64_t total = j.total;
    if (j.out_probe->capacity < total || j.out_build->capacity < total) return fail(RDF_MEMORY_ERROR, "join: output capacity too small (need %lld rows)", (long long)total);
    if ((j.outer && !j.out_build->validity) || (j.full && !j.out_probe->validity)) return fail(RDF_INVALID_ARGUMENT, "output validity buffer required");
    // device outputs
    const size_t words = (size_t)((total + 31) / 32 + 2);
    RDF_TRY(arena_alloc((size_t)(total + 1) * 4, &j.dop));
    RDF_TRY(arena_alloc((size_t)(total + 1) * 4, &j.dob));
    RDF_TRY(arena_alloc(words * 4, &j.dvp));
    RDF_TRY(arena_alloc(words * 4, &j.dvb));
    HIP_TRY(hipMemsetAsync(j.dvp, 0xFF, words * 4, ctx.stream));
    HIP_TRY(hipMemsetAsync(j.dvb, 0xFF, words * 4, ctx.stream));
    JoinProbeArgs& ja = j.ja;
    ja.offsets = (const int64_t*)j.poffs;
    ja.out_probe = (uint32_t*)j.dop;
    ja.out_build = (uint32_t*)j.dob;
    ja.out_build_validity = (uint32_t*)j.dvb;
    ja.matched = nullptr;
    HIP_TRY(launch_join_write(ja, ctx.stream));
    if (j.full) {
        JoinAppendArgs& aa = j.aa;
        unsigned long long start = (unsigned long long)j.probe_rows;
        HIP_TRY(hipMemcpyAsync(j.d_cnt + 1, &start, 8, hipMemcpyHostToDevice, ctx.stream));
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        aa.count_only = 0;
        aa.out_probe = (uint32_t*)j.dop;
        aa.out_build = (uint32_t*)j.dob;
        aa.out_probe_validity = (uint32_t*)j.dvp;
        HIP_TRY(launch_join_append(aa, ctx.stream));
    }
    return RDF_OK;
}

rdf_status join_deliver(JoinState& j) {
    Ctx& ctx = g_ctx;
    const int64_t total = j.total;
    rdf_out *out_probe = j.out_probe, *out_build = j.out_build;
    const hipMemcpyKind kind = j.mem == RDF_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (total > 0) {
        HIP_TRY(hipMemcpyAsync(out_probe->values, j.dop, (size_t)total * 4, kind, ctx.stream));
        HIP_TRY(hipMemcpyAsync(out_build->values, j.dob, (size_t)total * 4, kind, ctx.stream));
        if (out_probe->validity) HIP_TRY(hipMemcpyAsync(out_probe->validity, j.dvp, (size_t)((total + 7) / 8), kind, ctx.stream));
        if (out_build->validity) HIP_TRY(hipMemcpyAsync(out_build->validity, j.dvb, (size_t)((total + 7) / 8), kind, ctx.stream));
    }
    // null counts: build-side NULLs = probe rows without a partner; probe-side NULLs = appended rows
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    out_probe->length = out_build->length = total;
    out_probe->null_count = (int64_t)j.appended;
    out_build->null_count = (int64_t)j.unmatched;
    return RDF_OK;
}

// One run of a checked call.  *overflowed: the table's placement ran past its margin (keys that crowd on the last slots); nothing
// was delivered and the caller runs the bucket route.
rdf_status join_run(JoinState& j, JoinRoute route, int64_t* out_rows, bool* overflowed) {
    *overflowed = false;
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();
    j.hashed = route == kJoinTableWhenEligible && j.nkeys == 1 && j.nb > 0 && j.nb < ((int64_t)1 << 31) - 1;
    RDF_TRY(join_stage(j));
    KernelTimer kt;
    RDF_TRY(join_sort_build(j));
    RDF_TRY(join_probe_keys(j));
    if (j.hashed && j.nrv > 0) {
        RDF_TRY(join_build_table(j, overflowed));
        if (*overflowed) { kt.stop(); return RDF_OK; }
    } else RDF_TRY(join_build_buckets(j));
    RDF_TRY(join_count(j));
    *out_rows = j.total;
    if (!j.out_probe) { kt.stop(); return RDF_OK; }
    RDF_TRY(join_write(j));
    kt.stop();
    ctx.last_kernel = "join_write_kernel";
    return join_deliver(j);
}
}  // namespace

rdf_status rdf_equijoin_indices(const rdf_array* left_keys, int64_t left_nchunks, const rdf_array* right_keys, int64_t right_nchunks,
                                int32_t join_type, rdf_out* out_left, rdf_out* out_right, int64_t* out_rows) {
    return rdf_equijoin_indices_multi(left_keys, left_nchunks, right_keys, right_nchunks, 1, join_type, out_left, out_right, out_rows);
}

rdf_status rdf_equijoin_indices_multi(const rdf_array* left_keys, int64_t left_nchunks, const rdf_array* right_keys, int64_t right_nchunks,
                                      int32_t nkeys, int32_t join_type, rdf_out* out_left, rdf_out* out_right, int64_t* out_rows) {
    const JoinRoute route = g_ctx.opt_join_table == 0 ? kJoinBucketIndex : kJoinTableWhenEligible;
    JoinState j;
    RDF_TRY(join_check(left_keys, left_nchunks, right_keys, right_nchunks, nkeys, join_type, out_left, out_right, out_rows, j));
    if (j.np == 0 && (!j.full || j.nb == 0)) {
        *out_rows = 0;
        if (out_left) { out_left->length = out_right->length = 0; out_left->null_count = out_right->null_count = 0; }
        return RDF_OK;
    }
    bool overflowed = false;
    RDF_TRY(join_run(j, route, out_rows, &overflowed));
    if (overflowed) RDF_TRY(join_run(j, kJoinBucketIndex, out_rows, &overflowed));
    return RDF_OK;
}
