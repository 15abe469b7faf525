// rdf_capi_groupby.inc — host side of the second-generation GROUP BY (rdf_groupby.hip); textually included by rdf_capi.cpp
// (it uses that file's per-thread context, arena and staging helpers).
//
//   rdf_groupby_agg            Transformation::GroupAggregate(groups, [Sum | Min | Max | Count]) over 1..4 integer grouping
//                              columns (Dataset::try_aggregate, src/expression.rs:114-221; AggregateFunction :696-711)
//   rdf_groupby_merge          (key, partial, count) triples -> groups: the merge step of the multi-GPU exchange
//   rdf_group_exchange_pack / _unpack   partial groups bucketed by owning rank for all_to_all_single (SURVEY.md §8e)

namespace {

// device scratch shared by every path: [0] special sums[2] | [16] special counts[2] | [32] special flags[2] |
// [40] cursor | [44] null-key flag out | [48] flags | [56] value nulls (u64) | [64] key nulls[4] (u64)
struct GbScratch {
    char* p = nullptr;
    unsigned long long* sums() const { return (unsigned long long*)p; }
    unsigned long long* counts() const { return (unsigned long long*)(p + 16); }
    unsigned int* special() const { return (unsigned int*)(p + 32); }
    unsigned int* cursor() const { return (unsigned int*)(p + 40); }
    uint32_t* flags() const { return (uint32_t*)(p + 48); }
    unsigned long long* value_nulls() const { return (unsigned long long*)(p + 56); }
    unsigned long long* key_nulls() const { return (unsigned long long*)(p + 64); }
};

rdf_status gb_scratch_init(GbScratch& s, int op) {
    void* p = nullptr;
    RDF_TRY(arena_alloc(128, &p));
    s.p = (char*)p;
    HIP_TRY(hipMemsetAsync(p, 0, 128, g_ctx.stream));
    if (op == AGG_MIN) HIP_TRY(hipMemsetAsync(p, 0xFF, 16, g_ctx.stream));   // identity of MIN
    return RDF_OK;
}

rdf_status gb_table_alloc(GroupTable& t, unsigned int** cursor, int64_t max_groups, int op) {
    int64_t capacity = 1024;
    while (capacity < 2 * max_groups) capacity <<= 1;
    void* p = nullptr;
    RDF_TRY(arena_alloc(sizeof(uint64_t) * (size_t)(3 * capacity + 4) + 64, &p));
    t.keys = (unsigned long long*)p;
    t.sums = t.keys + capacity;
    t.counts = t.sums + capacity + 2;
    t.special = (unsigned int*)(t.counts + capacity + 2);
    t.ngroups = t.special + 2;
    t.flags = (uint32_t*)(t.special + 4);
    *cursor = t.special + 6;
    t.capacity = capacity;
    hipStream_t s = g_ctx.stream;
    HIP_TRY(launch_gb2_fill((uint64_t*)t.keys, capacity, kGroupEmpty, s));
    HIP_TRY(launch_gb2_fill((uint64_t*)t.sums, capacity + 2, op == AGG_MIN ? ~0ull : 0ull, s));
    HIP_TRY(hipMemsetAsync(t.counts, 0, sizeof(uint64_t) * (size_t)(capacity + 2) + 64, s));
    return RDF_OK;
}

// dense group results in device temporaries
struct GbDense {
    char*     keys = nullptr;      // [cap] key dtype (or packed u64)
    uint64_t* acc = nullptr;       // [cap]
    int64_t*  counts = nullptr;    // [cap]
    uint8_t*  kvalid = nullptr;    // bitmap, cap bits
    uint8_t*  vvalid = nullptr;    // bitmap, cap bits (MIN / MAX)
    int64_t   cap = 0, ng = 0;
    int64_t   key_nulls = 0, value_nulls = 0;
};
rdf_status gb_dense_alloc(GbDense& d, int64_t cap, size_t kes) {
    void* p;
    const size_t bm = (size_t)((cap + 63) / 64 * 8) + 8;
    RDF_TRY(arena_alloc((size_t)cap * kes + 64, &p)); d.keys = (char*)p;
    RDF_TRY(arena_alloc((size_t)cap * 8 + 64, &p)); d.acc = (uint64_t*)p;
    RDF_TRY(arena_alloc((size_t)cap * 8 + 64, &p)); d.counts = (int64_t*)p;
    RDF_TRY(arena_alloc(bm, &p)); d.kvalid = (uint8_t*)p;
    RDF_TRY(arena_alloc(bm, &p)); d.vvalid = (uint8_t*)p;
    HIP_TRY(hipMemsetAsync(d.kvalid, 0, bm, g_ctx.stream));
    d.cap = cap;
    return RDF_OK;
}

// The groups the kernels set aside (the key whose hash is the LDS free marker; the NULL key) join the dense arrays
// on the host side of one small round trip; then cursor / flags decide the call's fate.
rdf_status gb_collect(const GbScratch& sc, GbDense& d, size_t kes, int64_t max_groups, int64_t ng_main_known, bool main_all_valid,
                      const unsigned int* table_cursor, const uint32_t* table_flags, size_t pin_off, uint32_t* flags_out) {
    Ctx& ctx = g_ctx;
    RDF_TRY(pinned_reserve(pin_off + 256));
    char* pin = ctx.pinned + pin_off;
    HIP_TRY(hipMemcpyAsync(pin, sc.p, 64, hipMemcpyDeviceToHost, ctx.stream));
    if (table_cursor) HIP_TRY(hipMemcpyAsync(pin + 64, table_cursor, 4, hipMemcpyDeviceToHost, ctx.stream));
    if (table_flags) HIP_TRY(hipMemcpyAsync(pin + 72, table_flags, 4, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    unsigned long long hs[4];
    unsigned int hf[4];
    uint32_t flags = 0, tflags = 0;
    unsigned int tcur = 0;
    memcpy(hs, pin, 32);
    memcpy(hf, pin + 32, 16);     // special[0], special[1], cursor, -
    memcpy(&flags, pin + 48, 4);
    if (table_cursor) memcpy(&tcur, pin + 64, 4);
    if (table_flags) memcpy(&tflags, pin + 72, 4);
    flags |= tflags;
    *flags_out = flags;
    if (flags & (16u | 32u | 64u)) return RDF_OK;   // the caller re-runs another path (16: a scatter region overflowed; 32: a partition's LDS table filled up)
    int64_t ng = ng_main_known >= 0 ? ng_main_known : (table_cursor ? (int64_t)tcur : (int64_t)hf[2]);
    const int64_t nspecial = (hf[0] ? 1 : 0) + (hf[1] ? 1 : 0);
    if ((flags & 4u) || ng + nspecial > d.cap || ng > max_groups + (table_cursor ? 2 : 0))
        return fail(RDF_MEMORY_ERROR, "groupby: more than max_groups (%lld) distinct keys", (long long)max_groups);
    if (main_all_valid && ng > 0) {   // the partition path emits no NULL key itself
        HIP_TRY(hipMemsetAsync(d.kvalid, 0xFF, (size_t)(ng / 8), ctx.stream));
        if (ng & 7) { const uint8_t last = (uint8_t)((1u << (ng & 7)) - 1); HIP_TRY(hipMemcpyAsync(d.kvalid + ng / 8, &last, 1, hipMemcpyHostToDevice, ctx.stream)); HIP_TRY(hipStreamSynchronize(ctx.stream)); }
    }
    auto put = [&](uint64_t key, unsigned long long sum, unsigned long long cnt, bool valid_key) -> rdf_status {
        HIP_TRY(hipMemcpyAsync(d.keys + (size_t)ng * kes, &key, kes, hipMemcpyHostToDevice, ctx.stream));
        HIP_TRY(hipMemcpyAsync(d.acc + ng, &sum, 8, hipMemcpyHostToDevice, ctx.stream));
        HIP_TRY(hipMemcpyAsync(d.counts + ng, &cnt, 8, hipMemcpyHostToDevice, ctx.stream));
        // the bitmap byte holding bit ng: bits below ng are final, bits above are still zero
        uint8_t byte = 0;
        HIP_TRY(hipMemcpyAsync(&byte, d.kvalid + ng / 8, 1, hipMemcpyDeviceToHost, ctx.stream));
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        if (valid_key) byte |= (uint8_t)(1u << (ng & 7)); else byte &= (uint8_t)~(1u << (ng & 7));
        HIP_TRY(hipMemcpyAsync(d.kvalid + ng / 8, &byte, 1, hipMemcpyHostToDevice, ctx.stream));
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        ++ng;
        return RDF_OK;
    };
    if (hf[0]) {   // inverse of g2_hash at ~0
        uint64_t z = ~0ull;
        z ^= z >> 32; z *= 0xF1DE83E19937733Dull; z ^= z >> 32;
        RDF_TRY(put(z, hs[0], hs[2], true));
    }
    if (hf[1]) RDF_TRY(put(0, hs[1], hs[3], false));
    d.ng = ng;
    return RDF_OK;
}

// raw accumulators -> values (+ MIN / MAX validity), key null count
rdf_status gb_finish_values(const GbScratch& sc, GbDense& d, int op, int vcls, size_t pin_off) {
    Ctx& ctx = g_ctx;
    if (d.ng > 0 && op != AGG_SUM) {
        Gb2FinishArgs fa;
        memset(&fa, 0, sizeof fa);
        fa.acc = d.acc; fa.counts = d.counts; fa.validity = d.vvalid; fa.n = d.ng; fa.op = op; fa.vcls = vcls; fa.native_in = 0;
        fa.nulls = sc.value_nulls();
        HIP_TRY(launch_gb2_finish(fa, ctx.stream));
        RDF_TRY(pinned_reserve(pin_off + 64));
        HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, sc.value_nulls(), 8, hipMemcpyDeviceToHost, ctx.stream));
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        unsigned long long vn = 0;
        memcpy(&vn, ctx.pinned + pin_off, 8);
        d.value_nulls = (int64_t)vn;
    }
    return RDF_OK;
}

rdf_status gb_copy_out(const void* dev, size_t bytes, void* dst, int32_t mem) {
    if (!bytes) return RDF_OK;
    HIP_TRY(hipMemcpyAsync(dst, dev, bytes, mem == RDF_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, g_ctx.stream));
    return RDF_OK;
}
rdf_status gb_fill_valid(rdf_out* o, int64_t ng, int32_t mem) {
    if (o->validity && ng > 0) {
        if (mem == RDF_MEM_HOST) memset(o->validity, 0xFF, (size_t)((ng + 7) / 8));
        else HIP_TRY(hipMemsetAsync(o->validity, 0xFF, (size_t)((ng + 7) / 8), g_ctx.stream));
    }
    return RDF_OK;
}

int gb_acc_dtype(int op, int vdt) {   // dtype of the value output
    if (vdt < 0) return RDF_I64;
    if (is_float(vdt)) return RDF_F64;
    if (op != AGG_SUM && vdt == RDF_U64) return RDF_U64;
    return RDF_I64;
}

// ---- the engine: ONE key column (chunked like the values) -> dense groups ----
struct GbInput {
    std::vector<DevChunkCol> keys, values;   // device views, nchunks each (values empty: count rows)
    std::vector<int64_t> clen;
    int kdt = RDF_I64, vdt = -1;
    // a pinned frame's tables (rdf_groupby_agg_frame): nothing is built or uploaded per call.  keys / values / clen above then
    // hold chunk 0 only (the one-chunk kernels read their descriptors from the launch arguments).
    const DevChunkCol* d_keys = nullptr;
    const DevChunkCol* d_values = nullptr;
    const int64_t* d_tile_start = nullptr;     // tiles of kEvalTile rows
    const int64_t* d_len = nullptr;
    int64_t f_nchunks = 0, f_ntiles = 0, f_nrows = 0;
    bool f_fast = false;                       // 8-byte keys / values, no bitmaps, every chunk 16-byte aligned
};

// returns RDF_OK with *skewed = true when the partition path gave up (region overflow): the caller picks another path
rdf_status gb_engine(const GbInput& in, int op, int64_t max_groups, int force_path /* -1 auto, 0 table, 1 partition, 2 stream */,
                     GbScratch& sc, GbDense& d, size_t& pin_off, bool* skewed, bool* lds_full, bool allow_compact = true, bool allow_hot = true) {
    Ctx& ctx = g_ctx;
    *skewed = false;
    *lds_full = false;
    const bool framed = in.d_keys != nullptr;
    const int64_t nchunks = framed ? in.f_nchunks : (int64_t)in.clen.size();
    const size_t kes = (size_t)dtype_size(in.kdt);
    const int vcls = in.vdt < 0 ? CLS_UNSIGNED : value_class(in.vdt);
    std::vector<int64_t> tile_start;
    int64_t nrows = framed ? in.f_nrows : 0;
    TableBuilder tb;
    size_t o_k = 0, o_v = 0, o_ts = 0, o_len = 0;
    if (!framed) {
        tile_start.assign((size_t)nchunks + 1, 0);
        for (int64_t c = 0; c < nchunks; ++c) { tile_start[(size_t)c + 1] = tile_start[(size_t)c] + (in.clen[(size_t)c] + kEvalTile - 1) / kEvalTile; nrows += in.clen[(size_t)c]; }
        o_k = tb.reserve(sizeof(DevChunkCol) * (size_t)nchunks);
        o_v = tb.reserve(sizeof(DevChunkCol) * (size_t)nchunks);
        o_ts = tb.reserve(sizeof(int64_t) * tile_start.size());
        o_len = tb.reserve(sizeof(int64_t) * in.clen.size());
        RDF_TRY(tb.bind(pin_off));
        memcpy(tb.at<char>(o_k), in.keys.data(), sizeof(DevChunkCol) * (size_t)nchunks);
        if (!in.values.empty()) memcpy(tb.at<char>(o_v), in.values.data(), sizeof(DevChunkCol) * (size_t)nchunks);
        memcpy(tb.at<char>(o_ts), tile_start.data(), sizeof(int64_t) * tile_start.size());
        memcpy(tb.at<char>(o_len), in.clen.data(), sizeof(int64_t) * in.clen.size());
        RDF_TRY(tb.alloc());
        RDF_TRY(tb.upload(pin_off));
        pin_off += (tb.size + 255) & ~(size_t)255;
    }
    const int64_t ntiles = framed ? in.f_ntiles : tile_start[(size_t)nchunks];

    RDF_TRY(gb_scratch_init(sc, op));
    const int64_t cap_out = std::min<int64_t>(max_groups, nrows) + 4;
    RDF_TRY(gb_dense_alloc(d, cap_out, kes));

    Gb2Args a;
    memset(&a, 0, sizeof a);
    a.keys = framed ? in.d_keys : tb.dev_at<DevChunkCol>(o_k);
    a.values = framed ? in.d_values : tb.dev_at<DevChunkCol>(o_v);
    a.chunk_tile_start = framed ? in.d_tile_start : tb.dev_at<int64_t>(o_ts);
    a.chunk_len = framed ? in.d_len : tb.dev_at<int64_t>(o_len);
    a.nchunks = nchunks;
    a.ntiles = ntiles;
    if (nchunks == 1) { a.key0 = in.keys[0]; if (!in.values.empty()) a.val0 = in.values[0]; a.len0 = in.clen[0]; }
    a.key_dtype = in.kdt;
    a.value_dtype = in.vdt;
    a.op = op;
    a.vcls = vcls;
    a.special_sums = sc.sums();
    a.special_counts = sc.counts();
    a.special = sc.special();
    a.flags = sc.flags();
    {   // the fast loader: 8-byte integer keys and 8-byte (or no) values, no bitmap, every chunk 16-byte aligned
        bool fast = (in.kdt == RDF_I64 || in.kdt == RDF_U64) && (in.vdt < 0 || in.vdt == RDF_F64 || in.vdt == RDF_I64 || in.vdt == RDF_U64);
        if (framed) fast = fast && in.f_fast;
        for (int64_t c = 0; c < nchunks && fast && !framed; ++c) {
            if (in.clen[(size_t)c] == 0) continue;
            const DevChunkCol& k = in.keys[(size_t)c];
            if (k.validity || (((uintptr_t)k.values + (uintptr_t)k.offset * 8) & 15) != 0) fast = false;
            if (in.vdt >= 0) {
                const DevChunkCol& v = in.values[(size_t)c];
                if (v.validity || (((uintptr_t)v.values + (uintptr_t)v.offset * 8) & 15) != 0) fast = false;
            }
        }
        a.fast = fast ? 1 : 0;
    }

    int path = force_path;
    if (path < 0) path = max_groups <= kG2StreamGroups ? 2 : max_groups <= kG2MaxGroups ? 1 : 0;
    if (path == 2 && max_groups > 2600) path = 1;
    if (path == 1 && max_groups > kG2MaxGroups) path = 0;
    uint32_t flags = 0;
    const int ncu = std::max(1, eval_grid_limit() / 8);

    if (path == 1) {
        // scatter (two blocks per CU, fixed-capacity regions) -> aggregate (one block per partition)
        constexpr int P = 1 << kG2PartBits;
        const int64_t nsuper = (ntiles + kG2Super / kEvalTile - 1) / (kG2Super / kEvalTile);
        const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(nsuper, std::min<int64_t>(kG2MaxBlocks, kG2BlocksPerCU * (int64_t)ncu)));
        const int64_t m = (nrows + (int64_t)nb * P - 1) / ((int64_t)nb * P);     // mean records per region
        const int64_t cap_rec = m + m / 8 + (int64_t)(6.0 * std::sqrt((double)m)) + 16;
        // 12-byte records: keys of at most 32 bits always fit their type's window; 8-byte keys when the probe's sample spans
        // less than 2^38 (the scatter checks every key against the 2^39 window and the call falls back to 16-byte records on a miss)
        // Measured (1e9 rows, 1e6 groups): rows only counted, 4-byte records 7.0 ms against 8.1 with 16-byte records; with values,
        // 12-byte records 10.7 against 9.6 — the scatter's time is its write TRANSACTIONS (a 64-byte run of key words costs what a
        // 128-byte line costs: one per 8 records in either layout) plus LDS phases that the second array lengthens, and the
        // aggregate pass is bound by its LDS table, not by the 12 or 16 GB it reads.  So the default compacts COUNT only.
        bool compact = allow_compact && (ctx.opt_gb_compact == 2 || (ctx.opt_gb_compact == 1 && in.vdt < 0));
        uint64_t key_base = 0;
        // (window bases are multiples of 2^31: the probe's compact histogram, taken with base 0, is then the real one rotated)
        if (in.kdt == RDF_I32 || in.kdt == RDF_I16 || in.kdt == RDF_I8) key_base = (uint64_t)(int64_t)INT32_MIN;
        const bool need_window = compact && kes == 8;
        int LREC = compact && !need_window ? kG2LineC : kG2Line;   // records per line (settled after the probe for 8-byte keys)
        int64_t cap_lines = (cap_rec + LREC - 1) / LREC + 1;
        if ((int64_t)P * nb * ((cap_rec + kG2Line - 1) / kG2Line + 1) >= ((int64_t)1 << 32) - 1) { *skewed = true; return RDF_OK; }   // line numbers are 32-bit on the device: another path
        // capacity plan for skewed keys (filled from the probe's histogram below): per-partition region sizes, and the big
        // partitions cut into several aggregate items that meet in the global table
        std::vector<uint32_t> plan_off, plan_cap;
        std::vector<Gb2Work> plan_work;
        bool plan_multi = false;
        uint64_t plan_lines = 0;
        bool dense_keys = false;      // the sampled keys span at most 4 x max_groups values
        bool hot = false;             // heavy-hitter split: the hot keys go through gb2_stream_kernel, the scatter path takes the rest
        int hot_keys = 0;
        const bool want_skew = (nrows >= ((int64_t)1 << 22) && force_path != 1) || ctx.opt_gb_skew_plan == 2;
        if (want_skew || need_window) {
            // skew probe: would a partition's share overflow its regions (capacity cap_rec / m of the mean)?
            const int64_t tile_step = std::max<int64_t>(1, ntiles / 16384);
            void* ph = nullptr;
            constexpr size_t kHotBins = 65536;
            const bool want_hot = want_skew && allow_hot && ctx.opt_gb_hot != 0;      // also sample the hash's top 16 bits: where the heavy hitters are
            RDF_TRY(arena_alloc(P * 8 + 64 + (want_hot ? kHotBins * 4 : 0), &ph));
            HIP_TRY(hipMemsetAsync(ph, 0, P * 8 + 64 + (want_hot ? kHotBins * 4 : 0), ctx.stream));
            unsigned long long* pmm = (unsigned long long*)((char*)ph + P * 8);   // [min, max] of the sampled keys
            unsigned int* phb = want_hot ? (unsigned int*)((char*)ph + P * 8 + 64) : nullptr;
            HIP_TRY(hipMemsetAsync(pmm, 0xFF, 8, ctx.stream));
            HIP_TRY(launch_gb2_skew_probe(a, tile_step, (unsigned int*)ph, pmm, phb, nullptr, ctx.stream));
            RDF_TRY(pinned_reserve(pin_off + P * 8 + 64 + kHotBins * 4 + 8192 + 2048 + 4096 * 16 + 512));     // (everything the heavy-hitter search reads back: the buffer must not move under hprobe)
            HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, ph, P * 8 + 16, hipMemcpyDeviceToHost, ctx.stream));
            HIP_TRY(hipStreamSynchronize(ctx.stream));
            const unsigned int* hprobe = (const unsigned int*)(ctx.pinned + pin_off);
            {
                // Keys packed into a range a few times their number (dictionary codes, row numbers modulo something, TPC-H keys) never
                // collide under the multiplicative hash: one key per probe is the cheapest table for them (same-box A/B per 1e9 rows:
                // 9.24 against 9.48 ms); keys that hash like random numbers want the buckets of four (11.9 against 14.7 ms)
                unsigned long long mm[2];
                memcpy(mm, ctx.pinned + pin_off + P * 8, 16);
                dense_keys = mm[0] <= mm[1] && (mm[1] - mm[0]) / 4 < (uint64_t)std::max<int64_t>(max_groups, 1);
            }
            if (need_window) {
                unsigned long long mm[2];
                memcpy(mm, ctx.pinned + pin_off + P * 8, 16);
                const uint64_t flip = in.kdt == RDF_I64 ? 0x8000000000000000ull : 0ull;
                constexpr uint64_t kWindow = ((uint64_t)1 << 39) - 1;
                compact = mm[0] <= mm[1] && mm[1] - mm[0] < ((uint64_t)1 << 38);
                if (compact) {   // the window: the sample's span in the middle of 2^39 consecutive keys
                    const uint64_t slack = (kWindow - (mm[1] - mm[0])) / 2;
                    uint64_t lo = mm[0] >= slack ? mm[0] - slack : 0;
                    lo = std::min<uint64_t>(lo, ~0ull - kWindow) & ~(((uint64_t)1 << 31) - 1);   // (rounding down costs < 2^31 of a slack of >= 2^37)
                    key_base = lo ^ flip;
                    LREC = kG2LineC;
                    cap_lines = (cap_rec + LREC - 1) / LREC + 1;
                }
                if (getenv("RDF_DEBUG")) fprintf(stderr, "[rdf] key window: sampled [%llu, %llu] (ordered image) -> %s\n", mm[0], mm[1], compact ? "12-byte records" : "16-byte records");
            }
          if (want_skew && want_hot) {
            // Heavy hitters.  When the 64-bit hash's partitions are uneven, look at the sample by the hash's top 16 bits: a Zipf-like
            // input has a few dozen classes far above the mean; a second run over the same sample counts the KEYS inside those
            // classes, and the up to 100 keys that stand out (the bench's s = 1.1: 100 keys hold ~62 % of the rows) get a pass of
            // their own — gb2_stream_kernel over their rows only, folded per block in replicated LDS sub-tables like any small
            // GROUP BY, merged into a small table in HBM — while the scatter path runs over the OTHER rows, which are as even as
            // uniform keys, need no capacity plan and write that much less.  (Per 1e9 rows: 19.1 ms on the first-generation
            // combining path, where these inputs used to go.)
            const unsigned int* h0 = hprobe;
            uint64_t total = 0, mx = 0;
            for (int i = 0; i < P; ++i) { total += h0[i]; mx = std::max<uint64_t>(mx, h0[i]); }
            const double mean = (double)total / P;
            const double limit = mean * (1.0 + 0.6 * ((double)cap_rec / (double)m - 1.0));
            if (total >= 65536 && (double)mx > std::max(limit, mean + 5.0 * std::sqrt(mean))) {
                unsigned int* hb = (unsigned int*)(ctx.pinned + pin_off + P * 8 + 64);
                HIP_TRY(hipMemcpyAsync(hb, phb, kHotBins * 4, hipMemcpyDeviceToHost, ctx.stream));
                HIP_TRY(hipStreamSynchronize(ctx.stream));
                const double mean_bin = (double)total / (double)kHotBins;
                const unsigned int floor_count = (unsigned int)std::max(48.0, 6.0 * mean_bin);
                uint32_t* bm = (uint32_t*)(ctx.pinned + pin_off + P * 8 + 64 + kHotBins * 4);     // class bitmap [2048], then the hot keys' table [256 x 8 bytes]
                memset(bm, 0, 8192);
                size_t nclasses = 0;
                for (uint32_t b = 0; b < kHotBins; ++b) if (hb[b] >= floor_count) { bm[b >> 5] |= 1u << (b & 31); ++nclasses; }
                constexpr size_t kKeySlots = 4096;
                if (nclasses > 0 && nclasses <= 1200) {
                    void* pbm = nullptr;
                    void* pkt = nullptr;
                    RDF_TRY(arena_alloc(8192 + 2048 + 64, &pbm));
                    RDF_TRY(arena_alloc(kKeySlots * 16 + 64, &pkt));
                    HIP_TRY(hipMemcpyAsync(pbm, bm, 8192, hipMemcpyHostToDevice, ctx.stream));
                    HIP_TRY(hipMemsetAsync(pkt, 0, kKeySlots * 16, ctx.stream));
                    a.hot_bitmap = (const uint32_t*)pbm;
                    HIP_TRY(launch_gb2_skew_probe(a, tile_step, (unsigned int*)ph, nullptr, nullptr, (unsigned long long*)pkt, ctx.stream));   // (hist gets the samples a second time: not read again)
                    unsigned long long* pk = (unsigned long long*)((char*)bm + 8192 + 2048);
                    HIP_TRY(hipMemcpyAsync(pk, pkt, kKeySlots * 16, hipMemcpyDeviceToHost, ctx.stream));
                    HIP_TRY(hipStreamSynchronize(ctx.stream));
                    std::vector<std::pair<unsigned long long, unsigned long long>> keys;   // (samples, hashed key)
                    for (size_t i = 0; i < kKeySlots; ++i) if (pk[2 * i] != 0 && pk[2 * i + 1] >= floor_count) keys.emplace_back(pk[2 * i + 1], pk[2 * i]);
                    std::sort(keys.begin(), keys.end(), [](const std::pair<unsigned long long, unsigned long long>& x, const std::pair<unsigned long long, unsigned long long>& y) { return x.first > y.first; });
                    if (keys.size() > 100) keys.resize(100);
                    uint64_t hot_samples = 0;
                    std::vector<uint64_t> cold(P);
                    for (int i = 0; i < P; ++i) cold[(size_t)i] = h0[i];
                    for (auto& k : keys) { hot_samples += k.first; uint64_t& c = cold[(size_t)(k.second >> (64 - kG2PartBits))]; c -= std::min<uint64_t>(c, k.first); }
                    const double hot_frac = (double)hot_samples / (double)total;
                    uint64_t ctotal = 0, cmx = 0;
                    for (int i = 0; i < P; ++i) { ctotal += cold[(size_t)i]; cmx = std::max(cmx, cold[(size_t)i]); }
                    const double cmean = (double)ctotal / P;
                    // the other rows' regions are sized at 1.6 x their mean share: every partition must sit well below that
                    const bool cold_even = ctotal > 0 && (double)cmx <= cmean * 1.4 + 5.0 * std::sqrt(cmean);
                    if (getenv("RDF_DEBUG")) fprintf(stderr, "[rdf] heavy hitters: %zu classes, %zu keys hold %.1f %% of %llu samples; the others' largest partition %.3f x their mean -> %s\n", nclasses, keys.size(),
                                                     100.0 * hot_frac, (unsigned long long)total, cmean > 0 ? cmx / cmean : 0.0, (!keys.empty() && hot_frac >= 0.05 && cold_even) ? "split" : "no split");
                    if (!keys.empty() && hot_frac >= 0.05 && cold_even) {
                        hot = true;
                        compact = false; LREC = kG2Line;                 // (the hot keys are known by their 64-bit hash: 16-byte records)
                        memset(bm, 0, 8192);
                        unsigned long long* ktab = (unsigned long long*)((char*)bm + 8192);
                        for (int i = 0; i < 256; ++i) ktab[i] = ~0ull;
                        for (auto& k : keys) {
                            const uint32_t cls = (uint32_t)(k.second >> 48);
                            bm[cls >> 5] |= 1u << (cls & 31);
                            uint32_t sl = (uint32_t)(k.second >> 24) & 255u;
                            while (ktab[sl] != ~0ull) sl = (sl + 1) & 255u;
                            ktab[sl] = k.second;
                        }
                        HIP_TRY(hipMemcpyAsync(pbm, bm, 8192 + 2048, hipMemcpyHostToDevice, ctx.stream));
                        hot_keys = (int)keys.size();
                        // regions for the other rows: their share of a block's rows per partition, 1.6 x (keys just below the hot
                        // threshold still lean on their partitions) + noise
                        const double cold_rows = (double)nrows * std::min(1.0, (1.0 - hot_frac) * 1.05 + 0.01);
                        const double mc = cold_rows / ((double)nb * P);
                        const int64_t cap_c = (int64_t)(1.6 * mc + 8.0 * std::sqrt(mc) + 64.0);
                        cap_lines = (cap_c + LREC - 1) / LREC + 1;
                        pin_off += (P * 8 + 64 + kHotBins * 4 + 8192 + 2048 + kKeySlots * 16 + 255) & ~(size_t)255;
                    } else a.hot_bitmap = nullptr;
                }
            }
          }
          if (want_skew && !hot) {
            // the histogram of the partitions this call's scatter will use
            unsigned int hh[P];
            const uint32_t rot = (uint32_t)(((key_base * kG2cMul) & (((uint64_t)1 << 39) - 1)) >> 31);
            for (int i = 0; i < P; ++i) hh[i] = compact ? hprobe[P + ((i + rot) & (P - 1))] : hprobe[i];
            uint64_t total = 0, mx = 0;
            for (int i = 0; i < P; ++i) { total += hh[i]; mx = std::max<uint64_t>(mx, hh[i]); }
            const double mean = (double)total / P;
            // flag at 60 % of the regions' head room, but never inside the sample's own noise (5 sigma)
            const double limit = mean * (1.0 + 0.6 * ((double)cap_rec / (double)m - 1.0));
            if (getenv("RDF_DEBUG")) fprintf(stderr, "[rdf] skew probe: %llu samples, largest partition %.3f x mean (limit %.3f)\n", (unsigned long long)total, mean > 0 ? mx / mean : 0.0, limit / std::max(mean, 1.0));
            const bool skew = total >= 65536 && (double)mx > std::max(limit, mean + 5.0 * std::sqrt(mean));
            if ((skew || ctx.opt_gb_skew_plan == 2) && ctx.opt_gb_skew_plan && total > 0) {
                // Zipf-like keys, one key holding a third of the rows, ...: the partitions are uneven but the scatter still works
                // when every partition's regions are sized for ITS share (1.25 x the sampled share + 8 sigma + a constant),
                // and the aggregate pass stays balanced when a partition that holds k times the mean is cut into ~k items
                const double rows_per_block = (double)nrows / nb;
                const double target = 1.5 * (double)nrows / P;
                plan_off.resize(P); plan_cap.resize(P);
                for (int p = 0; p < P; ++p) {
                    const double share = (double)std::max<unsigned int>(hh[p], 1u) / (double)total;
                    const double exp_rec = share * rows_per_block;
                    const double cap_r = 1.25 * exp_rec + 8.0 * std::sqrt(exp_rec) + 64.0;
                    plan_cap[(size_t)p] = (uint32_t)((cap_r + LREC - 1) / LREC) + 1;
                    plan_off[(size_t)p] = (uint32_t)plan_lines;
                    plan_lines += (uint64_t)nb * plan_cap[(size_t)p];
                    // a partition above 1.5 x the mean is cut into pieces of a quarter of the mean: the items are dealt to the blocks
                    // largest first, so the finest pieces even out what the whole partitions leave uneven
                    const double rows_p = share * (double)nrows;
                    int S = rows_p > target ? (int)std::ceil(rows_p / (target / 6.0)) : 1;
                    S = std::max(1, std::min(S, nb));
                    for (int q = 0; q < S; ++q) plan_work.push_back(Gb2Work{p, (int32_t)((int64_t)nb * q / S), (int32_t)((int64_t)nb * (q + 1) / S), S > 1 ? 1 : 0});
                    plan_multi |= S > 1;
                }
                {   // largest items first (size ~ the partition's sampled share x its fraction of the scatter blocks)
                    std::vector<double> sz(plan_work.size());
                    std::vector<size_t> ord(plan_work.size());
                    for (size_t i = 0; i < plan_work.size(); ++i) { ord[i] = i; sz[i] = (double)std::max<unsigned int>(hh[plan_work[i].p], 1u) * (plan_work[i].b1 - plan_work[i].b0); }
                    std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return sz[x] > sz[y]; });
                    std::vector<Gb2Work> sorted(plan_work.size());
                    for (size_t i = 0; i < ord.size(); ++i) sorted[i] = plan_work[ord[i]];
                    plan_work.swap(sorted);
                }
                if (plan_lines >= ((uint64_t)1 << 32) - 1) { *skewed = true; return RDF_OK; }
                // The plan pays when the weight sits in a FEW partitions (one key holding a third of the rows: 21.6 -> 13-13.8 ms per
                // 1e9 rows).  With a dozen or more heavy partitions (the bench's Zipf-like keys: a quarter of the rows in one key, then
                // keys of 7, 4, 2.5, ... %) the aggregate pass measured 14 ms however the pieces were cut or pre-combined, 22 ms in
                // all against 19 ms for the first-generation combining path: those inputs keep that path.
                int heavy = 0;
                for (int p = 0; p < P; ++p) heavy += (double)hh[p] / (double)total * (double)nrows > target;
                if (heavy > 6 && ctx.opt_gb_skew_plan != 2) { *skewed = true; return RDF_OK; }
                if (getenv("RDF_DEBUG")) fprintf(stderr, "[rdf] skew plan: %zu aggregate items over %d partitions, %.2f GB of regions (uniform layout: %.2f GB)\n", plan_work.size(), P, plan_lines * (compact ? 192e-9 : 128e-9), (double)P * nb * cap_lines * (compact ? 192e-9 : 128e-9));
            } else if (skew) { *skewed = true; return RDF_OK; }
          }
        }
        void *precs, *pnl, *preck = nullptr;
        const bool planned = !plan_work.empty();
        if (planned) {
            void* pp = nullptr;
            const size_t tb = (size_t)P * 8 + plan_work.size() * sizeof(Gb2Work);
            RDF_TRY(arena_alloc(tb + 64, &pp));
            RDF_TRY(pinned_reserve(pin_off + tb + 256));
            memcpy(ctx.pinned + pin_off, plan_off.data(), (size_t)P * 4);
            memcpy(ctx.pinned + pin_off + (size_t)P * 4, plan_cap.data(), (size_t)P * 4);
            memcpy(ctx.pinned + pin_off + (size_t)P * 8, plan_work.data(), plan_work.size() * sizeof(Gb2Work));
            HIP_TRY(hipMemcpyAsync(pp, ctx.pinned + pin_off, tb, hipMemcpyHostToDevice, ctx.stream));
            pin_off += (tb + 255) & ~(size_t)255;
            a.part_off = (const uint32_t*)pp;
            a.part_cap = a.part_off + P;
        }
        const size_t region_lines = planned ? (size_t)plan_lines : (size_t)P * (size_t)nb * (size_t)cap_lines;
        if (compact) {   // values (unless only rows are counted) and key words in areas of their own
            RDF_TRY(arena_alloc(in.vdt >= 0 ? region_lines * kG2LineC * 8 + 64 : 64, &precs));
            RDF_TRY(arena_alloc(region_lines * kG2LineC * 4 + 64, &preck));
        } else RDF_TRY(arena_alloc(region_lines * kG2Line * 16 + 64, &precs));
        RDF_TRY(arena_alloc((size_t)P * (size_t)nb * 4 + 64, &pnl));
        a.recs = (uint64_t*)precs;
        a.recs_k = (uint32_t*)preck;
        a.key_base = key_base;
        a.compact = compact ? 1 : 0;
        a.nlines = (uint32_t*)pnl;
        a.cap_lines = cap_lines;
        KernelTimer kt;
        unsigned int* tcur = nullptr;
        if (hot) {
            // pass 0: the rows of the hot classes, folded per block in LDS, merged into a small table in HBM
            RDF_TRY(gb_table_alloc(a.t, &tcur, 1024, op));
            a.hot_mode = 2;
            // replicated sub-tables (lane % replicas picks one) spread a wave's same-key LDS atomics, as for any small GROUP BY
            if (hot_keys <= 52) { a.sub_slots = 113; a.replicas = 16; }
            else { a.sub_slots = 241; a.replicas = 8; }
            a.table_slots = a.sub_slots * a.replicas;                       // <= 38 KB + 10 KB of class bitmap and hot keys: two blocks share a CU
            constexpr int TPI = 2;
            const int hgrid = (int)std::max<int64_t>(1, std::min<int64_t>((ntiles + TPI - 1) / TPI, 2 * (int64_t)ncu));
            HIP_TRY(launch_gb2_stream(a, hgrid, ctx.stream));
            a.hot_mode = 1;
        }
        HIP_TRY(launch_gb2_scatter(a, nb, ctx.stream));
        Gb2AggArgs ga;
        memset(&ga, 0, sizeof ga);
        ga.recs = (const uint64_t*)precs;
        ga.recs_k = (const uint32_t*)preck;
        ga.key_base = key_base;
        ga.compact = a.compact | ((ctx.opt_gb_bucket == 1 || (ctx.opt_gb_bucket == 0 && dense_keys)) ? 256 : 0);   // bit 8: one key per probe in the partition tables
        if (getenv("RDF_DEBUG")) fprintf(stderr, "[rdf] gb2 aggregate pass: %s\n", (ga.compact & 256) ? "one key per probe" : "buckets of four");
        ga.nlines = (const uint32_t*)pnl;
        ga.nb = nb;
        ga.cap_lines = cap_lines;
        ga.op = op; ga.vcls = vcls; ga.has_values = in.vdt >= 0; ga.key_dtype = in.kdt;
        ga.out_keys = d.keys; ga.out_acc = d.acc; ga.out_counts = d.counts;
        ga.cursor = sc.cursor();
        ga.flags = sc.flags();
        ga.max_out = cap_out - 2;
        if (planned) {
            ga.part_off = a.part_off; ga.part_cap = a.part_cap;
            ga.work = (const Gb2Work*)(a.part_cap + P);
            ga.nwork = (int32_t)plan_work.size();
            if (plan_multi) { RDF_TRY(gb_table_alloc(a.t, &tcur, max_groups, op)); ga.t = a.t; }
        }
        HIP_TRY(launch_gb2_aggregate(ga, ctx.stream));
        const bool table_groups = (planned && plan_multi) || hot;
        if (table_groups) {
            // the cut partitions' groups (the heavy hitters' classes) sit in the global table: append them to the groups emitted straight from LDS
            RDF_TRY(pinned_reserve(pin_off + 64));
            HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, a.t.special, 32, hipMemcpyDeviceToHost, ctx.stream));
            HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off + 32, sc.flags(), 4, hipMemcpyDeviceToHost, ctx.stream));
            HIP_TRY(hipMemcpyAsync(tcur, sc.cursor(), 4, hipMemcpyDeviceToDevice, ctx.stream));
            HIP_TRY(hipStreamSynchronize(ctx.stream));
            unsigned int tpin[9];
            memcpy(tpin, ctx.pinned + pin_off, 36);
            if (!(tpin[8] & (16u | 32u | 64u | 128u))) {   // (a region or an LDS table overflowed: what the table holds is incomplete, gb_collect sends the caller to another path)
                if ((tpin[4] & 4u) || (int64_t)tpin[2] > max_groups) return fail(RDF_MEMORY_ERROR, "groupby: more than max_groups (%lld) distinct keys", (long long)max_groups);
                GroupEmitArgs ea;
                memset(&ea, 0, sizeof ea);
                ea.t = a.t; ea.out_keys = d.keys; ea.out_keys_validity = nullptr; ea.out_sums = d.acc; ea.out_counts = d.counts; ea.cursor = tcur; ea.key_dtype = in.kdt;
                HIP_TRY(launch_gb2_emit(ea, ctx.stream));
            }
        }
        kt.stop();
        ctx.last_kernel = hot ? "gb2_stream_kernel (heavy hitters) + gb2_scatter_kernel+gb2_aggregate_kernel"
                        : compact ? (planned ? "gb2_scatter_kernel+gb2_aggregate_kernel (12-byte records, capacity plan)" : "gb2_scatter_kernel+gb2_aggregate_kernel (12-byte records)")
                                  : (planned ? "gb2_scatter_kernel+gb2_aggregate_kernel (capacity plan)" : "gb2_scatter_kernel+gb2_aggregate_kernel");
        RDF_TRY(gb_collect(sc, d, kes, max_groups, -1, true, table_groups ? tcur : nullptr, table_groups ? a.t.flags : nullptr, pin_off, &flags));
        if (getenv("RDF_DEBUG")) {
            std::vector<uint32_t> nl((size_t)P * (size_t)nb);
            (void)hipMemcpy(nl.data(), pnl, nl.size() * 4, hipMemcpyDeviceToHost);
            uint64_t tot = 0; uint32_t mx = 0;
            for (uint32_t x : nl) { tot += x; mx = std::max(mx, x); }
            fprintf(stderr, "[rdf] gb2 partition path: rows=%lld nb=%d cap_lines=%lld flags=0x%x lines total=%llu max=%u ng=%lld\n", (long long)nrows, nb, (long long)cap_lines, flags, (unsigned long long)tot, mx, (long long)d.ng);
        }
        if (hot && (flags & (128u | 16u | 32u))) {   // the others were not as even as sampled (16, 32); 128, a full table of hot keys, cannot happen with at most 100 of them (rdf_groupby.hip) and is kept as a guard: without the split
            if (getenv("RDF_DEBUG")) fprintf(stderr, "[rdf] gb2: the heavy-hitter split gave up (flags 0x%x), re-running without it\n", flags);
            return gb_engine(in, op, max_groups, force_path, sc, d, pin_off, skewed, lds_full, allow_compact, false);
        }
        if (flags & 64u) {   // a key outside the sampled window: the same call on 16-byte records
            if (getenv("RDF_DEBUG")) fprintf(stderr, "[rdf] gb2: a key outside the 2^39 window, re-running with 16-byte records\n");
            return gb_engine(in, op, max_groups, force_path, sc, d, pin_off, skewed, lds_full, false);
        }
        if (flags & 16u) { *skewed = true; return RDF_OK; }
        if (flags & 32u) { *skewed = true; *lds_full = true; return RDF_OK; }   // uneven GROUPS per partition (the probe measures rows): HBM table
        return gb_finish_values(sc, d, op, vcls, pin_off);
    }

    // both remaining paths end in the global table
    unsigned int* tcursor = nullptr;
    RDF_TRY(gb_table_alloc(a.t, &tcursor, max_groups, op));
    {
        KernelTimer kt;
        if (path == 2) {
            // LDS table = R sub-tables of S slots (lane % R picks one): few groups would otherwise serialise the
            // same-address LDS atomics of a wave
            // (A 2729-slot table, three blocks per CU, was measured for up to ~1300 groups: slower at every group count, 2.97-3.2
            // ms against 2.57-2.9 ms per 1e9 rows — the smaller table's bank conflicts cost more than the extra waves hide.)
            static const int prime_slots[6] = {3989, 1993, 997, 491, 241, 113};      // (1 << r) * prime[r] <= table slots
            static_assert(2 * 1993 <= kGbSlots && 4 * 997 <= kGbSlots && 8 * 491 <= kGbSlots && 16 * 241 <= kGbSlots && 32 * 113 <= kGbSlots, "sub-tables fit the LDS table");
            a.table_slots = prime_slots[0];
            int r = 0;
            while (r < 5 && (int64_t)prime_slots[r + 1] >= 2 * max_groups + 2) ++r;
            a.replicas = 1 << r;
            a.sub_slots = prime_slots[r];
            if (getenv("RDF_DEBUG")) fprintf(stderr, "[rdf] gb2 stream path: %d sub-tables of %d slots for max_groups %lld\n", a.replicas, a.sub_slots, (long long)max_groups);
            constexpr int TPI = 2;
            int grid = (int)std::max<int64_t>(1, std::min<int64_t>((ntiles + TPI - 1) / TPI, 2 * (int64_t)ncu));
            HIP_TRY(launch_gb2_stream(a, grid, ctx.stream));
            ctx.last_kernel = "gb2_stream_kernel";
        } else {
            HIP_TRY(launch_gb2_table_rows(a, ctx.stream));
            ctx.last_kernel = "gb2_table_rows_kernel";
        }
        kt.stop();
    }
    GroupEmitArgs ea;
    memset(&ea, 0, sizeof ea);
    ea.t = a.t;
    ea.out_keys = d.keys;
    ea.out_keys_validity = d.kvalid;
    ea.out_sums = d.acc;
    ea.out_counts = d.counts;
    ea.cursor = tcursor;
    ea.key_dtype = in.kdt;
    // emit only when the table's distinct-key count fits the dense buffers: read it first
    RDF_TRY(pinned_reserve(pin_off + 64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, a.t.special, 32, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    unsigned int tpin[8];
    memcpy(tpin, ctx.pinned + pin_off, 32);
    if ((tpin[4] & 4u) || (int64_t)tpin[2] > max_groups) return fail(RDF_MEMORY_ERROR, "groupby: more than max_groups (%lld) distinct keys", (long long)max_groups);
    HIP_TRY(launch_gb2_emit(ea, ctx.stream));
    RDF_TRY(gb_collect(sc, d, kes, max_groups, -1, false, tcursor, a.t.flags, pin_off, &flags));
    return gb_finish_values(sc, d, op, vcls, pin_off);
}

// the first-generation histogram / combining scatter / aggregate path (rdf_capi.cpp): sums and counts of one integer key column
bool gb_fallback_in_range(int64_t max_groups, int64_t nrows);
rdf_status groupby_sum_fallback(const rdf_array* keys, const rdf_array* values, int64_t nchunks, int64_t max_groups,
                                rdf_out* out_keys, rdf_out* out_sums, rdf_out* out_counts, int64_t slack);

// Several grouping columns <-> ONE packed 64-bit key, shared by rdf_groupby_agg and rdf_groupby_multi (and through them the
// Utf8 compositions): every column range-compressed to bits(max - min) (+ a code for NULL), one min / max pass per column
// decides the layout.  Columns whose ranges together need more than 64 bits (several sparse keys) are dictionary-coded
// instead: a count-only GROUP BY of the column alone gives its distinct values (at most max_groups of them), their sorted
// order is the code
struct GbKeyPack {
    KeyPackArgs kp;
    int range_bits[kMaxKeyCols] = {0, 0, 0, 0};
    bool use_dict[kMaxKeyCols] = {false, false, false, false};
    std::vector<uint64_t> hdict[kMaxKeyCols];
    GbKeyPack() { memset(&kp, 0, sizeof kp); }

    // the field layout: one min / max pass per column (nkeys > 1; one column is grouped as it is)
    rdf_status plan(const rdf_array* keys, int32_t nkeys, int64_t nchunks, const int* kdt, const bool* knullable, int64_t max_groups, int64_t nrows) {
        if (nkeys > 1) {
            int total_bits = 0;
            for (int k = 0; k < nkeys; ++k) {
                rdf_agg_result r;
                RDF_TRY(agg_column(keys + (int64_t)k * nchunks, nchunks, false, &r));
                const bool sgn = is_signed_int(kdt[k]);
                uint64_t lo = 0, hi = 0;
                if (r.is_some) {
                    lo = sgn ? ((uint64_t)r.min_i64 ^ 0x8000000000000000ull) : h_normalize_int(kdt[k], (uint64_t)r.min_i64);
                    hi = sgn ? ((uint64_t)r.max_i64 ^ 0x8000000000000000ull) : h_normalize_int(kdt[k], (uint64_t)r.max_i64);
                }
                uint64_t span = hi - lo;                       // largest field code before the NULL shift
                int bits = 0;
                if (knullable[k] && span == ~0ull) bits = 65;  // a full-range nullable column has no spare code: dictionary only
                else {
                    if (knullable[k]) ++span;
                    while (bits < 64 && (span >> bits) != 0) ++bits;
                    if (bits == 0) bits = 1;
                }
                kp.dtype[k] = kdt[k];
                kp.nullable[k] = knullable[k] ? 1 : 0;
                kp.bias[k] = lo;
                range_bits[k] = bits;
                total_bits += bits;
            }
            if (total_bits > 64) {
                // widest columns first, until the tuple fits with every dictionary column priced at bits(max_groups + 1)
                const int64_t dmax = std::min<int64_t>(max_groups, std::max<int64_t>(nrows, 1)) + 1;
                int dbits = 1;
                while (dbits < 63 && ((uint64_t)dmax >> dbits) != 0) ++dbits;
                while (total_bits > 64) {
                    int w = -1;
                    for (int k = 0; k < nkeys; ++k) if (!use_dict[k] && range_bits[k] > dbits && (w < 0 || range_bits[k] > range_bits[w])) w = k;
                    if (w < 0) return fail(RDF_INVALID_ARGUMENT, "groupby: the grouping columns need %d bits even dictionary-coded; at most 64 are supported", total_bits);
                    use_dict[w] = true;
                    total_bits -= range_bits[w] - dbits;
                }
            }
        }
        return RDF_OK;
    }

    // one attempt's packed key column (in the arena) -> in.keys / in.kdt; dev: the staged chunks, the key columns first
    rdf_status pack(const std::vector<DevChunkCol>& dev, const int* kdt, const bool* knullable, int32_t nkeys, int64_t nchunks, int64_t nrows,
                    const std::vector<int64_t>& clen, const std::vector<int64_t>& row_start, int64_t max_groups, size_t& pin_off, GbInput& in) {
        Ctx& ctx = g_ctx;
        TableBuilder ktb;
        size_t o_cols = 0, o_rs = 0;
        void* ppk = nullptr;
        RDF_TRY(arena_alloc((size_t)std::max<int64_t>(nrows, 1) * 8 + 64, &ppk));
        o_cols = ktb.reserve(sizeof(DevChunkCol) * (size_t)nkeys * (size_t)nchunks);
        o_rs = ktb.reserve(sizeof(int64_t) * row_start.size());
        RDF_TRY(ktb.bind(pin_off));
        memcpy(ktb.at<char>(o_cols), dev.data(), sizeof(DevChunkCol) * (size_t)nkeys * (size_t)nchunks);
        memcpy(ktb.at<char>(o_rs), row_start.data(), sizeof(int64_t) * row_start.size());
        RDF_TRY(ktb.alloc());
        RDF_TRY(ktb.upload(pin_off));
        pin_off += (ktb.size + 255) & ~(size_t)255;
        kp.cols = ktb.dev_at<DevChunkCol>(o_cols);
        kp.chunk_row_start = ktb.dev_at<int64_t>(o_rs);
        kp.nchunks = nchunks; kp.n = nrows; kp.nkeys = nkeys;
        kp.packed = (uint64_t*)ppk;
        // dictionaries of the sparse columns (built once, uploaded per attempt), then the field layout
        int total_bits = 0;
        for (int k = 0; k < nkeys; ++k) {
            int bits = range_bits[k];
            kp.dict[k] = nullptr; kp.dict_n[k] = 0;
            if (use_dict[k] && nrows > 0) {
                if (hdict[k].empty()) {
                    GbInput din;
                    din.clen = clen; din.kdt = kdt[k]; din.vdt = -1;
                    din.keys.assign(dev.begin() + (size_t)k * (size_t)nchunks, dev.begin() + (size_t)(k + 1) * (size_t)nchunks);
                    GbScratch dsc; GbDense dd; bool dskew = false;
                    bool dfull = false;
                    RDF_TRY(gb_engine(din, AGG_SUM, max_groups, ctx.opt_gb_partition == 0 ? 0 : -1, dsc, dd, pin_off, &dskew, &dfull));
                    if (dskew) RDF_TRY(gb_engine(din, AGG_SUM, max_groups, 0, dsc, dd, pin_off, &dskew, &dfull));
                    const size_t es = (size_t)dtype_size(kdt[k]);
                    std::vector<char> hk((size_t)dd.ng * es);
                    std::vector<uint8_t> hv((size_t)((dd.ng + 7) / 8), 0xFF);
                    if (dd.ng) HIP_TRY(hipMemcpyAsync(hk.data(), dd.keys, hk.size(), hipMemcpyDeviceToHost, ctx.stream));
                    if (dd.ng && knullable[k]) HIP_TRY(hipMemcpyAsync(hv.data(), dd.kvalid, hv.size(), hipMemcpyDeviceToHost, ctx.stream));
                    HIP_TRY(hipStreamSynchronize(ctx.stream));
                    hdict[k].reserve((size_t)dd.ng);
                    for (int64_t i = 0; i < dd.ng; ++i) {
                        if (!((hv[(size_t)(i >> 3)] >> (i & 7)) & 1)) continue;
                        uint64_t raw = 0;
                        memcpy(&raw, hk.data() + (size_t)i * es, es);
                        const uint64_t nv = h_normalize_int(kdt[k], raw);
                        hdict[k].push_back(is_signed_int(kdt[k]) ? nv ^ 0x8000000000000000ull : nv);
                    }
                    std::sort(hdict[k].begin(), hdict[k].end());
                    if (hdict[k].empty()) hdict[k].push_back(0);   // an all-NULL column: one unused code
                }
                void* pd = nullptr;
                RDF_TRY(arena_alloc(hdict[k].size() * 8 + 64, &pd));
                HIP_TRY(hipMemcpyAsync(pd, hdict[k].data(), hdict[k].size() * 8, hipMemcpyHostToDevice, ctx.stream));
                HIP_TRY(hipStreamSynchronize(ctx.stream));
                kp.dict[k] = (const uint64_t*)pd;
                kp.dict_n[k] = (int64_t)hdict[k].size();
                uint64_t span = (uint64_t)hdict[k].size() - 1 + (knullable[k] ? 1 : 0);
                bits = 0;
                while (bits < 64 && (span >> bits) != 0) ++bits;
                if (bits == 0) bits = 1;
            }
            kp.shift[k] = total_bits;
            kp.mask[k] = bits >= 64 ? ~0ull : ((1ull << bits) - 1);
            total_bits += bits;
        }
        if (total_bits > 64) return fail(RDF_INVALID_ARGUMENT, "groupby: the grouping columns need %d bits after range / dictionary coding; at most 64 are supported", total_bits);
        if (getenv("RDF_DEBUG")) for (int k = 0; k < nkeys; ++k) fprintf(stderr, "[rdf] groupby key column %d: %s\n", k, use_dict[k] ? "dictionary-coded" : "range-packed");
        HIP_TRY(launch_key_pack(kp, ctx.stream));
        in.kdt = RDF_U64;
        in.keys.resize((size_t)nchunks);
        for (int64_t c = 0; c < nchunks; ++c) in.keys[(size_t)c] = DevChunkCol{ppk, nullptr, row_start[(size_t)c]};
        return RDF_OK;
    }

    // the dense packed keys of ng groups -> one array per grouping column, copied out with validity and null counts
    rdf_status unpack(const void* packed, int64_t ng, const int* kdt, int32_t nkeys, unsigned long long* key_nulls, rdf_out* out_keys, int32_t mem, size_t pin_off) {
        Ctx& ctx = g_ctx;
        // unpack the tuple into one dense array per grouping column
        void* pouts[kMaxKeyCols]; void* pval[kMaxKeyCols];
        for (int k = 0; k < nkeys; ++k) {
            RDF_TRY(arena_alloc((size_t)std::max<int64_t>(ng, 1) * (size_t)dtype_size(kdt[k]) + 64, &pouts[k]));
            RDF_TRY(arena_alloc((size_t)((ng + 63) / 64 * 8) + 8, &pval[k]));
            kp.out_values[k] = pouts[k];
            kp.out_validity[k] = (uint8_t*)pval[k];
        }
        kp.packed = (uint64_t*)packed;
        kp.n = ng;
        kp.out_nulls = key_nulls;
        HIP_TRY(hipMemsetAsync(key_nulls, 0, 32, ctx.stream));
        HIP_TRY(launch_key_unpack(kp, ctx.stream));
        RDF_TRY(pinned_reserve(pin_off + 64));
        HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, key_nulls, 32, hipMemcpyDeviceToHost, ctx.stream));
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        unsigned long long kn[4];
        memcpy(kn, ctx.pinned + pin_off, 32);
        for (int k = 0; k < nkeys; ++k) {
            RDF_TRY(gb_copy_out(pouts[k], (size_t)ng * (size_t)dtype_size(kdt[k]), out_keys[k].values, mem));
            if (out_keys[k].validity) RDF_TRY(gb_copy_out(pval[k], (size_t)((ng + 7) / 8), out_keys[k].validity, mem));
            out_keys[k].length = ng;
            out_keys[k].null_count = (int64_t)kn[k];
        }
        return RDF_OK;
    }
};

// rdf_groupby_agg.  slack: groups beyond max_groups the caller accepts — 0 for the public entries, whose promise counts every
// group; 2 for rdf_groupby_agg_keys over Utf8 keys, where the up to two set-aside groups (the NULL key; the code whose hash is
// the LDS free marker) never counted
rdf_status groupby_agg_impl(const rdf_array* keys, int32_t nkeys, const rdf_array* values, int64_t nchunks, int32_t agg, int64_t max_groups,
                            rdf_out* out_keys, rdf_out* out_values, rdf_out* out_counts, int64_t slack) {
    if (nchunks < 1 || !keys) return fail(RDF_INVALID_ARGUMENT, "groupby: a column has at least one chunk");
    if (nkeys < 1 || nkeys > kMaxKeyCols) return fail(RDF_INVALID_ARGUMENT, "groupby: 1..%d grouping columns", kMaxKeyCols);
    if (!out_keys || !out_values || !out_counts) return fail(RDF_INVALID_ARGUMENT, "groupby: null output");
    if (max_groups < 1) return fail(RDF_INVALID_ARGUMENT, "groupby: max_groups must be positive");
    if (agg < RDF_AGG_SUM || agg > RDF_AGG_COUNT) return fail(RDF_INVALID_ARGUMENT, "groupby: unknown aggregate %d", agg);
    if (agg == RDF_AGG_COUNT) values = nullptr;
    else if (!values) agg = RDF_AGG_COUNT;
    const int op = agg == RDF_AGG_MIN ? AGG_MIN : agg == RDF_AGG_MAX ? AGG_MAX : AGG_SUM;
    int32_t mem = -1;
    RDF_TRY(check_mem(keys, (int64_t)nkeys * nchunks, &mem));
    if (values) RDF_TRY(check_mem(values, nchunks, &mem));
    RDF_TRY(check_out_mem(out_keys, nkeys, mem));
    RDF_TRY(check_out_mem(out_values, 1, mem));
    RDF_TRY(check_out_mem(out_counts, 1, mem));
    int kdt[kMaxKeyCols];
    bool knullable[kMaxKeyCols];
    for (int k = 0; k < nkeys; ++k) {
        kdt[k] = keys[(int64_t)k * nchunks].dtype;
        if (!(kdt[k] >= RDF_I8 && kdt[k] <= RDF_U64)) return fail(RDF_INVALID_ARGUMENT, "groupby: integer key column required");
        knullable[k] = false;
        for (int64_t c = 0; c < nchunks; ++c) {
            const rdf_array& kc = keys[(int64_t)k * nchunks + c];
            if (kc.dtype != kdt[k]) return fail(RDF_INVALID_ARGUMENT, "groupby: chunks differ in dtype");
            if (kc.length != keys[c].length) return fail(RDF_COMPUTE_ERROR, "groupby: grouping columns differ in length");
            knullable[k] |= kc.validity != nullptr;
        }
        if (out_keys[k].dtype != kdt[k]) return fail(RDF_INVALID_ARGUMENT, "groupby: key output %d must have the key dtype", k);
        if (knullable[k] && !out_keys[k].validity) return fail(RDF_INVALID_ARGUMENT, "output validity buffer required");
    }
    const int vdt = values ? values[0].dtype : -1;
    if (values && !is_numeric(vdt)) return fail(RDF_INVALID_ARGUMENT, "groupby: numeric value column required");
    bool vnullable = false;
    int64_t nrows = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        if (values && values[c].dtype != vdt) return fail(RDF_INVALID_ARGUMENT, "groupby: chunks differ in dtype");
        if (values && values[c].length != keys[c].length) return fail(RDF_COMPUTE_ERROR, "groupby: key and value chunks differ in length");
        vnullable |= values && values[c].validity != nullptr;
        nrows += keys[c].length;
    }
    const int odt = gb_acc_dtype(op, vdt);
    if (out_values->dtype != odt || out_counts->dtype != RDF_I64)
        return fail(RDF_INVALID_ARGUMENT, "groupby: outputs must be (key dtypes, %s, Int64)", odt == RDF_F64 ? "Float64" : odt == RDF_U64 ? "UInt64" : "Int64");
    if (op != AGG_SUM && vnullable && !out_values->validity) return fail(RDF_INVALID_ARGUMENT, "groupby: min / max of a nullable column needs an output validity buffer");
    const int64_t cap_needed = std::min<int64_t>(max_groups + 2, nrows + 2);
    for (int k = 0; k < nkeys; ++k) if (out_keys[k].capacity < cap_needed) return fail(RDF_MEMORY_ERROR, "output capacity too small (need max_groups + 2)");
    if (out_values->capacity < cap_needed || out_counts->capacity < cap_needed) return fail(RDF_MEMORY_ERROR, "output capacity too small (need max_groups + 2)");

    // host-resident batches beyond one slab, one Int64 / UInt64 grouping column without NULLs: streamed — every slab is
    // aggregated on the device while the next one crosses the link, and the partial groups are merged slab by slab
    if (mem == RDF_MEM_HOST && nkeys == 1 && !knullable[0] && (kdt[0] == RDF_I64 || kdt[0] == RDF_U64) && g_ctx.opt_stream_slab >= 0 && !g_ctx.in_stream) {
        int64_t bytes = host_input_bytes(keys, 1, nchunks);
        if (values) bytes += host_input_bytes(values, 1, nchunks);
        if (bytes > stream_slab_bytes()) return groupby_stream(keys, values, nchunks, agg, max_groups, out_keys, out_values, out_counts, slack);
    }

    GbKeyPack pk;
    RDF_TRY(pk.plan(keys, nkeys, nchunks, kdt, knullable, max_groups, nrows));

    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    for (int attempt = 0; attempt < 2; ++attempt) {
        arena_begin();
        size_t pin_off = 0, used = 0;
        InputStager st;
        for (int64_t i = 0; i < (int64_t)nkeys * nchunks; ++i) st.add(&keys[i]);
        if (values) for (int64_t c = 0; c < nchunks; ++c) st.add(&values[c]);
        RDF_TRY(st.finish(pin_off, &used));
        pin_off += (used + 255) & ~(size_t)255;
        GbInput in;
        in.clen.resize((size_t)nchunks);
        std::vector<int64_t> row_start((size_t)nchunks + 1, 0);
        for (int64_t c = 0; c < nchunks; ++c) { in.clen[(size_t)c] = keys[c].length; row_start[(size_t)c + 1] = row_start[(size_t)c] + keys[c].length; }
        in.vdt = vdt;
        if (values) in.values.assign(st.dev.begin() + (size_t)nkeys * (size_t)nchunks, st.dev.end());
        if (nkeys == 1) {
            in.kdt = kdt[0];
            in.keys.assign(st.dev.begin(), st.dev.begin() + (size_t)nchunks);
        } else {
            RDF_TRY(pk.pack(st.dev, kdt, knullable, nkeys, nchunks, nrows, in.clen, row_start, max_groups, pin_off, in));
        }
        GbScratch sc;
        GbDense d;
        bool skewed = false, lds_full = false;
        int force = ctx.opt_gb_partition == 0 ? 0 : -1;     // rdf_set_option("gb_partition", 0): always the HBM table (A/B)
        if (ctx.opt_gb_partition == 4) force = 1;           // tests: the partition path whatever max_groups says
        if (attempt == 1) force = 0;                        // the partition path gave up on skewed keys
        if (nrows == 0) {
            for (int k = 0; k < nkeys; ++k) { out_keys[k].length = 0; out_keys[k].null_count = 0; }
            out_values->length = out_counts->length = 0; out_values->null_count = out_counts->null_count = 0;
            return RDF_OK;
        }
        RDF_TRY(gb_engine(in, op, max_groups, force, sc, d, pin_off, &skewed, &lds_full));
        if (skewed && lds_full) continue;                   // too many groups landed in one partition: the HBM table takes any distribution
        if (skewed) {
            // heavily skewed keys overflowed a scatter region: sums of a single key column take the first-generation
            // histogram + combining path (built for exactly this) where its tables hold max_groups, everything else the HBM table
            if (op == AGG_SUM && nkeys == 1 && ctx.opt_gb_partition != 4 && gb_fallback_in_range(max_groups, nrows))
                return groupby_sum_fallback(keys, values, nchunks, max_groups, out_keys, out_values, out_counts, slack);
            continue;
        }
        const int64_t ng = d.ng;
        // the header's promise counts every group: gb_collect appends the up to two set-aside groups (the NULL key; the key whose hash
        // is the LDS free marker) to as many as max_groups others, and the engine's other callers (the dictionary build) rely on that slack
        if (ng > max_groups + slack) return fail(RDF_MEMORY_ERROR, "groupby: more than max_groups (%lld) distinct keys", (long long)max_groups);
        if (nkeys == 1) {
            RDF_TRY(gb_copy_out(d.keys, (size_t)ng * (size_t)dtype_size(kdt[0]), out_keys->values, mem));
            if (out_keys->validity) RDF_TRY(gb_copy_out(d.kvalid, (size_t)((ng + 7) / 8), out_keys->validity, mem));
            // NULL-key groups: the bitmap's zero bits below ng
            RDF_TRY(pinned_reserve(pin_off + 64));
            unsigned long long* cnt = sc.key_nulls();
            HIP_TRY(hipMemsetAsync(cnt, 0, 8, ctx.stream));
            // count set bits: one byte-count kernel over the bitmap would do; the only NULL group is a single one, so look at counts instead
            out_keys->null_count = 0;
            if (knullable[0]) {
                std::vector<uint8_t> bm((size_t)((ng + 7) / 8));
                if (!bm.empty()) { HIP_TRY(hipMemcpyAsync(bm.data(), d.kvalid, bm.size(), hipMemcpyDeviceToHost, ctx.stream)); HIP_TRY(hipStreamSynchronize(ctx.stream)); }
                int64_t set = 0;
                for (int64_t i = 0; i < ng; ++i) set += (bm[(size_t)(i >> 3)] >> (i & 7)) & 1;
                out_keys->null_count = ng - set;
            }
            out_keys->length = ng;
        } else {
            RDF_TRY(pk.unpack(d.keys, ng, kdt, nkeys, sc.key_nulls(), out_keys, mem, pin_off));
        }
        RDF_TRY(gb_copy_out(d.acc, (size_t)ng * 8, out_values->values, mem));
        RDF_TRY(gb_copy_out(d.counts, (size_t)ng * 8, out_counts->values, mem));
        if (op != AGG_SUM && out_values->validity) RDF_TRY(gb_copy_out(d.vvalid, (size_t)((ng + 7) / 8), out_values->validity, mem));
        else RDF_TRY(gb_fill_valid(out_values, ng, mem));
        RDF_TRY(gb_fill_valid(out_counts, ng, mem));
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        out_values->length = out_counts->length = ng;
        out_values->null_count = op != AGG_SUM ? d.value_nulls : 0;
        out_counts->null_count = 0;
        return RDF_OK;
    }
    return fail(RDF_COMPUTE_ERROR, "groupby: no path completed");
}

}  // namespace

extern "C" {

rdf_status rdf_groupby_agg(const rdf_array* keys, int32_t nkeys, const rdf_array* values, int64_t nchunks, int32_t agg, int64_t max_groups,
                           rdf_out* out_keys, rdf_out* out_values, rdf_out* out_counts) {
    return groupby_agg_impl(keys, nkeys, values, nchunks, agg, max_groups, out_keys, out_values, out_counts, 0);
}

rdf_status rdf_groupby_sum(const rdf_array* keys, const rdf_array* values, int64_t nchunks, int64_t max_groups,
                           rdf_out* out_keys, rdf_out* out_sums, rdf_out* out_counts) {
    if ((g_ctx.opt_gb_partition == 1 || g_ctx.opt_gb_debug == 3) && keys && nchunks >= 1) {   // A/B, tests: the first-generation fallback where its range holds
        int64_t nrows = 0;
        for (int64_t c = 0; c < nchunks; ++c) nrows += keys[c].length;
        if (gb_fallback_in_range(max_groups, nrows)) return groupby_sum_fallback(keys, values, nchunks, max_groups, out_keys, out_sums, out_counts, 0);
    }
    return rdf_groupby_agg(keys, 1, values, nchunks, values ? RDF_AGG_SUM : RDF_AGG_COUNT, max_groups, out_keys, out_sums, out_counts);
}

rdf_status rdf_groupby_merge(const rdf_array* keys, const rdf_array* partial, const rdf_array* counts, int32_t agg, int64_t max_groups,
                             rdf_out* out_keys, rdf_out* out_values, rdf_out* out_counts) {
    if (!keys || !counts || !out_keys || !out_values || !out_counts) return fail(RDF_INVALID_ARGUMENT, "groupby_merge: null argument");
    if (agg < RDF_AGG_SUM || agg > RDF_AGG_COUNT) return fail(RDF_INVALID_ARGUMENT, "groupby_merge: unknown aggregate %d", agg);
    if (max_groups < 1) return fail(RDF_INVALID_ARGUMENT, "groupby_merge: max_groups must be positive");
    const int op = agg == RDF_AGG_MIN ? AGG_MIN : agg == RDF_AGG_MAX ? AGG_MAX : AGG_SUM;
    int32_t mem = -1;
    RDF_TRY(check_mem(keys, 1, &mem));
    if (partial) RDF_TRY(check_mem(partial, 1, &mem));
    RDF_TRY(check_mem(counts, 1, &mem));
    RDF_TRY(check_out_mem(out_keys, 1, mem)); RDF_TRY(check_out_mem(out_values, 1, mem)); RDF_TRY(check_out_mem(out_counts, 1, mem));
    const int kdt = keys->dtype;
    if (kdt != RDF_I64 && kdt != RDF_U64) return fail(RDF_INVALID_ARGUMENT, "groupby_merge: Int64 / UInt64 keys (cast narrower keys first)");
    const int vdt = partial ? partial->dtype : RDF_I64;
    if (partial && vdt != RDF_F64 && vdt != RDF_I64 && vdt != RDF_U64) return fail(RDF_INVALID_ARGUMENT, "groupby_merge: partial aggregates are Float64 / Int64 / UInt64");
    if (counts->dtype != RDF_I64) return fail(RDF_INVALID_ARGUMENT, "groupby_merge: counts are Int64");
    const int64_t n = keys->length;
    if ((partial && partial->length != n) || counts->length != n) return fail(RDF_COMPUTE_ERROR, "groupby_merge: arrays differ in length");
    if (out_keys->dtype != kdt || out_values->dtype != vdt || out_counts->dtype != RDF_I64) return fail(RDF_INVALID_ARGUMENT, "groupby_merge: outputs must be (key dtype, partial dtype, Int64)");
    if (keys->validity && !out_keys->validity) return fail(RDF_INVALID_ARGUMENT, "output validity buffer required");
    const int64_t cap_needed = std::min<int64_t>(max_groups + 2, n + 2);
    if (out_keys->capacity < cap_needed || out_values->capacity < cap_needed || out_counts->capacity < cap_needed) return fail(RDF_MEMORY_ERROR, "output capacity too small (need max_groups + 2)");
    if (n == 0) { out_keys->length = out_values->length = out_counts->length = 0; out_keys->null_count = out_values->null_count = out_counts->null_count = 0; return RDF_OK; }
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();
    size_t pin_off = 0, used = 0;
    InputStager st;
    st.add(keys); st.add(counts);
    if (partial) st.add(partial);
    RDF_TRY(st.finish(pin_off, &used));
    pin_off += (used + 255) & ~(size_t)255;
    const int vcls = value_class(vdt);
    GbScratch sc;
    RDF_TRY(gb_scratch_init(sc, op));
    GbDense d;
    RDF_TRY(gb_dense_alloc(d, std::min<int64_t>(max_groups, n) + 4, 8));
    // partial values -> table form (a partial with count 0 or a NULL contributes the identity)
    void* pacc = nullptr;
    if (partial) {
        RDF_TRY(arena_alloc((size_t)n * 8 + 64, &pacc));
        HIP_TRY(hipMemcpyAsync(pacc, (const char*)st.dev[2].values + st.dev[2].offset * 8, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx.stream));
        if (op != AGG_SUM) {
            Gb2FinishArgs fa;
            memset(&fa, 0, sizeof fa);
            fa.acc = (uint64_t*)pacc; fa.counts = (const int64_t*)st.dev[1].values + st.dev[1].offset; fa.n = n; fa.op = op; fa.vcls = vcls; fa.native_in = 1;
            HIP_TRY(launch_gb2_finish(fa, ctx.stream));
        }
    }
    Gb2MergeArgs ma;
    memset(&ma, 0, sizeof ma);
    unsigned int* tcursor = nullptr;
    RDF_TRY(gb_table_alloc(ma.t, &tcursor, max_groups, op));
    ma.keys = (const uint64_t*)st.dev[0].values + st.dev[0].offset;
    ma.acc = (const uint64_t*)pacc;
    ma.counts = (const int64_t*)st.dev[1].values + st.dev[1].offset;
    const void* kvalid_dev = st.dev[0].validity;
    if (kvalid_dev && (st.dev[0].offset & 7)) return fail(RDF_INVALID_ARGUMENT, "groupby_merge: a key bitmap offset must be a multiple of 8");
    ma.key_validity = kvalid_dev ? st.dev[0].validity + (st.dev[0].offset >> 3) : nullptr;
    ma.n = n; ma.op = op; ma.vcls = vcls;
    {
        KernelTimer kt;
        HIP_TRY(launch_gb2_merge(ma, ctx.stream));
        kt.stop();
    }
    RDF_TRY(pinned_reserve(pin_off + 64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, ma.t.special, 32, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    unsigned int tpin[8];
    memcpy(tpin, ctx.pinned + pin_off, 32);
    if ((tpin[4] & 4u) || (int64_t)tpin[2] > max_groups) return fail(RDF_MEMORY_ERROR, "groupby: more than max_groups (%lld) distinct keys", (long long)max_groups);
    GroupEmitArgs ea;
    memset(&ea, 0, sizeof ea);
    ea.t = ma.t; ea.out_keys = d.keys; ea.out_keys_validity = d.kvalid; ea.out_sums = d.acc; ea.out_counts = d.counts; ea.cursor = tcursor; ea.key_dtype = kdt;
    HIP_TRY(launch_gb2_emit(ea, ctx.stream));
    uint32_t flags = 0;
    RDF_TRY(gb_collect(sc, d, 8, max_groups, -1, false, tcursor, ma.t.flags, pin_off, &flags));
    RDF_TRY(gb_finish_values(sc, d, op, vcls, pin_off));
    const int64_t ng = d.ng;
    if (ng > cap_needed) return fail(RDF_MEMORY_ERROR, "groupby: more than max_groups (%lld) distinct keys", (long long)max_groups);
    RDF_TRY(gb_copy_out(d.keys, (size_t)ng * 8, out_keys->values, mem));
    if (out_keys->validity) RDF_TRY(gb_copy_out(d.kvalid, (size_t)((ng + 7) / 8), out_keys->validity, mem));
    RDF_TRY(gb_copy_out(d.acc, (size_t)ng * 8, out_values->values, mem));
    RDF_TRY(gb_copy_out(d.counts, (size_t)ng * 8, out_counts->values, mem));
    if (op != AGG_SUM && out_values->validity) RDF_TRY(gb_copy_out(d.vvalid, (size_t)((ng + 7) / 8), out_values->validity, mem));
    else RDF_TRY(gb_fill_valid(out_values, ng, mem));
    RDF_TRY(gb_fill_valid(out_counts, ng, mem));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    out_keys->length = out_values->length = out_counts->length = ng;
    out_keys->null_count = tpin[1] ? 1 : 0;
    out_values->null_count = op != AGG_SUM ? d.value_nulls : 0;
    out_counts->null_count = 0;
    return RDF_OK;
}

static rdf_status exchange_pack(const char* who, const rdf_array* keys, const rdf_array* partial, const rdf_array* counts, int32_t world,
                                void* packed_dev, int64_t* owner_counts) {
    if (!keys || !partial || !packed_dev || !owner_counts) return fail(RDF_INVALID_ARGUMENT, "%s: null argument", who);
    if (world < 1 || world > 64) return fail(RDF_INVALID_ARGUMENT, "%s: 1..64 ranks", who);
    if (keys->mem != RDF_MEM_DEVICE || partial->mem != RDF_MEM_DEVICE || (counts && counts->mem != RDF_MEM_DEVICE)) return fail(RDF_INVALID_ARGUMENT, "%s: device-resident arrays only", who);
    if (dtype_size(keys->dtype) != 8 || dtype_size(partial->dtype) != 8 || (counts && counts->dtype != RDF_I64)) return fail(RDF_INVALID_ARGUMENT, "%s: 8-byte keys and values, Int64 counts", who);
    if (keys->validity || (!counts && partial->validity)) return fail(RDF_INVALID_ARGUMENT, "%s: NULLs are not exchanged", who);
    const int64_t n = keys->length;
    if (partial->length != n || (counts && counts->length != n)) return fail(RDF_COMPUTE_ERROR, "%s: arrays differ in length", who);
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();
    void* pc = nullptr;
    RDF_TRY(arena_alloc(2 * 64 * 8, &pc));
    HIP_TRY(hipMemsetAsync(pc, 0, 2 * 64 * 8, ctx.stream));
    GxPackArgs a;
    memset(&a, 0, sizeof a);
    a.keys = (const uint64_t*)keys->values + keys->offset;
    a.acc = (const uint64_t*)partial->values + partial->offset;
    a.counts = counts ? (const int64_t*)counts->values + counts->offset : nullptr;
    a.words = counts ? 3 : 2;
    a.n = n; a.world = world;
    a.owner_counts = (unsigned long long*)pc;
    a.cursors = a.owner_counts + 64;
    a.packed = (uint64_t*)packed_dev;
    a.phase = 0;
    HIP_TRY(launch_gx_pack(a, ctx.stream));
    RDF_TRY(pinned_reserve(1024));
    HIP_TRY(hipMemcpyAsync(ctx.pinned, a.owner_counts, (size_t)world * 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    unsigned long long oc[64], cur[64], run = 0;
    memcpy(oc, ctx.pinned, (size_t)world * 8);
    for (int r = 0; r < world; ++r) { owner_counts[r] = (int64_t)oc[r]; cur[r] = run; run += oc[r]; }
    memcpy(ctx.pinned + 512, cur, (size_t)world * 8);
    HIP_TRY(hipMemcpyAsync(a.cursors, ctx.pinned + 512, (size_t)world * 8, hipMemcpyHostToDevice, ctx.stream));
    a.phase = 1;
    HIP_TRY(launch_gx_pack(a, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    return RDF_OK;
}

rdf_status rdf_group_exchange_pack(const rdf_array* keys, const rdf_array* partial, const rdf_array* counts, int32_t world,
                                   void* packed_dev, int64_t* owner_counts) {
    if (!counts) return fail(RDF_INVALID_ARGUMENT, "group_exchange_pack: null argument");
    return exchange_pack("group_exchange_pack", keys, partial, counts, world, packed_dev, owner_counts);
}
// the row-shuffle fallback (SURVEY.md 8e): when local pre-aggregation cannot shrink the data (about as many groups as rows) the
// ROWS themselves travel, 16 bytes each, and every rank runs a plain rdf_groupby_agg over what it receives
rdf_status rdf_row_exchange_pack(const rdf_array* keys, const rdf_array* values, int32_t world, void* packed_dev, int64_t* owner_counts) {
    return exchange_pack("row_exchange_pack", keys, values, nullptr, world, packed_dev, owner_counts);
}
rdf_status rdf_row_exchange_unpack(const void* packed_dev, int64_t n, rdf_out* keys, rdf_out* values) {
    if (!keys || !values || (n > 0 && !packed_dev)) return fail(RDF_INVALID_ARGUMENT, "row_exchange_unpack: null argument");
    if (keys->mem != RDF_MEM_DEVICE || values->mem != RDF_MEM_DEVICE) return fail(RDF_INVALID_ARGUMENT, "row_exchange_unpack: device-resident outputs only");
    if (dtype_size(keys->dtype) != 8 || dtype_size(values->dtype) != 8) return fail(RDF_INVALID_ARGUMENT, "row_exchange_unpack: 8-byte keys and values");
    if (keys->capacity < n || values->capacity < n) return fail(RDF_MEMORY_ERROR, "output capacity too small");
    RDF_TRY(ensure_ready());
    HIP_TRY(launch_gx_unpack((const uint64_t*)packed_dev, n, (uint64_t*)keys->values, (uint64_t*)values->values, nullptr, 2, g_ctx.stream));
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    keys->length = values->length = n;
    keys->null_count = values->null_count = 0;
    return RDF_OK;
}

rdf_status rdf_group_exchange_unpack(const void* packed_dev, int64_t n, rdf_out* keys, rdf_out* partial, rdf_out* counts) {
    if (!keys || !partial || !counts || (n > 0 && !packed_dev)) return fail(RDF_INVALID_ARGUMENT, "group_exchange_unpack: null argument");
    if (keys->mem != RDF_MEM_DEVICE || partial->mem != RDF_MEM_DEVICE || counts->mem != RDF_MEM_DEVICE) return fail(RDF_INVALID_ARGUMENT, "group_exchange_unpack: device-resident outputs only");
    if (dtype_size(keys->dtype) != 8 || dtype_size(partial->dtype) != 8 || counts->dtype != RDF_I64) return fail(RDF_INVALID_ARGUMENT, "group_exchange_unpack: 8-byte keys and partials, Int64 counts");
    if (keys->capacity < n || partial->capacity < n || counts->capacity < n) return fail(RDF_MEMORY_ERROR, "output capacity too small");
    RDF_TRY(ensure_ready());
    HIP_TRY(launch_gx_unpack((const uint64_t*)packed_dev, n, (uint64_t*)keys->values, (uint64_t*)partial->values, (int64_t*)counts->values, 3, g_ctx.stream));
    HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    keys->length = partial->length = counts->length = n;
    keys->null_count = partial->null_count = counts->null_count = 0;
    return RDF_OK;
}

}  // extern "C"
