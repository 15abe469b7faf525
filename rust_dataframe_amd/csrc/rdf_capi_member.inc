// rdf_capi_member.inc — host side of rdf_member_mask (LEFT SEMI / LEFT ANTI / x IN (...)) and rdf_first_occurrence
// (drop_duplicates); kernels: rdf_member.hip, table size and route: rdf_member_plan.h.  Textually included by rdf_capi.cpp
// after rdf_capi_dict.inc (it uses that file's dict_check_chunks, DictCodes and dict_encode_device, and rdf_capi.cpp's
// per-thread context, arena and staging helpers).
//
//   rdf_member_mask / rdf_first_occurrence   member_check (every refusal, the lengths, the plan: no device work), then
//                                            member_encode (Utf8 keys -> UInt32 codes) and member_run
//   member_run                               the driver over the steps below, one MemberState on the caller's stack:
//     member_stage                             inputs, chunk and tile tables, output descriptors in HBM
//     member_table                             the table, its flags, the counters
//     member_keys                              2..4 key columns: words, NULL bits and hashes of a side (member_prep_kernel)
//     member_build / member_fold               the build side into the table / every row folded into its key's slot;
//                                              then the wait that tells whether the table held the keys
//     member_probe / member_first              the mask words and the per-block counts
//     member_deliver                           the count, the NULL counts, host outputs copied back

namespace {

struct MemberState {
    // the call (member_check)
    const char* fn;
    bool first;                         // rdf_first_occurrence: one side (probe), no build side
    int nkeys, kdt[4];
    int32_t mem, kind;
    int64_t pnc, bnc, np, nb;
    std::vector<int64_t> prs, brs;      // first row of every chunk, per side
    rdf_out* out;                       // pnc outputs, or nullptr (count only)
    int64_t* out_rows;
    MemberPlan plan;
    // the numeric call (member_encode): key k's chunks at [k * nchunks + c]
    std::vector<rdf_array> pflat, bflat;
    std::string enc_kernels;
    // one run
    size_t pin_off;
    Region outr;
    std::vector<int> oi;
    MemberArgs a;
    int grid;
    unsigned long long* d_count;        // [0] TRUE rows, [1] fold atomics saved
    unsigned long long saved;           // rdf_first_occurrence: rows whose atomic the load-and-compare of the fold saved
};

int64_t member_key_rows(const rdf_sort_key& k, int64_t c) { return k.values ? k.values[c].length : utf8_rows(k.utf8[c]); }

// one side's keys: exactly one of values / utf8 per key, numeric or Boolean chunks of one dtype, one memory kind
rdf_status member_check_side(const char* fn, const char* side, const rdf_sort_key* keys, int nkeys, int64_t nchunks, int32_t* mem) {
    for (int k = 0; k < nkeys; ++k) {
        const rdf_sort_key& key = keys[k];
        if ((key.values != nullptr) == (key.utf8 != nullptr)) return fail(RDF_INVALID_ARGUMENT, "%s: %s key %d must set exactly one of values / utf8", fn, side, k);
        if (key.values) {
            RDF_TRY(check_mem(key.values, nchunks, mem));
            for (int64_t c = 0; c < nchunks; ++c) {
                const int dt = key.values[c].dtype;
                if (!(is_numeric(dt) || dt == RDF_BOOL) || dt != key.values[0].dtype)
                    return fail(RDF_INVALID_ARGUMENT, "%s: %s key %d: numeric or Boolean chunks of one dtype", fn, side, k);
            }
        } else {
            int64_t rows = 0;
            RDF_TRY(dict_check_chunks(fn, key.utf8, nchunks, mem, &rows));
        }
    }
    return RDF_OK;
}
rdf_status member_row_starts(const char* fn, const rdf_sort_key* keys, int nkeys, int64_t nchunks, std::vector<int64_t>& rs) {
    rs.assign((size_t)nchunks + 1, 0);
    for (int64_t c = 0; c < nchunks; ++c) rs[(size_t)c + 1] = rs[(size_t)c] + member_key_rows(keys[0], c);
    for (int k = 1; k < nkeys; ++k)
        for (int64_t c = 0; c < nchunks; ++c)
            if (member_key_rows(keys[k], c) != rs[(size_t)c + 1] - rs[(size_t)c])
                return fail(RDF_COMPUTE_ERROR, "%s: key columns of one side differ in their chunks' rows", fn);
    return RDF_OK;
}

// Everything that can be refused without the device, in the order the header lists; sets *out_rows = 0 and, once the rows
// are known, every output's length.
rdf_status member_check(MemberState& m, const rdf_sort_key* pkeys, int64_t pnc, const rdf_sort_key* bkeys, int64_t bnc, int32_t nkeys, int32_t kind,
                        rdf_out* out, int64_t* out_rows) {
    const char* fn = m.fn;
    if (!pkeys || pnc < 1 || !out_rows || (!m.first && (!bkeys || bnc < 1))) return fail(RDF_INVALID_ARGUMENT, "%s: bad arguments", fn);
    *out_rows = 0;
    if (nkeys < 1 || nkeys > RDF_MEMBER_MAX_KEYS) return fail(RDF_INVALID_ARGUMENT, "%s: 1 to %d key columns", fn, RDF_MEMBER_MAX_KEYS);
    if (m.first) { if (kind < RDF_KEEP_FIRST || kind > RDF_KEEP_NONE) return fail(RDF_INVALID_ARGUMENT, "%s: bad keep %d", fn, kind); }
    else {
        if (kind < RDF_MEMBER_SEMI || kind > RDF_MEMBER_IS_IN) return fail(RDF_INVALID_ARGUMENT, "%s: bad kind %d", fn, kind);
        if (kind == RDF_MEMBER_IS_IN && nkeys != 1) return fail(RDF_INVALID_ARGUMENT, "%s: IS_IN takes one key column", fn);
    }
    m.nkeys = nkeys; m.kind = kind; m.pnc = pnc; m.bnc = m.first ? 0 : bnc; m.out = out; m.out_rows = out_rows;
    m.mem = -1;
    RDF_TRY(member_check_side(fn, m.first ? "" : "left", pkeys, nkeys, pnc, &m.mem));
    if (!m.first) RDF_TRY(member_check_side(fn, "right", bkeys, nkeys, bnc, &m.mem));
    for (int k = 0; k < 4; ++k) m.kdt[k] = 0;
    for (int k = 0; k < nkeys; ++k) {
        m.kdt[k] = pkeys[k].values ? pkeys[k].values[0].dtype : RDF_U32;
        if (m.first) continue;
        if ((pkeys[k].utf8 != nullptr) != (bkeys[k].utf8 != nullptr)) return fail(RDF_INVALID_ARGUMENT, "%s: pair %d: a Utf8 key pairs with a Utf8 key only", fn, k);
        if (pkeys[k].values && pkeys[k].values[0].dtype != bkeys[k].values[0].dtype)
            return fail(RDF_INVALID_ARGUMENT, "%s: pair %d: key columns must share one dtype (cast first)", fn, k);
    }
    RDF_TRY(member_row_starts(fn, pkeys, nkeys, pnc, m.prs));
    if (!m.first) RDF_TRY(member_row_starts(fn, bkeys, nkeys, bnc, m.brs)); else m.brs.assign(1, 0);
    m.np = m.prs[(size_t)pnc]; m.nb = m.brs.back();
    if (m.np + m.nb >= (int64_t)1 << 32) return fail(RDF_INVALID_ARGUMENT, "%s: at most 2^32-1 rows in all", fn);
    if (out) {
        RDF_TRY(check_out_mem(out, pnc, m.mem));
        for (int64_t c = 0; c < pnc; ++c) {
            if (out[c].dtype != RDF_BOOL) return fail(RDF_INVALID_ARGUMENT, "%s: the mask is Boolean", fn);
            if (out[c].capacity < 0 || (out[c].capacity > 0 && !out[c].values)) return fail(RDF_INVALID_ARGUMENT, "%s: mask %lld: capacity without a buffer", fn, (long long)c);
            if (m.mem == RDF_MEM_DEVICE && ((((uintptr_t)out[c].values) | ((uintptr_t)out[c].validity)) & 7)) return fail(RDF_INVALID_ARGUMENT, "%s: mask %lld: device bitmaps start on an 8-byte boundary", fn, (long long)c);
            if (!m.first && kind == RDF_MEMBER_IS_IN && !out[c].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output validity buffer required", fn);
        }
    }
    const int route = m.first ? MEMBER_ROUTE_HBM : g_ctx.opt_member_route;
    m.plan = member_plan(m.first ? m.np : m.nb, nkeys == 1, g_ctx.opt_member_table_bits, g_ctx.opt_member_slots, route);
    if (!m.plan.ok) return fail(RDF_INVALID_ARGUMENT, "%s: the LDS route takes one key column and at most %lld build rows", fn, (long long)m.plan.lds_capacity);
    if (out) {
        bool fits = true;
        for (int64_t c = 0; c < pnc; ++c) {
            out[c].length = m.prs[(size_t)c + 1] - m.prs[(size_t)c];
            out[c].null_count = 0;
            fits &= out[c].capacity >= out[c].length;
        }
        if (!fits) return fail(RDF_MEMORY_ERROR, "%s: a mask output is shorter than its chunk", fn);
    }
    return RDF_OK;
}

// numeric keys as they are; a Utf8 key as the UInt32 codes of one dictionary (member: left chunks then right chunks)
rdf_status member_encode(MemberState& m, const rdf_sort_key* pkeys, const rdf_sort_key* bkeys, DictCodes (&codes)[4]) {
    m.pflat.resize((size_t)m.nkeys * (size_t)m.pnc);
    m.bflat.resize((size_t)m.nkeys * (size_t)m.bnc);
    for (int k = 0; k < m.nkeys; ++k) {
        if (pkeys[k].values) {
            for (int64_t c = 0; c < m.pnc; ++c) m.pflat[(size_t)k * m.pnc + c] = pkeys[k].values[c];
            for (int64_t c = 0; c < m.bnc; ++c) m.bflat[(size_t)k * m.bnc + c] = bkeys[k].values[c];
            continue;
        }
        std::vector<rdf_utf8_array> both(pkeys[k].utf8, pkeys[k].utf8 + m.pnc);
        if (!m.first) both.insert(both.end(), bkeys[k].utf8, bkeys[k].utf8 + m.bnc);
        const int64_t nboth = m.pnc + m.bnc;
        RDF_TRY(codes[k].make(both.data(), nboth, m.mem));
        int64_t count = 0;
        if (m.np + m.nb > 0) {
            RDF_TRY(dict_encode_device(m.fn, both.data(), nboth, m.np + m.nb, m.mem, codes[k].outs.data(), nullptr, nullptr, &count));
            m.enc_kernels = g_ctx.last_kernel + " + ";
        }
        const bool pnull = utf8_nullable(both.data(), m.pnc), bnull = !m.first && utf8_nullable(both.data() + m.pnc, m.bnc);
        for (int64_t c = 0; c < nboth; ++c) {
            const rdf_out& o = codes[k].outs[(size_t)c];
            const bool nl = c < m.pnc ? pnull : bnull;
            const rdf_array arr{o.values, nl ? o.validity : nullptr, 0, utf8_rows(both[(size_t)c]), nl ? o.null_count : 0, RDF_U32, m.mem};
            if (c < m.pnc) m.pflat[(size_t)k * m.pnc + c] = arr;
            else m.bflat[(size_t)k * m.bnc + (c - m.pnc)] = arr;
        }
    }
    return RDF_OK;
}

rdf_status member_stage(MemberState& m) {
    m.pin_off = 0;
    size_t used = 0;
    InputStager in;   // staged order: probe key 0 chunks, probe key 1 chunks, ..., then the build side the same way
    for (auto& x : m.pflat) in.add(&x);
    for (auto& x : m.bflat) in.add(&x);
    RDF_TRY(in.finish(m.pin_off, &used));
    m.pin_off += (used + 255) & ~(size_t)255;
    m.oi.assign((size_t)m.pnc * 2, -1);
    if (m.out && m.mem == RDF_MEM_HOST) {   // (an item is padded by 16 bytes: the last 64-bit word fits)
        for (int64_t c = 0; c < m.pnc; ++c) {
            const int64_t len = m.out[c].length;
            if (len == 0) continue;
            m.oi[2 * c] = m.outr.add(m.out[c].values, (size_t)((len + 7) / 8));
            if (m.out[c].validity) m.oi[2 * c + 1] = m.outr.add(m.out[c].validity, (size_t)((len + 7) / 8));
        }
        RDF_TRY(m.outr.layout());
    }
    const size_t np_ch = (size_t)m.nkeys * (size_t)m.pnc, nb_ch = (size_t)m.nkeys * (size_t)m.bnc;
    TableBuilder tb;
    const size_t o_ch = tb.reserve(sizeof(DevChunkCol) * (np_ch + nb_ch));
    const size_t o_prs = tb.reserve(sizeof(int64_t) * ((size_t)m.pnc + 1)), o_pts = tb.reserve(sizeof(int64_t) * ((size_t)m.pnc + 1));
    const size_t o_brs = tb.reserve(sizeof(int64_t) * ((size_t)m.bnc + 1)), o_bts = tb.reserve(sizeof(int64_t) * ((size_t)m.bnc + 1));
    const size_t o_out = tb.reserve(sizeof(DtOut) * (size_t)m.pnc);
    RDF_TRY(tb.bind(m.pin_off));
    memcpy(tb.at<char>(o_ch), in.dev.data(), sizeof(DevChunkCol) * in.dev.size());
    int64_t *hprs = tb.at<int64_t>(o_prs), *hpts = tb.at<int64_t>(o_pts), *hbrs = tb.at<int64_t>(o_brs), *hbts = tb.at<int64_t>(o_bts);
    hpts[0] = hbts[0] = 0;
    for (int64_t c = 0; c <= m.pnc; ++c) hprs[c] = m.prs[(size_t)c];
    for (int64_t c = 0; c <= m.bnc; ++c) hbrs[c] = m.brs[(size_t)c];
    for (int64_t c = 0; c < m.pnc; ++c) hpts[c + 1] = hpts[c] + (hprs[c + 1] - hprs[c] + kCsTile - 1) / kCsTile;
    for (int64_t c = 0; c < m.bnc; ++c) hbts[c + 1] = hbts[c] + (hbrs[c + 1] - hbrs[c] + kCsTile - 1) / kCsTile;
    DtOut* hout = tb.at<DtOut>(o_out);
    for (int64_t c = 0; c < m.pnc; ++c) {
        hout[c].values = nullptr; hout[c].validity = nullptr;
        if (!m.out) continue;
        if (m.mem == RDF_MEM_HOST) {
            if (m.oi[2 * c] >= 0) hout[c].values = m.outr.ptr(m.oi[2 * c]);
            if (m.oi[2 * c + 1] >= 0) hout[c].validity = (uint8_t*)m.outr.ptr(m.oi[2 * c + 1]);
        } else { hout[c].values = m.out[c].values; hout[c].validity = m.out[c].validity; }
    }
    MemberArgs& a = m.a;
    memset(&a, 0, sizeof a);
    a.probe.col.nchunks = m.pnc; a.probe.col.n = m.np; a.probe.col.ntiles = hpts[m.pnc];
    a.build.col.nchunks = m.bnc; a.build.col.n = m.nb; a.build.col.ntiles = hbts[m.bnc];
    RDF_TRY(tb.alloc());
    RDF_TRY(tb.upload(m.pin_off));
    m.pin_off += (tb.size + 255) & ~(size_t)255;
    a.probe.col.chunks = tb.dev_at<DevChunkCol>(o_ch);
    a.build.col.chunks = tb.dev_at<DevChunkCol>(o_ch) + np_ch;
    a.probe.col.row_start = tb.dev_at<int64_t>(o_prs); a.probe.col.tile_start = tb.dev_at<int64_t>(o_pts);
    a.build.col.row_start = tb.dev_at<int64_t>(o_brs); a.build.col.tile_start = tb.dev_at<int64_t>(o_bts);
    a.outs = m.out ? tb.dev_at<DtOut>(o_out) : nullptr;
    a.probe.nkeys = a.build.nkeys = m.nkeys;
    for (int k = 0; k < 4; ++k) a.probe.dtype[k] = a.build.dtype[k] = m.kdt[k];
    a.kind = m.kind;
    return RDF_OK;
}

rdf_status member_table(MemberState& m) {
    Ctx& ctx = g_ctx;
    MemberArgs& a = m.a;
    const size_t slots = (size_t)m.plan.slots, entries = slots + 2;
    a.t.mask = m.plan.slots - 1;
    a.t.tshift = m.plan.tshift;
    void* p;
    if (m.nkeys == 1) {
        RDF_TRY(arena_alloc(slots * 8, &p));
        a.t.keys = (uint64_t*)p;
        HIP_TRY(launch_cs_fill64(a.t.keys, (int64_t)slots, kMemberEmpty, ctx.stream));
    }
    if (m.nkeys > 1 || m.first) {
        RDF_TRY(arena_alloc(entries * 4, &p));
        a.t.lo = (uint32_t*)p;
        HIP_TRY(hipMemsetAsync(p, 0xFF, entries * 4, ctx.stream));
    }
    if (m.first) {
        RDF_TRY(arena_alloc(entries * 4, &p));
        a.t.hi = (uint32_t*)p;
        HIP_TRY(hipMemsetAsync(p, 0, entries * 4, ctx.stream));
    }
    const bool lds = m.plan.route == MEMBER_ROUTE_LDS;
    m.grid = member_grid(a.probe.col.ntiles, lds);
    const size_t words = (size_t)MEMBER_F_WORDS * 4 + 16 + (size_t)m.grid * 8 + (size_t)m.pnc * 8;
    RDF_TRY(arena_alloc(words, &p));
    HIP_TRY(hipMemsetAsync(p, 0, words, ctx.stream));
    a.t.flags = (unsigned int*)p;
    m.d_count = (unsigned long long*)((char*)p + MEMBER_F_WORDS * 4);
    a.partial = m.d_count + 2;
    a.chunk_nulls = a.partial + m.grid;
    a.skipped = m.first ? m.d_count + 1 : nullptr;
    return RDF_OK;
}

// 2..4 key columns: the columns' words, the NULL bits and the tuple's hash of every row of a side
rdf_status member_keys(MemberState& m, MemberSide& s, int64_t n) {
    if (m.nkeys == 1 || n == 0) return RDF_OK;
    void* p;
    RDF_TRY(arena_alloc((size_t)n * 8, &p));
    s.hash = (uint64_t*)p;
    for (int k = 0; k < m.nkeys; ++k) { RDF_TRY(arena_alloc((size_t)n * 8, &p)); s.bits[k] = (uint64_t*)p; }
    RDF_TRY(arena_alloc((size_t)n, &p));
    s.nullbits = (uint8_t*)p;
    HIP_TRY(launch_member_prep(s, m.first ? 1 : 0, g_ctx.stream));
    return RDF_OK;
}

// the wait between the table and its readers: a table that could not hold the keys answers nothing
rdf_status member_table_held(MemberState& m) {
    Ctx& ctx = g_ctx;
    RDF_TRY(pinned_reserve(m.pin_off + 256));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + m.pin_off, m.a.t.flags, MEMBER_F_WORDS * 4, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    unsigned int fl[MEMBER_F_WORDS];
    memcpy(fl, ctx.pinned + m.pin_off, sizeof fl);
    if (fl[MEMBER_F_OVERFLOW]) return fail(RDF_MEMORY_ERROR, "%s: the table of %llu slots (\"member_table_bits\") does not hold the keys", m.fn, (unsigned long long)m.plan.slots);
    return RDF_OK;
}

rdf_status member_build(MemberState& m) {
    HIP_TRY(launch_member_build(m.a, g_ctx.stream));
    return member_table_held(m);
}
rdf_status member_fold(MemberState& m) {
    if (m.kind != RDF_KEEP_LAST) { m.a.descending = 0; HIP_TRY(launch_member_fold(m.a, g_ctx.stream)); }
    if (m.kind != RDF_KEEP_FIRST) { m.a.descending = 1; HIP_TRY(launch_member_fold(m.a, g_ctx.stream)); }
    return member_table_held(m);
}
rdf_status member_probe(MemberState& m) {
    Ctx& ctx = g_ctx;
    if (m.first) HIP_TRY(launch_member_first(m.a, m.grid, ctx.stream));
    else HIP_TRY(launch_member_probe(m.a, m.grid, (size_t)m.plan.lds_bytes, ctx.stream));
    HIP_TRY(launch_member_total(m.a.partial, m.grid, m.d_count, ctx.stream));
    return RDF_OK;
}

rdf_status member_deliver(MemberState& m) {
    Ctx& ctx = g_ctx;
    const size_t nb = 16 + (size_t)m.grid * 8 + (size_t)m.pnc * 8;
    RDF_TRY(pinned_reserve(m.pin_off + nb + 64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + m.pin_off, m.d_count, nb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    unsigned long long head[2];
    memcpy(head, ctx.pinned + m.pin_off, 16);
    *m.out_rows = (int64_t)head[0];
    m.saved = head[1];
    if (!m.out) return RDF_OK;
    std::vector<unsigned long long> nulls((size_t)m.pnc);
    memcpy(nulls.data(), ctx.pinned + m.pin_off + 16 + (size_t)m.grid * 8, (size_t)m.pnc * 8);
    if (m.mem == RDF_MEM_HOST) {
        const size_t off = m.pin_off + ((nb + 255) & ~(size_t)255);
        RDF_TRY(pinned_reserve(off + m.outr.small_bytes));
        RDF_TRY(m.outr.download(off));
    }
    for (int64_t c = 0; c < m.pnc; ++c) m.out[c].null_count = (int64_t)nulls[(size_t)c];
    return RDF_OK;
}

rdf_status member_run(MemberState& m) {
    Ctx& ctx = g_ctx;
    arena_begin();
    RDF_TRY(member_stage(m));
    RDF_TRY(member_table(m));
    KernelTimer kt;
    RDF_TRY(member_keys(m, m.a.probe, m.np));
    if (m.first) RDF_TRY(member_fold(m));
    else {
        RDF_TRY(member_keys(m, m.a.build, m.nb));
        RDF_TRY(member_build(m));
    }
    RDF_TRY(member_probe(m));
    kt.stop();
    RDF_TRY(member_deliver(m));
    std::string k = m.enc_kernels;
    if (m.nkeys > 1) k += "member_prep_kernel + ";
    if (m.first) {
        const unsigned long long folds = (unsigned long long)m.np * (m.kind == RDF_KEEP_NONE ? 2 : 1);
        k += "member_fold_kernel + member_first_kernel (" + std::to_string(m.saved) + " of " + std::to_string(folds) + " folds without an atomic)";
    }
    else k += m.plan.route == MEMBER_ROUTE_LDS ? "member_build_kernel + member_probe_kernel<lds>" : "member_build_kernel + member_probe_kernel<hbm>";
    ctx.last_kernel = k;
    return RDF_OK;
}

rdf_status member_call(MemberState& m, const rdf_sort_key* pkeys, int64_t pnc, const rdf_sort_key* bkeys, int64_t bnc, int32_t nkeys, int32_t kind,
                       rdf_out* out, int64_t* out_rows) {
    RDF_TRY(member_check(m, pkeys, pnc, bkeys, bnc, nkeys, kind, out, out_rows));
    if (m.np == 0) return RDF_OK;      // (no rows, no bits: every length is 0 already)
    RDF_TRY(ensure_ready());
    DictCodes codes[4];
    RDF_TRY(member_encode(m, pkeys, bkeys, codes));
    return member_run(m);
}

}  // namespace

extern "C" {

rdf_status rdf_member_mask(const rdf_sort_key* left_keys, int64_t left_nchunks, const rdf_sort_key* right_keys, int64_t right_nchunks,
                           int32_t nkeys, int32_t kind, rdf_out* out_mask, int64_t* out_rows) {
    MemberState m;
    m.fn = "member_mask";
    m.first = false;
    return member_call(m, left_keys, left_nchunks, right_keys, right_nchunks, nkeys, kind, out_mask, out_rows);
}

rdf_status rdf_first_occurrence(const rdf_sort_key* keys, int32_t nkeys, int64_t nchunks, int32_t keep, rdf_out* out_mask, int64_t* out_rows) {
    MemberState m;
    m.fn = "first_occurrence";
    m.first = true;
    return member_call(m, keys, nchunks, nullptr, 0, nkeys, keep, out_mask, out_rows);
}

}  // extern "C"
