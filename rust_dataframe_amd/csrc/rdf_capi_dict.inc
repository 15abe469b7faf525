// rdf_capi_dict.inc — text keys: rdf_utf8_dictionary_encode (kernels: the cs_dict_* passes of rdf_colstats.hip, next to the
// passes of rdf_utf8_uniques they share) and the two entry points that are host-side compositions over it; textually
// included by rdf_capi.cpp after rdf_capi_sort_utf8.inc and rdf_capi_colstats.inc (it uses their staging and checks).
//
//   rdf_utf8_dictionary_encode   hash route: hash -> (hash, smallest row) table -> one pass that verifies every row against
//                                its hash's representative and keeps it (rep[], flags[]); exact route (table full, a
//                                mismatch, or "uniques_route" 1): rdf_lexsort_to_indices' stable order, run starts flagged
//                                and scanned, every run's first row spread over the run.  Either way: launch_scan over the
//                                "is its own representative" flags = rank of first occurrence, the representatives in that
//                                order gathered by the Utf8 take path, codes = rank[rep[row]] written per output chunk.
//   rdf_groupby_agg_keys         Utf8 keys -> codes -> rdf_groupby_agg -> rdf_utf8_take of the dictionary by the code column
//   rdf_equijoin_indices_keys    Utf8 pairs -> codes over one dictionary of both sides -> rdf_equijoin_indices_multi

namespace {

// a buffer of the call's memory kind that outlives the arena resets of the entry points called in between
struct DictBuf {
    std::vector<uint64_t> h;
    CsPoolBuf d;
    void* p = nullptr;
    rdf_status alloc(size_t bytes, int32_t mem) {
        if (mem == RDF_MEM_HOST) { h.assign((bytes + 71) / 8, 0); p = h.data(); return RDF_OK; }
        RDF_TRY(d.alloc(bytes + 64));
        p = d.p;
        return RDF_OK;
    }
};

int64_t utf8_rows(const rdf_utf8_array& c) { return c.offsets.length - 1; }

// What every entry point here asks of a list of Utf8 chunks before any device work.
rdf_status dict_check_chunks(const char* fn, const rdf_utf8_array* chunks, int64_t nchunks, int32_t* mem, int64_t* rows) {
    for (int64_t i = 0; i < nchunks; ++i) {
        const rdf_utf8_array& c = chunks[i];
        if (c.offsets.dtype != RDF_I32 || c.offsets.length < 1)
            return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: offsets must be an Int32 array of rows + 1 entries", fn, (long long)i);
        if (c.data.dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: data must be a UInt8 array", fn, (long long)i);
        RDF_TRY(check_mem(&c.offsets, 1, mem));
        RDF_TRY(check_mem(&c.data, 1, mem));
        *rows += utf8_rows(c);
    }
    return RDF_OK;
}

// The device half of rdf_utf8_dictionary_encode; the arguments are checked.  out_dict_offsets == nullptr: codes only (the
// join needs no dictionary).  n > 0.
rdf_status dict_encode_device(const char* fn, const rdf_utf8_array* chunks, int64_t nchunks, int64_t n, int32_t mem, rdf_out* out_codes,
                              rdf_out* out_dict_offsets, rdf_out* out_dict_data, int64_t* out_count) {
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    CsPoolBuf rep, rank, firsts;   // (the take path in between resets the arena)
    RDF_TRY(rep.alloc((size_t)(n + 64) * 4));
    RDF_TRY(rank.alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8));
    CsDictArgs a;
    memset(&a, 0, sizeof a);
    a.rep = (uint32_t*)rep.p;
    int64_t* const drank = (int64_t*)rank.p;
    std::string route;
    bool have = false;
    if (ctx.opt_uniques_route != 1) {
        arena_begin();
        CsUtf8Staged st;
        RDF_TRY(cs_utf8_stage(chunks, nchunks, mem, nullptr, st));
        const uint64_t slots = cs_table_slots(n);
        CsUtf8Args& u = a.u;
        u.chunks = st.d_chunks; u.nchunks = nchunks; u.n = n;
        u.set.mask = slots - 1;
        u.set.max_fill = slots / 2;
        void *ptab, *prep, *phash, *pflags;
        RDF_TRY(arena_alloc((size_t)slots * 8, &ptab));
        RDF_TRY(arena_alloc((size_t)slots * 4, &prep));
        RDF_TRY(arena_alloc((size_t)n * 8, &phash));
        RDF_TRY(arena_alloc((size_t)n * 8, &pflags));
        u.set.table = (uint64_t*)ptab; u.set.rep = (uint32_t*)prep; u.hash = (uint64_t*)phash;
        a.flags = (int64_t*)pflags;
        RDF_TRY(cs_counters(&u.set.g));
        KernelTimer kt;
        route = "cs_utf8_hash_kernel + cs_dict_rep_kernel";
        HIP_TRY(launch_cs_fill64(u.set.table, (int64_t)slots, kCsEmpty, s));
        HIP_TRY(hipMemsetAsync(prep, 0xFF, (size_t)slots * 4, s));
        HIP_TRY(launch_cs_utf8_hash(u, s));
        HIP_TRY(launch_cs_dict_rep(a, s));   // (a table that gave up leaves rows without a slot: a mismatch)
        HIP_TRY(launch_scan(a.flags, drank, n, drank + n + 1, s));
        kt.stop();
        uint64_t g[8];
        RDF_TRY(cs_read_counters(u.set.g, g));
        have = !g[CS_G_OVERFLOW] && !g[CS_G_MISMATCH];
    }
    DictBuf perm;
    if (!have) {   // the exact route: sorted order, every run's first row is its smallest
        RDF_TRY(perm.alloc((size_t)(n + 64) * 4, mem));
        rdf_out idx;
        memset(&idx, 0, sizeof idx);
        idx.values = perm.p; idx.capacity = n; idx.dtype = RDF_U32; idx.mem = mem;
        rdf_sort_key key;
        memset(&key, 0, sizeof key);
        key.utf8 = chunks;
        RDF_TRY(rdf_lexsort_to_indices(&key, 1, nchunks, &idx));
        arena_begin();
        const rdf_array permv{idx.values, nullptr, 0, n, 0, RDF_U32, mem};
        CsUtf8Staged st;
        RDF_TRY(cs_utf8_stage(chunks, nchunks, mem, &permv, st));
        memset(&a.u, 0, sizeof a.u);
        a.u.chunks = st.d_chunks; a.u.nchunks = nchunks; a.u.n = n;
        a.u.perm = (const uint32_t*)st.extra;
        void *pflags, *pscan, *pheads;
        RDF_TRY(arena_alloc((size_t)n * 8, &pflags));
        RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &pscan));
        RDF_TRY(arena_alloc((size_t)(n + 1) * 4, &pheads));
        a.flags = (int64_t*)pflags;
        a.scan = (const int64_t*)pscan;
        a.heads = (uint32_t*)pheads;
        KernelTimer kt;
        route = "utf8 lexsort + cs_dict_heads_kernel + cs_dict_spread_kernel";
        HIP_TRY(launch_cs_dict_heads(a, s));
        HIP_TRY(launch_scan(a.flags, (int64_t*)pscan, n, (int64_t*)pscan + n + 1, s));
        HIP_TRY(launch_cs_dict_spread(a, s));
        HIP_TRY(launch_scan(a.flags, drank, n, drank + n + 1, s));
        kt.stop();
    }
    a.scan = drank;
    int64_t count = 0;
    HIP_TRY(hipMemcpyAsync(&count, drank + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out_count = count;

    // ---- the sizing rule: every length reported, nothing written unless everything fits
    bool codes_fit = true;
    for (int64_t i = 0; i < nchunks; ++i) {
        out_codes[i].length = utf8_rows(chunks[i]);
        codes_fit &= out_codes[i].capacity >= utf8_rows(chunks[i]);
    }
    if (count > 0 && (out_dict_offsets || !codes_fit)) {
        RDF_TRY(firsts.alloc((size_t)(count + 64) * 4));
        a.firsts = (uint32_t*)firsts.p;
        HIP_TRY(launch_cs_dict_firsts(a, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (out_dict_offsets) {
        if (count == 0) {
            if (!codes_fit) {
                out_dict_offsets->length = 1; out_dict_data->length = 0;
                return fail(RDF_MEMORY_ERROR, "%s: a codes output is shorter than its chunk", fn);
            }
            RDF_TRY(cs_utf8_empty(out_dict_offsets, out_dict_data, mem));
        } else if (!codes_fit || out_dict_offsets->capacity < count + 1) {   // only the lengths: the take path sizes into buffers of its own
            DictBuf toffs;
            RDF_TRY(toffs.alloc((size_t)(count + 1) * 4, mem));
            rdf_out to, td;
            memset(&to, 0, sizeof to);
            memset(&td, 0, sizeof td);
            to.values = toffs.p; to.capacity = count + 1; to.dtype = RDF_I32; to.mem = mem;
            td.dtype = RDF_U8; td.mem = mem;
            const rdf_status st = cs_utf8_gather(chunks, nchunks, mem, a.firsts, count, &to, &td);
            if (st != RDF_OK && st != RDF_MEMORY_ERROR) return st;
            out_dict_offsets->length = count + 1;
            out_dict_data->length = td.length;
            return fail(RDF_MEMORY_ERROR, "%s: output capacity too small (%lld values; the needed lengths are in the outputs' length fields)", fn, (long long)count);
        } else {
            RDF_TRY(cs_utf8_gather(chunks, nchunks, mem, a.firsts, count, out_dict_offsets, out_dict_data));
            route += " + utf8_span_kernel + utf8_copy_kernel";
        }
    } else if (!codes_fit) return fail(RDF_MEMORY_ERROR, "%s: a codes output is shorter than its chunk", fn);

    // ---- the codes, written per output chunk (host outputs through device staging)
    std::vector<CsDictOut> ho((size_t)nchunks);
    std::vector<size_t> voff((size_t)nchunks, 0);
    size_t vbytes = 0;
    int64_t row = 0, tile = 0;
    for (int64_t i = 0; i < nchunks; ++i) {
        const int64_t rows = utf8_rows(chunks[i]);
        ho[i].row_start = row;
        ho[i].tile_start = tile;
        ho[i].rows = rows;
        voff[i] = vbytes;
        if (out_codes[i].validity) vbytes += (size_t)((rows + 63) / 64) * 8;
        row += rows;
        tile += (rows + kCsThreads - 1) / kCsThreads;
    }
    arena_begin();
    void *dcodes = nullptr, *dvalid = nullptr, *douts, *dnulls;
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(arena_alloc((size_t)n * 4, &dcodes));
        RDF_TRY(arena_alloc(vbytes + 8, &dvalid));
    }
    const size_t tb = (size_t)nchunks * sizeof(CsDictOut), nb = (size_t)nchunks * 8;
    RDF_TRY(arena_alloc(tb, &douts));
    RDF_TRY(arena_alloc(nb, &dnulls));
    for (int64_t i = 0; i < nchunks; ++i) {
        if (mem == RDF_MEM_HOST) {
            ho[i].codes = (uint32_t*)dcodes + ho[i].row_start;
            ho[i].valid = out_codes[i].validity ? (uint8_t*)dvalid + voff[i] : nullptr;
        } else {
            ho[i].codes = (uint32_t*)out_codes[i].values;
            ho[i].valid = out_codes[i].validity;
        }
    }
    const size_t pin_n = (tb + 63) & ~(size_t)63;
    RDF_TRY(pinned_reserve(pin_n + nb + 64));
    memcpy(ctx.pinned, ho.data(), tb);
    HIP_TRY(hipMemcpyAsync(douts, ctx.pinned, tb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(dnulls, 0, nb, s));
    a.outs = (const CsDictOut*)douts;
    a.nouts = nchunks;
    a.ntiles = tile;
    a.nulls = (unsigned long long*)dnulls;
    {
        KernelTimer kt;
        HIP_TRY(launch_cs_dict_codes(a, s));
        kt.stop();
    }
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_n, dnulls, nb, hipMemcpyDeviceToHost, s));
    if (mem == RDF_MEM_HOST)
        for (int64_t i = 0; i < nchunks; ++i) {
            if (ho[i].rows == 0) continue;
            HIP_TRY(hipMemcpyAsync(out_codes[i].values, ho[i].codes, (size_t)ho[i].rows * 4, hipMemcpyDeviceToHost, s));
            if (ho[i].valid) HIP_TRY(hipMemcpyAsync(out_codes[i].validity, ho[i].valid, (size_t)((ho[i].rows + 7) / 8), hipMemcpyDeviceToHost, s));
        }
    HIP_TRY(hipStreamSynchronize(s));
    for (int64_t i = 0; i < nchunks; ++i) {
        int64_t nulls;
        memcpy(&nulls, ctx.pinned + pin_n + (size_t)i * 8, 8);
        out_codes[i].null_count = nulls;
    }
    ctx.last_kernel = route + " + cs_dict_codes_kernel";
    return RDF_OK;
}

// codes of `nchunks` Utf8 chunks in buffers of the call's memory kind, every chunk with a validity bitmap: what the two
// compositions hand to the integer kernels as a UInt32 key column
struct DictCodes {
    DictBuf buf;
    std::vector<rdf_out> outs;
    std::vector<rdf_array> arrays;
    rdf_status make(const rdf_utf8_array* chunks, int64_t nchunks, int32_t mem) {
        std::vector<size_t> off((size_t)nchunks * 2);
        size_t bytes = 0;
        for (int64_t i = 0; i < nchunks; ++i) {
            const int64_t rows = utf8_rows(chunks[i]);
            off[2 * i] = bytes; bytes += ((size_t)rows * 4 + 255) & ~(size_t)255;
            off[2 * i + 1] = bytes; bytes += ((size_t)((rows + 63) / 64) * 8 + 255 + 8) & ~(size_t)255;
        }
        RDF_TRY(buf.alloc(bytes + 256, mem));
        outs.resize((size_t)nchunks);
        for (int64_t i = 0; i < nchunks; ++i) {
            rdf_out& o = outs[i];
            memset(&o, 0, sizeof o);
            o.values = (char*)buf.p + off[2 * i];
            o.validity = (uint8_t*)buf.p + off[2 * i + 1];
            o.capacity = utf8_rows(chunks[i]);
            o.dtype = RDF_U32; o.mem = mem;
        }
        return RDF_OK;
    }
    void finish(bool nullable) {
        arrays.resize(outs.size());
        for (size_t i = 0; i < outs.size(); ++i)
            arrays[i] = rdf_array{outs[i].values, nullable ? outs[i].validity : nullptr, 0, outs[i].length, nullable ? outs[i].null_count : 0, RDF_U32, outs[i].mem};
    }
};

bool utf8_nullable(const rdf_utf8_array* chunks, int64_t nchunks) {
    for (int64_t i = 0; i < nchunks; ++i) if (chunks[i].offsets.validity) return true;
    return false;
}

}  // namespace

extern "C" {

rdf_status rdf_utf8_dictionary_encode(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_codes, rdf_out* out_dict_offsets,
                                      rdf_out* out_dict_data, int64_t* out_count) {
    const char* fn = "utf8_dictionary_encode";
    if (nchunks < 0 || (nchunks > 0 && !chunks)) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk list", fn);
    if (!out_count || !out_dict_offsets || !out_dict_data || (nchunks > 0 && !out_codes)) return fail(RDF_INVALID_ARGUMENT, "%s: null output", fn);
    *out_count = 0;
    int32_t mem = -1;
    int64_t n = 0;
    RDF_TRY(dict_check_chunks(fn, chunks, nchunks, &mem, &n));
    if (out_dict_offsets->dtype != RDF_I32 || out_dict_data->dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: the dictionary is (Int32 offsets, UInt8 data)", fn);
    if (mem < 0) mem = out_dict_offsets->mem;
    if (mem != RDF_MEM_HOST && mem != RDF_MEM_DEVICE) return fail(RDF_INVALID_ARGUMENT, "bad mem tag %d", mem);
    RDF_TRY(check_out_mem(out_dict_offsets, 1, mem));
    RDF_TRY(check_out_mem(out_dict_data, 1, mem));
    RDF_TRY(check_out_mem(out_codes, nchunks, mem));
    for (int64_t i = 0; i < nchunks; ++i) {
        if (out_codes[i].dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "%s: codes are UInt32", fn);
        if (out_codes[i].capacity < 0 || (out_codes[i].capacity > 0 && !out_codes[i].values)) return fail(RDF_INVALID_ARGUMENT, "%s: codes %lld: capacity without a buffer", fn, (long long)i);
        if (chunks[i].offsets.validity && !out_codes[i].validity) return fail(RDF_INVALID_ARGUMENT, "%s: codes %lld need a validity buffer", fn, (long long)i);
    }
    if (!out_dict_offsets->values || out_dict_offsets->capacity < 1) return fail(RDF_INVALID_ARGUMENT, "%s: the dictionary has no offsets buffer", fn);
    if (out_dict_data->capacity < 0 || (out_dict_data->capacity > 0 && !out_dict_data->values)) return fail(RDF_INVALID_ARGUMENT, "%s: data capacity without a buffer", fn);
    if (n >= (int64_t)1 << 32) return fail(RDF_INVALID_ARGUMENT, "%s: a column holds at most 2^32-1 rows (src/table.rs:218)", fn);
    RDF_TRY(ensure_ready());
    if (n == 0) {
        for (int64_t i = 0; i < nchunks; ++i) { out_codes[i].length = 0; out_codes[i].null_count = 0; }
        return cs_utf8_empty(out_dict_offsets, out_dict_data, mem);
    }
    return dict_encode_device(fn, chunks, nchunks, n, mem, out_codes, out_dict_offsets, out_dict_data, out_count);
}

rdf_status rdf_groupby_agg_keys(const rdf_sort_key* keys, int32_t nkeys, const rdf_array* values, int64_t nchunks, int32_t agg,
                                int64_t max_groups, rdf_key_out* out_keys, rdf_out* out_values, rdf_out* out_counts) {
    const char* fn = "groupby_keys";
    if (nchunks < 1 || !keys) return fail(RDF_INVALID_ARGUMENT, "%s: a column has at least one chunk", fn);
    if (nkeys < 1 || nkeys > kMaxKeyCols) return fail(RDF_INVALID_ARGUMENT, "%s: 1..%d grouping columns", fn, kMaxKeyCols);
    if (!out_keys || !out_values || !out_counts) return fail(RDF_INVALID_ARGUMENT, "%s: null output", fn);
    if (max_groups < 1) return fail(RDF_INVALID_ARGUMENT, "%s: max_groups must be positive", fn);
    if (agg < RDF_AGG_SUM || agg > RDF_AGG_COUNT) return fail(RDF_INVALID_ARGUMENT, "%s: unknown aggregate %d", fn, agg);
    int32_t mem = -1;
    bool any_utf8 = false;
    RDF_TRY(lexsort_check_keys(keys, nkeys, nchunks, fn, &mem, &any_utf8));
    std::vector<int64_t> row_start;
    RDF_TRY(lexsort_row_starts(keys, nkeys, nchunks, fn, row_start));
    const int64_t nrows = row_start[(size_t)nchunks];
    if (values && agg != RDF_AGG_COUNT) {
        RDF_TRY(check_mem(values, nchunks, &mem));
        for (int64_t c = 0; c < nchunks; ++c)
            if (values[c].length != row_start[(size_t)c + 1] - row_start[(size_t)c]) return fail(RDF_COMPUTE_ERROR, "%s: key and value chunks differ in length", fn);
    }
    const int64_t cap_needed = std::min<int64_t>(max_groups + 2, nrows + 2);
    for (int k = 0; k < nkeys; ++k) {
        const rdf_key_out& o = out_keys[k];
        if (keys[k].values) {
            if (!o.values || o.utf8_offsets || o.utf8_data) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d: a numeric key comes back in `values` alone", fn, k);
            if (!(keys[k].values[0].dtype >= RDF_I8 && keys[k].values[0].dtype <= RDF_U64)) return fail(RDF_INVALID_ARGUMENT, "%s: integer or Utf8 key column required", fn);
            continue;
        }
        if (o.values || !o.utf8_offsets || !o.utf8_data) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d: a Utf8 key comes back in the (utf8_offsets, utf8_data) pair alone", fn, k);
        if (o.utf8_offsets->dtype != RDF_I32 || o.utf8_data->dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d: (Int32 offsets, UInt8 data)", fn, k);
        RDF_TRY(check_out_mem(o.utf8_offsets, 1, mem));
        RDF_TRY(check_out_mem(o.utf8_data, 1, mem));
        if (!o.utf8_offsets->values || o.utf8_offsets->capacity < 1) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d has no offsets buffer", fn, k);
        if (o.utf8_data->capacity < 0 || (o.utf8_data->capacity > 0 && !o.utf8_data->values)) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d: data capacity without a buffer", fn, k);
        if (utf8_nullable(keys[k].utf8, nchunks) && !o.utf8_offsets->validity) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d needs a validity buffer", fn, k);
    }
    RDF_TRY(check_out_mem(out_values, 1, mem));
    RDF_TRY(check_out_mem(out_counts, 1, mem));

    // the integer call's own list: numeric keys as they are, Utf8 keys as their codes
    std::vector<rdf_array> flat((size_t)nkeys * (size_t)nchunks);
    rdf_out ok[kMaxKeyCols];
    if (!any_utf8) {
        for (int k = 0; k < nkeys; ++k) {
            for (int64_t c = 0; c < nchunks; ++c) flat[(size_t)k * nchunks + c] = keys[k].values[c];
            ok[k] = *out_keys[k].values;
        }
        const rdf_status st = rdf_groupby_agg(flat.data(), nkeys, values, nchunks, agg, max_groups, ok, out_values, out_counts);
        for (int k = 0; k < nkeys; ++k) *out_keys[k].values = ok[k];
        return st;
    }
    // what rdf_groupby_agg refuses without the device is refused here, before the encoding touches it
    if (agg == RDF_AGG_COUNT) values = nullptr;
    else if (!values) agg = RDF_AGG_COUNT;
    const int op = agg == RDF_AGG_MIN ? AGG_MIN : agg == RDF_AGG_MAX ? AGG_MAX : AGG_SUM;
    const int vdt = values ? values[0].dtype : -1;
    if (values && !is_numeric(vdt)) return fail(RDF_INVALID_ARGUMENT, "%s: numeric value column required", fn);
    bool vnullable = false;
    for (int64_t c = 0; values && c < nchunks; ++c) {
        if (values[c].dtype != vdt) return fail(RDF_INVALID_ARGUMENT, "%s: chunks differ in dtype", fn);
        vnullable |= values[c].validity != nullptr;
    }
    const int odt = gb_acc_dtype(op, vdt);
    if (out_values->dtype != odt || out_counts->dtype != RDF_I64)
        return fail(RDF_INVALID_ARGUMENT, "%s: outputs must be (key dtypes, %s, Int64)", fn, odt == RDF_F64 ? "Float64" : odt == RDF_U64 ? "UInt64" : "Int64");
    if (op != AGG_SUM && vnullable && !out_values->validity) return fail(RDF_INVALID_ARGUMENT, "%s: min / max of a nullable column needs an output validity buffer", fn);
    for (int k = 0; k < nkeys; ++k) {
        if (!keys[k].values) continue;
        RDF_TRY(check_out_mem(out_keys[k].values, 1, mem));
        if (out_keys[k].values->dtype != keys[k].values[0].dtype) return fail(RDF_INVALID_ARGUMENT, "%s: key output %d must have the key dtype", fn, k);
        bool kn = false;
        for (int64_t c = 0; c < nchunks; ++c) kn |= keys[k].values[c].validity != nullptr;
        if (kn && !out_keys[k].values->validity) return fail(RDF_INVALID_ARGUMENT, "output validity buffer required");
    }
    if (out_values->capacity < cap_needed || out_counts->capacity < cap_needed) return fail(RDF_MEMORY_ERROR, "output capacity too small (need max_groups + 2)");
    for (int k = 0; k < nkeys; ++k)
        if (keys[k].values && out_keys[k].values->capacity < cap_needed) return fail(RDF_MEMORY_ERROR, "output capacity too small (need max_groups + 2)");
    RDF_TRY(ensure_ready());

    DictCodes codes[kMaxKeyCols];
    DictBuf doffs[kMaxKeyCols], ddata[kMaxKeyCols], gcodes[kMaxKeyCols], toffs[kMaxKeyCols];
    rdf_utf8_array dict[kMaxKeyCols];
    bool nullable[kMaxKeyCols] = {false, false, false, false};
    for (int k = 0; k < nkeys; ++k) {
        if (keys[k].values) {
            for (int64_t c = 0; c < nchunks; ++c) flat[(size_t)k * nchunks + c] = keys[k].values[c];
            ok[k] = *out_keys[k].values;
            continue;
        }
        const rdf_utf8_array* ch = keys[k].utf8;
        nullable[k] = utf8_nullable(ch, nchunks);
        int64_t bytes = 0;
        for (int64_t c = 0; c < nchunks; ++c) bytes += ch[c].data.length;
        RDF_TRY(codes[k].make(ch, nchunks, mem));
        RDF_TRY(doffs[k].alloc((size_t)(nrows + 1) * 4, mem));
        RDF_TRY(ddata[k].alloc((size_t)bytes + 8, mem));
        rdf_out o_off, o_dat;
        memset(&o_off, 0, sizeof o_off);
        memset(&o_dat, 0, sizeof o_dat);
        o_off.values = doffs[k].p; o_off.capacity = nrows + 1; o_off.dtype = RDF_I32; o_off.mem = mem;
        o_dat.values = ddata[k].p; o_dat.capacity = bytes + 8; o_dat.dtype = RDF_U8; o_dat.mem = mem;
        int64_t count = 0;
        RDF_TRY(rdf_utf8_dictionary_encode(ch, nchunks, codes[k].outs.data(), &o_off, &o_dat, &count));
        codes[k].finish(nullable[k]);
        for (int64_t c = 0; c < nchunks; ++c) flat[(size_t)k * nchunks + c] = codes[k].arrays[c];
        dict[k].offsets = rdf_array{o_off.values, nullptr, 0, o_off.length, 0, RDF_I32, mem};
        dict[k].data = rdf_array{o_dat.values, nullptr, 0, o_dat.length, 0, RDF_U8, mem};
        // the group codes come back in a buffer of the call's own: the caller's outputs stay untouched until every one fits
        RDF_TRY(gcodes[k].alloc((size_t)cap_needed * 4 + 256 + (size_t)((cap_needed + 63) / 64) * 8 + 8, mem));
        memset(&ok[k], 0, sizeof ok[k]);
        ok[k].values = gcodes[k].p;
        ok[k].validity = nullable[k] ? (uint8_t*)gcodes[k].p + (((size_t)cap_needed * 4 + 255) & ~(size_t)255) : nullptr;
        ok[k].capacity = cap_needed; ok[k].dtype = RDF_U32; ok[k].mem = mem;
    }
    // numeric outputs go through buffers of the call's own for the same reason
    DictBuf tvals, tcnts, tkeys[kMaxKeyCols];
    rdf_out tv = *out_values, tc = *out_counts;
    const size_t vb = (size_t)cap_needed * 8, vbits = ((size_t)cap_needed + 63) / 64 * 8 + 8;
    RDF_TRY(tvals.alloc(vb + 256 + vbits, mem));
    RDF_TRY(tcnts.alloc(vb + 256 + vbits, mem));
    tv.values = tvals.p; tv.validity = out_values->validity ? (uint8_t*)tvals.p + ((vb + 255) & ~(size_t)255) : nullptr; tv.capacity = cap_needed;
    tc.values = tcnts.p; tc.validity = out_counts->validity ? (uint8_t*)tcnts.p + ((vb + 255) & ~(size_t)255) : nullptr; tc.capacity = cap_needed;
    for (int k = 0; k < nkeys; ++k) {
        if (!keys[k].values) continue;
        RDF_TRY(tkeys[k].alloc(vb + 256 + vbits, mem));
        ok[k].values = tkeys[k].p;
        ok[k].validity = out_keys[k].values->validity ? (uint8_t*)tkeys[k].p + ((vb + 255) & ~(size_t)255) : nullptr;
        ok[k].capacity = cap_needed;
    }
    // (over Utf8 keys the NULL group and the code whose hash is the LDS free marker never counted against max_groups: kept)
    RDF_TRY(groupby_agg_impl(flat.data(), nkeys, values, nchunks, agg, max_groups, ok, &tv, &tc, 2));
    const std::string gb_kernels = g_ctx.last_kernel;
    const int64_t groups = tc.length;

    // ---- Utf8 key columns: the dictionary taken by the group codes (a NULL code gives a NULL row); sized first
    rdf_array gidx[kMaxKeyCols];
    bool fits = true;
    for (int k = 0; k < nkeys; ++k) {
        if (keys[k].values) continue;
        gidx[k] = rdf_array{ok[k].values, ok[k].validity, 0, groups, ok[k].validity ? ok[k].null_count : 0, RDF_U32, mem};
        RDF_TRY(toffs[k].alloc((size_t)(groups + 1) * 4 + (size_t)((groups + 63) / 64) * 8 + 256 + 8, mem));
        rdf_out to, td;
        memset(&to, 0, sizeof to);
        memset(&td, 0, sizeof td);
        to.values = toffs[k].p; to.validity = (uint8_t*)toffs[k].p + (((size_t)(groups + 1) * 4 + 255) & ~(size_t)255);
        to.capacity = groups + 1; to.dtype = RDF_I32; to.mem = mem;
        td.dtype = RDF_U8; td.mem = mem;
        const rdf_status st = rdf_utf8_take(&dict[k], 1, &gidx[k], &to, &td);
        if (st != RDF_OK && st != RDF_MEMORY_ERROR) return st;
        out_keys[k].utf8_offsets->length = groups + 1;
        out_keys[k].utf8_data->length = td.length;
        if (out_keys[k].utf8_offsets->capacity < groups + 1 || out_keys[k].utf8_data->capacity < td.length) fits = false;
    }
    if (!fits) return fail(RDF_MEMORY_ERROR, "%s: a Utf8 key output is too small (the needed lengths are in its length fields)", fn);
    for (int k = 0; k < nkeys; ++k)
        if (!keys[k].values) RDF_TRY(rdf_utf8_take(&dict[k], 1, &gidx[k], out_keys[k].utf8_offsets, out_keys[k].utf8_data));
    auto deliver = [&](const rdf_out& from, rdf_out* to) -> rdf_status {
        const size_t bytes = (size_t)groups * (size_t)dtype_size(from.dtype), bits = (size_t)((groups + 7) / 8);
        if (mem == RDF_MEM_HOST) {
            if (bytes) memcpy(to->values, from.values, bytes);
            if (to->validity && from.validity && bits) memcpy(to->validity, from.validity, bits);
        } else {
            if (bytes) HIP_TRY(hipMemcpyAsync(to->values, from.values, bytes, hipMemcpyDeviceToDevice, g_ctx.stream));
            if (to->validity && from.validity && bits) HIP_TRY(hipMemcpyAsync(to->validity, from.validity, bits, hipMemcpyDeviceToDevice, g_ctx.stream));
        }
        to->length = from.length;
        to->null_count = from.null_count;
        return RDF_OK;
    };
    RDF_TRY(deliver(tv, out_values));
    RDF_TRY(deliver(tc, out_counts));
    for (int k = 0; k < nkeys; ++k)
        if (keys[k].values) RDF_TRY(deliver(ok[k], out_keys[k].values));
    if (mem == RDF_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(g_ctx.stream));
    g_ctx.last_kernel = "cs_dict_codes_kernel + " + gb_kernels + " + utf8_span_kernel + utf8_copy_kernel";
    return RDF_OK;
}

rdf_status rdf_equijoin_indices_keys(const rdf_sort_key* left_keys, int64_t left_nchunks, const rdf_sort_key* right_keys, int64_t right_nchunks,
                                     int32_t nkeys, int32_t join_type, rdf_out* out_left, rdf_out* out_right, int64_t* out_rows) {
    const char* fn = "join_keys";
    if (!left_keys || !right_keys || left_nchunks < 1 || right_nchunks < 1 || !out_rows) return fail(RDF_INVALID_ARGUMENT, "%s: bad arguments", fn);
    if (nkeys < 1 || nkeys > 4) return fail(RDF_INVALID_ARGUMENT, "%s: 1 to 4 key pairs", fn);
    if (join_type < RDF_JOIN_LEFT || join_type > RDF_JOIN_FULL) return fail(RDF_INVALID_ARGUMENT, "%s: bad join type", fn);
    if ((out_left == nullptr) != (out_right == nullptr)) return fail(RDF_INVALID_ARGUMENT, "%s: give both outputs or neither (count only)", fn);
    int32_t mem = -1;
    bool any_utf8 = false;
    RDF_TRY(lexsort_check_keys(left_keys, nkeys, left_nchunks, fn, &mem, &any_utf8));
    RDF_TRY(lexsort_check_keys(right_keys, nkeys, right_nchunks, fn, &mem, &any_utf8));
    for (int k = 0; k < nkeys; ++k) {
        if ((left_keys[k].utf8 != nullptr) != (right_keys[k].utf8 != nullptr)) return fail(RDF_INVALID_ARGUMENT, "%s: pair %d: a Utf8 key pairs with a Utf8 key only", fn, k);
        if (left_keys[k].values && left_keys[k].values[0].dtype != right_keys[k].values[0].dtype)
            return fail(RDF_INVALID_ARGUMENT, "%s: pair %d: key columns must share one dtype (cast first)", fn, k);
    }
    std::vector<int64_t> lrs, rrs;
    {
        auto rows_agree = [&](const rdf_sort_key* keys, int64_t nch, std::vector<int64_t>& rs) -> rdf_status {
            auto total = [&](int k) { int64_t t = 0; for (int64_t c = 0; c < nch; ++c) t += keys[k].values ? keys[k].values[c].length : utf8_rows(keys[k].utf8[c]); return t; };
            // (the integer join asks for equal totals per side, and for equal chunking only of what it is handed: a Utf8
            // key's codes keep its chunking, so the chunk rows must agree as well)
            rs.assign((size_t)nch + 1, 0);
            for (int64_t c = 0; c < nch; ++c) rs[(size_t)c + 1] = rs[(size_t)c] + (keys[0].values ? keys[0].values[c].length : utf8_rows(keys[0].utf8[c]));
            for (int k = 1; k < nkeys; ++k) {
                if (total(k) != rs[(size_t)nch]) return fail(RDF_COMPUTE_ERROR, "%s: key columns of one side differ in length", fn);
                for (int64_t c = 0; c < nch; ++c)
                    if ((keys[k].values ? keys[k].values[c].length : utf8_rows(keys[k].utf8[c])) != rs[(size_t)c + 1] - rs[(size_t)c])
                        return fail(RDF_COMPUTE_ERROR, "%s: key columns of one side differ in their chunks' rows", fn);
            }
            return RDF_OK;
        };
        RDF_TRY(rows_agree(left_keys, left_nchunks, lrs));
        RDF_TRY(rows_agree(right_keys, right_nchunks, rrs));
    }
    const int64_t nleft = lrs[(size_t)left_nchunks], nright = rrs[(size_t)right_nchunks];
    if (nleft + nright >= (int64_t)1 << 32) return fail(RDF_INVALID_ARGUMENT, "%s: the two sides together hold at most 2^32-1 rows", fn);
    if (out_left) {
        RDF_TRY(check_out_mem(out_left, 1, mem));
        RDF_TRY(check_out_mem(out_right, 1, mem));
        if (out_left->dtype != RDF_U32 || out_right->dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "%s: indices are UInt32", fn);
    }
    std::vector<rdf_array> lflat((size_t)nkeys * (size_t)left_nchunks), rflat((size_t)nkeys * (size_t)right_nchunks);
    DictCodes codes[4];
    if (any_utf8) RDF_TRY(ensure_ready());
    std::string enc_kernels;
    for (int k = 0; k < nkeys; ++k) {
        if (left_keys[k].values) {
            for (int64_t c = 0; c < left_nchunks; ++c) lflat[(size_t)k * left_nchunks + c] = left_keys[k].values[c];
            for (int64_t c = 0; c < right_nchunks; ++c) rflat[(size_t)k * right_nchunks + c] = right_keys[k].values[c];
            continue;
        }
        // one dictionary for both sides: the left chunks followed by the right chunks
        std::vector<rdf_utf8_array> both(left_keys[k].utf8, left_keys[k].utf8 + left_nchunks);
        both.insert(both.end(), right_keys[k].utf8, right_keys[k].utf8 + right_nchunks);
        const int64_t nb = left_nchunks + right_nchunks;
        RDF_TRY(codes[k].make(both.data(), nb, mem));
        int64_t count = 0;
        if (nleft + nright > 0) RDF_TRY(dict_encode_device(fn, both.data(), nb, nleft + nright, mem, codes[k].outs.data(), nullptr, nullptr, &count));
        enc_kernels = g_ctx.last_kernel + " + ";
        const bool lnull = utf8_nullable(both.data(), left_nchunks), rnull = utf8_nullable(both.data() + left_nchunks, right_nchunks);
        for (int64_t c = 0; c < nb; ++c) {
            const rdf_out& o = codes[k].outs[(size_t)c];
            const bool nl = c < left_nchunks ? lnull : rnull;
            const rdf_array a{o.values, nl ? o.validity : nullptr, 0, utf8_rows(both[(size_t)c]), nl ? o.null_count : 0, RDF_U32, mem};
            if (c < left_nchunks) lflat[(size_t)k * left_nchunks + c] = a;
            else rflat[(size_t)k * right_nchunks + (c - left_nchunks)] = a;
        }
    }
    const rdf_status st = rdf_equijoin_indices_multi(lflat.data(), left_nchunks, rflat.data(), right_nchunks, nkeys, join_type, out_left, out_right, out_rows);
    if (st == RDF_OK && any_utf8) g_ctx.last_kernel = enc_kernels + g_ctx.last_kernel;
    return st;
}

}  // extern "C"
