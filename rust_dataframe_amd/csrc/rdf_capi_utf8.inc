// rdf_capi_utf8.inc — host side of the Utf8 entry points (rdf_utf8.hip); textually included by rdf_capi.cpp (it uses that
// file's per-thread context, arena and staging helpers).
//
//   rdf_utf8_filter / rdf_utf8_take                 Column::filter / Column::take over StringArray chunks (src/table.rs)
//   rdf_utf8_trim / _ltrim / _rtrim / _substring    ScalarFunctions over Utf8 (src/functions/scalar.rs)
//   rdf_utf8_lower / _upper
//
// One call = validate everything -> stage host inputs -> span pass -> scans -> per-chunk totals read back -> the sizing
// rule -> write pass.  Nothing is written to the caller's buffers before the sizing rule has passed.

namespace {

// lohi[2c], lohi[2c + 1] = the first and last value offset of chunk c, checked against its data array before a byte of it
// is read (device-resident offsets are read by a kernel).  Uses the pinned staging buffer from offset 0.
rdf_status utf8_value_ranges(const rdf_utf8_array* chunks, int64_t nchunks, int32_t mem, std::vector<int32_t>& lohi, const char* fn) {
    Ctx& ctx = g_ctx;
    lohi.assign((size_t)nchunks * 2, 0);
    if (mem == RDF_MEM_HOST) {
        for (int64_t i = 0; i < nchunks; ++i) {
            const int32_t* off = (const int32_t*)chunks[i].offsets.values + chunks[i].offsets.offset;
            lohi[2 * i] = off[0];
            lohi[2 * i + 1] = off[chunks[i].offsets.length - 1];
        }
    } else if (nchunks > 0) {
        std::vector<Utf8Chunk> hc((size_t)nchunks);
        for (int64_t i = 0; i < nchunks; ++i) {
            memset(&hc[i], 0, sizeof(Utf8Chunk));
            hc[i].offs = (const int32_t*)chunks[i].offsets.values + chunks[i].offsets.offset;
            hc[i].rows = chunks[i].offsets.length - 1;
        }
        const size_t tb = (size_t)nchunks * sizeof(Utf8Chunk), bb = (size_t)nchunks * 8;
        void *dtab, *dbounds;
        RDF_TRY(arena_alloc(tb, &dtab));
        RDF_TRY(arena_alloc(bb, &dbounds));
        RDF_TRY(pinned_reserve(tb + bb + 64));
        memcpy(ctx.pinned, hc.data(), tb);
        HIP_TRY(hipMemcpyAsync(dtab, ctx.pinned, tb, hipMemcpyHostToDevice, ctx.stream));
        Utf8Args b;
        memset(&b, 0, sizeof b);
        b.chunks = (const Utf8Chunk*)dtab;
        b.nchunks = nchunks;
        b.bounds = (int32_t*)dbounds;
        HIP_TRY(launch_utf8_bounds(b, ctx.stream));
        char* pin_b = ctx.pinned + ((tb + 63) & ~(size_t)63);
        HIP_TRY(hipMemcpyAsync(pin_b, dbounds, bb, hipMemcpyDeviceToHost, ctx.stream));
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        memcpy(lohi.data(), pin_b, bb);
    }
    for (int64_t i = 0; i < nchunks; ++i)
        if (lohi[2 * i] < 0 || lohi[2 * i + 1] < lohi[2 * i] || lohi[2 * i + 1] > chunks[i].data.length)
            return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: value offsets [%d, %d] outside the %lld data bytes", fn, (long long)i,
                        lohi[2 * i], lohi[2 * i + 1], (long long)chunks[i].data.length);
    return RDF_OK;
}

rdf_status utf8_run(int op, const rdf_utf8_array* chunks, int64_t nchunks, const rdf_array* mask, const rdf_array* indices,
                    int64_t pos, int64_t len, rdf_out* out_offsets, rdf_out* out_data, const char* fn) {
    const bool take = op == UTF8_TAKE, filter = op == UTF8_FILTER;
    if (nchunks < 0 || (nchunks > 0 && !chunks)) return fail(RDF_INVALID_ARGUMENT, "%s: bad chunk list", fn);
    if (filter && nchunks > 0 && !mask) return fail(RDF_INVALID_ARGUMENT, "%s: null mask list", fn);
    if (take && !indices) return fail(RDF_INVALID_ARGUMENT, "%s: null indices", fn);
    if (op == UTF8_SUBSTRING && (pos < 0 || len < 0)) return fail(RDF_INVALID_ARGUMENT, "%s: position and length must be >= 0", fn);
    int32_t mem = -1;
    int64_t total_rows = 0;
    bool any_validity = false;
    for (int64_t i = 0; i < nchunks; ++i) {
        const rdf_utf8_array& c = chunks[i];
        if (c.offsets.dtype != RDF_I32 || c.offsets.length < 1)
            return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: offsets must be an Int32 array of rows + 1 entries", fn, (long long)i);
        if (c.data.dtype != RDF_U8) return fail(RDF_INVALID_ARGUMENT, "%s: chunk %lld: data must be a UInt8 array", fn, (long long)i);
        RDF_TRY(check_mem(&c.offsets, 1, &mem));
        RDF_TRY(check_mem(&c.data, 1, &mem));
        const int64_t rows = c.offsets.length - 1;
        total_rows += rows;
        any_validity |= c.offsets.validity != nullptr;
        if (filter) {
            if (mask[i].dtype != RDF_BOOL) return fail(RDF_INVALID_ARGUMENT, "%s: mask %lld must be Boolean", fn, (long long)i);
            if (mask[i].length != rows) return fail(RDF_INVALID_ARGUMENT, "%s: mask %lld has %lld rows, the chunk %lld", fn, (long long)i, (long long)mask[i].length, (long long)rows);
            RDF_TRY(check_mem(&mask[i], 1, &mem));
        }
    }
    if (take) {
        if (indices->dtype != RDF_U32 && indices->dtype != RDF_U64) return fail(RDF_INVALID_ARGUMENT, "%s: indices must be UInt32 or UInt64", fn);
        RDF_TRY(check_mem(indices, 1, &mem));
        any_validity |= indices->validity != nullptr;
    }
    const int64_t nout = take ? 1 : nchunks;
    if (nout > 0 && (!out_offsets || !out_data)) return fail(RDF_INVALID_ARGUMENT, "%s: null output list", fn);
    for (int64_t o = 0; o < nout; ++o) {
        if (out_offsets[o].dtype != RDF_I32 || out_data[o].dtype != RDF_U8)
            return fail(RDF_INVALID_ARGUMENT, "%s: outputs are (Int32 offsets, UInt8 data)", fn);
        if (mem >= 0) {
            RDF_TRY(check_out_mem(&out_offsets[o], 1, mem));
            RDF_TRY(check_out_mem(&out_data[o], 1, mem));
        }
        if (!out_offsets[o].values || out_offsets[o].capacity < 1) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld has no offsets buffer", fn, (long long)o);
        if (out_data[o].capacity < 0 || (out_data[o].capacity > 0 && !out_data[o].values))
            return fail(RDF_INVALID_ARGUMENT, "%s: output %lld: data capacity without a buffer", fn, (long long)o);
        const bool nullable = take ? any_validity : chunks[o].offsets.validity != nullptr;
        if (nullable && !out_offsets[o].validity) return fail(RDF_INVALID_ARGUMENT, "%s: output %lld needs a validity buffer", fn, (long long)o);
        const int64_t rows = take ? indices->length : chunks[o].offsets.length - 1;
        if (!filter && out_offsets[o].capacity < rows + 1) {
            out_offsets[o].length = rows + 1;
            return fail(RDF_MEMORY_ERROR, "%s: output %lld: offsets need %lld entries", fn, (long long)o, (long long)(rows + 1));
        }
    }
    RDF_TRY(ensure_ready());
    if (nout == 0) return RDF_OK;
    Ctx& ctx = g_ctx;
    arena_begin();

    // ---- the value-offset range of every chunk, checked against its data array before a byte of it is read
    std::vector<int32_t> lohi;
    RDF_TRY(utf8_value_ranges(chunks, nchunks, mem, lohi, fn));

    // ---- inputs on the device (host arrays staged, device arrays aliased)
    std::vector<rdf_array> views;
    views.reserve((size_t)nchunks * 4 + 1);
    std::vector<int> vi((size_t)nchunks * 4, -1);
    InputStager in;
    for (int64_t i = 0; i < nchunks; ++i) {
        const rdf_utf8_array& c = chunks[i];
        const int64_t rows = c.offsets.length - 1;
        rdf_array offs = c.offsets;
        offs.validity = nullptr; offs.null_count = 0;
        views.push_back(offs); vi[4 * i] = (int)views.size() - 1;
        if (c.offsets.validity) {   // staged as a bitmap of `rows` bits: it is not read past the last row
            views.push_back(rdf_array{c.offsets.validity, nullptr, c.offsets.offset, rows, 0, RDF_BOOL, c.offsets.mem});
            vi[4 * i + 1] = (int)views.size() - 1;
        }
        views.push_back(rdf_array{c.data.values, nullptr, c.data.offset + lohi[2 * i], (int64_t)lohi[2 * i + 1] - lohi[2 * i], 0, RDF_U8, c.data.mem});
        vi[4 * i + 2] = (int)views.size() - 1;
        if (filter) { views.push_back(mask[i]); vi[4 * i + 3] = (int)views.size() - 1; }
    }
    int idx_view = -1;
    if (take) { views.push_back(*indices); idx_view = (int)views.size() - 1; }
    for (const rdf_array& v : views) in.add(&v);
    size_t pin_used = 0;
    RDF_TRY(in.finish(0, &pin_used));
    size_t pin = (pin_used + 255) & ~(size_t)255;

    std::vector<Utf8Chunk> hc((size_t)nchunks);
    int64_t row_start = 0;
    for (int64_t i = 0; i < nchunks; ++i) {
        Utf8Chunk& u = hc[i];
        memset(&u, 0, sizeof u);
        const DevChunkCol& d_off = in.dev[vi[4 * i]];
        u.offs = (const int32_t*)d_off.values + d_off.offset;
        if (vi[4 * i + 1] >= 0) { u.valid = (const uint8_t*)in.dev[vi[4 * i + 1]].values; u.valid_off = in.dev[vi[4 * i + 1]].offset; }
        const DevChunkCol& d_dat = in.dev[vi[4 * i + 2]];
        u.data = (const uint8_t*)d_dat.values + d_dat.offset - lohi[2 * i];   // data[o] = the byte at value offset o
        if (filter) {
            const DevChunkCol& d_m = in.dev[vi[4 * i + 3]];
            u.mask = (const uint8_t*)d_m.values; u.mask_valid = d_m.validity; u.mask_off = d_m.offset;
        }
        u.rows = chunks[i].offsets.length - 1;
        u.row_start = row_start;
        row_start += u.rows;
        u.lo = lohi[2 * i]; u.hi = lohi[2 * i + 1];
    }
    const int64_t n = take ? indices->length : total_rows;
    void *dtab = nullptr, *pkeep = nullptr, *pblen, *psrc, *pflags, *pbscan, *prscan = nullptr, *perr, *ptot;
    const size_t tb = (size_t)std::max<int64_t>(nchunks, 1) * sizeof(Utf8Chunk);
    RDF_TRY(arena_alloc(tb, &dtab));
    RDF_TRY(arena_alloc((size_t)n * 8, &pblen));
    RDF_TRY(arena_alloc((size_t)n * 8, &psrc));
    RDF_TRY(arena_alloc((size_t)n, &pflags));
    RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &pbscan));
    if (filter) {
        RDF_TRY(arena_alloc((size_t)n * 8, &pkeep));
        RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &prscan));
    }
    RDF_TRY(arena_alloc(16, &perr));
    RDF_TRY(arena_alloc((size_t)nout * 16, &ptot));
    RDF_TRY(pinned_reserve(pin + tb + 64));
    if (nchunks > 0) {
        memcpy(ctx.pinned + pin, hc.data(), (size_t)nchunks * sizeof(Utf8Chunk));
        HIP_TRY(hipMemcpyAsync(dtab, ctx.pinned + pin, (size_t)nchunks * sizeof(Utf8Chunk), hipMemcpyHostToDevice, ctx.stream));
    }
    HIP_TRY(hipMemsetAsync(perr, 0, 16, ctx.stream));

    Utf8Args a;
    memset(&a, 0, sizeof a);
    a.chunks = (const Utf8Chunk*)dtab;
    a.nchunks = nchunks;
    a.op = op;
    a.n = n;
    if (take) {
        const DevChunkCol& d_i = in.dev[idx_view];
        a.idx = d_i.values; a.idx_valid = d_i.validity; a.idx_off = d_i.offset;
        a.idx64 = indices->dtype == RDF_U64;
    }
    a.total_rows = total_rows;
    a.pos = (int32_t)std::min<int64_t>(pos, INT32_MAX);
    a.len = (int32_t)std::min<int64_t>(len, INT32_MAX);
    a.keep = (int64_t*)pkeep;
    a.blen = (int64_t*)pblen;
    a.src = (uint64_t*)psrc;
    a.flags = (uint8_t*)pflags;
    a.bscan = (const int64_t*)pbscan;
    a.rscan = (const int64_t*)prscan;
    a.err = (uint32_t*)perr;
    a.tot = (int64_t*)ptot;
    a.nout = nout;
    KernelTimer kt;
    ctx.last_kernel = "utf8_span_kernel + utf8_copy_kernel";
    HIP_TRY(launch_utf8_span(a, ctx.stream));
    HIP_TRY(launch_scan(a.blen, (int64_t*)pbscan, n, (int64_t*)pbscan + n + 1, ctx.stream));
    if (filter) HIP_TRY(launch_scan(a.keep, (int64_t*)prscan, n, (int64_t*)prscan + n + 1, ctx.stream));
    HIP_TRY(launch_utf8_totals(a, ctx.stream));
    const size_t totb = (size_t)nout * 16;
    size_t pin_r = (pin + tb + 63) & ~(size_t)63;
    RDF_TRY(pinned_reserve(pin_r + totb + 64));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_r, ptot, totb, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_r + totb, perr, 4, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    std::vector<int64_t> tot((size_t)nout * 2);
    memcpy(tot.data(), ctx.pinned + pin_r, totb);
    uint32_t err = 0;
    memcpy(&err, ctx.pinned + pin_r + totb, 4);
    if (err) return fail(RDF_COMPUTE_ERROR, "%s: index out of bounds (%lld rows)", fn, (long long)total_rows);

    // ---- the sizing rule: every length reported, nothing written unless every chunk fits
    bool fits = true;
    for (int64_t o = 0; o < nout; ++o)
        if (tot[2 * o] > INT32_MAX)
            return fail(RDF_COMPUTE_ERROR, "%s: output %lld holds %lld bytes, beyond the Int32 offsets", fn, (long long)o, (long long)tot[2 * o]);
    for (int64_t o = 0; o < nout; ++o) {
        out_data[o].length = tot[2 * o];
        out_offsets[o].length = tot[2 * o + 1] + 1;
        if (out_data[o].capacity < tot[2 * o] || out_offsets[o].capacity < tot[2 * o + 1] + 1) fits = false;
    }
    if (!fits) return fail(RDF_MEMORY_ERROR, "%s: output capacity too small (the needed lengths are in out_data[i].length / out_offsets[i].length)", fn);

    // ---- write
    Region outr;
    std::vector<int> oi((size_t)nout * 3, -1);
    if (mem == RDF_MEM_HOST) {
        for (int64_t o = 0; o < nout; ++o) {
            const int64_t rows = tot[2 * o + 1], bytes = tot[2 * o];
            oi[3 * o] = outr.add(out_offsets[o].values, (size_t)(rows + 1) * 4);
            if (out_offsets[o].validity && rows > 0) oi[3 * o + 1] = outr.add(out_offsets[o].validity, (size_t)((rows + 7) / 8));
            if (bytes > 0) oi[3 * o + 2] = outr.add(out_data[o].values, (size_t)bytes);
        }
        RDF_TRY(outr.layout());
    }
    std::vector<Utf8OutChunk> ho((size_t)nout);
    int64_t orow = 0, obyte = 0, otile = 0;
    for (int64_t o = 0; o < nout; ++o) {
        Utf8OutChunk& u = ho[o];
        u.rows = tot[2 * o + 1];
        u.bytes = tot[2 * o];
        if (mem == RDF_MEM_HOST) {
            u.offs = (int32_t*)outr.ptr(oi[3 * o]);
            u.valid = oi[3 * o + 1] >= 0 ? (uint8_t*)outr.ptr(oi[3 * o + 1]) : nullptr;
            u.data = oi[3 * o + 2] >= 0 ? (uint8_t*)outr.ptr(oi[3 * o + 2]) : nullptr;
        } else {
            u.offs = (int32_t*)out_offsets[o].values;
            u.valid = u.rows > 0 ? out_offsets[o].validity : nullptr;
            u.data = (uint8_t*)out_data[o].values;
        }
        u.row_start = orow;
        u.byte_start = obyte;
        u.tile_start = otile;
        orow += u.rows;
        obyte += u.bytes;
        otile += (u.bytes + kUtf8CopyTile - 1) / kUtf8CopyTile;
    }
    const size_t ob = (size_t)nout * sizeof(Utf8OutChunk);
    void *douts, *posrc, *poflags, *pnulls;
    RDF_TRY(arena_alloc(ob, &douts));
    RDF_TRY(arena_alloc((size_t)orow * 8, &posrc));
    RDF_TRY(arena_alloc((size_t)orow, &poflags));
    RDF_TRY(arena_alloc((size_t)nout * 8, &pnulls));
    void* ptiles;
    RDF_TRY(arena_alloc((size_t)otile * 8 + 8, &ptiles));
    size_t pin_o = (pin_r + totb + 64 + 63) & ~(size_t)63;
    RDF_TRY(pinned_reserve(pin_o + ob + (size_t)nout * 8 + 64));
    memcpy(ctx.pinned + pin_o, ho.data(), ob);
    HIP_TRY(hipMemcpyAsync(douts, ctx.pinned + pin_o, ob, hipMemcpyHostToDevice, ctx.stream));
    HIP_TRY(hipMemsetAsync(pnulls, 0, (size_t)nout * 8, ctx.stream));
    a.outs = (const Utf8OutChunk*)douts;
    a.ntiles = otile;
    a.osrc = (uint64_t*)posrc;
    a.oflags = (uint8_t*)poflags;
    a.tile_row = (int64_t*)ptiles;
    a.null_counts = (unsigned long long*)pnulls;
    HIP_TRY(launch_utf8_write(a, ctx.stream));
    kt.stop();
    const size_t pin_n = (pin_o + ob + 63) & ~(size_t)63;
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_n, pnulls, (size_t)nout * 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    std::vector<int64_t> nulls((size_t)nout);
    memcpy(nulls.data(), ctx.pinned + pin_n, (size_t)nout * 8);
    if (mem == RDF_MEM_HOST) {
        RDF_TRY(pinned_reserve(outr.small_bytes));   // (inputs copied directly leave the staging buffer smaller than the packed outputs)
        RDF_TRY(outr.download(0));
    }
    for (int64_t o = 0; o < nout; ++o) {
        out_offsets[o].null_count = nulls[o];
        out_data[o].null_count = 0;
    }
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_utf8_filter(const rdf_utf8_array* chunks, const rdf_array* mask, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_run(UTF8_FILTER, chunks, nchunks, mask, nullptr, 0, 0, out_offsets, out_data, "utf8_filter");
}
rdf_status rdf_utf8_take(const rdf_utf8_array* chunks, int64_t nchunks, const rdf_array* indices, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_run(UTF8_TAKE, chunks, nchunks, nullptr, indices, 0, 0, out_offsets, out_data, "utf8_take");
}
rdf_status rdf_utf8_trim(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_run(UTF8_TRIM, chunks, nchunks, nullptr, nullptr, 0, 0, out_offsets, out_data, "utf8_trim");
}
rdf_status rdf_utf8_ltrim(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_run(UTF8_LTRIM, chunks, nchunks, nullptr, nullptr, 0, 0, out_offsets, out_data, "utf8_ltrim");
}
rdf_status rdf_utf8_rtrim(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_run(UTF8_RTRIM, chunks, nchunks, nullptr, nullptr, 0, 0, out_offsets, out_data, "utf8_rtrim");
}
rdf_status rdf_utf8_substring(const rdf_utf8_array* chunks, int64_t nchunks, int64_t pos, int64_t len, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_run(UTF8_SUBSTRING, chunks, nchunks, nullptr, nullptr, pos, len, out_offsets, out_data, "utf8_substring");
}
rdf_status rdf_utf8_lower(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_run(UTF8_LOWER, chunks, nchunks, nullptr, nullptr, 0, 0, out_offsets, out_data, "utf8_lower");
}
rdf_status rdf_utf8_upper(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data) {
    return utf8_run(UTF8_UPPER, chunks, nchunks, nullptr, nullptr, 0, 0, out_offsets, out_data, "utf8_upper");
}

}  // extern "C"
