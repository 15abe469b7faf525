// rdf_capi_collect.inc — host side of rdf_groupby_collect (collect_list / collect_set per group) and rdf_list_explode
// (kernels: rdf_collect.hip, argument blocks: rdf_collect.h); textually included by rdf_capi.cpp after
// rdf_capi_group_sorted.inc.  Collect runs rdf_window's device front unchanged — SET with the value as the one order key,
// exactly as rdf_groupby_sorted does, LIST with the value as a passenger column — and compacts the item list the front
// leaves (count per tile, launch_scan, emit; count and scan are skipped when no value chunk carries validity).  Explode
// counts per list row, scans, and expands from the output side.

namespace {

void collect_all_valid(rdf_out* o, int64_t len, int32_t mem, hipStream_t s) {
    if (!o || !o->validity || len <= 0) return;
    if (mem == RDF_MEM_HOST) memset(o->validity, 0xFF, (size_t)((len + 7) / 8));
    else (void)hipMemsetAsync(o->validity, 0xFF, (size_t)((len + 7) / 8), s);
}

}  // namespace

rdf_status rdf_groupby_collect(const rdf_sort_key* group_by, int32_t ngroup, const rdf_sort_key* value, int64_t nchunks,
                               int32_t kind, rdf_out* out_group_rows, rdf_out* out_offsets, rdf_out* out_child_rows,
                               rdf_out* out_values, int64_t* out_groups, int64_t* out_elements) {
    // ---- everything that can be refused is refused before any device work
    const char* fn = "groupby_collect";
    if (!out_groups || !out_elements) return fail(RDF_INVALID_ARGUMENT, "%s: null out_groups / out_elements", fn);
    if (kind != RDF_COLLECT_LIST && kind != RDF_COLLECT_SET) return fail(RDF_INVALID_ARGUMENT, "%s: unknown kind %d", fn, kind);
    if (ngroup < 0 || ngroup > RDF_MAX_GROUP_KEYS) return fail(RDF_INVALID_ARGUMENT, "%s: 0 .. %d grouping keys", fn, RDF_MAX_GROUP_KEYS);
    if (ngroup > 0 && !group_by) return fail(RDF_INVALID_ARGUMENT, "%s: null key list", fn);
    if (!value) return fail(RDF_INVALID_ARGUMENT, "%s: null value column", fn);
    if (nchunks < 1) return fail(RDF_INVALID_ARGUMENT, "%s: bad arguments", fn);
    const bool set = kind == RDF_COLLECT_SET;
    const int ncols = ngroup + 1;
    WinFront wf;
    wf.nkeys = set ? ncols : ngroup;
    wf.nextra = set ? 0 : 1;
    wf.keys.resize((size_t)ncols);
    for (int k = 0; k < ncols; ++k) {
        wf.keys[k] = k < ngroup ? group_by[k] : *value;
        wf.keys[k].options = rdf_sort_options{0, 0};
    }
    bool any_utf8 = false;
    RDF_TRY(lexsort_check_keys(wf.keys.data(), ncols, nchunks, fn, &wf.mem, &any_utf8));
    const bool value_utf8 = value->utf8 != nullptr;
    const int vdtype = value_utf8 ? RDF_U8 : value->values[0].dtype;
    bool value_nullable = false;
    for (int64_t c = 0; c < nchunks; ++c) value_nullable |= (value->values ? value->values[c].validity : value->utf8[c].offsets.validity) != nullptr;
    if (out_values && value_utf8) return fail(RDF_INVALID_ARGUMENT, "%s: out_values of a Utf8 value column (gather the child with rdf_utf8_take)", fn);
    if (out_group_rows && out_group_rows->dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "%s: group rows are UInt32", fn);
    if (out_offsets && out_offsets->dtype != RDF_I32) return fail(RDF_INVALID_ARGUMENT, "%s: offsets are Int32", fn);
    if (out_child_rows && out_child_rows->dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "%s: child rows are UInt32", fn);
    if (out_values && out_values->dtype != vdtype) return fail(RDF_INVALID_ARGUMENT, "%s: out_values has the value's dtype", fn);
    const int32_t mem = wf.mem;
    rdf_out* const all_outs[4] = {out_group_rows, out_offsets, out_child_rows, out_values};
    for (rdf_out* o : all_outs)
        if (o) RDF_TRY(check_out_mem(o, 1, mem));
    wf.nch = nchunks;
    RDF_TRY(lexsort_row_starts(wf.keys.data(), ncols, nchunks, fn, wf.row_start));
    const int64_t n = wf.n = wf.row_start[(size_t)nchunks];
    for (rdf_out* o : all_outs)
        if (o && n > 0 && o->capacity > 0 && !o->values) return fail(RDF_INVALID_ARGUMENT, "%s: null output buffer", fn);
    auto set_lengths = [&](int64_t g, int64_t e, bool any) {
        *out_groups = g;
        *out_elements = e;
        if (out_group_rows) { out_group_rows->length = g; out_group_rows->null_count = 0; }
        if (out_offsets) { out_offsets->length = any ? g + 1 : 0; out_offsets->null_count = 0; }
        if (out_child_rows) { out_child_rows->length = e; out_child_rows->null_count = 0; }
        if (out_values) { out_values->length = e; out_values->null_count = 0; }
    };
    if (n == 0) { set_lengths(0, 0, false); return RDF_OK; }   // nothing is written: no offsets either

    // ---- the order, then the group (and pair) structure: rdf_window's front.  A Utf8 passenger rides as its Int32 offsets —
    // only its validity is read — and LIST over all rows as one group needs neither sort nor flags.
    std::vector<rdf_array> passenger;
    if (!set && value_utf8) {
        passenger.resize((size_t)nchunks);
        for (int64_t c = 0; c < nchunks; ++c) {
            const rdf_array& o = value->utf8[c].offsets;
            passenger[(size_t)c] = rdf_array{o.values, o.validity, o.offset, o.length - 1, o.null_count, RDF_I32, o.mem};
        }
        wf.keys[(size_t)ngroup] = rdf_sort_key{passenger.data(), nullptr, rdf_sort_options{0, 0}};
    }
    const bool one_group_list = !set && ngroup == 0;
    if (one_group_list) {
        RDF_TRY(ensure_ready());
        arena_begin();
        RDF_TRY(lexsort_keys_to_device(wf.keys.data(), ncols, nchunks, mem, wf.row_start, fn, wf.pin_off, wf.d));
        wf.d_row_start = wf.d.tb.dev_at<int64_t>(wf.d.o_rs);
        wf.kt.reset(new KernelTimer());
    } else {
        RDF_TRY(window_front_device(fn, ngroup, wf));
    }
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    const size_t pin_off = wf.pin_off;
    RDF_TRY(pinned_reserve(pin_off + 64));

    CollectArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.scan = wf.scan;
    ca.perm = wf.perm;
    if (set && value_utf8) ca.vutf8 = wf.d.ucols[ngroup].d_chunks;
    else ca.vchunks = wf.d.tb.dev_at<DevChunkCol>(wf.d.o_ch) + (size_t)ngroup * nchunks;
    ca.row_start = wf.d_row_start;
    ca.nchunks = nchunks;
    ca.esize = value_utf8 ? 0 : dtype_size(vdtype);
    ca.canon = set && vdtype == RDF_F32 && !value_utf8 ? 4 : set && vdtype == RDF_F64 && !value_utf8 ? 8 : 0;
    ca.nullable = value_nullable ? 1 : 0;

    // ---- G, D and E in one small copy.  With validity the count pass parks the front's total next to the tile scan's.
    int64_t G = 1, D = n, E = n;
    uint64_t total = 0;
    const int64_t* tile_base = nullptr;
    if (value_nullable) {
        // SET: the host does not know D yet; the count pass reads it from the front's total and walks the ceil(n / tile) tiles
        // a head list can have at most — the tiles past the last head count 0, and the tile numbering is the emit pass's.
        ca.m = n;
        ca.m_dev = set ? wf.scan + n : nullptr;
        ca.gstart = set ? wf.gstart : nullptr;
        const int64_t tiles = collect_tiles(n);
        void *pcounts, *ptscan, *pscratch;
        RDF_TRY(arena_alloc((size_t)tiles * 8, &pcounts));
        RDF_TRY(arena_alloc((size_t)(tiles + 2) * 8, &ptscan));
        RDF_TRY(arena_alloc((size_t)scan_scratch_words(tiles) * 8, &pscratch));
        ca.tile_counts = (int64_t*)pcounts;
        ca.front_total = one_group_list ? nullptr : wf.scan + n;
        ca.front_total_out = (int64_t*)ptscan + tiles + 1;
        HIP_TRY(launch_collect_count(ca, s));
        HIP_TRY(launch_scan((const int64_t*)pcounts, (int64_t*)ptscan, tiles, (int64_t*)pscratch, s));
        HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, (int64_t*)ptscan + tiles, 16, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        memcpy(&E, ctx.pinned + pin_off, 8);
        memcpy(&total, ctx.pinned + pin_off + 8, 8);
        tile_base = (const int64_t*)ptscan;
    } else if (!one_group_list) {
        HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, wf.scan + n, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        memcpy(&total, ctx.pinned + pin_off, 8);
    }
    if (!one_group_list) {
        G = (int64_t)(total >> 32);
        D = (int64_t)(uint32_t)total;
        if (!value_nullable) E = set ? D : n;
    }
    if (G < 1 || D < G || D > n || E < 0 || E > (set ? D : n)) {
        wf.kt->stop();
        return fail(RDF_COMPUTE_ERROR, "internal: %s: %lld groups, %lld pairs, %lld elements over %lld rows", fn, (long long)G, (long long)D, (long long)E, (long long)n);
    }
    set_lengths(G, E, true);
    if (E > INT32_MAX) {
        wf.kt->stop();
        return fail(RDF_COMPUTE_ERROR, "%s: %lld elements overflow the Int32 offsets", fn, (long long)E);
    }
    const bool fits = (!out_group_rows || out_group_rows->capacity >= G) && (!out_offsets || out_offsets->capacity >= G + 1) &&
                      (!out_child_rows || out_child_rows->capacity >= E) && (!out_values || out_values->capacity >= E);
    if (!fits) {
        wf.kt->stop();
        return fail(RDF_MEMORY_ERROR, "output capacity too small (the counts are in *out_groups, *out_elements and every length)");
    }
    const std::string front_kernels = one_group_list ? std::string() : wf.sort_kernels + "win_flags_kernel + win_starts_kernel + ";
    const std::string count_kernels = value_nullable ? "collect_count_kernel + " : "";
    if (!out_group_rows && !out_offsets && !out_child_rows && !out_values) {   // the count-only call
        wf.kt->stop();
        ctx.last_kernel = front_kernels + count_kernels;
        if (ctx.last_kernel.size() >= 3) ctx.last_kernel.resize(ctx.last_kernel.size() - 3);
        return RDF_OK;
    }

    // ---- emit: host outputs are written on the device and copied back
    ca.m = set ? D : n;
    ca.m_dev = nullptr;
    ca.gstart = set ? wf.gstart : nullptr;
    ca.tile_base = tile_base;
    ca.groups = G;
    const size_t es = (size_t)(value_utf8 ? 1 : dtype_size(vdtype));
    void *d_rows = nullptr, *d_offs = nullptr, *d_child = nullptr, *d_vals = nullptr;
    if (out_group_rows) { d_rows = out_group_rows->values; if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)G * 4, &d_rows)); }
    if (out_offsets) { d_offs = out_offsets->values; if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)(G + 1) * 4, &d_offs)); }
    if (out_child_rows) { d_child = out_child_rows->values; if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)E * 4 + 8, &d_child)); }
    if (out_values) { d_vals = out_values->values; if (mem == RDF_MEM_HOST) RDF_TRY(arena_alloc((size_t)E * es + 8, &d_vals)); }
    ca.group_rows = set ? nullptr : (uint32_t*)d_rows;     // SET: a group starts with its smallest VALUE, not its first row
    ca.offsets = (int32_t*)d_offs;
    ca.child_rows = (uint32_t*)d_child;
    ca.values = d_vals;
    if (ca.group_rows || ca.offsets || ca.child_rows || ca.values) HIP_TRY(launch_collect_emit(ca, s));
    int levels = 0;
    if (set && out_group_rows) {   // the first row of every group: rdf_groupby_sorted's fold over the heads, no calls
        GrpFoldArgs fa;
        memset(&fa, 0, sizeof fa);
        fa.scan = wf.scan;
        fa.gstart = wf.gstart;
        fa.perm = wf.perm;
        fa.row_start = wf.d_row_start;
        fa.nchunks = nchunks;
        fa.vdtype = RDF_U8;
        fa.groups = G;
        fa.group_rows = (uint32_t*)d_rows;
        int64_t m = D;
        const GrpState* in = nullptr;
        for (;; ++levels) {
            fa.level = levels;
            fa.in = in;
            fa.m = m;
            fa.part = nullptr;
            const int64_t next = 2 * grp_tiles(m);
            if (m > kGrpTile) {
                void* pp;
                RDF_TRY(arena_alloc((size_t)next * sizeof(GrpState), &pp));
                fa.part = (GrpState*)pp;
            }
            HIP_TRY(launch_grp_fold(fa, s));
            if (!fa.part) break;
            in = fa.part;
            m = next;
        }
        ++levels;
    }
    wf.kt->stop();

    // ---- results to the caller
    if (mem == RDF_MEM_HOST) {
        if (out_group_rows) HIP_TRY(hipMemcpyAsync(out_group_rows->values, d_rows, (size_t)G * 4, hipMemcpyDeviceToHost, s));
        if (out_offsets) HIP_TRY(hipMemcpyAsync(out_offsets->values, d_offs, (size_t)(G + 1) * 4, hipMemcpyDeviceToHost, s));
        if (out_child_rows && E > 0) HIP_TRY(hipMemcpyAsync(out_child_rows->values, d_child, (size_t)E * 4, hipMemcpyDeviceToHost, s));
        if (out_values && E > 0) HIP_TRY(hipMemcpyAsync(out_values->values, d_vals, (size_t)E * es, hipMemcpyDeviceToHost, s));
    }
    collect_all_valid(out_group_rows, G, mem, s);
    collect_all_valid(out_offsets, G + 1, mem, s);
    collect_all_valid(out_child_rows, E, mem, s);
    collect_all_valid(out_values, E, mem, s);
    HIP_TRY(hipStreamSynchronize(s));
    ctx.last_kernel = front_kernels + count_kernels + "collect_emit_kernel" + (levels ? " + " + std::to_string(levels) + " x grp_fold_kernel" : std::string());
    return RDF_OK;
}

rdf_status rdf_list_explode(const rdf_list_array* list, int32_t outer, rdf_out* out_parent_rows, rdf_out* out_child_index,
                            rdf_out* out_pos, int64_t* out_rows) {
    // ---- everything that can be refused is refused before any device work
    const char* fn = "explode";
    if (!list || !out_rows) return fail(RDF_INVALID_ARGUMENT, "%s: null argument", fn);
    if (list->offsets.dtype != RDF_I32) return fail(RDF_INVALID_ARGUMENT, "%s: value_offsets must be Int32", fn);
    if (list->offsets.length < 1) return fail(RDF_INVALID_ARGUMENT, "%s: value_offsets hold rows + 1 entries", fn);
    const int64_t n = list->offsets.length - 1;
    if (n >= (int64_t)1 << 32) return fail(RDF_INVALID_ARGUMENT, "%s: UInt32 row indices cap a call at 2^32-1 list rows", fn);
    int32_t mem = -1;
    RDF_TRY(check_mem(&list->offsets, 1, &mem));
    if (out_parent_rows && out_parent_rows->dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "%s: parent rows are UInt32", fn);
    if (out_child_index && out_child_index->dtype != RDF_U32) return fail(RDF_INVALID_ARGUMENT, "%s: child indices are UInt32", fn);
    if (out_pos && out_pos->dtype != RDF_I32) return fail(RDF_INVALID_ARGUMENT, "%s: positions are Int32", fn);
    if (outer && ((out_child_index && !out_child_index->validity) || (out_pos && !out_pos->validity)))
        return fail(RDF_INVALID_ARGUMENT, "%s: outer needs a validity bitmap for the child indices and the positions", fn);
    rdf_out* const all_outs[3] = {out_parent_rows, out_child_index, out_pos};
    for (rdf_out* o : all_outs) {
        if (!o) continue;
        RDF_TRY(check_out_mem(o, 1, mem));
        if (n > 0 && o->capacity > 0 && !o->values) return fail(RDF_INVALID_ARGUMENT, "%s: null output buffer", fn);
    }
    auto set_lengths = [&](int64_t r) {
        *out_rows = r;
        for (rdf_out* o : all_outs)
            if (o) { o->length = r; o->null_count = 0; }
    };
    if (n == 0) { set_lengths(0); return RDF_OK; }

    // ---- count per list row, scan, the total back
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    const hipStream_t s = ctx.stream;
    arena_begin();
    size_t pin_off = 0, used = 0;
    // value_offsets (n + 1 entries) and the list validity (n bits) are staged as two arrays: the bitmap is not read past bit n
    rdf_array offs = list->offsets, lv = list->offsets;
    offs.length = n + 1; offs.validity = nullptr; offs.null_count = 0;
    lv.values = list->offsets.validity; lv.validity = nullptr; lv.dtype = RDF_BOOL; lv.length = n; lv.null_count = 0;
    InputStager in;
    in.add(&offs);
    if (list->offsets.validity) in.add(&lv);
    RDF_TRY(in.finish(pin_off, &used));
    pin_off += (used + 255) & ~(size_t)255;
    RDF_TRY(pinned_reserve(pin_off + 64));
    void *pcounts, *pstart, *pnulls;
    RDF_TRY(arena_alloc((size_t)n * 8, &pcounts));
    RDF_TRY(arena_alloc((size_t)(n + 2 + scan_scratch_words(n)) * 8, &pstart));
    RDF_TRY(arena_alloc(8, &pnulls));
    HIP_TRY(hipMemsetAsync(pnulls, 0, 8, s));
    ExplodeArgs ea;
    memset(&ea, 0, sizeof ea);
    ea.offsets = in.dev[0];
    if (list->offsets.validity) ea.offsets.validity = (const uint8_t*)in.dev[1].values;   // same bit offset as the value_offsets by construction
    ea.n = n;
    ea.outer = outer ? 1 : 0;
    ea.counts = (int64_t*)pcounts;
    KernelTimer kt;
    HIP_TRY(launch_explode_count(ea, s));
    HIP_TRY(launch_scan((const int64_t*)pcounts, (int64_t*)pstart, n, (int64_t*)pstart + n + 1, s));
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, (int64_t*)pstart + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int64_t R = 0;
    memcpy(&R, ctx.pinned + pin_off, 8);
    if (R < 0) { kt.stop(); return fail(RDF_COMPUTE_ERROR, "internal: %s: %lld output rows", fn, (long long)R); }
    set_lengths(R);
    bool fits = true;
    for (rdf_out* o : all_outs) fits &= !o || o->capacity >= R;
    if (!fits) {
        kt.stop();
        return fail(RDF_MEMORY_ERROR, "output capacity too small (the row count is in *out_rows and every length)");
    }
    if ((!out_parent_rows && !out_child_index && !out_pos) || R == 0) {   // the count-only call, or nothing to write
        kt.stop();
        ctx.last_kernel = "explode_count_kernel";
        return RDF_OK;
    }

    // ---- expansion, driven by the output
    const bool host = mem == RDF_MEM_HOST;
    void *d_parent = nullptr, *d_child = nullptr, *d_pos = nullptr, *d_vbytes = nullptr, *d_words = nullptr;
    if (out_parent_rows) { d_parent = out_parent_rows->values; if (host) RDF_TRY(arena_alloc((size_t)R * 4, &d_parent)); }
    if (out_child_index) { d_child = out_child_index->values; if (host) RDF_TRY(arena_alloc((size_t)R * 4, &d_child)); }
    if (out_pos) { d_pos = out_pos->values; if (host) RDF_TRY(arena_alloc((size_t)R * 4, &d_pos)); }
    const bool masked = outer && (out_child_index || out_pos);
    if (masked) {
        RDF_TRY(arena_alloc((size_t)R, &d_vbytes));
        RDF_TRY(arena_alloc((size_t)((R + 63) / 64) * 8, &d_words));   // whole words here, the caller's bitmaps get their bytes
    }
    ea.start = (const int64_t*)pstart;
    ea.rows = R;
    ea.parent_rows = (uint32_t*)d_parent;
    ea.child_index = (uint32_t*)d_child;
    ea.pos = (int32_t*)d_pos;
    ea.vbytes = (uint8_t*)d_vbytes;
    ea.nulls = masked ? (unsigned long long*)pnulls : nullptr;
    HIP_TRY(launch_explode_expand(ea, s));
    if (masked) HIP_TRY(launch_win_pack((const uint8_t*)d_vbytes, R, (uint64_t*)d_words, s));
    kt.stop();

    // ---- results to the caller
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t vlen = (size_t)((R + 7) / 8);
    HIP_TRY(hipMemcpyAsync(ctx.pinned + pin_off, pnulls, 8, hipMemcpyDeviceToHost, s));
    if (host) {
        if (out_parent_rows) HIP_TRY(hipMemcpyAsync(out_parent_rows->values, d_parent, (size_t)R * 4, kind, s));
        if (out_child_index) HIP_TRY(hipMemcpyAsync(out_child_index->values, d_child, (size_t)R * 4, kind, s));
        if (out_pos) HIP_TRY(hipMemcpyAsync(out_pos->values, d_pos, (size_t)R * 4, kind, s));
    }
    if (masked) {
        if (out_child_index) HIP_TRY(hipMemcpyAsync(out_child_index->validity, d_words, vlen, kind, s));
        if (out_pos) HIP_TRY(hipMemcpyAsync(out_pos->validity, d_words, vlen, kind, s));
    } else {
        collect_all_valid(out_child_index, R, mem, s);
        collect_all_valid(out_pos, R, mem, s);
    }
    collect_all_valid(out_parent_rows, R, mem, s);
    HIP_TRY(hipStreamSynchronize(s));
    unsigned long long nulls = 0;
    memcpy(&nulls, ctx.pinned + pin_off, 8);
    if (masked) {
        if (out_child_index) out_child_index->null_count = (int64_t)nulls;
        if (out_pos) out_pos->null_count = (int64_t)nulls;
    }
    ctx.last_kernel = "explode_count_kernel + explode_expand_kernel";
    return RDF_OK;
}
