// rdf_capi_stream.inc — the batch loop over HOST-resident RecordBatches, streamed; textually included by rdf_capi.cpp.
//
// Evaluate::evaluate walks the frame batch by batch (src/evaluation.rs:66-96) and the frames it walks come out of readers that
// hand over host memory (DataFrame::from_csv / from_arrow, src/dataframe.rs:349-407).  rdf_pipeline over RDF_MEM_HOST arrays
// used to stage the WHOLE frame into HBM and then compute: the link idles while the kernel runs, the kernel waits for the last
// byte, and a frame larger than free HBM cannot run at all.  Above one slab of input an aggregating program is streamed instead:
//
//   * the batch list is cut into slabs of whole batches (a batch longer than a quarter slab is cut on 64-row boundaries:
//     zero-copy slices, src/table.rs:77-95), two slab buffers in HBM;
//   * a helper thread brings slab k + 1 over — column buffers the caller holds in page-locked memory (rdf_host_alloc /
//     rdf_host_register, an Arrow IPC image pinned in place) go straight out of it with one asynchronous copy each, anything
//     else (pageable memory, the readers' 8 KiB batches) is packed into a page-locked staging buffer by a few threads and leaves
//     with ONE copy — on the copy stream, while the calling thread runs the fused kernel over slab k on the compute stream;
//   * the slabs' partial {sum, min, max, count} are folded in slab order, exactly AggregateFunctions' left fold over chunks
//     (src/functions/aggregate.rs:82-93) one level up.
// HBM in use: two slabs, whatever the frame's size.

namespace {

// (StreamItem / StreamSlab / StreamPlan, the planner, DownLayout and bits_append: rdf_stream_plan.h, pure host code)
bool host_pointer_is_pinned(const void* p) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

struct StreamShared {
    std::mutex mu;
    std::condition_variable cv;
    int64_t issued = 0, consumed = 0;
    bool failed = false, stop = false;
    std::string error;
};

// copy a slab into staging buffer `pin` (the small / pageable items, a few threads) and queue its uploads
hipError_t stream_issue(const StreamSlab& s, char* dev, char* pin, hipStream_t copy, hipEvent_t done) {
    if (s.pin_bytes) {
        std::vector<StageItem> st;
        st.reserve(s.items.size());
        size_t big = 0;
        for (const StreamItem& it : s.items) if (!it.direct && it.bytes) { st.push_back(StageItem{it.src, it.bytes, it.pin_off, true}); big += it.bytes; }
        packed_copy(st, pin, true, big);
        hipError_t e = hipMemcpyAsync(dev, pin, s.pin_bytes, hipMemcpyHostToDevice, copy);
        if (e != hipSuccess) return e;
    }
    for (const StreamItem& it : s.items)
        if (it.direct && it.bytes) {
            hipError_t e = hipMemcpyAsync(dev + it.dev_off, it.src, it.bytes, hipMemcpyHostToDevice, copy);
            if (e != hipSuccess) return e;
        }
    return hipEventRecord(done, copy);
}

void agg_fold(rdf_agg_result& t, const rdf_agg_result& p, bool& have) {
    const int dt = t.dtype;
    t.sum_f64 += p.sum_f64;
    t.sum_i64 = (int64_t)((uint64_t)t.sum_i64 + (uint64_t)p.sum_i64);
    t.count += p.count;
    if (!p.is_some) return;
    if (is_float(dt)) {
        // NaN-ignoring like the device fold: a NaN partial never displaces a number
        if (!have || p.min_f64 < t.min_f64 || t.min_f64 != t.min_f64) t.min_f64 = p.min_f64;
        if (!have || p.max_f64 > t.max_f64 || t.max_f64 != t.max_f64) t.max_f64 = p.max_f64;
    } else if (is_unsigned_int(dt)) {
        if (!have || (uint64_t)p.min_i64 < (uint64_t)t.min_i64) t.min_i64 = p.min_i64;
        if (!have || (uint64_t)p.max_i64 > (uint64_t)t.max_i64) t.max_i64 = p.max_i64;
    } else {
        if (!have || p.min_i64 < t.min_i64) t.min_i64 = p.min_i64;
        if (!have || p.max_i64 > t.max_i64) t.max_i64 = p.max_i64;
    }
    have = true;
}

int64_t stream_slab_bytes() { return g_ctx.opt_stream_slab > 0 ? g_ctx.opt_stream_slab : ((int64_t)256 << 20); }

// how many bytes rdf_pipeline would stage for these host arrays
int64_t host_input_bytes(const rdf_array* cols, int32_t ncols, int64_t nchunks) {
    int64_t b = 0;
    for (int64_t i = 0; i < (int64_t)ncols * nchunks; ++i) {
        const rdf_array& a = cols[i];
        if (a.length <= 0) continue;
        b += a.dtype == RDF_BOOL ? (a.length + 7) / 8 : a.length * dtype_size(a.dtype);
        if (a.validity) b += (a.length + 7) / 8;
    }
    return b;
}

// ---- the plan (rdf_stream_plan.h: stream_plan_build) under this thread's slab size and the runtime's word on page-locked memory
rdf_status stream_plan(const rdf_array* cols, int32_t ncols, int64_t nchunks, const char* msg, size_t extra_row_bytes, StreamPlan& plan) {
    int bad_col = 0;
    switch (stream_plan_build(cols, ncols, nchunks, extra_row_bytes, (size_t)stream_slab_bytes(), host_pointer_is_pinned, plan, &bad_col)) {
        case kStreamPlanLengths: return fail(RDF_COMPUTE_ERROR, "%s", msg);
        case kStreamPlanDtypes: return fail(RDF_INVALID_ARGUMENT, "column %d: chunks differ in dtype", bad_col);
        default: break;
    }
    Ctx& ctx = g_ctx;
    ctx.stream_slabs = (int64_t)plan.slabs.size();
    ctx.stream_bytes_staged = ctx.stream_bytes_direct = 0;
    for (const StreamSlab& s : plan.slabs) for (const StreamItem& it : s.items) (it.direct ? ctx.stream_bytes_direct : ctx.stream_bytes_staged) += (int64_t)it.bytes;
    return RDF_OK;
}

// ---- the loop: an uploader thread keeps two slabs ahead of `per_slab(k, slab, views (column-major device arrays), npieces)`,
// which runs on the calling thread with the slab's uploads ordered in front of the compute stream
template <class PerSlab>
rdf_status stream_run(StreamPlan& plan, int32_t ncols, PerSlab&& per_slab) {
    Ctx& ctx = g_ctx;
    std::vector<StreamSlab>& slabs = plan.slabs;
    // buffers: two slabs in HBM, two staging buffers in page-locked memory (kept for the thread's next call)
    if (ctx.sbuf_dev_cap < plan.max_dev + 512) {
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        for (int b = 0; b < 2; ++b) { if (ctx.sbuf_dev[b]) (void)hipFree(ctx.sbuf_dev[b]); ctx.sbuf_dev[b] = nullptr; }
        ctx.sbuf_dev_cap = 0;
        for (int b = 0; b < 2; ++b) {
            hipError_t e = hipMalloc(&ctx.sbuf_dev[b], plan.max_dev + 512);
            if (e != hipSuccess) return fail(RDF_MEMORY_ERROR, "hipMalloc(%zu) for a stream slab failed: %s", plan.max_dev + 512, hipGetErrorString(e));
        }
        ctx.sbuf_dev_cap = plan.max_dev + 512;
    }
    if (plan.max_pin && ctx.sbuf_pin_cap < plan.max_pin + 512) {
        for (int b = 0; b < 2; ++b) { if (ctx.sbuf_pin[b]) (void)hipHostFree(ctx.sbuf_pin[b]); ctx.sbuf_pin[b] = nullptr; }
        ctx.sbuf_pin_cap = 0;
        for (int b = 0; b < 2; ++b) {
            hipError_t e = hipHostMalloc(&ctx.sbuf_pin[b], plan.max_pin + 512, hipHostMallocDefault);
            if (e != hipSuccess) return fail(RDF_MEMORY_ERROR, "hipHostMalloc(%zu) for a stream staging buffer failed: %s", plan.max_pin + 512, hipGetErrorString(e));
        }
        ctx.sbuf_pin_cap = plan.max_pin + 512;
    }
    if (!ctx.copy_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx.copy_stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) if (!ctx.sbuf_ev[b]) HIP_TRY(hipEventCreateWithFlags(&ctx.sbuf_ev[b], hipEventDisableTiming));
    // the uploader: slab k + 1 crosses the link while slab k is computed on
    struct Streaming { Ctx& c; bool was; explicit Streaming(Ctx& c_) : c(c_), was(c_.streaming) { c.streaming = true; } ~Streaming() { c.streaming = was; } } streaming_guard(ctx);
    StreamShared sh;
    const int device = ctx.device;
    hipStream_t copy = ctx.copy_stream;
    char* dev[2] = {(char*)ctx.sbuf_dev[0], (char*)ctx.sbuf_dev[1]};
    char* pin[2] = {(char*)ctx.sbuf_pin[0], (char*)ctx.sbuf_pin[1]};
    hipEvent_t ev[2] = {ctx.sbuf_ev[0], ctx.sbuf_ev[1]};
    std::thread uploader([&]() {
        if (hipSetDevice(device) != hipSuccess) { std::lock_guard<std::mutex> lk(sh.mu); sh.failed = true; sh.error = "hipSetDevice failed in the upload thread"; sh.cv.notify_all(); return; }
        for (int64_t k = 0; k < (int64_t)slabs.size(); ++k) {
            {
                std::unique_lock<std::mutex> lk(sh.mu);
                sh.cv.wait(lk, [&] { return sh.stop || k - sh.consumed < 2; });    // buffer k % 2 is free once slab k - 2 has been computed on
                if (sh.stop) return;
            }
            const hipError_t e = stream_issue(slabs[(size_t)k], dev[k & 1], pin[k & 1], copy, ev[k & 1]);
            std::lock_guard<std::mutex> lk(sh.mu);
            if (e != hipSuccess) { sh.failed = true; sh.error = std::string("upload of a slab: ") + hipGetErrorString(e); sh.cv.notify_all(); return; }
            sh.issued = k + 1;
            sh.cv.notify_all();
        }
    });
    // (on every way out: the thread stopped, and no copy left in flight out of buffers the caller may free once the call has returned)
    struct Joiner { std::thread& t; StreamShared& s; hipStream_t copy; ~Joiner() { { std::lock_guard<std::mutex> lk(s.mu); s.stop = true; } s.cv.notify_all(); if (t.joinable()) t.join(); (void)hipStreamSynchronize(copy); } } joiner{uploader, sh, copy};
    std::vector<rdf_array> views;
    for (int64_t k = 0; k < (int64_t)slabs.size(); ++k) {
        StreamSlab& s = slabs[(size_t)k];
        {
            std::unique_lock<std::mutex> lk(sh.mu);
            sh.cv.wait(lk, [&] { return sh.failed || sh.issued > k; });
            if (sh.failed) return fail(RDF_DEVICE_ERROR, "%s", sh.error.c_str());
        }
        HIP_TRY(hipStreamWaitEvent(ctx.stream, ev[k & 1], 0));
        // the slab's batches as device-resident arrays, column-major like every cols[] argument
        views.resize((size_t)ncols * (size_t)s.npieces);
        char* base = dev[k & 1];
        for (int64_t p = 0; p < s.npieces; ++p)
            for (int kcol = 0; kcol < ncols; ++kcol) {
                const size_t src = (size_t)p * (size_t)ncols + (size_t)kcol;
                rdf_array v = s.views[src];
                v.values = base + s.items[s.values_item[src]].dev_off + s.values_off[src];
                v.validity = s.validity_item[src] == kNoItem ? nullptr : (const uint8_t*)(base + s.items[s.validity_item[src]].dev_off + s.validity_off[src]);
                views[(size_t)kcol * (size_t)s.npieces + (size_t)p] = v;
            }
        const rdf_status st = per_slab(k, s, views.data(), s.npieces);     // returns with the compute stream drained
        if (st != RDF_OK) return st;
        { std::lock_guard<std::mutex> lk(sh.mu); sh.consumed = k + 1; }
        sh.cv.notify_all();
    }
    return RDF_OK;
}

// ---- sink: aggregates.  The slabs' partial {sum, min, max, count} are folded in slab order.
rdf_status pipeline_stream(const ProgramSpec& ps, const rdf_array* cols, int32_t ncols, int64_t nchunks, rdf_agg_result* aggs, const char* msg) {
    RDF_TRY(ensure_ready());
    StreamPlan plan;
    RDF_TRY(stream_plan(cols, ncols, nchunks, msg, 0, plan));
    if (plan.slabs.empty()) {          // nothing but empty batches: the plain path answers
        g_ctx.stream_slabs = 0;
        return run_program(ps, cols, ncols, nchunks, nullptr, aggs, msg);
    }
    rdf_agg_result total[RDF_MAX_VALUES];
    bool have[RDF_MAX_VALUES];
    memset(total, 0, sizeof total);
    for (int v = 0; v < RDF_MAX_VALUES; ++v) have[v] = false;
    RDF_TRY(stream_run(plan, ncols, [&](int64_t k, StreamSlab&, const rdf_array* views, int64_t npieces) -> rdf_status {
        rdf_agg_result part[RDF_MAX_VALUES];
        memset(part, 0, sizeof part);
        RDF_TRY(run_program(ps, views, ncols, npieces, nullptr, part, msg));
        for (int v = 0; v < ps.nvalues; ++v) {
            if (k == 0) total[v].dtype = part[v].dtype;
            agg_fold(total[v], part[v], have[v]);
        }
        return RDF_OK;
    }));
    for (int v = 0; v < ps.nvalues; ++v) {
        if (!is_float(total[v].dtype)) total[v].sum_i64 = (int64_t)h_normalize_int(total[v].dtype, (uint64_t)total[v].sum_i64);
        total[v].is_some = total[v].count > 0;
        aggs[v] = total[v];
    }
    return RDF_OK;
}

// ---- the way back: what a slab's kernel wrote leaves on a third stream while the next slab is computed on and the one after
// that comes in (the link is full duplex).  Two output buffers in HBM, two page-locked staging buffers; destinations the caller
// holds in page-locked memory (>= 256 KiB) are written by the DMA engine directly, everything else lands in staging with one
// copy per slab and is unpacked into the caller's buffers by a helper thread.
struct Downloader {
    Ctx& ctx;
    std::mutex mu;
    std::condition_variable cv;
    std::thread th;
    int64_t submitted = 0, unpacked = 0;
    bool stop = false, failed = false;
    std::string error;
    std::vector<DownItem> pending[2];
    size_t pending_pin[2] = {0, 0};
    std::function<void(int64_t, char*)> on_landed;     // instead of the plain unpack: called by the download thread once slab k's copies are in staging
    explicit Downloader(Ctx& c) : ctx(c) {}
    ~Downloader() {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        if (th.joinable()) th.join();
        if (ctx.d2h_stream) (void)hipStreamSynchronize(ctx.d2h_stream);
    }
    rdf_status begin(size_t max_dev, size_t max_pin) {
        if (ctx.dbuf_dev_cap < max_dev + 512) {
            HIP_TRY(hipStreamSynchronize(ctx.stream));
            if (ctx.d2h_stream) HIP_TRY(hipStreamSynchronize(ctx.d2h_stream));
            for (int b = 0; b < 2; ++b) { if (ctx.dbuf_dev[b]) (void)hipFree(ctx.dbuf_dev[b]); ctx.dbuf_dev[b] = nullptr; }
            ctx.dbuf_dev_cap = 0;
            for (int b = 0; b < 2; ++b) {
                hipError_t e = hipMalloc(&ctx.dbuf_dev[b], max_dev + 512);
                if (e != hipSuccess) return fail(RDF_MEMORY_ERROR, "hipMalloc(%zu) for a stream output slab failed: %s", max_dev + 512, hipGetErrorString(e));
            }
            ctx.dbuf_dev_cap = max_dev + 512;
        }
        if (max_pin && ctx.dbuf_pin_cap < max_pin + 512) {
            if (ctx.d2h_stream) HIP_TRY(hipStreamSynchronize(ctx.d2h_stream));
            for (int b = 0; b < 2; ++b) { if (ctx.dbuf_pin[b]) (void)hipHostFree(ctx.dbuf_pin[b]); ctx.dbuf_pin[b] = nullptr; }
            ctx.dbuf_pin_cap = 0;
            for (int b = 0; b < 2; ++b) {
                hipError_t e = hipHostMalloc(&ctx.dbuf_pin[b], max_pin + 512, hipHostMallocDefault);
                if (e != hipSuccess) return fail(RDF_MEMORY_ERROR, "hipHostMalloc(%zu) for a stream output staging buffer failed: %s", max_pin + 512, hipGetErrorString(e));
            }
            ctx.dbuf_pin_cap = max_pin + 512;
        }
        if (!ctx.d2h_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx.d2h_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) if (!ctx.dbuf_ev[b]) HIP_TRY(hipEventCreateWithFlags(&ctx.dbuf_ev[b], hipEventDisableTiming));
        const int device = ctx.device;
        th = std::thread([this, device]() {
            if (hipSetDevice(device) != hipSuccess) { std::lock_guard<std::mutex> lk(mu); failed = true; error = "hipSetDevice failed in the download thread"; cv.notify_all(); return; }
            for (int64_t k = 0;; ++k) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return stop || submitted > k; });
                    if (submitted <= k) return;          // stop, nothing left
                }
                const hipError_t e = hipEventSynchronize(ctx.dbuf_ev[k & 1]);
                if (e == hipSuccess && on_landed) on_landed(k, (char*)ctx.dbuf_pin[k & 1]);
                else if (e == hipSuccess && pending_pin[k & 1]) {
                    std::vector<StageItem> st;
                    st.reserve(pending[k & 1].size());
                    size_t big = 0;
                    for (const DownItem& it : pending[k & 1]) if (!it.direct && it.bytes) { st.push_back(StageItem{it.dst, it.bytes, it.off, true}); big += it.bytes; }
                    packed_copy(st, (char*)ctx.dbuf_pin[k & 1], false, big);
                }
                std::lock_guard<std::mutex> lk(mu);
                if (e != hipSuccess) { failed = true; error = std::string("download of a slab: ") + hipGetErrorString(e); cv.notify_all(); return; }
                unpacked = k + 1;
                cv.notify_all();
            }
        });
        return RDF_OK;
    }
    char* dev(int64_t k) const { return (char*)ctx.dbuf_dev[k & 1]; }
    // before slab k's kernel may write dev(k): the copies out of it (slab k - 2) have left
    rdf_status before_kernel(int64_t k) {
        if (k >= 2) HIP_TRY(hipStreamWaitEvent(ctx.stream, ctx.dbuf_ev[k & 1], 0));
        return RDF_OK;
    }
    // after slab k's kernel (compute stream drained): queue its copies.  `items`: staged ones occupy [0, pin_bytes) of dev(k).
    rdf_status submit(int64_t k, std::vector<DownItem>&& items, size_t pin_bytes) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return failed || unpacked >= k - 1; });      // staging buffer k % 2 has been unpacked (slab k - 2)
            if (failed) return fail(RDF_DEVICE_ERROR, "%s", error.c_str());
        }
        char* d = dev(k);
        if (pin_bytes) HIP_TRY(hipMemcpyAsync(ctx.dbuf_pin[k & 1], d, pin_bytes, hipMemcpyDeviceToHost, ctx.d2h_stream));
        for (const DownItem& it : items)
            if (it.direct && it.bytes) HIP_TRY(hipMemcpyAsync(it.dst, d + it.off, it.bytes, hipMemcpyDeviceToHost, ctx.d2h_stream));
        HIP_TRY(hipEventRecord(ctx.dbuf_ev[k & 1], ctx.d2h_stream));
        std::lock_guard<std::mutex> lk(mu);
        pending[k & 1] = std::move(items);
        pending_pin[k & 1] = pin_bytes;
        submitted = k + 1;
        cv.notify_all();
        return RDF_OK;
    }
    // slab k has been unpacked (k < 0: nothing to wait for)
    rdf_status wait_unpacked(int64_t k) {
        if (k < 1) return RDF_OK;
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return failed || unpacked >= k; });
        if (failed) return fail(RDF_DEVICE_ERROR, "%s", error.c_str());
        return RDF_OK;
    }
    // copies out of buffers the caller names (items[i].dev_src -> staging + items[i].off), then on_landed(k)
    rdf_status submit_gather(int64_t k, std::vector<DownItem>&& items) {
        RDF_TRY(wait_unpacked(k - 1));
        for (const DownItem& it : items)
            if (it.bytes) HIP_TRY(hipMemcpyAsync((char*)ctx.dbuf_pin[k & 1] + it.off, it.dev_src, it.bytes, hipMemcpyDeviceToHost, ctx.d2h_stream));
        HIP_TRY(hipEventRecord(ctx.dbuf_ev[k & 1], ctx.d2h_stream));
        std::lock_guard<std::mutex> lk(mu);
        pending[k & 1] = std::move(items);
        pending_pin[k & 1] = 0;
        submitted = k + 1;
        cv.notify_all();
        return RDF_OK;
    }
    rdf_status finish(int64_t nslabs) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return failed || unpacked >= nslabs; });
        if (failed) return fail(RDF_DEVICE_ERROR, "%s", error.c_str());
        return RDF_OK;
    }
};


// ---- sink: new columns.  Evaluate::evaluate's Calculate step over a host-resident frame (src/evaluation.rs:66-96): every
// batch in, one new column batch out, both on the host — slab k + 1 comes in and slab k - 1's column leaves while the fused
// kernel runs over slab k.
rdf_status pipeline_stream_store(const ProgramSpec& ps, const rdf_array* cols, int32_t ncols, int64_t nchunks, rdf_out* outs, const char* msg) {
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    if (ps.nvalues != 1) return fail(RDF_INVALID_ARGUMENT, "a stored program has one value");
    const int odt = outs[0].dtype;
    const size_t oes = odt == RDF_BOOL ? 0 : (size_t)dtype_size(odt);
    for (int64_t c = 0; c < nchunks; ++c) {
        if (outs[c].dtype != odt) return fail(RDF_INVALID_ARGUMENT, "output chunks differ in dtype");
        if (outs[c].capacity < cols[c].length) return fail(RDF_INVALID_ARGUMENT, "output chunk %lld holds %lld of %lld rows", (long long)c, (long long)outs[c].capacity, (long long)cols[c].length);
        if (cols[c].length > 0 && !outs[c].values) return fail(RDF_INVALID_ARGUMENT, "output chunk %lld: null values pointer", (long long)c);
    }
    StreamPlan plan;
    RDF_TRY(stream_plan(cols, ncols, nchunks, msg, (odt == RDF_BOOL ? 1 : oes) + 1, plan));
    if (plan.slabs.empty()) {
        ctx.stream_slabs = 0;
        return run_program(ps, cols, ncols, nchunks, outs, nullptr, msg);
    }
    // the largest slab's outputs: values + validity per piece, every item on a 256-byte boundary
    size_t max_out = 0;
    for (const std::vector<PieceOrigin>& o : plan.origin) {
        size_t b = 0;
        for (const PieceOrigin& p : o) b += (((odt == RDF_BOOL ? (size_t)(p.rows + 7) / 8 : (size_t)p.rows * oes) + 16 + 255) & ~(size_t)255) + ((((size_t)(p.rows + 7) / 8) + 16 + 255) & ~(size_t)255);
        max_out = std::max(max_out, b);
    }
    Downloader down(ctx);
    RDF_TRY(down.begin(max_out, max_out));
    for (int64_t c = 0; c < nchunks; ++c) { outs[c].length = cols[c].length; outs[c].null_count = 0; }
    DownLayout lay(host_pointer_is_pinned);
    std::vector<rdf_out> pouts;
    std::vector<size_t> vi, bi;
    RDF_TRY(stream_run(plan, ncols, [&](int64_t k, StreamSlab&, const rdf_array* views, int64_t npieces) -> rdf_status {
        const std::vector<PieceOrigin>& org = plan.origin[(size_t)k];
        lay.reset();
        vi.assign((size_t)npieces, 0); bi.assign((size_t)npieces, kNoItem);
        for (int64_t p = 0; p < npieces; ++p) {
            const PieceOrigin& o = org[(size_t)p];
            rdf_out& dst = outs[o.chunk];
            if (odt == RDF_BOOL) vi[(size_t)p] = lay.add((char*)dst.values + o.row0 / 8, (size_t)(o.rows + 7) / 8, dst.values);
            else vi[(size_t)p] = lay.add((char*)dst.values + (size_t)o.row0 * oes, (size_t)o.rows * oes, dst.values);
            if (dst.validity) bi[(size_t)p] = lay.add((char*)dst.validity + o.row0 / 8, (size_t)(o.rows + 7) / 8, dst.validity);
        }
        lay.close();
        RDF_TRY(down.before_kernel(k));
        char* d = down.dev(k);
        pouts.assign((size_t)npieces, rdf_out{});
        for (int64_t p = 0; p < npieces; ++p) {
            rdf_out& o = pouts[(size_t)p];
            o.values = d + lay.items[vi[(size_t)p]].off;
            o.validity = bi[(size_t)p] == kNoItem ? nullptr : (uint8_t*)(d + lay.items[bi[(size_t)p]].off);
            o.capacity = org[(size_t)p].rows; o.dtype = odt; o.mem = RDF_MEM_DEVICE;
        }
        RDF_TRY(run_program(ps, views, ncols, npieces, pouts.data(), nullptr, msg));
        for (int64_t p = 0; p < npieces; ++p) outs[org[(size_t)p].chunk].null_count += pouts[(size_t)p].null_count;
        std::vector<DownItem> items = lay.copies;
        return down.submit(k, std::move(items), lay.pin);
    }));
    return down.finish((int64_t)plan.slabs.size());
}

// ---- sink: the fused grouped aggregation (rdf_group_pipeline, config C5 / TPC-H Q1) over host-resident batches: the slabs'
// per-group sums and counts are added up in slab order (the same left fold, one level up).
rdf_status group_pipeline_stream(const ProgramSpec& ps, const rdf_array* cols, int32_t ncols, int64_t nchunks, const char* msg) {
    RDF_TRY(ensure_ready());
    StreamPlan plan;
    RDF_TRY(stream_plan(cols, ncols, nchunks, msg, 0, plan));
    if (plan.slabs.empty()) {
        g_ctx.stream_slabs = 0;
        return run_program(ps, cols, ncols, nchunks, nullptr, nullptr, msg);
    }
    const int S = ps.ngroups + 1;
    const size_t slots = (size_t)S * (size_t)ps.nvalues;
    std::vector<rdf_group_result> part(slots), total(slots);
    std::vector<int64_t> prow((size_t)S, 0), trow((size_t)S, 0);
    memset(total.data(), 0, slots * sizeof(rdf_group_result));
    ProgramSpec sps = ps;
    sps.gout = part.data();
    sps.grows = prow.data();
    RDF_TRY(stream_run(plan, ncols, [&](int64_t k, StreamSlab&, const rdf_array* views, int64_t npieces) -> rdf_status {
        RDF_TRY(run_program(sps, views, ncols, npieces, nullptr, nullptr, msg));
        for (size_t i = 0; i < slots; ++i) {
            if (k == 0) total[i].dtype = part[i].dtype;
            total[i].sum_f64 += part[i].sum_f64;
            total[i].sum_i64 = (int64_t)((uint64_t)total[i].sum_i64 + (uint64_t)part[i].sum_i64);
            total[i].count += part[i].count;
        }
        for (int g = 0; g < S; ++g) trow[(size_t)g] += prow[(size_t)g];
        return RDF_OK;
    }));
    for (size_t i = 0; i < slots; ++i) { total[i].is_some = total[i].count > 0; ps.gout[i] = total[i]; }
    if (ps.grows) for (int g = 0; g < S; ++g) ps.grows[g] = trow[(size_t)g];
    return RDF_OK;
}

// ---- sink: DataFrame::filter (src/dataframe.rs:178-189) over host-resident batches, host-resident result.  Per slab the
// batches become a frame (rdf_frame_pin over the upload slab), the frame operator runs (rdf_filter_frame: predicate and
// compaction of every column in one pass where the predicate allows), and the kept rows go back: every output column buffer
// of the slab leaves with ONE copy on the download stream into page-locked staging, and a helper thread appends each batch's
// kept rows (and validity bits) behind what its output chunk already holds.  An output chunk keeps its input batch's identity
// (ChunkedArray::filter, src/table.rs:97-107): chunk c of the result = the kept rows of batch c.

struct FilterUnpack {                      // one slab's way home, run by the download thread
    struct Col { size_t stage_off; const char* dev_base; size_t bytes; const char* vdev_base; size_t vstage_off, vbytes; };
    struct Piece { int64_t chunk, kept, written_before; };
    std::vector<Col> cols;
    std::vector<Piece> pieces;
    std::vector<DevChunkCol> dev;          // [ncols * npieces] of the output frame
    int ncols = 0;
};

rdf_status filter_stream(const rdf_expr_node* nodes, int32_t nnodes, int32_t root, const rdf_array* cols, int32_t ncols, int64_t nchunks, rdf_out* outs) {
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    const char* msg = "columns of a batch differ in length";
    int es[kMaxFrameCols];
    for (int k = 0; k < ncols; ++k) {
        const int dt = cols[(int64_t)k * nchunks].dtype;
        if (!is_numeric(dt)) return fail(RDF_INVALID_ARGUMENT, "filter_pipeline: column %d: numeric columns only (dtype %d)", k, dt);
        es[k] = dtype_size(dt);
        for (int64_t c = 0; c < nchunks; ++c) {
            const rdf_out& o = outs[(int64_t)k * nchunks + c];
            const rdf_array& a = cols[(int64_t)k * nchunks + c];
            if (o.mem != RDF_MEM_HOST) return fail(RDF_INVALID_ARGUMENT, "filter_pipeline: host-resident outputs (RDF_MEM_HOST)");
            if (o.dtype != dt) return fail(RDF_INVALID_ARGUMENT, "filter_pipeline: output %d has dtype %d, its column %d", k, o.dtype, dt);
            if (o.capacity < a.length) return fail(RDF_INVALID_ARGUMENT, "filter_pipeline: output chunk holds %lld of %lld rows", (long long)o.capacity, (long long)a.length);
            if (a.length > 0 && !o.values) return fail(RDF_INVALID_ARGUMENT, "filter_pipeline: null values pointer");
            if (a.validity && a.length > 0 && !o.validity) return fail(RDF_INVALID_ARGUMENT, "filter_pipeline: column %d carries a validity bitmap, its output has none", k);
        }
    }
    for (int64_t i = 0; i < (int64_t)ncols * nchunks; ++i) { outs[i].length = 0; outs[i].null_count = 0; }
    StreamPlan plan;
    RDF_TRY(stream_plan(cols, ncols, nchunks, msg, 0, plan));
    if (plan.slabs.empty()) { ctx.stream_slabs = 0; return RDF_OK; }
    // staging: the output frame's column buffers are as long as the slab's input columns at most (+ 64-row padding per batch)
    size_t max_stage = 0;
    for (size_t si = 0; si < plan.slabs.size(); ++si) {
        size_t b = 0;
        for (const PieceOrigin& o : plan.origin[si]) for (int k = 0; k < ncols; ++k) b += (size_t)((o.rows + 63) / 64 * 64) * (size_t)es[k] + (size_t)((o.rows + 63) / 64 * 8) + 64;
        max_stage = std::max(max_stage, b + 4096 * (size_t)ncols);
    }
    std::vector<int64_t> written((size_t)nchunks, 0);
    std::vector<std::vector<int64_t>> nulls((size_t)ncols, std::vector<int64_t>((size_t)nchunks, 0));
    rdf_frame* live[2] = {nullptr, nullptr};
    std::shared_ptr<FilterUnpack> unpack[2];
    struct Cleanup { rdf_frame** l; ~Cleanup() { for (int b = 0; b < 2; ++b) if (l[b]) (void)rdf_frame_release(l[b]); } } cleanup{live};
    Downloader down(ctx);          // (declared last: destroyed first — its thread and its copies end before the frames and tables above go)
    RDF_TRY(down.begin(256, max_stage));
    double t_phase_unpack = 0;
    // the download thread's per-slab work: after the copies have landed, append every batch's kept rows behind its output chunk
    down.on_landed = [&](int64_t k, char* stage) {
        const double tl0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
        struct Lap { double& acc; double t0; ~Lap() { acc += std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0; } } lapl{t_phase_unpack, tl0};
        const FilterUnpack& u = *unpack[k & 1];
        const int64_t np = (int64_t)u.pieces.size();
        std::vector<StageItem> st;
        st.reserve((size_t)np * (size_t)u.ncols);
        size_t big = 0;
        for (int kc = 0; kc < u.ncols; ++kc) {
            const FilterUnpack::Col& c = u.cols[(size_t)kc];
            for (int64_t p = 0; p < np; ++p) {
                const FilterUnpack::Piece& pc = u.pieces[(size_t)p];
                if (pc.kept == 0) continue;
                const DevChunkCol& d = u.dev[(size_t)kc * (size_t)np + (size_t)p];
                rdf_out& o = outs[(int64_t)kc * nchunks + pc.chunk];
                const size_t src = c.stage_off + (size_t)(((const char*)d.values + d.offset * es[kc]) - c.dev_base);
                st.push_back(StageItem{(char*)o.values + (size_t)pc.written_before * (size_t)es[kc], (size_t)pc.kept * (size_t)es[kc], src, true});
                big += (size_t)pc.kept * (size_t)es[kc];
                if (o.validity) {
                    if (d.validity) {
                        const uint8_t* vsrc = (const uint8_t*)stage + c.vstage_off + (size_t)(((const char*)d.validity + (d.offset >> 3)) - c.vdev_base);
                        nulls[(size_t)kc][(size_t)pc.chunk] += bits_append(o.validity, pc.written_before, vsrc, d.offset & 7, pc.kept);
                    } else {
                        static const uint8_t ones[64] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,
                                                         0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
                        for (int64_t i = 0; i < pc.kept; i += 512) (void)bits_append(o.validity, pc.written_before + i, ones, 0, std::min<int64_t>(512, pc.kept - i));
                    }
                }
            }
        }
        packed_copy(st, stage, false, big);
    };
    static const bool trace = getenv("RDF_STREAM_TRACE") != nullptr;
    double t_phase[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    RDF_TRY(stream_run(plan, ncols, [&](int64_t k, StreamSlab&, const rdf_array* views, int64_t npieces) -> rdf_status {
        const std::vector<PieceOrigin>& org = plan.origin[(size_t)k];
        double t0 = now();
        auto lap = [&](int i) { const double t = now(); t_phase[i] += t - t0; t0 = t; };
        // slab k - 2 has left (its frame's buffers go back to the pool, its staging buffer is free)
        RDF_TRY(down.wait_unpacked(k - 1));
        lap(0);
        if (live[k & 1]) { (void)rdf_frame_release(live[k & 1]); live[k & 1] = nullptr; }
        rdf_frame* in = nullptr;
        RDF_TRY(rdf_frame_pin(views, ncols, npieces, &in));
        lap(1);
        rdf_frame* out = nullptr;
        // (the three-pass form of the operator: its result is DENSE — kept rows on 64-row boundaries —, so what travels back is the
        // kept rows; the one-pass form leaves every batch at its input position and the way back would carry the input's bytes.
        // The kernels' extra ~1 ms per GB is hidden behind the link either way.)
        const int fused_saved = ctx.opt_filter_fused;
        ctx.opt_filter_fused = 0;
        const rdf_status fs = rdf_filter_frame(in, nodes, nnodes, root, &out);
        ctx.opt_filter_fused = fused_saved;
        (void)rdf_frame_release(in);
        RDF_TRY(fs);
        live[k & 1] = out;
        lap(2);
        RDF_TRY(frame_host(*out));                 // kept rows per batch, where every batch of the result lies
        lap(3);
        auto u = std::make_shared<FilterUnpack>();
        u->ncols = ncols;
        u->dev = out->dev;
        u->pieces.resize((size_t)npieces);
        for (int64_t p = 0; p < npieces; ++p) {
            FilterUnpack::Piece& pc = u->pieces[(size_t)p];
            pc.chunk = org[(size_t)p].chunk;
            pc.kept = out->clen[(size_t)p];
            pc.written_before = written[(size_t)pc.chunk];
            written[(size_t)pc.chunk] += pc.kept;
        }
        // one copy per column buffer: [lowest batch pointer, highest batch end)
        std::vector<DownItem> items;
        size_t stage = 0;
        u->cols.resize((size_t)ncols);
        for (int kc = 0; kc < ncols; ++kc) {
            const char *lo = nullptr, *hi = nullptr, *vlo = nullptr, *vhi = nullptr;
            for (int64_t p = 0; p < npieces; ++p) {
                const DevChunkCol& d = out->dev[(size_t)kc * (size_t)npieces + (size_t)p];
                const int64_t kept = out->clen[(size_t)p];
                if (kept == 0 || !d.values) continue;
                const char* b = (const char*)d.values + d.offset * es[kc];
                const char* e = b + kept * es[kc];
                if (!lo || b < lo) lo = b;
                if (!hi || e > hi) hi = e;
                if (d.validity) {
                    const char* vb = (const char*)d.validity + (d.offset >> 3);
                    const char* ve = (const char*)d.validity + ((d.offset + kept + 7) >> 3);
                    if (!vlo || vb < vlo) vlo = vb;
                    if (!vhi || ve > vhi) vhi = ve;
                }
            }
            FilterUnpack::Col& c = u->cols[(size_t)kc];
            c.dev_base = lo; c.bytes = lo ? (size_t)(hi - lo) : 0; c.stage_off = stage;
            stage += (c.bytes + 255) & ~(size_t)255;
            c.vdev_base = vlo; c.vbytes = vlo ? (size_t)(vhi - vlo) : 0; c.vstage_off = stage;
            stage += (c.vbytes + 255) & ~(size_t)255;
            if (c.bytes) items.push_back(DownItem{nullptr, c.bytes, c.stage_off, false, lo});
            if (c.vbytes) items.push_back(DownItem{nullptr, c.vbytes, c.vstage_off, false, vlo});
        }
        if (stage > ctx.dbuf_pin_cap) return fail(RDF_DEVICE_ERROR, "filter_pipeline: a slab's result (%zu bytes) passes its staging buffer (%zu)", stage, ctx.dbuf_pin_cap);
        unpack[k & 1] = u;
        lap(4);
        const rdf_status ss = down.submit_gather(k, std::move(items));
        lap(5);
        return ss;
    }));
    const double t_run = now();
    RDF_TRY(down.finish((int64_t)plan.slabs.size()));
    if (trace) fprintf(stderr, "[rdf] filter_stream: %zu slabs, %.1f ms in all (plan + first upload before the first slab: see wait), per slab: wait for the unpacker %.2f, pin %.2f, filter_frame %.2f, frame_host %.2f, unpack plan %.2f, submit %.2f ms; unpack thread %.2f ms per slab; tail %.1f ms\n", plan.slabs.size(), (now() - t_begin) * 1e3, t_phase[0] * 1e3 / plan.slabs.size(), t_phase[1] * 1e3 / plan.slabs.size(), t_phase[2] * 1e3 / plan.slabs.size(), t_phase[3] * 1e3 / plan.slabs.size(), t_phase[4] * 1e3 / plan.slabs.size(), t_phase[5] * 1e3 / plan.slabs.size(), t_phase_unpack * 1e3 / plan.slabs.size(), (now() - t_run) * 1e3);
    for (int k = 0; k < ncols; ++k)
        for (int64_t c = 0; c < nchunks; ++c) {
            rdf_out& o = outs[(int64_t)k * nchunks + c];
            o.length = written[(size_t)c];
            o.null_count = nulls[(size_t)k][(size_t)c];
        }
    return RDF_OK;
}

// ---- sink: hash GROUP BY (rdf_groupby_agg, config C4) over host-resident batches.  Every slab is aggregated on the device
// (the same call, over device views) into the tail of a device-resident list of partial groups, and that list — what the
// slabs before it left + this slab's groups — is merged (rdf_groupby_merge) into the head of the other list: partial tables
// carried across slabs, never more than (max_groups + a slab's groups) rows of them.  One grouping column, Int64 / UInt64,
// no NULL keys (what the merge takes); anything else keeps the one-shot path.
rdf_status groupby_stream(const rdf_array* keys, const rdf_array* values, int64_t nchunks, int32_t agg, int64_t max_groups,
                          rdf_out* out_keys, rdf_out* out_values, rdf_out* out_counts, int64_t slack) {
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    const char* msg = "groupby: key and value chunks differ in length";
    const int ncols = values ? 2 : 1;
    std::vector<rdf_array> cols((size_t)ncols * (size_t)nchunks);
    for (int64_t c = 0; c < nchunks; ++c) { cols[(size_t)c] = keys[c]; if (values) cols[(size_t)(nchunks + c)] = values[c]; }
    StreamPlan plan;
    RDF_TRY(stream_plan(cols.data(), ncols, nchunks, msg, 0, plan));
    if (plan.slabs.empty()) {
        ctx.stream_slabs = 0;
        out_keys->length = out_values->length = out_counts->length = 0;
        out_keys->null_count = out_values->null_count = out_counts->null_count = 0;
        return RDF_OK;
    }
    const int kdt = keys[0].dtype, odt = out_values->dtype;
    const int64_t cap_l = std::min<int64_t>(max_groups, plan.max_rows) + 2;        // a slab's groups
    const int64_t cap_c = max_groups + 2 + cap_l + 64;                              // a list: merged groups + a slab's
    struct Bufs {
        void* p[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Bufs() { for (void* q : p) if (q) (void)hipFree(q); }
    } bufs;
    // [set][keys, values, counts] + one validity buffer per set (the merge's / the first slab's) + a scratch validity
    for (int i = 0; i < 6; ++i) { hipError_t e = hipMalloc(&bufs.p[i], (size_t)cap_c * 8); if (e != hipSuccess) return fail(RDF_MEMORY_ERROR, "hipMalloc(%zu) for the partial groups failed: %s", (size_t)cap_c * 8, hipGetErrorString(e)); }
    for (int i = 6; i < 8; ++i) { hipError_t e = hipMalloc(&bufs.p[i], (size_t)(cap_c / 8 + 64) * 2); if (e != hipSuccess) return fail(RDF_MEMORY_ERROR, "hipMalloc for the partial groups' validity failed: %s", hipGetErrorString(e)); }
    auto K = [&](int set) { return (char*)bufs.p[set * 3 + 0]; };
    auto V = [&](int set) { return (char*)bufs.p[set * 3 + 1]; };
    auto N = [&](int set) { return (char*)bufs.p[set * 3 + 2]; };
    auto VALID = [&](int set) { return (uint8_t*)bufs.p[6 + set]; };
    uint8_t* scratch_valid = (uint8_t*)bufs.p[6] + (size_t)(cap_c / 8 + 64);       // second half of buffer 6 / 7: a slab's own bitmap when it is not the list's head
    int cur = 0;
    int64_t nA = 0, value_nulls = 0;
    struct InStream { Ctx& c; InStream(Ctx& c_) : c(c_) { c.in_stream = true; } ~InStream() { c.in_stream = false; } } guard(ctx);
    RDF_TRY(stream_run(plan, ncols, [&](int64_t, StreamSlab&, const rdf_array* views, int64_t npieces) -> rdf_status {
        // this slab's groups behind the list's head
        rdf_out lk{K(cur) + nA * 8, nullptr, cap_l, 0, 0, kdt, RDF_MEM_DEVICE};
        rdf_out lv{V(cur) + nA * 8, nA == 0 ? VALID(cur) : scratch_valid, cap_l, 0, 0, odt, RDF_MEM_DEVICE};
        rdf_out lc{N(cur) + nA * 8, nullptr, cap_l, 0, 0, RDF_I64, RDF_MEM_DEVICE};
        RDF_TRY(rdf_groupby_agg(views, 1, values ? views + npieces : nullptr, npieces, agg, max_groups, &lk, &lv, &lc));
        if (nA == 0) { nA = lk.length; value_nulls = lv.null_count; return RDF_OK; }
        if (lk.length == 0) return RDF_OK;
        const int64_t n = nA + lk.length;
        rdf_array ck{K(cur), nullptr, 0, n, 0, kdt, RDF_MEM_DEVICE};
        rdf_array cv{V(cur), nullptr, 0, n, 0, odt, RDF_MEM_DEVICE};          // (a NULL partial has count 0: the merge needs no bitmap)
        rdf_array cc{N(cur), nullptr, 0, n, 0, RDF_I64, RDF_MEM_DEVICE};
        const int nxt = cur ^ 1;
        rdf_out mk{K(nxt), nullptr, cap_c, 0, 0, kdt, RDF_MEM_DEVICE};
        rdf_out mv{V(nxt), VALID(nxt), cap_c, 0, 0, odt, RDF_MEM_DEVICE};
        rdf_out mc{N(nxt), nullptr, cap_c, 0, 0, RDF_I64, RDF_MEM_DEVICE};
        RDF_TRY(rdf_groupby_merge(&ck, &cv, &cc, agg, max_groups, &mk, &mv, &mc));
        cur = nxt;
        nA = mk.length;
        value_nulls = mv.null_count;
        return RDF_OK;
    }));
    if (nA > max_groups + slack) return fail(RDF_MEMORY_ERROR, "groupby: more than max_groups (%lld) distinct keys", (long long)max_groups);   // (the merge keeps the engine's slack of two; the call's promise does not)
    if (nA > out_keys->capacity || nA > out_values->capacity || nA > out_counts->capacity) return fail(RDF_MEMORY_ERROR, "output capacity too small (need max_groups + 2)");
    HIP_TRY(hipMemcpyAsync(out_keys->values, K(cur), (size_t)nA * 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(out_values->values, V(cur), (size_t)nA * 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(out_counts->values, N(cur), (size_t)nA * 8, hipMemcpyDeviceToHost, ctx.stream));
    const bool minmax = agg == RDF_AGG_MIN || agg == RDF_AGG_MAX;
    if (out_values->validity) {
        if (minmax) HIP_TRY(hipMemcpyAsync(out_values->validity, VALID(cur), (size_t)((nA + 7) / 8), hipMemcpyDeviceToHost, ctx.stream));
        else memset(out_values->validity, 0xFF, (size_t)((nA + 7) / 8));
    }
    if (out_counts->validity) memset(out_counts->validity, 0xFF, (size_t)((nA + 7) / 8));
    if (out_keys->validity) memset(out_keys->validity, 0xFF, (size_t)((nA + 7) / 8));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    out_keys->length = out_values->length = out_counts->length = nA;
    out_keys->null_count = 0;
    out_values->null_count = minmax ? value_nulls : 0;
    out_counts->null_count = 0;
    return RDF_OK;
}

}  // namespace
