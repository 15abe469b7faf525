// rdf_stream_plan.h — the pure host parts of the streamed batch loop (rdf_capi_stream.inc): the planner that cuts a batch list
// into pieces and slabs and lays every slab out in its HBM buffer, the layout of a slab's outputs on the way back, and the
// bit-level appender the filter sink builds its validity bitmaps with.  Plain descriptors in, plain structs out: the slab size
// and the answer to "is this pointer page-locked" come in as parameters.  No HIP in here: tests/cpp/test_stream_plan.cpp runs it
// on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <vector>

#include "../../include/rdf_mi355x.h"
#include "rdf_stage_copy.h"

struct StreamItem { const char* src; size_t bytes, pin_off, dev_off; bool direct; };
struct StreamSlab {
    std::vector<StreamItem> items;
    std::vector<rdf_array> views;        // [ncols * npieces], RDF_MEM_DEVICE once `base` is known
    std::vector<size_t> values_item, validity_item;   // per view: index into items (or npos)
    std::vector<size_t> values_off, validity_off;     // per view: where its bytes start inside the item (runs of batches that are consecutive in host memory travel as ONE item)
    int64_t npieces = 0;
    size_t pin_bytes = 0, dev_bytes = 0;
};
constexpr size_t kNoItem = ~(size_t)0;

// ---- the plan: pieces (whole batches; a long batch is cut on 1024-row boundaries) grouped into slabs of at most S bytes
struct PieceOrigin { int64_t chunk, row0, rows; };
struct StreamPlan {
    std::vector<StreamSlab> slabs;
    std::vector<std::vector<PieceOrigin>> origin;     // per slab, per piece: where its rows come from
    size_t max_pin = 0, max_dev = 0;
    int64_t max_rows = 0, max_pieces = 0;             // of a slab
};

using StreamPinnedFn = std::function<bool(const void*)>;      // is the buffer that starts here page-locked?

inline size_t stream_elem_size(int dt) {                      // bytes of a fixed-width element (RDF_BOOL: bit-packed, 0)
    switch (dt) {
        case RDF_I8: case RDF_U8: return 1;
        case RDF_I16: case RDF_U16: return 2;
        case RDF_I32: case RDF_U32: case RDF_F32: return 4;
        case RDF_I64: case RDF_U64: case RDF_F64: return 8;
        default: return 0;
    }
}

// what the slabs cannot check for each other
enum StreamPlanError { kStreamPlanOk = 0, kStreamPlanLengths = 1, kStreamPlanDtypes = 2 };

// -> kStreamPlanOk, kStreamPlanLengths (batch lengths differ across columns), kStreamPlanDtypes (*bad_col: the column whose chunks
// differ in dtype).  S: the slab budget in bytes.
inline StreamPlanError stream_plan_build(const rdf_array* cols, int32_t ncols, int64_t nchunks, size_t extra_row_bytes, size_t S,
                                         const StreamPinnedFn& pinned, StreamPlan& plan, int* bad_col) {
    // validation the slabs cannot do for each other: batch lengths across columns (dtypes are checked slab by slab)
    size_t row_bytes = extra_row_bytes;
    for (int k = 0; k < ncols; ++k) {
        const rdf_array& a0 = cols[(int64_t)k * nchunks];
        row_bytes += a0.dtype == RDF_BOOL ? 1 : stream_elem_size(a0.dtype);
        for (int64_t c = 0; c < nchunks; ++c) {
            const rdf_array& a = cols[(int64_t)k * nchunks + c];
            if (a.length != cols[c].length) return kStreamPlanLengths;
            if (a.dtype != a0.dtype) { if (bad_col) *bad_col = k; return kStreamPlanDtypes; }
        }
    }
    if (row_bytes == 0) row_bytes = 8;
    int64_t piece_rows = (int64_t)(S / 4 / (row_bytes + 1)) / 1024 * 1024;
    if (piece_rows < 1024) piece_rows = 1024;
    std::map<const void*, bool> pinned_cache;
    auto is_pinned = [&](const void* base) {
        auto it = pinned_cache.find(base);
        if (it != pinned_cache.end()) return it->second;
        const bool p = pinned(base);
        pinned_cache.emplace(base, p);
        return p;
    };
    StreamSlab cur;
    std::vector<PieceOrigin> cur_origin;
    int64_t cur_rows = 0;
    std::vector<StreamItem> piece_items;
    std::vector<rdf_array> piece_views((size_t)ncols);
    std::vector<size_t> piece_vi((size_t)ncols), piece_bi((size_t)ncols);
    auto flush = [&]() {
        if (cur.npieces == 0) return;
        // Batches that are consecutive slices of one page-locked buffer (a reader's column, an Arrow IPC image) leave with ONE
        // copy per column and slab instead of one per batch: a 1M-row batch of an i8 column is a 1 MB copy, and a few dozen of
        // those per slab cost the link a tenth of its rate in per-copy overhead.  A run ends where the next batch does not start
        // at the previous one's end, or where a batch's bytes would leave its successor off a 256-byte boundary in HBM.
        {
            const size_t nv = cur.views.size();
            cur.values_off.assign(nv, 0); cur.validity_off.assign(nv, 0);
            std::vector<StreamItem> merged;
            merged.reserve(cur.items.size());
            std::vector<size_t> remap(cur.items.size(), kNoItem);
            const size_t ncol = nv / (size_t)cur.npieces;
            for (int pass = 0; pass < 2; ++pass)                     // values, then bitmaps
                for (size_t k = 0; k < ncol; ++k) {
                    size_t run = kNoItem;                             // index into `merged` of the open run
                    const char* run_end = nullptr;
                    for (int64_t p = 0; p < cur.npieces; ++p) {
                        const size_t v = (size_t)p * ncol + k;
                        const size_t it_i = pass == 0 ? cur.values_item[v] : cur.validity_item[v];
                        if (it_i == kNoItem) { run = kNoItem; continue; }
                        const StreamItem& it = cur.items[it_i];
                        size_t off = 0;
                        if (run != kNoItem && it.direct && merged[run].direct && it.src == run_end && (merged[run].bytes & 255) == 0) {
                            off = merged[run].bytes;
                            merged[run].bytes += it.bytes;
                        } else {
                            merged.push_back(it);
                            run = merged.size() - 1;
                        }
                        run_end = it.src + it.bytes;
                        remap[it_i] = run;
                        (pass == 0 ? cur.values_off[v] : cur.validity_off[v]) = off;
                        if (!it.direct) run = kNoItem;
                    }
                }
            for (size_t v = 0; v < nv; ++v) {
                cur.values_item[v] = remap[cur.values_item[v]];
                if (cur.validity_item[v] != kNoItem) cur.validity_item[v] = remap[cur.validity_item[v]];
            }
            cur.items.swap(merged);
        }
        // layout: the staged items mirror the staging buffer at the front of the slab, the direct ones follow
        size_t pin = 0;
        for (StreamItem& it : cur.items) if (!it.direct) { it.pin_off = pin; it.dev_off = pin; pin += (it.bytes + 16 + 63) & ~(size_t)63; }
        size_t dev = (pin + 255) & ~(size_t)255;
        for (StreamItem& it : cur.items) if (it.direct) { it.dev_off = dev; dev += (it.bytes + 16 + 255) & ~(size_t)255; }
        cur.pin_bytes = pin; cur.dev_bytes = dev;
        plan.max_pin = std::max(plan.max_pin, pin); plan.max_dev = std::max(plan.max_dev, dev);
        plan.max_rows = std::max(plan.max_rows, cur_rows); plan.max_pieces = std::max(plan.max_pieces, cur.npieces);
        plan.slabs.push_back(std::move(cur));
        plan.origin.push_back(std::move(cur_origin));
        cur = StreamSlab();
        cur_origin.clear();
        cur_rows = 0;
    };
    size_t cur_bytes = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t L = cols[c].length;
        for (int64_t r0 = 0; r0 < L; r0 += piece_rows) {
            const int64_t n = std::min(piece_rows, L - r0);
            piece_items.clear();
            size_t pbytes = 0;
            for (int k = 0; k < ncols; ++k) {
                const rdf_array& a = cols[(int64_t)k * nchunks + c];
                const int64_t eff = a.offset + r0, kk = eff & 7, s0 = eff - kk;
                const size_t b0 = (size_t)(s0 >> 3), b1 = (size_t)((eff + n + 7) >> 3);
                StreamItem vi;
                if (a.dtype == RDF_BOOL) vi = StreamItem{(const char*)a.values + b0, b1 - b0, 0, 0, false};
                else { const size_t es = stream_elem_size(a.dtype); vi = StreamItem{(const char*)a.values + (size_t)s0 * es, (size_t)(n + kk) * es, 0, 0, false}; }
                vi.direct = vi.bytes >= kSmallCopy && is_pinned(a.values);
                piece_vi[(size_t)k] = piece_items.size();
                piece_items.push_back(vi);
                pbytes += vi.bytes + 256;
                piece_bi[(size_t)k] = kNoItem;
                if (a.validity) {
                    StreamItem bi{(const char*)a.validity + b0, b1 - b0, 0, 0, false};
                    bi.direct = bi.bytes >= kSmallCopy && is_pinned(a.validity);
                    piece_bi[(size_t)k] = piece_items.size();
                    piece_items.push_back(bi);
                    pbytes += bi.bytes + 256;
                }
                rdf_array v = a;
                v.offset = kk; v.length = n;
                v.null_count = (r0 == 0 && n == L) ? a.null_count : (a.null_count == 0 ? 0 : -1);
                v.mem = RDF_MEM_DEVICE;
                piece_views[(size_t)k] = v;
            }
            pbytes += (size_t)n * extra_row_bytes;
            if (cur.npieces > 0 && cur_bytes + pbytes > S) { flush(); cur_bytes = 0; }
            const size_t base = cur.items.size();
            for (const StreamItem& it : piece_items) cur.items.push_back(it);
            for (int k = 0; k < ncols; ++k) {
                cur.views.push_back(piece_views[(size_t)k]);            // piece-major for now; transposed per slab
                cur.values_item.push_back(base + piece_vi[(size_t)k]);
                cur.validity_item.push_back(piece_bi[(size_t)k] == kNoItem ? kNoItem : base + piece_bi[(size_t)k]);
            }
            cur_origin.push_back(PieceOrigin{c, r0, n});
            ++cur.npieces;
            cur_rows += n;
            cur_bytes += pbytes;
        }
    }
    flush();
    return kStreamPlanOk;
}

// ---- the way back
struct DownItem { char* dst; size_t bytes, off; bool direct; const char* dev_src = nullptr; };     // off: inside the slab's output buffer (staged items: also inside staging); dev_src: submit_gather's source

// lays the outputs of a slab out in its output buffer: staged items first (contiguous: ONE copy into staging), direct ones behind
struct DownLayout {
    std::vector<DownItem> items;
    size_t pin = 0, dev = 0;
    StreamPinnedFn pinned;
    std::map<const void*, bool> pinned_cache;
    explicit DownLayout(StreamPinnedFn fn) : pinned(std::move(fn)) {}
    bool dst_pinned(const void* base) {
        auto it = pinned_cache.find(base);
        if (it != pinned_cache.end()) return it->second;
        const bool p = pinned(base);
        pinned_cache.emplace(base, p);
        return p;
    }
    void reset() { items.clear(); pin = dev = 0; }
    size_t add(char* dst, size_t bytes, const void* dst_base) {   // -> index; offsets are final after close()
        items.push_back(DownItem{dst, bytes, 0, bytes >= kSmallCopy && dst_pinned(dst_base)});
        return items.size() - 1;
    }
    std::vector<DownItem> copies;     // what actually travels: the staged region is one copy (Downloader), direct items that are
                                      // consecutive in the caller's memory (batches sliced from one column buffer) one copy per run
    void close() {
        pin = 0;
        for (DownItem& it : items) if (!it.direct) { it.off = pin; pin += (it.bytes + 16 + 255) & ~(size_t)255; }
        dev = pin;
        copies.clear();
        size_t run = kNoItem;
        for (DownItem& it : items) {
            if (!it.direct) { copies.push_back(it); continue; }
            if (run != kNoItem && copies[run].dst + copies[run].bytes == it.dst && (copies[run].bytes & 255) == 0) {
                it.off = copies[run].off + copies[run].bytes;
                copies[run].bytes += it.bytes;
            } else {
                if (run != kNoItem) dev = copies[run].off + ((copies[run].bytes + 16 + 255) & ~(size_t)255);
                it.off = dev;
                copies.push_back(it);
                run = copies.size() - 1;
            }
        }
        if (run != kNoItem) dev = copies[run].off + ((copies[run].bytes + 16 + 255) & ~(size_t)255);
    }
};

// ---- appends nbits bits of src (from bit src_bit) behind bit dst_bit of dst; every other bit of dst keeps its value
inline int64_t bits_append(uint8_t* dst, int64_t dst_bit, const uint8_t* src, int64_t src_bit, int64_t nbits) {   // -> zero bits appended
    int64_t zeros = 0, i = 0;
    auto few = [&](int64_t upto) {          // bit runs of at most a byte
        while (i < upto) {
            const int64_t sb = src_bit + i, db = dst_bit + i;
            const int take = (int)std::min<int64_t>(std::min<int64_t>(8 - (sb & 7), 8 - (db & 7)), upto - i);
            const unsigned bits = ((unsigned)src[sb >> 3] >> (sb & 7)) & ((1u << take) - 1u);
            const unsigned mask = ((1u << take) - 1u) << (db & 7);
            dst[db >> 3] = (uint8_t)((dst[db >> 3] & ~mask) | (bits << (db & 7)));
            zeros += take - __builtin_popcount(bits);
            i += take;
        }
    };
    if (((src_bit ^ dst_bit) & 7) == 0) {   // same phase (whole batches: both 0): head bits, whole bytes, tail bits
        few(std::min<int64_t>(nbits, (8 - (dst_bit & 7)) & 7));
        const int64_t nbytes = (nbits - i) >> 3;
        if (nbytes > 0) {
            const uint8_t* sp = src + ((src_bit + i) >> 3);
            memcpy(dst + ((dst_bit + i) >> 3), sp, (size_t)nbytes);
            int64_t ones = 0, b = 0;
            for (; b + 8 <= nbytes; b += 8) { uint64_t w; memcpy(&w, sp + b, 8); ones += __builtin_popcountll(w); }
            for (; b < nbytes; ++b) ones += __builtin_popcount(sp[b]);
            zeros += nbytes * 8 - ones;
            i += nbytes * 8;
        }
    }
    few(nbits);
    return zeros;
}
