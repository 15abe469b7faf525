// rdf_utf8_regex.hip — the kernels of rdf_utf8_regexp_match / _count / _extract / _replace / _split (host side:
// rdf_capi_utf8_regex.inc; the pattern compiler and what is decided about one row, for hipcc and g++ alike: rdf_utf8_regex.h).
//
//   tables   every block copies the compiled pattern's image (class map, forward and reverse table) into LDS, 16 bytes a
//            lane a step, when it fits kUtf8RegexLdsBytes; a larger image is walked where it lies in HBM.
//   measure  rlike and regexp_count: the tiles and outputs of rdf_utf8_pred.hip, a lane a row.  rlike walks the forward DFA
//            only and stops at the first flagged state.
//   size     extract / replace / split: the row's output bytes (split: and its elements), a lane a row.
//   scan     launch_scan and utf8_rewrite_totals_kernel, unchanged.
//   write    the SOURCE-driven form of rdf_utf8_rewrite.hip: runs of rows assembled in the kUtf8RewriteImage LDS image,
//            streamed out in aligned 16-byte stores with byte stores at a run's two ends; a row whose output alone exceeds
//            the image goes to HBM directly; offsets, validity words and split's child offsets are written on the way.
//   long rows  a DFA walk is sequential, so a row of any length stays on ONE lane.  The rows of a tile (or run) beyond
//            kUtf8ShortRow are listed in LDS and dealt round-robin over the block's four waves, so one wave never holds
//            them all; their results go back to the owning lane through LDS.
// Row bytes are read 8 at a time where the address allows (utf8_regex_forward / _backward).  No atomics touch data, offsets or
// validity (one atomicAdd per block and tile counts NULL rows); every byte is a function of the inputs alone.  No kernel uses
// scratch (profiles/utf8_regex_resources.md).
#include <algorithm>

#define RDF_UTF8_REGEX_NO_COMPILER
#include "rdf_utf8.h"
#include "rdf_utf8_regex.h"

namespace {

constexpr int kThreads = kUtf8PredThreads;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ bool bit_at(const uint8_t* b, int64_t i) { return (b[i >> 3] >> (i & 7)) & 1; }
__device__ int64_t find_tile_chunk(const int64_t* ts, int64_t nch, int64_t t) {
    int64_t lo = 0, hi = nch;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ts[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
__device__ __forceinline__ void store_word(uint8_t* bitmap, int64_t r0, int nrows, uint64_t word, int lane) {
    uint8_t* p = bitmap + (r0 >> 3);
    if (nrows == 64 && ((uintptr_t)p & 7) == 0) {
        if (lane == 0) *(uint64_t*)p = word;
    } else if (lane < ((nrows + 7) >> 3)) {
        p[lane] = (uint8_t)(word >> (8 * lane));
    }
}
__device__ __forceinline__ void row_span(const Utf8Chunk& c, int64_t r, int32_t& o0, int32_t& o1) {
    o0 = c.offs[r];
    o1 = c.offs[r + 1];
    o0 = min(max(o0, c.lo), c.hi);
    o1 = min(max(o1, o0), c.hi);
}
__device__ __forceinline__ bool row_valid(const Utf8Chunk& c, int64_t r) { return !c.valid || bit_at(c.valid, c.valid_off + r); }

// the image into LDS (LDS) or left in HBM; the view of it
template <bool LDS>
__device__ __forceinline__ Utf8RegexView load_tables(const uint8_t* image, uint4* s_tab) {
    const Utf8RegexHeader h = *(const Utf8RegexHeader*)image;
    if (LDS) {
        const uint4* src = (const uint4*)image;
        const int pieces = min(h.table_bytes, kUtf8RegexLdsBytes) >> 4;
        for (int i = threadIdx.x; i < pieces; i += kThreads) s_tab[i] = src[i];
        __syncthreads();
        return utf8_regex_view(h, (const uint8_t*)s_tab);
    }
    return utf8_regex_view(h, image);
}
// The block's lanes with is_long listed in s_list and dealt over the waves: the lane whose row this lane takes, or -1.
// Called by the whole block; a barrier must pass before s_list is used again.
__device__ __forceinline__ int deal_long_rows(bool is_long, int* s_cnt, int* s_list) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t m = __ballot(is_long);
    if (lane == 0) s_cnt[w] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
    for (int k = 0; k < kWaves; ++k) {
        if (k < w) base += s_cnt[k];
        total += s_cnt[k];
    }
    if (is_long) s_list[base + __popcll(m & ((1ull << lane) - 1))] = threadIdx.x;
    __syncthreads();
    const int j = lane * kWaves + w;   // long row j goes to wave j % kWaves
    return j < total ? s_list[j] : -1;
}

// ---- rlike / regexp_count
template <bool LDS, bool COUNT>
__global__ __launch_bounds__(kThreads) void utf8_regex_measure_kernel(Utf8PredArgs a) {
    __shared__ uint4 s_tab[LDS ? kUtf8RegexLdsBytes / 16 : 1];
    __shared__ int s_cnt[kWaves], s_list[kThreads], s_res[kThreads], s_nulls[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const Utf8RegexView v = load_tables<LDS>(a.regex, s_tab);
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const Utf8Chunk& ch = a.a[c];
        const int64_t tr0 = (t - a.tile_start[c]) * kThreads, r0 = tr0 + (int64_t)w * 64;
        const int64_t left = ch.rows - r0;
        const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        const int64_t r = r0 + lane;
        const bool valid = lane < nrows && row_valid(ch, r);
        bool is_long = false;
        int32_t val = 0, o0 = 0, o1 = 0;
        if (valid) {
            row_span(ch, r, o0, o1);
            const int len = o1 - o0;
            if (len > kUtf8ShortRow) is_long = true;
            else val = COUNT ? (int32_t)utf8_regex_count(v, ch.data + o0, len) : (int32_t)utf8_regex_any(v, ch.data + o0, len);
        }
        const int owner = deal_long_rows(is_long, s_cnt, s_list);
        if (owner >= 0) {
            int32_t q0, q1;
            row_span(ch, tr0 + owner, q0, q1);
            s_res[owner] = COUNT ? (int32_t)min((int64_t)INT32_MAX, utf8_regex_count(v, ch.data + q0, q1 - q0)) : (int32_t)utf8_regex_any(v, ch.data + q0, q1 - q0);
        }
        __syncthreads();
        if (is_long) val = s_res[tid];
        const uint64_t vmask = __ballot(valid);
        const uint64_t rmask = __ballot(valid && val != 0);
        if (nrows > 0) {
            const Utf8PredOut o = a.outs[c];
            if (COUNT) {
                if (lane < nrows) ((int32_t*)o.values)[r] = valid ? val : 0;
            } else store_word((uint8_t*)o.values, r0, nrows, rmask, lane);
            if (o.valid) store_word(o.valid, r0, nrows, vmask, lane);
        }
        if (a.nulls) {
            if (lane == 0) s_nulls[w] = nrows - __popcll(vmask);
            __syncthreads();
            if (tid == 0) {
                int n = 0;
                for (int k = 0; k < kWaves; ++k) n += s_nulls[k];
                if (n) atomicAdd(&a.nulls[c], (unsigned long long)n);
            }
        }
        __syncthreads();   // s_list, s_res and s_nulls are the next tile's to overwrite
    }
}

// ---- 1. size
template <bool LDS, int OP>
__global__ __launch_bounds__(kThreads) void utf8_regex_size_kernel(Utf8RewriteArgs a) {
    __shared__ uint4 s_tab[LDS ? kUtf8RegexLdsBytes / 16 : 1];
    __shared__ int s_cnt[kWaves], s_list[kThreads], s_nulls[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const Utf8RegexView v = load_tables<LDS>(a.regex, s_tab);
    const int64_t rb = OP == U8X_REPLACE ? a.rep_bytes : 0;
    const auto none = [](int64_t, int64_t) {};
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const Utf8Chunk& ch = a.chunks[c];
        const int64_t tr0 = (t - a.tile_start[c]) * kThreads, r0 = tr0 + (int64_t)w * 64;
        const int64_t left = ch.rows - r0;
        const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        const int64_t r = r0 + lane;
        const bool valid = lane < nrows && row_valid(ch, r);
        bool is_long = false;
        if (lane < nrows) {
            int64_t out = 0, elems = 0;
            if (valid) {
                int32_t o0, o1;
                row_span(ch, r, o0, o1);
                if (o1 - o0 > kUtf8ShortRow) is_long = true;
                else out = utf8_regex_row(v, OP, ch.data + o0, o1 - o0, nullptr, rb, a.maxhits, nullptr, &elems, none);
            }
            if (!is_long) {
                const int64_t g = ch.row_start + r;
                a.blen[g] = utf8_build_clamp(out);
                if (OP == U8X_SPLIT) a.elen[g] = elems;
            }
        }
        const int owner = deal_long_rows(is_long, s_cnt, s_list);
        if (owner >= 0) {
            int32_t q0, q1;
            int64_t elems = 0;
            row_span(ch, tr0 + owner, q0, q1);
            const int64_t out = utf8_regex_row(v, OP, ch.data + q0, q1 - q0, nullptr, rb, a.maxhits, nullptr, &elems, none);
            const int64_t g = ch.row_start + tr0 + owner;
            a.blen[g] = utf8_build_clamp(out);
            if (OP == U8X_SPLIT) a.elen[g] = elems;
        }
        const uint64_t vmask = __ballot(valid);
        if (lane == 0) s_nulls[w] = nrows - __popcll(vmask);
        __syncthreads();
        if (tid == 0) {
            int n = 0;
            for (int k = 0; k < kWaves; ++k) n += s_nulls[k];
            if (n) atomicAdd(&a.null_counts[c], (unsigned long long)n);
        }
        __syncthreads();
    }
}

// ---- 3. write
// one row into `out` (LDS image or HBM); split's child offsets from element 1 on go to eo
template <int OP>
__device__ __forceinline__ void write_row(const Utf8RegexView& v, const Utf8RewriteArgs& a, const uint8_t* b, int len, const uint8_t* s_rep, uint8_t* out,
                                          int32_t* eo, int32_t ob) {
    int64_t elems = 0;
    if (OP == U8X_SPLIT) utf8_regex_row(v, OP, b, len, s_rep, 0, a.maxhits, out, &elems, [&](int64_t j, int64_t at) { eo[j] = ob + (int32_t)at; });
    else utf8_regex_row(v, OP, b, len, s_rep, OP == U8X_REPLACE ? a.rep_bytes : 0, a.maxhits, out, &elems, [](int64_t, int64_t) {});
}

template <bool LDS, int OP>
__global__ __launch_bounds__(kThreads) void utf8_regex_write_kernel(Utf8RewriteArgs a) {
    __shared__ uint4 s_tab[LDS ? kUtf8RegexLdsBytes / 16 : 1];
    __shared__ uint4 s_img[(kUtf8RewriteImage + 32) / 16];   // image byte i goes to the run's first destination byte - head + i
    __shared__ uint8_t s_rep[OP == U8X_REPLACE ? kUtf8PatternMax : 16];
    __shared__ int64_t s_end[kThreads];   // where the output of the tile's rows ends (in the scan)
    __shared__ int s_cnt[kWaves], s_list[kThreads];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (OP == U8X_REPLACE)
        for (int i = tid; i < a.rep_bytes; i += kThreads) s_rep[i] = a.rep[i];
    const Utf8RegexView v = load_tables<LDS>(a.regex, s_tab);
    __syncthreads();
    if (blockIdx.x == 0)   // a chunk without rows has no tile: its one offset
        for (int64_t c = tid; c < a.nchunks; c += kThreads)
            if (a.outs[c].rows == 0) {
                a.outs[c].offs[0] = 0;
                if (OP == U8X_SPLIT) a.outs[c].list_offs[0] = 0;
            }
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const Utf8Chunk& ch = a.chunks[c];
        const Utf8RewriteOut& o = a.outs[c];
        const int64_t tr0 = (t - a.tile_start[c]) * kThreads;
        const int64_t tleft = o.rows - tr0;
        const int trows = tleft >= kThreads ? kThreads : (int)tleft;
        const int64_t r = tr0 + tid;
        const int64_t g = o.row_start + r;
        bool valid = false;
        int64_t b0 = 0, b1 = 0, e0 = 0;
        int32_t o0 = 0, o1 = 0;
        if (tid < trows) {
            valid = row_valid(ch, r);
            if (valid) row_span(ch, r, o0, o1);
            b0 = a.bscan[g];
            b1 = a.bscan[g + 1];
            if (OP == U8X_SPLIT) {
                e0 = a.escan[g] - o.elem_start;
                o.list_offs[r] = (int32_t)e0;
                if (valid) o.offs[e0] = (int32_t)(b0 - o.byte_start);   // element 0; the others where their hits are found
                if (r == o.rows - 1) {
                    const int64_t e1 = a.escan[g + 1] - o.elem_start;
                    o.list_offs[o.rows] = (int32_t)e1;
                    o.offs[e1] = (int32_t)(b1 - o.byte_start);
                }
            } else {
                o.offs[r] = (int32_t)(b0 - o.byte_start);
                if (r == o.rows - 1) o.offs[o.rows] = (int32_t)(b1 - o.byte_start);
            }
            s_end[tid] = b1;
        }
        if (o.valid) {
            const int64_t r0 = tr0 + (int64_t)w * 64;
            const int nrows = (int)min((int64_t)64, max((int64_t)0, o.rows - r0));
            const uint64_t vmask = __ballot(valid);
            if (nrows > 0) store_word(o.valid, r0, nrows, vmask, lane);
        }
        __syncthreads();
        const int64_t tile_b0 = a.bscan[o.row_start + tr0];
        const int len = o1 - o0;
        int p0 = 0;
        while (p0 < trows) {   // (p0, and everything that decides a barrier, is the same in every lane of the block)
            const int64_t base = p0 == 0 ? tile_b0 : s_end[p0 - 1];
            const int cnt = __syncthreads_count(tid >= p0 && tid < trows && s_end[tid] - base <= kUtf8RewriteImage);
            if (cnt == 0) {   // row p0's output alone exceeds the image: one lane writes it to HBM directly
                if (tid == 0 && row_valid(ch, tr0 + p0)) {
                    const int64_t rr = tr0 + p0;
                    int32_t q0, q1;
                    row_span(ch, rr, q0, q1);
                    const int32_t ob = (int32_t)(base - o.byte_start);
                    int32_t* eo = OP == U8X_SPLIT ? o.offs + (a.escan[o.row_start + rr] - o.elem_start) : nullptr;
                    write_row<OP>(v, a, ch.data + q0, q1 - q0, s_rep, o.data + ob, eo, ob);
                }
                p0 += 1;
                continue;
            }
            const int p1 = p0 + cnt;
            const int span = (int)(s_end[p1 - 1] - base);
            if (span > 0 || OP == U8X_SPLIT) {   // (rows of a split without bytes still have elements)
                uint8_t* dst0 = o.data + (base - o.byte_start);
                const int head = (int)((uintptr_t)dst0 & 15);
                uint8_t* img = (uint8_t*)s_img + head;
                const bool mine = tid >= p0 && tid < p1 && valid;
                if (mine && len <= kUtf8ShortRow)
                    write_row<OP>(v, a, ch.data + o0, len, s_rep, img + (int)(b0 - base), OP == U8X_SPLIT ? o.offs + e0 : nullptr, (int32_t)(b0 - o.byte_start));
                const int owner = deal_long_rows(mine && len > kUtf8ShortRow, s_cnt, s_list);
                if (owner >= 0) {
                    const int64_t rr = tr0 + owner, gg = o.row_start + rr;
                    int32_t q0, q1;
                    row_span(ch, rr, q0, q1);
                    const int64_t qb0 = a.bscan[gg];
                    int32_t* eo = OP == U8X_SPLIT ? o.offs + (a.escan[gg] - o.elem_start) : nullptr;
                    write_row<OP>(v, a, ch.data + q0, q1 - q0, s_rep, img + (int)(qb0 - base), eo, (int32_t)(qb0 - o.byte_start));
                }
                __syncthreads();
                if (span > 0) {
                    const int npieces = (head + span + 15) >> 4;
                    for (int k = tid; k < npieces; k += kThreads) {
                        const int i0 = k << 4;
                        if (i0 >= head && i0 + 16 <= head + span) *(uint4*)(dst0 - head + i0) = s_img[k];
                        else
                            for (int i = max(i0, head); i < min(i0 + 16, head + span); ++i) dst0[i - head] = ((const uint8_t*)s_img)[i];
                    }
                    __syncthreads();
                }
            }
            p0 = p1;
        }
        __syncthreads();   // s_end is the next tile's to overwrite
    }
}

}  // namespace

#define UTF8_REGEX_DISPATCH(KERNEL, LDSV, OPV, ...)                                                          \
    if (LDSV) switch (OPV) {                                                                                 \
        case U8X_EXTRACT: hipLaunchKernelGGL((KERNEL<true, U8X_EXTRACT>), __VA_ARGS__); break;               \
        case U8X_REPLACE: hipLaunchKernelGGL((KERNEL<true, U8X_REPLACE>), __VA_ARGS__); break;               \
        default: hipLaunchKernelGGL((KERNEL<true, U8X_SPLIT>), __VA_ARGS__); break;                          \
    } else switch (OPV) {                                                                                    \
        case U8X_EXTRACT: hipLaunchKernelGGL((KERNEL<false, U8X_EXTRACT>), __VA_ARGS__); break;              \
        case U8X_REPLACE: hipLaunchKernelGGL((KERNEL<false, U8X_REPLACE>), __VA_ARGS__); break;              \
        default: hipLaunchKernelGGL((KERNEL<false, U8X_SPLIT>), __VA_ARGS__); break;                         \
    }

hipError_t launch_utf8_regex_measure(const Utf8PredArgs& a, int64_t image_bytes, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(a.ntiles, 256 * 16)), block(kThreads);
    const bool lds = image_bytes <= kUtf8RegexLdsBytes;
    if (lds) {
        if (a.measure) hipLaunchKernelGGL((utf8_regex_measure_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((utf8_regex_measure_kernel<true, false>), grid, block, 0, s, a);
    } else {
        if (a.measure) hipLaunchKernelGGL((utf8_regex_measure_kernel<false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((utf8_regex_measure_kernel<false, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}
hipError_t launch_utf8_regex_size(const Utf8RewriteArgs& a, int64_t image_bytes, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(a.ntiles, 256 * 16)), block(kThreads);
    const bool lds = image_bytes <= kUtf8RegexLdsBytes;
    UTF8_REGEX_DISPATCH(utf8_regex_size_kernel, lds, a.regex_op, grid, block, 0, s, a)
    return hipGetLastError();
}
hipError_t launch_utf8_regex_write(const Utf8RewriteArgs& a, int64_t image_bytes, hipStream_t s) {
    if (a.nchunks <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>(a.ntiles, 1), 256 * 16)), block(kThreads);
    const bool lds = image_bytes <= kUtf8RegexLdsBytes;
    UTF8_REGEX_DISPATCH(utf8_regex_write_kernel, lds, a.regex_op, grid, block, 0, s, a)
    return hipGetLastError();
}
