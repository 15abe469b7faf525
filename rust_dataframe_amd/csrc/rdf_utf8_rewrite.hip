// rdf_utf8_rewrite.hip — the kernels of rdf_utf8_replace / _translate / _initcap / _split: text rows rewritten by what they
// hold (host side: rdf_capi_utf8_rewrite.inc; what is decided about one row, for hipcc and g++ alike: rdf_utf8_rewrite.h).
// The three steps of rdf_utf8.hip / rdf_utf8_build.hip; output chunk c holds the rows of input chunk c.
//
//   size    the tiles of rdf_utf8_pred.hip: a block takes 256 rows of ONE chunk, a lane a row.  A row of up to kUtf8ShortRow
//           bytes is sized on its lane through the header (the hits counted, the mapped lengths added up); a longer one by
//           its wave, 64 bytes a step (below).  split also counts the row's elements.  replace with a replacement as long as
//           its search, and split with limit 1, read no row byte here.  NULL rows are counted per wave.
//   scan    launch_scan over the lengths (split: and over the element counts, which gives the list offsets); the host applies
//           the sizing rule to the per-chunk totals before anything is written.
//   write   SOURCE-driven: where an output byte comes from depends on every hit or mapped length before it in its row, so a
//           destination-driven search (utf8_build_copy_kernel) would redo the row's scan for every 16-byte piece.  Instead a
//           block takes the same tiles again and cuts each into RUNS of rows whose output span fits an LDS image of
//           kUtf8RewriteImage bytes (the scan says where every row's output lies).  Lanes write their short rows, waves
//           their long rows, into the image, which keeps the destination's alignment modulo 16; then the block streams the
//           image to HBM: every aligned 16-byte piece that lies inside the span is ONE uint4 store, the partial pieces at
//           the run's two ends go byte by byte (a neighbouring run, of this block or another, owns the rest of those pieces).
//           A row whose output alone exceeds the image is written to HBM by a wave directly.  The offsets, the validity
//           words (one 64-bit word per wave, rdf_textconv.hip's rule) and split's child offsets are written on the way.
//
//   long rows on the wave
//     replace / split   lane i tests the candidate start base + i (first-byte filter, then the compare); __ballot gives the
//                       window's 64-bit candidate mask; the greedy non-overlapping choice is a scalar loop over its set bits
//                       (utf8_select_hits) that carries the earliest allowed start from window to window, so literals longer
//                       than 64 bytes and self-overlapping ones work; a byte's output position follows from the popcount of
//                       the chosen hits at or before it (utf8_window_byte).  Replacements are written by the whole wave.
//     translate / initcap   lane i decides about byte base + i alone (utf8_unit_at looks 3 bytes back and 4 ahead): the byte
//                       that begins a mapped unit emits the mapping, the unit's other bytes nothing, copied bytes themselves;
//                       a wave prefix sum of the emitted lengths places them.  Only a lane that holds U+03A3 away from a
//                       word's start walks its context for Final_Sigma, as in utf8_wide_kernel.
//
// No atomics touch data, offsets or validity (one atomicAdd per block and tile counts NULL rows); every byte is a function of
// the inputs alone, so chunking, memory kind and repetition change nothing.  No kernel uses scratch
// (profiles/utf8_rewrite_resources.md).
#include <algorithm>

#include "rdf_utf8.h"
#include "rdf_utf8_rewrite.h"

namespace {

constexpr int kThreads = kUtf8PredThreads;
constexpr int kTableWords = (int)(sizeof(Utf8TranslateTable) / 4);

__device__ __forceinline__ bool bit_at(const uint8_t* b, int64_t i) { return (b[i >> 3] >> (i & 7)) & 1; }

__device__ int64_t find_tile_chunk(const int64_t* ts, int64_t nch, int64_t t) {
    int64_t lo = 0, hi = nch;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ts[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
__device__ __forceinline__ int first_lane(uint64_t mask) { return __builtin_ctzll(mask); }
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
// one word of a bitmap whose bit 0 is row r0 (a multiple of 64) of the chunk: the wave's nrows bits
__device__ __forceinline__ void store_word(uint8_t* bitmap, int64_t r0, int nrows, uint64_t word, int lane) {
    uint8_t* p = bitmap + (r0 >> 3);
    if (nrows == 64 && ((uintptr_t)p & 7) == 0) {
        if (lane == 0) *(uint64_t*)p = word;
    } else if (lane < ((nrows + 7) >> 3)) {
        p[lane] = (uint8_t)(word >> (8 * lane));
    }
}
// a row's span, clamped into the bytes the host checked
__device__ __forceinline__ void row_span(const Utf8Chunk& c, int64_t r, int32_t& o0, int32_t& o1) {
    o0 = c.offs[r];
    o1 = c.offs[r + 1];
    o0 = min(max(o0, c.lo), c.hi);
    o1 = min(max(o1, o0), c.hi);
}
__device__ __forceinline__ bool row_valid(const Utf8Chunk& c, int64_t r) { return !c.valid || bit_at(c.valid, c.valid_off + r); }

constexpr bool op_searches(int op) { return op == U8R_REPLACE || op == U8R_SPLIT; }

// ---- the wave's forms.  Every argument is the same in all 64 lanes, and so is the result.
// replace / split of one row: the hits (at most maxhits).  WRITE: the row's output goes to out; eoffs (split): the slot of
// the row's element 0, element j begins at output byte obase + (its position in the row's output).
template <bool WRITE>
__device__ int64_t wave_search_row(const uint8_t* b, int len, const uint8_t* d, int m, const uint8_t* rep, int r, int64_t maxhits, uint8_t* out,
                                   int32_t* eoffs, int32_t obase, int lane) {
    int64_t allowed = 0, k = 0;
    const int64_t grow = (int64_t)r - m;
    for (int base = 0; base < len; base += 64) {
        if (!WRITE && k >= maxhits) break;
        const int q = base + lane;
        const bool c = m > 0 && q + m <= len && b[q] == d[0] && utf8_bytes_at(b + q, d, m);
        const uint64_t cand = __ballot(c);
        const int64_t k0 = k, end0 = allowed;
        const uint64_t sel = utf8_select_hits(cand, base, m, maxhits, &allowed, &k);
        if (WRITE) {
            if (q < len) {
                int64_t h = 0;
                bool covered = false;
                utf8_window_byte(sel, lane, base, m, k0, end0, &h, &covered);
                if ((sel >> lane) & 1) {
                    if (eoffs) eoffs[h] = obase + (int32_t)(q + m + h * grow);
                } else if (!covered) out[q + h * grow] = b[q];
            }
            if (r > 0) {
                uint64_t s = sel;
                int64_t h = k0;
                while (s) {   // wave-uniform
                    const int i = first_lane(s);
                    s &= s - 1;
                    uint8_t* dst = out + (base + i) + h * grow;
                    ++h;
                    for (int j = lane; j < r; j += 64) dst[j] = rep[j];
                }
            }
        }
    }
    return k;
}
// translate / initcap of one row: its output bytes
template <int OP, bool WRITE>
__device__ int64_t wave_map_row(const uint8_t* b, int len, const Utf8TranslateTable* t, uint8_t* out, int lane) {
    int64_t o = 0;
    for (int base = 0; base < len; base += 64) {
        const int q = base + lane;
        Utf8Emit e = {0, 0, 0, 0};
        int adv = 0;
        if (q < len) e = OP == U8R_TRANSLATE ? utf8_translate_emit(b, len, q, *t, false, &adv) : utf8_initcap_emit(b, len, q, false, &adv);
        const int l = utf8_emit_len(e);
        const int incl = wave_inclusive_scan(l, lane);
        if (WRITE && l) utf8_emit_put(e, out + o + (incl - l));
        o += __shfl(incl, 63);
    }
    return o;
}

// the literals and the table into LDS (the same in every block)
template <int OP>
__device__ __forceinline__ void load_constants(const Utf8RewriteArgs& a, uint8_t* s_lit, uint8_t* s_rep, uint32_t* s_tab) {
    if (op_searches(OP)) {
        for (int i = threadIdx.x; i < a.lit_bytes; i += kThreads) s_lit[i] = a.lit[i];
        if (OP == U8R_REPLACE && s_rep)
            for (int i = threadIdx.x; i < a.rep_bytes; i += kThreads) s_rep[i] = a.rep[i];
    }
    if (OP == U8R_TRANSLATE) {
        const uint32_t* src = (const uint32_t*)a.table;
        for (int i = threadIdx.x; i < kTableWords; i += kThreads) s_tab[i] = src[i];
    }
    __syncthreads();
}

// ---- 1. size
template <int OP>
__global__ __launch_bounds__(kThreads) void utf8_rewrite_size_kernel(Utf8RewriteArgs a) {
    __shared__ uint8_t s_lit[op_searches(OP) ? kUtf8PatternMax : 16];
    __shared__ uint32_t s_tab[OP == U8R_TRANSLATE ? kTableWords : 4];
    __shared__ int s_nulls[kThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    load_constants<OP>(a, s_lit, nullptr, s_tab);   // (the size pass never reads the replacement)
    const Utf8TranslateTable* tab = (const Utf8TranslateTable*)s_tab;
    const int m = a.lit_bytes, rb = a.rep_bytes;
    // replace: nothing to count when the search is empty or the replacement as long as it; split: when no hit may split
    const bool reads = OP == U8R_REPLACE ? (m > 0 && rb != m) : OP == U8R_SPLIT ? a.maxhits > 0 : true;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const Utf8Chunk& ch = a.chunks[c];
        const int64_t r0 = (t - a.tile_start[c]) * kThreads + (int64_t)w * 64;
        const int64_t left = ch.rows - r0;
        const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        const int64_t r = r0 + lane;
        bool valid = false, is_long = false;
        int64_t out = 0, elems = 0;
        int32_t o0 = 0, o1 = 0;
        if (lane < nrows && row_valid(ch, r)) {
            valid = true;
            row_span(ch, r, o0, o1);
            const uint8_t* b = ch.data + o0;
            const int len = o1 - o0;
            out = len;
            elems = 1;
            if (reads && len > 0) {
                if (len > kUtf8ShortRow) is_long = true;
                else if (op_searches(OP)) {
                    const int64_t k = utf8_count_hits(b, len, s_lit, m, a.maxhits);
                    out = utf8_replace_bytes(len, k, m, OP == U8R_SPLIT ? 0 : rb);
                    elems = k + 1;
                } else out = OP == U8R_TRANSLATE ? utf8_translate_row(b, len, *tab, nullptr) : utf8_initcap_row(b, len, nullptr);
            }
        }
        uint64_t longs = __ballot(is_long);
        while (longs) {   // wave-uniform
            const int l = first_lane(longs);
            longs &= longs - 1;
            const int32_t q0 = __shfl(o0, l), q1 = __shfl(o1, l);
            const uint8_t* b = ch.data + q0;
            const int len = q1 - q0;
            int64_t res, el = 1;
            if (op_searches(OP)) {
                const int64_t k = wave_search_row<false>(b, len, s_lit, m, nullptr, 0, a.maxhits, nullptr, nullptr, 0, lane);
                res = utf8_replace_bytes(len, k, m, OP == U8R_SPLIT ? 0 : rb);
                el = k + 1;
            } else res = wave_map_row<OP, false>(b, len, tab, nullptr, lane);
            if (lane == l) { out = res; elems = el; }
        }
        if (lane < nrows) {
            const int64_t g = ch.row_start + r;
            a.blen[g] = utf8_build_clamp(out);
            if (OP == U8R_SPLIT) a.elen[g] = elems;
        }
        const uint64_t vmask = __ballot(valid);   // (the same in every lane of the block: the barriers are uniform)
        if (lane == 0) s_nulls[w] = nrows - __popcll(vmask);
        __syncthreads();
        if (threadIdx.x == 0) {
            int n = 0;
            for (int k = 0; k < kThreads / 64; ++k) n += s_nulls[k];
            if (n) atomicAdd(&a.null_counts[c], (unsigned long long)n);
        }
        __syncthreads();
    }
}

// ---- 2. per chunk totals (after the scans)
__global__ void utf8_rewrite_totals_kernel(Utf8RewriteArgs a) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.nchunks; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = a.chunks[c].row_start, e = s + a.chunks[c].rows;
        a.tot[3 * c] = a.bscan[e] - a.bscan[s];
        a.tot[3 * c + 1] = a.chunks[c].rows;
        a.tot[3 * c + 2] = a.op == U8R_SPLIT ? a.escan[e] - a.escan[s] : 0;
    }
}

// ---- 3. write
// one row's output by the wave: to `out`; split's child offsets from element 1 on
template <int OP>
__device__ __forceinline__ void wave_write_row(const Utf8RewriteArgs& a, const uint8_t* b, int len, const uint8_t* s_lit, const uint8_t* s_rep,
                                               const Utf8TranslateTable* tab, uint8_t* out, int32_t* eoffs, int32_t obase, int lane) {
    if (op_searches(OP))
        wave_search_row<true>(b, len, s_lit, a.lit_bytes, s_rep, OP == U8R_SPLIT ? 0 : a.rep_bytes, a.maxhits, out, OP == U8R_SPLIT ? eoffs : nullptr, obase, lane);
    else wave_map_row<OP, true>(b, len, tab, out, lane);
}

template <int OP>
__global__ __launch_bounds__(kThreads) void utf8_rewrite_write_kernel(Utf8RewriteArgs a) {
    __shared__ uint4 s_img[(kUtf8RewriteImage + 32) / 16];   // image byte i goes to the run's first destination byte - head + i
    __shared__ uint8_t s_lit[op_searches(OP) ? kUtf8PatternMax : 16];
    __shared__ uint8_t s_rep[OP == U8R_REPLACE ? kUtf8PatternMax : 16];
    __shared__ uint32_t s_tab[OP == U8R_TRANSLATE ? kTableWords : 4];
    __shared__ int64_t s_end[kThreads];   // where the output of the tile's rows ends (in the scan)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    load_constants<OP>(a, s_lit, s_rep, s_tab);
    const Utf8TranslateTable* tab = (const Utf8TranslateTable*)s_tab;
    if (blockIdx.x == 0)   // a chunk without rows has no tile: its one offset
        for (int64_t c = tid; c < a.nchunks; c += kThreads)
            if (a.outs[c].rows == 0) {
                a.outs[c].offs[0] = 0;
                if (OP == U8R_SPLIT) a.outs[c].list_offs[0] = 0;
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
            if (OP == U8R_SPLIT) {
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
            if (cnt == 0) {   // row p0's output alone exceeds the image: wave 0 writes it to HBM directly
                if (w == 0) {
                    const int64_t rr = tr0 + p0;
                    int32_t q0, q1;
                    row_span(ch, rr, q0, q1);
                    const int32_t ob = (int32_t)(base - o.byte_start);
                    int32_t* eo = OP == U8R_SPLIT ? o.offs + (a.escan[o.row_start + rr] - o.elem_start) : nullptr;
                    wave_write_row<OP>(a, ch.data + q0, q1 - q0, s_lit, s_rep, tab, o.data + ob, eo, ob, lane);
                }
                p0 += 1;
                continue;
            }
            const int p1 = p0 + cnt;
            const int span = (int)(s_end[p1 - 1] - base);
            if (span > 0 || OP == U8R_SPLIT) {   // (rows of a split without bytes still have elements)
                uint8_t* dst0 = o.data + (base - o.byte_start);
                const int head = (int)((uintptr_t)dst0 & 15);
                uint8_t* img = (uint8_t*)s_img + head;
                const bool mine = tid >= p0 && tid < p1 && valid;
                const int32_t ob = (int32_t)(b0 - o.byte_start);
                if (mine && len <= kUtf8ShortRow) {
                    const uint8_t* b = ch.data + o0;
                    uint8_t* out = img + (int)(b0 - base);
                    if (OP == U8R_REPLACE) utf8_replace_emit(b, len, s_lit, a.lit_bytes, s_rep, a.rep_bytes, a.maxhits, out, [](int64_t, int64_t) {});
                    else if (OP == U8R_SPLIT) {
                        int32_t* eo = o.offs + e0;
                        utf8_replace_emit(b, len, s_lit, a.lit_bytes, s_lit, 0, a.maxhits, out, [&](int64_t j, int64_t at) { eo[j] = ob + (int32_t)at; });
                    } else if (OP == U8R_TRANSLATE) utf8_translate_row(b, len, *tab, out);
                    else utf8_initcap_row(b, len, out);
                }
                uint64_t longs = __ballot(mine && len > kUtf8ShortRow);
                while (longs) {   // wave-uniform
                    const int l = first_lane(longs);
                    longs &= longs - 1;
                    const int32_t q0 = __shfl(o0, l), q1 = __shfl(o1, l), qob = __shfl(ob, l);
                    const int qat = __shfl((int)(b0 - base), l);
                    const int64_t qe0 = __shfl(e0, l);
                    wave_write_row<OP>(a, ch.data + q0, q1 - q0, s_lit, s_rep, tab, img + qat, OP == U8R_SPLIT ? o.offs + qe0 : nullptr, qob, lane);
                }
                if (span > 0) {
                    __syncthreads();
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

#define UTF8_REWRITE_DISPATCH(KERNEL, OPV, ...)                                                    \
    switch (OPV) {                                                                                 \
        case U8R_REPLACE: hipLaunchKernelGGL((KERNEL<U8R_REPLACE>), __VA_ARGS__); break;           \
        case U8R_TRANSLATE: hipLaunchKernelGGL((KERNEL<U8R_TRANSLATE>), __VA_ARGS__); break;       \
        case U8R_INITCAP: hipLaunchKernelGGL((KERNEL<U8R_INITCAP>), __VA_ARGS__); break;           \
        default: hipLaunchKernelGGL((KERNEL<U8R_SPLIT>), __VA_ARGS__); break;                      \
    }

hipError_t launch_utf8_rewrite_size(const Utf8RewriteArgs& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(a.ntiles, 256 * 16)), block(kThreads);
    UTF8_REWRITE_DISPATCH(utf8_rewrite_size_kernel, a.op, grid, block, 0, s, a)
    return hipGetLastError();
}
hipError_t launch_utf8_rewrite_totals(const Utf8RewriteArgs& a, hipStream_t s) {
    if (a.nchunks <= 0) return hipSuccess;
    const int64_t b = (a.nchunks + 255) / 256;
    hipLaunchKernelGGL(utf8_rewrite_totals_kernel, dim3((unsigned)(b > 65536 ? 65536 : b)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_rewrite_write(const Utf8RewriteArgs& a, hipStream_t s) {
    if (a.nchunks <= 0) return hipSuccess;
    // (without a tile one block still writes the one offset of every chunk, all of them empty)
    const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>(a.ntiles, 1), 256 * 16)), block(kThreads);
    UTF8_REWRITE_DISPATCH(utf8_rewrite_write_kernel, a.op, grid, block, 0, s, a)
    return hipGetLastError();
}
