// rdf_textfloat.hip — the kernels of rdf_utf8_parse_float / rdf_utf8_format_float (host side: rdf_capi_textconv.inc; what is
// decided about one row, for hipcc and g++ alike: rdf_textfloat.h).  Tile layout, LDS staging of a tile's bytes, ballot-word
// bitmaps and the LDS image of the write pass are those of rdf_textconv.hip, shared through rdf_texttile.hip.h: a block of 256
// lanes takes tiles of 256 rows of ONE chunk, a wave 64 consecutive rows, a lane a row.
//
//   parse     ONE streaming kernel, no scratch: scan the row, the 128-bit fast path, store the bits.  A row the fast path leaves
//             undecided stores 0 and sets its bit in the wave's flag word (one word per tile and wave, always written); the
//             undecided rows are counted like the failed ones, one add per block and tile and only when not zero.  A row longer
//             than kUtf8ShortRow stays on its lane: bounded by its bytes (a wave form is an open point).
//   resolve   launched by the host only when a chunk's undecided count is not zero: the same geometry, a lane looks at its bit
//             and runs the exact path (two big integers in scratch) out of global memory.
//   format    size (the length from the value) -> launch_scan -> the sizing rule on the host -> write through the LDS image of
//             the tile's output span and aligned 16-byte stores.
//   table     the 10 704 bytes of powers of ten are read from global memory through the caches; a copy in LDS per block was
//             measured against it and lost.
#include <algorithm>

#include "rdf_textfloat.h"
#include "rdf_texttile.hip.h"

#define RDF_TF_TABLE_QUAL __device__
#include "rdf_pow10_tables.h"

static_assert(kTfPow10TableMin == kTfPow10Min && kTfPow10TableMax == kTfPow10Max && kTfPow10TableExactMax == kTfPow10ExactMax, "rdf_textfloat.h restates the table's range");
static_assert(sizeof(kTfPow10) == sizeof(uint64_t) * kTfPow10Words, "the table's size");

namespace {

template <bool F32>
__global__ __launch_bounds__(kTcTile) void textfloat_parse_kernel(TfParseArgs a) {
    typedef TfType<F32> T;
    __shared__ uint4 s_img[kTcLdsBytes / 16 + 1];
    __shared__ int s_cnt[3 * (kTcTile / 64)];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t* tab = kTfPow10;
    uint8_t* img = (uint8_t*)s_img;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const Utf8Chunk& ch = a.chunks[c];
        const int64_t tr0 = (t - a.tile_start[c]) * kTcTile;
        const int64_t tleft = ch.rows - tr0;
        const int trows = tleft >= kTcTile ? kTcTile : (tleft > 0 ? (int)tleft : 0);
        // ---- the tile's bytes into LDS when they fit
        int32_t s0 = min(max(ch.offs[tr0], ch.lo), ch.hi);
        int32_t s1 = min(max(ch.offs[tr0 + trows], s0), ch.hi);
        const int span = s1 - s0;
        const bool staged = a.stage != 0 && span > 0 && span <= kTcLdsBytes;
        const uint8_t* g0 = ch.data + s0;
        const int head = (int)((uintptr_t)g0 & 15);   // image byte i is source byte g0 - head + i; the span is [head, head + span)
        if (staged) tile_stage_in(s_img, g0, head, span, kTcTile);
        __syncthreads();
        const int64_t r0 = tr0 + (int64_t)w * 64;
        const int64_t left = ch.rows - r0;
        const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        const int64_t r = r0 + lane;
        bool valid = false, ok = false, undecided = false;
        uint64_t bits = 0;
        if (lane < nrows) valid = !ch.valid || bit_at(ch.valid, ch.valid_off + r);
        if (valid) {
            int32_t o0, o1;
            row_span(ch, r, o0, o1);
            const bool in_img = staged && o0 >= s0 && o1 <= s1;
            const uint8_t* b = in_img ? img + head + (o0 - s0) : ch.data + o0;
            const TfScan sc = tf_scan(b, b + (o1 - o0));
            ok = sc.kind != TF_FAIL;
            if (sc.kind == TF_NAN) bits = T::QNAN;
            else if (sc.kind == TF_INF) bits = T::INF | (sc.neg ? T::SIGN : 0ull);
            else if (sc.kind == TF_NUM) {
                uint64_t mag = 0;
                undecided = a.exact != 0 || !tf_fast<F32>(tab, sc.m, sc.q, sc.sticky, &mag);
                bits = undecided ? 0ull : mag | (sc.neg ? T::SIGN : 0ull);
            }
        }
        const bool good = valid && ok;
        const uint64_t gmask = __ballot(good);
        const uint64_t fmask = __ballot(valid && !ok);
        const uint64_t umask = __ballot(undecided);
        if (nrows > 0) {
            const TcParseOut o = a.outs[c];
            if (lane < nrows) {
                if (F32) ((uint32_t*)o.values)[r] = (uint32_t)bits;
                else ((uint64_t*)o.values)[r] = bits;
            }
            store_word(o.valid, r0, nrows, gmask, lane);
        }
        if (lane == 0) {
            a.flags[t * (kTcTile / 64) + w] = umask;
            s_cnt[w] = nrows - __popcll(gmask);
            s_cnt[kTcTile / 64 + w] = __popcll(fmask);
            s_cnt[2 * (kTcTile / 64) + w] = __popcll(umask);
        }
        __syncthreads();   // (also: every lane is done with the image before the next tile overwrites it)
        if (threadIdx.x == 0) {
            int nn = 0, nf = 0, nu = 0;
            for (int k = 0; k < kTcTile / 64; ++k) { nn += s_cnt[k]; nf += s_cnt[kTcTile / 64 + k]; nu += s_cnt[2 * (kTcTile / 64) + k]; }
            if (nn) atomicAdd(&a.nulls[c], (unsigned long long)nn);
            if (nf) atomicAdd(&a.failed[c], (unsigned long long)nf);
            if (nu) atomicAdd(&a.undecided[c], (unsigned long long)nu);
        }
        __syncthreads();
    }
}

// the rows the parse kernel flagged, by the exact path: the value alone is written (the row is valid already)
template <bool F32>
__global__ __launch_bounds__(kTcTile) void textfloat_resolve_kernel(TfParseArgs a) {
    typedef TfType<F32> T;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const uint64_t word = a.flags[t * (kTcTile / 64) + w];
        if (!((word >> lane) & 1)) continue;
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const Utf8Chunk& ch = a.chunks[c];
        const int64_t r = (t - a.tile_start[c]) * kTcTile + (int64_t)w * 64 + lane;
        if (r >= ch.rows) continue;
        int32_t o0, o1;
        row_span(ch, r, o0, o1);
        const uint8_t* b = ch.data + o0;
        const uint8_t* e = b + (o1 - o0);
        const TfScan sc = tf_scan(b, e);
        if (sc.kind != TF_NUM) continue;
        const uint64_t bits = tf_exact<F32>(b, e) | (sc.neg ? T::SIGN : 0ull);
        const TcParseOut o = a.outs[c];
        if (F32) ((uint32_t*)o.values)[r] = (uint32_t)bits;
        else ((uint64_t*)o.values)[r] = bits;
    }
}

// ---------------------------------------------------------------------------------------------------------------- format
template <bool F32>
__device__ __forceinline__ uint64_t load_bits(const rdfk::DevChunkCol& c, int64_t r) {
    const int64_t i = c.offset + r;
    return F32 ? (uint64_t)((const uint32_t*)c.values)[i] : ((const uint64_t*)c.values)[i];
}

template <bool F32>
__global__ __launch_bounds__(kTcTile) void textfloat_size_kernel(TcFormatArgs a) {
    __shared__ int s_cnt[kTcTile / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t* tab = kTfPow10;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const rdfk::DevChunkCol ch = a.chunks[c];
        const int64_t rows = a.row_start[c + 1] - a.row_start[c];
        const int64_t r = (t - a.tile_start[c]) * kTcTile + threadIdx.x;
        bool valid = false;
        if (r < rows) {
            valid = !ch.validity || bit_at(ch.validity, ch.offset + r);
            a.blen[a.row_start[c] + r] = valid ? textfloat_length<F32>(tab, load_bits<F32>(ch, r)) : 0;
        }
        const uint64_t nmask = __ballot(r < rows && !valid);
        if (lane == 0) s_cnt[w] = __popcll(nmask);
        __syncthreads();
        if (threadIdx.x == 0) {
            int n = 0;
            for (int k = 0; k < kTcTile / 64; ++k) n += s_cnt[k];
            if (n) atomicAdd(&a.nulls[c], (unsigned long long)n);
        }
        __syncthreads();
    }
}

// one row's text into the image.  Kept out of line: inlined whole, Schubfach and the 17 unrolled digit positions take the write
// kernel from 57 to 81 VGPRs and from 8 to 5 waves a SIMD, and the format call 11 - 15 % more time.
template <bool F32>
__device__ __noinline__ void write_row(const uint64_t* tab, uint64_t bits, uint8_t* dst) {
    textfloat_write<F32>(tab, bits, dst);
}

constexpr int kTfImageBytes = kTcTile * kTfMaxRowF64 + 32;   // a tile's rows at the longest row, and the alignment slack

template <bool F32>
__global__ __launch_bounds__(kTcTile) void textfloat_write_kernel(TcFormatArgs a) {
    __shared__ uint4 s_img[kTfImageBytes / 16 + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (blockIdx.x == 0)   // a chunk without rows has no tile: its one offset
        for (int64_t c = threadIdx.x; c < a.nchunks; c += kTcTile)
            if (a.outs[c].rows == 0) a.outs[c].offs[0] = 0;
    const uint64_t* tab = kTfPow10;
    uint8_t* img = (uint8_t*)s_img;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const rdfk::DevChunkCol ch = a.chunks[c];
        const Utf8OutChunk& o = a.outs[c];
        const int64_t tr0 = (t - a.tile_start[c]) * kTcTile;
        const int64_t tleft = o.rows - tr0;
        const int trows = tleft >= kTcTile ? kTcTile : (int)tleft;
        const int64_t r = tr0 + threadIdx.x;
        const int64_t g = o.row_start + r;
        bool valid = false;
        int64_t b0 = 0, b1 = 0;
        if ((int)threadIdx.x < trows) {
            valid = !ch.validity || bit_at(ch.validity, ch.offset + r);
            b0 = a.bscan[g];
            b1 = a.bscan[g + 1];
            o.offs[r] = (int32_t)(b0 - o.byte_start);
            if (r == o.rows - 1) o.offs[o.rows] = (int32_t)(b1 - o.byte_start);
        }
        if (o.valid) {
            const int64_t r0 = tr0 + (int64_t)w * 64;
            const int nrows = (int)min((int64_t)64, max((int64_t)0, o.rows - r0));
            const uint64_t vmask = __ballot(valid);
            if (nrows > 0) store_word(o.valid, r0, nrows, vmask, lane);
        }
        const int64_t base = a.bscan[o.row_start + tr0], end = a.bscan[o.row_start + tr0 + trows];
        const int span = (int)(end - base);   // at most 256 rows of max_row bytes: the image holds the tile in one pass
        if (span > 0 && span <= kTcTile * a.max_row) {   // (the same in every lane of the block: the barriers are uniform)
            uint8_t* dst0 = o.data + (base - o.byte_start);
            const int head = (int)((uintptr_t)dst0 & 15);   // image byte i goes to dst0 - head + i; the span is [head, head + span)
            if ((int)threadIdx.x < trows && valid && b1 - b0 <= a.max_row && b0 >= base && b1 <= end)
                write_row<F32>(tab, load_bits<F32>(ch, r), img + head + (int)(b0 - base));
            __syncthreads();
            tile_stream_out(s_img, dst0, head, span, kTcTile);
            __syncthreads();
        }
    }
}

}  // namespace

#define TF_LAUNCH(KERNEL, ...)                                                     \
    if (f32) hipLaunchKernelGGL((KERNEL<true>), grid, block, 0, s, __VA_ARGS__);   \
    else hipLaunchKernelGGL((KERNEL<false>), grid, block, 0, s, __VA_ARGS__);

hipError_t launch_textfloat_parse(const TfParseArgs& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(a.ntiles, 256 * 16)), block(kTcTile);
    const bool f32 = a.f32 != 0;
    TF_LAUNCH(textfloat_parse_kernel, a)
    return hipGetLastError();
}
hipError_t launch_textfloat_resolve(const TfParseArgs& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(a.ntiles, 256 * 16)), block(kTcTile);
    const bool f32 = a.f32 != 0;
    TF_LAUNCH(textfloat_resolve_kernel, a)
    return hipGetLastError();
}
hipError_t launch_textfloat_size(const TcFormatArgs& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(a.ntiles, 256 * 16)), block(kTcTile);
    const bool f32 = a.dtype == RDF_F32;
    TF_LAUNCH(textfloat_size_kernel, a)
    return hipGetLastError();
}
hipError_t launch_textfloat_write(const TcFormatArgs& a, hipStream_t s) {
    if (a.nchunks <= 0) return hipSuccess;
    // (without a tile one block still writes the one offset of every chunk, all of them empty)
    const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>(a.ntiles, 1), 256 * 16)), block(kTcTile);
    const bool f32 = a.dtype == RDF_F32;
    TF_LAUNCH(textfloat_write_kernel, a)
    return hipGetLastError();
}
