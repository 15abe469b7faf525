// rdf_textconv.hip — the kernels of rdf_utf8_parse / rdf_utf8_format: text to values and back (host side:
// rdf_capi_textconv.inc; what is decided about one row, for hipcc and g++ alike: rdf_textconv.h).  The tile layout is that of
// rdf_utf8_pred.hip: a block of 256 lanes takes tiles of 256 rows of ONE chunk (the host's tile prefix), a wave owns 64
// consecutive rows that start on a multiple of 64 rows of its chunk, a lane a row; validity and Boolean results are ballot
// words written under store_word's rules, so no two waves write one byte and the same input gives the same bytes.
//
//   parse    ONE streaming kernel.  The bytes of a tile's rows are one contiguous span [offs[r0], offs[r0 + 256)), clamped
//            into the chunk's checked [lo, hi].  A span of at most kTcLdsBytes is brought into LDS by the whole block: the
//            pieces that are aligned 16-byte words of the source go as uint4 loads, the partial pieces at the two ends byte
//            by byte, and the image keeps the source's alignment modulo 16.  The lanes then parse out of LDS.  A longer span
//            (or a row whose offsets leave the tile's span) is read from global memory by its lane: the same functions over
//            the same bytes, so both forms give the same results.  A row of a CAST grammar longer than kUtf8ShortRow bytes is
//            taken by its wave: ballots over 16-byte pieces find the trimmed span, for INT the end of the leading zeros and
//            whether a fraction's tail is all digits; what is left is bounded (a sign, 20 digits, a date, five letters) and
//            is parsed once, the same in every lane.  Pattern rows need none of this: the pattern bounds what a row can cost.
//   format   size (a lane per row: the length from the value, no text is read) -> launch_scan -> the sizing rule on the host
//            -> write: a lane writes its row's text into the block's LDS image of the tile's output span, which keeps the
//            destination's alignment modulo 16; the block then streams the image out, whole aligned 16-byte pieces as uint4
//            stores, the partial pieces at the two ends of the span byte by byte.  The image holds as many waves' rows as fit
//            32 KiB (256 rows up to 128 bytes a row, 128 rows up to the 256-byte cap): a tile goes out in one or two passes.
//   counts   NULL rows and failed rows: one integer add each per block and tile, and only when not zero.
#include <algorithm>

#include "rdf_textconv.h"
#include "rdf_texttile.hip.h"

namespace {

__device__ __forceinline__ int first_lane(uint64_t mask) { return __builtin_ctzll(mask); }

constexpr int kPiece = 16, kStep = 64 * kPiece;   // bytes of a row a lane / the wave takes per step
enum : int { CLS_WS = 0, CLS_ZERO = 1, CLS_DIGIT = 2 };
__device__ __forceinline__ bool in_class(uint8_t c, int cls) { return cls == CLS_WS ? tc_is_ws(c) : cls == CLS_ZERO ? c == '0' : tc_is_digit(c); }

// ---- the wave's searches.  Every argument is the same in all 64 lanes, and so is the result.
// the first index in [from, to) whose byte is not of the class; `to` when there is none
__device__ int wave_first_not(const uint8_t* b, int from, int to, int cls, int lane) {
    for (int base = from; base < to; base += kStep) {
        const int off = base + lane * kPiece;
        const int n = min(kPiece, max(to - off, 0));
        int at = -1;
        for (int j = 0; j < n; ++j)
            if (!in_class(b[off + j], cls)) { at = off + j; break; }
        const uint64_t hits = __ballot(at >= 0);
        if (hits) return __shfl(at, first_lane(hits));
    }
    return to;
}
// one past the last index in [from, to) whose byte is not white space; `from` when there is none
__device__ int wave_last_not_ws(const uint8_t* b, int from, int to, int lane) {
    for (int base = to; base > from; base -= kStep) {
        const int hi = base - lane * kPiece;          // the lane's piece is [max(hi - 16, from), hi)
        const int lo = max(hi - kPiece, from);
        int at = -1;
        for (int j = hi - 1; j >= lo; --j)
            if (!tc_is_ws(b[j])) { at = j + 1; break; }
        const uint64_t hits = __ballot(at >= 0);
        if (hits) return __shfl(at, first_lane(hits));
    }
    return from;
}

// one row that a lane takes whole: [b, e) -> the value's bits
template <int KIND, bool PAT>
__device__ __forceinline__ bool parse_row(const TcParseArgs& a, const TcPattern& pt, const uint8_t* b, const uint8_t* e, uint64_t* bits) {
    if (KIND == TC_BOOL) {
        bool v = false;
        const bool ok = textconv_parse_bool(b, e, &v);
        *bits = v ? 1u : 0u;
        return ok;
    }
    if (KIND == TC_INT) return textconv_parse_int(b, e, a.dtype, bits);
    if (KIND == TC_DATE) {
        int32_t d = 0;
        const bool ok = PAT ? textconv_parse_date_pattern(pt, b, e, &d) : textconv_parse_date(b, e, &d);
        *bits = (uint64_t)(int64_t)d;
        return ok;
    }
    int64_t v = 0;
    const bool ok = PAT ? textconv_parse_timestamp_pattern(pt, b, e, a.unit, &v) : textconv_parse_timestamp(b, e, a.unit, &v);
    *bits = (uint64_t)v;
    return ok;
}

// a long row of a CAST grammar, by the whole wave: the same in every lane
template <int KIND>
__device__ bool wave_parse_row(const TcParseArgs& a, const uint8_t* b, int len, uint64_t* bits, int lane) {
    const int s = wave_first_not(b, 0, len, CLS_WS, lane);
    if (s == len) return false;
    const int e = wave_last_not_ws(b, s, len, lane);
    if (KIND == TC_BOOL) {
        if (e - s > 5) return false;
        bool v = false;
        const bool ok = textconv_parse_bool_trimmed(b + s, b + e, &v);
        *bits = v ? 1u : 0u;
        return ok;
    }
    if (KIND == TC_INT) {
        int p = s;
        bool neg = false;
        if (b[p] == '+' || b[p] == '-') { neg = b[p] == '-'; ++p; }
        const int z = wave_first_not(b, p, e, CLS_ZERO, lane);
        const uint8_t* frac = nullptr;
        if (!tc_int_core(b + z, b + e, neg, z > p, a.dtype, bits, &frac)) return false;   // at most 20 digits before it must stop
        return !frac || wave_first_not(b, (int)(frac - b), e, CLS_DIGIT, lane) == e;
    }
    if (KIND == TC_DATE) {   // a date and the byte after it are at most 15 bytes: what follows the window cannot change the result
        int32_t d = 0;
        const bool ok = textconv_parse_date_trimmed(b + s, b + min(e, s + 16), &d);
        *bits = (uint64_t)(int64_t)d;
        return ok;
    }
    int64_t v = 0;   // (a fraction of thousands of digits is walked by every lane alike: see DESIGN, open points)
    const bool ok = textconv_parse_timestamp_trimmed(b + s, b + e, a.unit, &v);
    *bits = (uint64_t)v;
    return ok;
}

template <int KIND, bool PAT>
__global__ __launch_bounds__(kTcTile) void textconv_parse_kernel(TcParseArgs a) {
    __shared__ uint4 s_img[kTcLdsBytes / 16 + 1];
    __shared__ TcPattern s_pat;
    __shared__ int s_cnt[2 * (kTcTile / 64)];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (PAT) {
        const uint32_t* src = (const uint32_t*)a.pattern;
        uint32_t* dst = (uint32_t*)&s_pat;
        for (int i = threadIdx.x; i < (int)(sizeof(TcPattern) / 4); i += kTcTile) dst[i] = src[i];
    }
    __syncthreads();
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
        if (staged) {
            const int npieces = (head + span + 15) >> 4;
            for (int k = threadIdx.x; k < npieces; k += kTcTile) {
                const int i0 = k << 4;
                if (i0 >= head && i0 + 16 <= head + span) s_img[k] = *(const uint4*)(g0 - head + i0);
                else
                    for (int i = max(i0, head); i < min(i0 + 16, head + span); ++i) img[i] = g0[i - head];
            }
        }
        __syncthreads();
        const int64_t r0 = tr0 + (int64_t)w * 64;
        const int64_t left = ch.rows - r0;
        const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        const int64_t r = r0 + lane;
        bool valid = false, ok = false, is_long = false, in_img = false;
        uint64_t bits = 0;
        int32_t o0 = 0, o1 = 0;
        if (lane < nrows) valid = !ch.valid || bit_at(ch.valid, ch.valid_off + r);
        if (valid) {
            row_span(ch, r, o0, o1);
            in_img = staged && o0 >= s0 && o1 <= s1;
            const uint8_t* b = in_img ? img + head + (o0 - s0) : ch.data + o0;
            const int len = o1 - o0;
            if (!PAT && len > kUtf8ShortRow) is_long = true;
            else ok = parse_row<KIND, PAT>(a, s_pat, b, b + len, &bits);
        }
        if (!PAT) {
            uint64_t longs = __ballot(is_long);
            while (longs) {   // wave-uniform
                const int l = first_lane(longs);
                longs &= longs - 1;
                const int32_t q0 = __shfl(o0, l), q1 = __shfl(o1, l);
                const bool qi = __shfl((int)in_img, l) != 0;
                const uint8_t* b = qi ? img + head + (q0 - s0) : ch.data + q0;
                uint64_t res = 0;
                const bool rok = wave_parse_row<KIND>(a, b, q1 - q0, &res, lane);
                if (lane == l) { ok = rok; bits = res; }
            }
        }
        const bool good = valid && ok;
        const uint64_t gmask = __ballot(good);
        const uint64_t fmask = __ballot(valid && !ok);
        if (nrows > 0) {
            const TcParseOut o = a.outs[c];
            const uint64_t v = good ? bits : 0ull;
            if (KIND == TC_BOOL) {
                store_word((uint8_t*)o.values, r0, nrows, __ballot(good && bits != 0), lane);
            } else if (lane < nrows) {
                switch (a.dtype & 3) {
                    case 0: ((uint8_t*)o.values)[r] = (uint8_t)v; break;
                    case 1: ((uint16_t*)o.values)[r] = (uint16_t)v; break;
                    case 2: ((uint32_t*)o.values)[r] = (uint32_t)v; break;
                    default: ((uint64_t*)o.values)[r] = v; break;
                }
            }
            store_word(o.valid, r0, nrows, gmask, lane);
        }
        if (lane == 0) {
            s_cnt[w] = nrows - __popcll(gmask);
            s_cnt[kTcTile / 64 + w] = __popcll(fmask);
        }
        __syncthreads();   // (also: every lane is done with the image before the next tile overwrites it)
        if (threadIdx.x == 0) {
            int nn = 0, nf = 0;
            for (int k = 0; k < kTcTile / 64; ++k) { nn += s_cnt[k]; nf += s_cnt[kTcTile / 64 + k]; }
            if (nn) atomicAdd(&a.nulls[c], (unsigned long long)nn);
            if (nf) atomicAdd(&a.failed[c], (unsigned long long)nf);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- format
// the value of row r of a chunk, extended to 64 bits (Boolean: 0 / 1)
__device__ __forceinline__ uint64_t load_bits(const rdfk::DevChunkCol& c, int64_t r, int dtype) {
    const int64_t i = c.offset + r;
    switch (dtype) {
        case RDF_I8: return (uint64_t)(int64_t)((const int8_t*)c.values)[i];
        case RDF_I16: return (uint64_t)(int64_t)((const int16_t*)c.values)[i];
        case RDF_I32: return (uint64_t)(int64_t)((const int32_t*)c.values)[i];
        case RDF_U8: return ((const uint8_t*)c.values)[i];
        case RDF_U16: return ((const uint16_t*)c.values)[i];
        case RDF_U32: return ((const uint32_t*)c.values)[i];
        case RDF_BOOL: return bit_at((const uint8_t*)c.values, i) ? 1u : 0u;
        default: return ((const uint64_t*)c.values)[i];
    }
}

template <bool PAT>
__global__ __launch_bounds__(kTcTile) void textconv_size_kernel(TcFormatArgs a) {
    __shared__ TcPattern s_pat;
    __shared__ int s_cnt[kTcTile / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (PAT) {
        const uint32_t* src = (const uint32_t*)a.pattern;
        uint32_t* dst = (uint32_t*)&s_pat;
        for (int i = threadIdx.x; i < (int)(sizeof(TcPattern) / 4); i += kTcTile) dst[i] = src[i];
    }
    __syncthreads();
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const rdfk::DevChunkCol ch = a.chunks[c];
        const int64_t rows = a.row_start[c + 1] - a.row_start[c];
        const int64_t r = (t - a.tile_start[c]) * kTcTile + threadIdx.x;
        bool valid = false;
        if (r < rows) {
            valid = !ch.validity || bit_at(ch.validity, ch.offset + r);
            a.blen[a.row_start[c] + r] = valid ? textconv_length(a.kind, a.dtype, a.unit, PAT ? &s_pat : nullptr, load_bits(ch, r, a.dtype)) : 0;
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

__global__ void textconv_totals_kernel(TcFormatArgs a) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.nchunks; c += (int64_t)gridDim.x * blockDim.x)
        a.tot[c] = a.bscan[a.row_start[c + 1]] - a.bscan[a.row_start[c]];
}

// rows of a tile whose text the LDS image holds at a time: whole waves, at most 32 KiB
__host__ __device__ inline int write_pass_rows(int max_row) {
    const int waves = (32 * 1024) / (64 * (max_row > 0 ? max_row : 1));
    return 64 * (waves < 1 ? 1 : waves > kTcTile / 64 ? kTcTile / 64 : waves);
}

template <bool PAT>
__global__ __launch_bounds__(kTcTile) void textconv_write_kernel(TcFormatArgs a) {
    extern __shared__ uint4 s_dyn[];   // the image: write_pass_rows * max_row bytes + 32
    __shared__ TcPattern s_pat;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (PAT) {
        const uint32_t* src = (const uint32_t*)a.pattern;
        uint32_t* dst = (uint32_t*)&s_pat;
        for (int i = threadIdx.x; i < (int)(sizeof(TcPattern) / 4); i += kTcTile) dst[i] = src[i];
    }
    if (blockIdx.x == 0)   // a chunk without rows has no tile: its one offset
        for (int64_t c = threadIdx.x; c < a.nchunks; c += kTcTile)
            if (a.outs[c].rows == 0) a.outs[c].offs[0] = 0;
    __syncthreads();
    uint8_t* img = (uint8_t*)s_dyn;
    const int prows = write_pass_rows(a.max_row);
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
        for (int p0 = 0; p0 < trows; p0 += prows) {
            const int p1 = min(p0 + prows, trows);
            const int64_t base = a.bscan[o.row_start + tr0 + p0], end = a.bscan[o.row_start + tr0 + p1];
            const int span = (int)(end - base);
            if (span > 0) {   // (the same in every lane of the block: the barriers are uniform)
                uint8_t* dst0 = o.data + (base - o.byte_start);
                const int head = (int)((uintptr_t)dst0 & 15);   // image byte i goes to dst0 - head + i; the span is [head, head + span)
                if ((int)threadIdx.x >= p0 && (int)threadIdx.x < p1 && valid && b1 - b0 <= a.max_row)
                    textconv_write(a.kind, a.dtype, a.unit, PAT ? &s_pat : nullptr, load_bits(ch, r, a.dtype), img + head + (int)(b0 - base));
                __syncthreads();
                const int npieces = (head + span + 15) >> 4;
                for (int k = threadIdx.x; k < npieces; k += kTcTile) {
                    const int i0 = k << 4;
                    if (i0 >= head && i0 + 16 <= head + span) *(uint4*)(dst0 - head + i0) = s_dyn[k];
                    else
                        for (int i = max(i0, head); i < min(i0 + 16, head + span); ++i) dst0[i - head] = img[i];
                }
                __syncthreads();
            }
        }
    }
}

}  // namespace

#define TC_PARSE_LAUNCH(KIND)                                                                                        \
    if (a.pattern) hipLaunchKernelGGL((textconv_parse_kernel<KIND, true>), grid, block, 0, s, a);                    \
    else hipLaunchKernelGGL((textconv_parse_kernel<KIND, false>), grid, block, 0, s, a);

hipError_t launch_textconv_parse(const TcParseArgs& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(a.ntiles, 256 * 16)), block(kTcTile);
    switch (a.kind) {
        case TC_BOOL: hipLaunchKernelGGL((textconv_parse_kernel<TC_BOOL, false>), grid, block, 0, s, a); break;
        case TC_INT: hipLaunchKernelGGL((textconv_parse_kernel<TC_INT, false>), grid, block, 0, s, a); break;
        case TC_DATE: TC_PARSE_LAUNCH(TC_DATE) break;
        default: TC_PARSE_LAUNCH(TC_TIMESTAMP) break;
    }
    return hipGetLastError();
}
hipError_t launch_textconv_size(const TcFormatArgs& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(a.ntiles, 256 * 16)), block(kTcTile);
    if (a.pattern) hipLaunchKernelGGL((textconv_size_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((textconv_size_kernel<false>), grid, block, 0, s, a);
    return hipGetLastError();
}
hipError_t launch_textconv_totals(const TcFormatArgs& a, hipStream_t s) {
    if (a.nchunks <= 0) return hipSuccess;
    const int64_t b = (a.nchunks + 255) / 256;
    hipLaunchKernelGGL(textconv_totals_kernel, dim3((unsigned)(b > 65536 ? 65536 : b)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_textconv_write(const TcFormatArgs& a, hipStream_t s) {
    if (a.nchunks <= 0) return hipSuccess;
    // (without a tile one block still writes the one offset of every chunk, all of them empty)
    const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>(a.ntiles, 1), 256 * 16)), block(kTcTile);
    const size_t lds = (size_t)write_pass_rows(a.max_row) * (size_t)a.max_row + 32;
    if (a.pattern) hipLaunchKernelGGL((textconv_write_kernel<true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((textconv_write_kernel<false>), grid, block, lds, s, a);
    return hipGetLastError();
}
