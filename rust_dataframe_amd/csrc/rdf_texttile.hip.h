// rdf_texttile.hip.h — what the text-conversion kernels (rdf_textconv.hip, rdf_textfloat.hip) share about a tile: a block of
// 256 lanes takes 256 rows of ONE chunk, a wave 64 consecutive rows that start on a multiple of 64 rows of its chunk.  The
// chunk search over the host's tile prefix, bitmaps as ballot words, a row's clamped span, and the two block-wide copies
// between global memory and an LDS image that keeps the global side's alignment modulo 16 (§22.3).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdf_utf8.h"

namespace {

__device__ __forceinline__ bool bit_at(const uint8_t* b, int64_t i) { return (b[i >> 3] >> (i & 7)) & 1; }

// last chunk whose first tile is <= t (empty chunks share the first tile of the next one and are skipped by this rule)
__device__ int64_t find_tile_chunk(const int64_t* ts, int64_t nch, int64_t t) {
    int64_t lo = 0, hi = nch;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ts[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
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

// The whole block brings `span` bytes at g0 into the image: image byte i is source byte g0 - head + i, head = g0 mod 16, so
// the span is [head, head + span).  Aligned 16-byte pieces go as uint4 loads, the partial pieces at the two ends byte by byte.
// The image holds at least head + span bytes rounded up to 16.  The caller synchronizes.
__device__ __forceinline__ void tile_stage_in(uint4* image, const uint8_t* g0, int head, int span, int threads) {
    uint8_t* img = (uint8_t*)image;
    const int npieces = (head + span + 15) >> 4;
    for (int k = threadIdx.x; k < npieces; k += threads) {
        const int i0 = k << 4;
        if (i0 >= head && i0 + 16 <= head + span) image[k] = *(const uint4*)(g0 - head + i0);
        else
            for (int i = max(i0, head); i < min(i0 + 16, head + span); ++i) img[i] = g0[i - head];
    }
}
// The inverse: image byte i goes to dst0 - head + i, head = dst0 mod 16; whole aligned pieces as uint4 stores.
__device__ __forceinline__ void tile_stream_out(const uint4* image, uint8_t* dst0, int head, int span, int threads) {
    const uint8_t* img = (const uint8_t*)image;
    const int npieces = (head + span + 15) >> 4;
    for (int k = threadIdx.x; k < npieces; k += threads) {
        const int i0 = k << 4;
        if (i0 >= head && i0 + 16 <= head + span) *(uint4*)(dst0 - head + i0) = image[k];
        else
            for (int i = max(i0, head); i < min(i0 + 16, head + span); ++i) dst0[i - head] = img[i];
    }
}

}  // namespace
