// rdf_digest.hip — the kernels of rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32 (host side: rdf_capi_digest.inc; what
// is computed about one row, for hipcc and g++ alike: rdf_digest.h).
//
// The predicates' tiling: a block of 256 lanes takes tiles of 256 rows of ONE chunk (the host's tile prefix, a binary search
// per tile); a wave owns 64 consecutive rows, starting on a multiple of 64 rows of its chunk.  A lane takes one row at every
// length: these chains are sequential per row, so a long row cannot be spread over a wave.
// What can be balanced is where the long rows run: for the SHA-2 digests the rows of a tile above kUtf8ShortRow are compacted
// into an LDS list (span and output row) and dealt one to a lane from lane 0 of the block on, so that a tile's long rows
// share as few waves as hold them instead of keeping up to four waves busy with one live lane each.  Measured on a column with
// 1 % of its rows at 16 KiB that halves sha2(256)'s time; for MD5, SHA-1, crc32 and the hashes it did not pay, and
// they keep the plain form.
//
//   hash_columns_kernel<kind>   loops over the column descriptors; a fixed-width column costs one load and one hashInt /
//                               hashLong, a Utf8 column's bytes are walked by the row's lane.  One 4- or 8-byte store per
//                               row, coalesced; the validity, if asked for, is all ones.  No atomics.
//   utf8_digest_kernel<kind>    the width is fixed, so sizing is a count: utf8_digest_count_kernel counts the non-NULL rows
//                               of every tile, the scan of the counts gives a tile's first output row, a ballot gives a lane's.
//                               The state and the message schedule stay in registers (rdf_digest.h); the hex text goes out
//                               in 16-byte pieces where the row starts on a 16-byte boundary (rows of 32, 64, 96 and 128
//                               characters always do), in 8-byte ones otherwise.  NULL rows write no byte.
//   utf8_crc32_kernel           the 256-entry table in LDS, filled by the block, a byte a step.
//
// Reads stay inside the bytes the host checked: every row is clamped into [data + lo, data + hi) of its chunk, and the
// functions of rdf_digest.h issue a 4- or 8-byte load only when it lies wholly inside the row they were handed.
#include <algorithm>

#include "rdf_digest_kernels.h"
#include "rdf_digest.h"

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

// the wave's rows of tile t of chunk c: first row, how many
__device__ __forceinline__ int wave_rows(int64_t rows, int64_t tile_in_chunk, int w, int64_t& r0) {
    r0 = tile_in_chunk * kUtf8PredThreads + (int64_t)w * 64;
    const int64_t left = rows - r0;
    return left >= 64 ? 64 : (left > 0 ? (int)left : 0);
}

template <int KIND>
__global__ __launch_bounds__(kUtf8PredThreads) void hash_columns_kernel(HashColsArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        int64_t r0;
        const int nrows = wave_rows(a.row_start[c + 1] - a.row_start[c], t - a.tile_start[c], w, r0);
        if (nrows == 0) continue;
        const int64_t r = r0 + lane;
        const Utf8PredOut o = a.outs[c];
        if (lane < nrows) {
            uint64_t h = (uint64_t)a.seed;
            for (int k = 0; k < a.ncols; ++k) {   // (the descriptors are the same in every lane: scalar loads)
                const HashCol col = a.cols[k];
                if (col.utf8) {
                    const Utf8Chunk& u = col.utf8[c];
                    if (u.valid && !bit_at(u.valid, u.valid_off + r)) continue;
                    int32_t o0, o1;
                    row_span(u, r, o0, o1);
                    h = dg_hash_bytes<KIND>(u.data + o0, u.data + o1, h);
                } else {
                    const rdfk::DevChunkCol ch = col.num[c];
                    const int64_t i = ch.offset + r;
                    if (ch.validity && !bit_at(ch.validity, i)) continue;
                    uint64_t raw;
                    switch (dg_type_bytes(col.dtype)) {
                        case 0:  raw = bit_at((const uint8_t*)ch.values, i); break;
                        case 1:  raw = ((const uint8_t*)ch.values)[i]; break;
                        case 2:  raw = ((const uint16_t*)ch.values)[i]; break;
                        case 4:  raw = ((const uint32_t*)ch.values)[i]; break;
                        default: raw = ((const uint64_t*)ch.values)[i]; break;
                    }
                    h = dg_hash_fixed<KIND>(col.dtype, raw, h);
                }
            }
            if (KIND == DGH_MURMUR3_32) ((int32_t*)o.values)[r] = (int32_t)(uint32_t)h;
            else ((int64_t*)o.values)[r] = (int64_t)h;
        }
        if (o.valid) store_word(o.valid, r0, nrows, nrows == 64 ? ~0ull : (1ull << nrows) - 1, lane);
    }
}

__global__ __launch_bounds__(kUtf8PredThreads) void utf8_digest_count_kernel(Utf8DigestArgs a) {
    __shared__ int s_cnt[kUtf8PredThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const Utf8Chunk& u = a.chunks[c];
        int64_t r0;
        const int nrows = wave_rows(u.rows, t - a.tile_start[c], w, r0);
        const bool valid = lane < nrows && (!u.valid || bit_at(u.valid, u.valid_off + r0 + lane));
        const uint64_t vmask = __ballot(valid);
        if (lane == 0) s_cnt[w] = __popcll(vmask);
        __syncthreads();
        if (threadIdx.x == 0) {
            int n = 0;
            for (int k = 0; k < kUtf8PredThreads / 64; ++k) n += s_cnt[k];
            a.tile_count[t] = n;
        }
        __syncthreads();
    }
}

// per chunk: the rows that are not NULL, and the chunk's last offset
__global__ void utf8_digest_totals_kernel(Utf8DigestArgs a) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchunks) return;
    a.tot[c] = a.ntiles > 0 ? a.tile_scan[a.tile_start[c + 1]] - a.tile_scan[a.tile_start[c]] : 0;
}

// the long rows of a tile, compacted: the waves' counts -> this wave's first place in the block's list, the block's total
__device__ __forceinline__ int long_list_place(const int* s_long, int w, uint64_t lmask, int lane, int& total) {
    int p = 0;
    total = 0;
#pragma unroll
    for (int j = 0; j < kUtf8PredThreads / 64; ++j) {
        if (j < w) p += s_long[j];
        total += s_long[j];
    }
    return p + __popcll(lmask & ((1ull << lane) - 1));
}


// one row's hex text: 16-byte pieces where the row starts on a 16-byte boundary, 8-byte ones otherwise
template <int KIND>
__device__ __forceinline__ void digest_row_out(const uint8_t* b, const uint8_t* e, uint8_t* dst) {
    constexpr int kWords = digest_hex_bytes(KIND) / 8;
    uint64_t hex[kDigestHexWords];
    digest_row_hex<KIND>(b, e, hex);
    if (((uintptr_t)dst & 15) == 0) {
#pragma unroll
        for (int i = 0; i + 1 < kWords; i += 2) *(ulonglong2*)(dst + 8 * i) = make_ulonglong2(hex[i], hex[i + 1]);
        if (kWords & 1) *(uint64_t*)(dst + 8 * (kWords - 1)) = hex[kWords - 1];
    } else if (((uintptr_t)dst & 7) == 0) {
#pragma unroll
        for (int i = 0; i < kWords; ++i) *(uint64_t*)(dst + 8 * i) = hex[i];
    } else {
#pragma unroll
        for (int i = 0; i < kWords; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) dst[8 * i + j] = (uint8_t)(hex[i] >> (8 * j));
    }
}

template <int KIND>
__global__ __launch_bounds__(kUtf8PredThreads) void utf8_digest_kernel(Utf8DigestArgs a) {
    constexpr int kWidth = digest_hex_bytes(KIND);
    // the long rows of a tile are dealt out for SHA-2 only: measured, it halves the skewed column's time there and costs the short
    // pool nothing; MD5 and SHA-1 lost 3 % and 14 % on the short pool to its registers (profiles/digest_resources.md)
    constexpr bool DEAL = KIND >= DG_SHA224;
    __shared__ int s_cnt[kUtf8PredThreads / 64], s_long[kUtf8PredThreads / 64];
    __shared__ int32_t s_o0[DEAL ? kUtf8PredThreads : 1], s_o1[DEAL ? kUtf8PredThreads : 1];
    __shared__ int64_t s_k[DEAL ? kUtf8PredThreads : 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // the last offset of every chunk (chunks without rows have no tile)
    for (int64_t c = (int64_t)blockIdx.x * kUtf8PredThreads + threadIdx.x; c < a.nchunks; c += (int64_t)gridDim.x * kUtf8PredThreads)
        a.outs[c].offs[a.chunks[c].rows] = (int32_t)(a.tot[c] * kWidth);
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const Utf8Chunk& u = a.chunks[c];
        const Utf8OutChunk& o = a.outs[c];
        int64_t r0;
        const int nrows = wave_rows(u.rows, t - a.tile_start[c], w, r0);
        const int64_t r = r0 + lane;
        const bool valid = lane < nrows && (!u.valid || bit_at(u.valid, u.valid_off + r));
        int32_t o0 = 0, o1 = 0;
        if (valid) row_span(u, r, o0, o1);
        const bool is_long = DEAL && o1 - o0 > kUtf8ShortRow;
        const uint64_t vmask = __ballot(valid), lmask = __ballot(is_long);
        if (lane == 0) { s_cnt[w] = __popcll(vmask); s_long[w] = __popcll(lmask); }
        __syncthreads();
        int64_t k = a.tile_scan[t] - a.tile_scan[a.tile_start[c]];   // the tile's first output row of its chunk
        for (int j = 0; j < w; ++j) k += s_cnt[j];
        k += __popcll(vmask & ((1ull << lane) - 1));
        if (lane < nrows) o.offs[r] = (int32_t)(k * kWidth);
        if (valid && !is_long) digest_row_out<KIND>(u.data + o0, u.data + o1, o.data + k * kWidth);
        if (nrows > 0 && o.valid) store_word(o.valid, r0, nrows, vmask, lane);
        if (DEAL) {   // the tile's long rows, one to a lane from lane 0 of the block on: they run side by side in as few waves as hold them
            int nlong;
            const int p = long_list_place(s_long, w, lmask, lane, nlong);
            if (nlong > 0) {   // (the same in every lane of the block: the barriers are uniform)
                if (is_long) { s_o0[p] = o0; s_o1[p] = o1; s_k[p] = k; }
                __syncthreads();
                if ((int)threadIdx.x < nlong)
                    digest_row_out<KIND>(u.data + s_o0[threadIdx.x], u.data + s_o1[threadIdx.x], o.data + s_k[threadIdx.x] * kWidth);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kUtf8PredThreads) void utf8_crc32_kernel(Utf8Crc32Args a) {
    __shared__ uint32_t s_table[256];
    __shared__ int s_nulls[kUtf8PredThreads / 64];
    static_assert(kUtf8PredThreads == 256, "a table entry a lane");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    s_table[threadIdx.x] = crc32_table_entry(threadIdx.x);
    __syncthreads();
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const Utf8Chunk& u = a.chunks[c];
        int64_t r0;
        const int nrows = wave_rows(u.rows, t - a.tile_start[c], w, r0);
        const int64_t r = r0 + lane;
        const bool valid = lane < nrows && (!u.valid || bit_at(u.valid, u.valid_off + r));
        int64_t val = 0;
        if (valid) {
            int32_t o0, o1;
            row_span(u, r, o0, o1);
            val = (int64_t)crc32_row(u.data + o0, u.data + o1, s_table);
        }
        const uint64_t vmask = __ballot(valid);
        if (nrows > 0) {
            const Utf8PredOut o = a.outs[c];
            if (lane < nrows) ((int64_t*)o.values)[r] = val;
            if (o.valid) store_word(o.valid, r0, nrows, vmask, lane);
        }
        if (a.nulls) {   // (the same in every lane of the block: the barriers are uniform)
            if (lane == 0) s_nulls[w] = nrows - __popcll(vmask);
            __syncthreads();
            if (threadIdx.x == 0) {
                int n = 0;
                for (int k = 0; k < kUtf8PredThreads / 64; ++k) n += s_nulls[k];
                if (n) atomicAdd(&a.nulls[c], (unsigned long long)n);
            }
            __syncthreads();
        }
    }
}

dim3 tile_grid(int64_t ntiles) { return dim3((unsigned)std::min<int64_t>(ntiles, 256 * 16)); }

}  // namespace

hipError_t launch_hash_columns(const HashColsArgs& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const dim3 block(kUtf8PredThreads);
    if (a.kind == DGH_MURMUR3_32) hipLaunchKernelGGL((hash_columns_kernel<DGH_MURMUR3_32>), tile_grid(a.ntiles), block, 0, s, a);
    else hipLaunchKernelGGL((hash_columns_kernel<DGH_XXHASH64>), tile_grid(a.ntiles), block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_utf8_digest_count(const Utf8DigestArgs& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(utf8_digest_count_kernel, tile_grid(a.ntiles), dim3(kUtf8PredThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_digest_totals(const Utf8DigestArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(utf8_digest_totals_kernel, dim3((unsigned)((a.nchunks + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_digest_write(const Utf8DigestArgs& a, hipStream_t s) {
    const dim3 grid = tile_grid(std::max<int64_t>(a.ntiles, 1)), block(kUtf8PredThreads);
    switch (a.kind) {
        case DG_MD5:    hipLaunchKernelGGL((utf8_digest_kernel<DG_MD5>), grid, block, 0, s, a); break;
        case DG_SHA1:   hipLaunchKernelGGL((utf8_digest_kernel<DG_SHA1>), grid, block, 0, s, a); break;
        case DG_SHA224: hipLaunchKernelGGL((utf8_digest_kernel<DG_SHA224>), grid, block, 0, s, a); break;
        case DG_SHA256: hipLaunchKernelGGL((utf8_digest_kernel<DG_SHA256>), grid, block, 0, s, a); break;
        case DG_SHA384: hipLaunchKernelGGL((utf8_digest_kernel<DG_SHA384>), grid, block, 0, s, a); break;
        default:        hipLaunchKernelGGL((utf8_digest_kernel<DG_SHA512>), grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_utf8_crc32(const Utf8Crc32Args& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(utf8_crc32_kernel, tile_grid(a.ntiles), dim3(kUtf8PredThreads), 0, s, a);
    return hipGetLastError();
}
