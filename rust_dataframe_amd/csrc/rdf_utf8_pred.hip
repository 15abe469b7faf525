// rdf_utf8_pred.hip — the kernel of rdf_utf8_predicate / rdf_utf8_compare / rdf_utf8_measure: masks and integers from text
// (host side: rdf_capi_utf8_pred.inc; what is decided about one row, for hipcc and g++ alike: rdf_utf8_pattern.h).
//
// One pass, nothing but streaming.  A block of 256 lanes takes tiles of 256 rows of ONE chunk (the host's tile prefix, a
// binary search per tile); a wave owns 64 consecutive rows, starting on a multiple of 64 rows of its chunk.
//
//   phase 1   a lane per row: offs[r], offs[r + 1] clamped into the chunk's [lo, hi], the row's validity bit.  Ops whose
//             cost the pattern bounds (EQ .. GE, STARTS_WITH, ENDS_WITH against a literal, OCTET_LENGTH) always finish here;
//             ops that scan the row (CONTAINS, LIKE, LENGTH, LOCATE, column against column) finish here when the row has at
//             most kUtf8ShortRow bytes.  The lane runs the functions of rdf_utf8_pattern.h, the pattern sits in LDS.
//   phase 2   longer rows are collected with a ballot and taken by the whole wave one after the other (a wave-uniform
//             loop): the 64 lanes stride the row, 16 bytes a lane, 1 KiB a step.  LENGTH adds up the lanes' counts of
//             non-continuation bytes; a segment is searched by every lane at the start positions of its piece, the leftmost
//             hit is the first set lane of a ballot and ends the search; LOCATE counts the code points before the hit the
//             same way; a compare takes the first lane whose pieces differ.  One long row costs what its bytes cost.
//   output    the wave's results are one ballot word, its validity another (the input's bits re-aligned to bit 0, value =
//             result & valid): one lane stores each with one 8-byte store, the last, partial word of a chunk goes out byte
//             by byte, so nothing is written past (rows + 7) / 8 bytes and bits beyond the last row are 0.  Int32 results are
//             a store per lane.  No two waves write one byte; the same input gives the same bytes.
//   NULLs     counted per chunk only where the host does not know them: one integer add per block and tile.
//
// Reads stay inside the bytes the host checked: every row is clamped into [data + lo, data + hi) of its chunk, and the
// functions of rdf_utf8_pattern.h issue an 8-byte load only when it lies wholly inside the row they were handed.
#include <algorithm>

#include "rdf_utf8.h"
#include "rdf_utf8_pattern.h"

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

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ int first_lane(uint64_t mask) { return __builtin_ctzll(mask); }

constexpr int kPiece = 16, kStep = 64 * kPiece;   // bytes of a row a lane / the wave takes per step

// ---- the wave's forms of rdf_utf8_pattern.h's functions.  Every argument is the same in all 64 lanes, and so is the result.
// code points of [b, b + len)
__device__ int wave_count_code_points(const uint8_t* b, int len, int lane) {
    int c = 0;
    for (int off = lane * kPiece; off < len; off += kStep) c += (int)utf8_count_code_points(b + off, min(kPiece, len - off));
    return wave_sum(c);
}
// the byte offset of the start of code point number k (from 0) of [b, b + len); k == the row's code points gives len; -1: fewer
__device__ int wave_skip_code_points(const uint8_t* b, int len, int k, int lane) {
    if (k == 0) return 0;
    for (int base = 0; base < len; base += kStep) {
        const int off = base + lane * kPiece;
        const int n = min(kPiece, max(len - off, 0));
        const int cnt = n > 0 ? (int)utf8_count_code_points(b + off, n) : 0;
        const int incl = wave_inclusive_scan(cnt, lane);
        const int total = __shfl(incl, 63);
        if (k < total) {   // the start lies in this step, in the first lane whose prefix passes k
            const bool mine = incl > k && incl - cnt <= k;
            int at = -1;
            if (mine) {
                int c = incl - cnt;
                for (int j = 0; j < n; ++j) {
                    if (utf8_is_cont(b[off + j])) continue;
                    if (c == k) { at = off + j; break; }
                    ++c;
                }
            }
            return __shfl(at, first_lane(__ballot(mine)));
        }
        k -= total;
    }
    return k == 0 ? len : -1;
}
// the leftmost match of segment s inside [b + from, b + limit): offsets of its start and end
__device__ bool wave_find(const Utf8Pattern& pt, int s, const uint8_t* b, int from, int limit, int* start, int* end, int lane) {
    const int k0 = pt.seg_begin[s], n = pt.seg_begin[s + 1] - k0;
    if (n == 0) { *start = from; *end = from; return true; }
    const uint8_t* e = b + limit;
    for (int base = from; base + n <= limit; base += kStep) {
        int st = -1, en = -1;
        const int p0 = base + lane * kPiece;
        for (int j = 0; j < kPiece; ++j) {
            const int p = p0 + j;
            if (p + n > limit) break;
            if (!utf8_may_start(pt, k0, b + p)) continue;
            const uint8_t* m = nullptr;
            if (utf8_match_at(pt, s, b + p, e, &m)) { st = p; en = (int)(m - b); break; }
        }
        const uint64_t hits = __ballot(st >= 0);
        if (hits) {
            const int l = first_lane(hits);
            *start = __shfl(st, l);
            *end = __shfl(en, l);
            return true;
        }
    }
    return false;
}
__device__ bool wave_like(const Utf8Pattern& pt, const uint8_t* b, int len, int lane) {
    const uint8_t *p = b, *q = b + len;
    if (!utf8_like_ends(pt, b, b + len, &p, &q)) return false;   // bounded by the pattern: every lane walks it, all read the same bytes
    int cur = (int)(p - b);
    const int limit = (int)(q - b);
    for (int s = 1; s + 1 < pt.nseg; ++s) {
        int st = 0;
        if (!wave_find(pt, s, b, cur, limit, &st, &cur, lane)) return false;
    }
    return true;
}
__device__ int32_t wave_locate(const Utf8Pattern& pt, const uint8_t* b, int len, int32_t pos, int lane) {
    const int from = wave_skip_code_points(b, len, pos - 1, lane);
    if (from < 0) return 0;
    if (pt.nitems == 0) return pos;
    int st = 0, en = 0;
    if (!wave_find(pt, 0, b, from, len, &st, &en, lane)) return 0;
    return pos + wave_count_code_points(b + from, st - from, lane);
}
__device__ int wave_compare(const uint8_t* a, int na, const uint8_t* b, int nb, int lane) {
    const int n = min(na, nb);
    for (int base = 0; base < n; base += kStep) {
        const int off = base + lane * kPiece;
        const int k = min(kPiece, max(n - off, 0));
        const int c = k > 0 ? utf8_compare_bytes(a + off, k, b + off, k) : 0;
        const uint64_t diff = __ballot(c != 0);
        if (diff) return __shfl(c, first_lane(diff));
    }
    return na < nb ? -1 : (na > nb ? 1 : 0);
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

template <int FAM, bool MEASURE>
__global__ __launch_bounds__(kUtf8PredThreads) void utf8_pred_kernel(Utf8PredArgs a) {
    __shared__ Utf8Pattern pt;
    __shared__ int s_nulls[kUtf8PredThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (a.pattern) {
        const uint32_t* src = (const uint32_t*)a.pattern;
        uint32_t* dst = (uint32_t*)&pt;
        for (int i = threadIdx.x; i < (int)(sizeof(Utf8Pattern) / 4); i += kUtf8PredThreads) dst[i] = src[i];
    }
    __syncthreads();
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t c = find_tile_chunk(a.tile_start, a.nchunks, t);
        const Utf8Chunk& ca = a.a[c];
        const Utf8Chunk& cb = FAM == UTF8_FAM_COMPARE ? a.b[c] : ca;
        const int64_t r0 = (t - a.tile_start[c]) * kUtf8PredThreads + (int64_t)w * 64;
        const int64_t left = ca.rows - r0;
        const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        const int64_t r = r0 + lane;
        bool valid = false, is_long = false;
        int32_t val = 0, o0 = 0, o1 = 0, p0 = 0, p1 = 0;
        if (lane < nrows) {
            valid = !ca.valid || bit_at(ca.valid, ca.valid_off + r);
            if (FAM == UTF8_FAM_COMPARE) valid = valid && (!cb.valid || bit_at(cb.valid, cb.valid_off + r));
        }
        if (valid) {
            row_span(ca, r, o0, o1);
            const uint8_t *b = ca.data + o0, *e = ca.data + o1;
            const int len = o1 - o0;
            if (FAM == UTF8_FAM_LITERAL) {
                val = MEASURE ? len : (int32_t)utf8_predicate_row(pt, b, e);
            } else if (FAM == UTF8_FAM_SCAN) {
                if (MEASURE && a.op == U8M_LOCATE && a.pos < 1) val = 0;
                else if (len > kUtf8ShortRow) is_long = true;
                else if (MEASURE) val = a.op == U8M_LENGTH ? (int32_t)utf8_count_code_points(b, len) : utf8_locate_row(pt, b, e, a.pos);
                else val = (int32_t)utf8_predicate_row(pt, b, e);
            } else {
                row_span(cb, r, p0, p1);
                const int len_b = p1 - p0;
                if ((a.op == U8P_EQ || a.op == U8P_NE) && len != len_b) val = a.op == U8P_NE;   // (rows of different lengths read no byte)
                else if (max(len, len_b) > kUtf8ShortRow) is_long = true;
                else val = (int32_t)utf8_compare_result(a.op, utf8_compare_bytes(b, len, cb.data + p0, len_b));
            }
        }
        if (FAM != UTF8_FAM_LITERAL) {
            uint64_t longs = __ballot(is_long);
            while (longs) {   // wave-uniform
                const int l = first_lane(longs);
                longs &= longs - 1;
                const int32_t q0 = __shfl(o0, l), q1 = __shfl(o1, l);
                const uint8_t* b = ca.data + q0;
                const int len = q1 - q0;
                int32_t res;
                if (FAM == UTF8_FAM_SCAN) {
                    if (MEASURE) res = a.op == U8M_LENGTH ? wave_count_code_points(b, len, lane) : wave_locate(pt, b, len, a.pos, lane);
                    else if (pt.kind == U8P_CONTAINS) { int st = 0, en = 0; res = (int32_t)wave_find(pt, 0, b, 0, len, &st, &en, lane); }
                    else res = (int32_t)wave_like(pt, b, len, lane);
                } else {
                    const int32_t s0 = __shfl(p0, l), s1 = __shfl(p1, l);
                    res = (int32_t)utf8_compare_result(a.op, wave_compare(b, len, cb.data + s0, s1 - s0, lane));
                }
                if (lane == l) val = res;
            }
        }
        const uint64_t vmask = __ballot(valid);
        const uint64_t rmask = __ballot(valid && val != 0);
        if (nrows > 0) {
            const Utf8PredOut o = a.outs[c];
            if (MEASURE) {
                if (lane < nrows) ((int32_t*)o.values)[r] = valid ? val : 0;
            } else {
                store_word((uint8_t*)o.values, r0, nrows, rmask, lane);
            }
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

}  // namespace

hipError_t launch_utf8_pred(const Utf8PredArgs& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(a.ntiles, 256 * 16)), block(kUtf8PredThreads);
    if (a.family == UTF8_FAM_LITERAL) {
        if (a.measure) hipLaunchKernelGGL((utf8_pred_kernel<UTF8_FAM_LITERAL, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((utf8_pred_kernel<UTF8_FAM_LITERAL, false>), grid, block, 0, s, a);
    } else if (a.family == UTF8_FAM_SCAN) {
        if (a.measure) hipLaunchKernelGGL((utf8_pred_kernel<UTF8_FAM_SCAN, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((utf8_pred_kernel<UTF8_FAM_SCAN, false>), grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((utf8_pred_kernel<UTF8_FAM_COMPARE, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}
