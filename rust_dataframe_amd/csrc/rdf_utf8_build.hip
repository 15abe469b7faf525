// rdf_utf8_build.hip — the kernels of rdf_utf8_concat / _pad / _repeat / _reverse / _substring_index: text columns made of
// more than one source (host side: rdf_capi_utf8_build.inc; what is decided about one row, for hipcc and g++ alike:
// rdf_utf8_build.h).  The span -> scan -> write engine of rdf_utf8.hip with its one assumption lifted: a row is a sequence
// of pieces instead of one span.  Output chunk c holds the rows of input chunk c.
//
//   size    the tiles of rdf_utf8_pred.hip: a block takes 256 rows of ONE chunk, a lane a row.  One read of every part's
//           offsets and validity bit gives the row's validity, its output length and a 31-bit note for the write pass (concat:
//           which parts are present; pad: the kept bytes of the row; substring_index: where the span starts; coalesce /
//           case_when (rdf_utf8_coalesce / rdf_utf8_case_when): the chosen part, O(1) per row from offsets and bitmaps).  Row bytes are
//           read only by pad (code points) and substring_index (the search): rows up to kUtf8ShortRow bytes on their lane
//           through rdf_utf8_build.h, longer ones by the whole wave one after the other, 16 bytes a lane and 1 KiB a step
//           (the occurrences of a delimiter are the set bits of the lanes' 16 start positions: the count-th one is found by
//           a prefix sum of the lanes' popcounts, from either end).  NULL rows are counted per wave: one add per block and tile.
//   scan    launch_scan over the lengths; the host applies the sizing rule to the per-chunk totals before anything is written.
//   write   offsets + validity per row (a lane per row; the word-wise atomicOr of utf8_place_kernel), then the copy, driven
//           by the DESTINATION: a lane owns one aligned 16-byte piece of the output, finds its row by a search over the
//           tile's output offsets in LDS (in HBM when more than kUtf8WindowRows rows end inside the tile), and its source
//           bytes through the piece function of rdf_utf8_build.h: part k of a concat row, the position modulo the pad / row
//           period, the mirror position for reverse.  K parts are read once and written once: there is no intermediate
//           column.  A 10 000-byte row costs its bytes; it never sits on one lane.  No atomics touch data bytes or offsets.
#include <algorithm>

#include "rdf_utf8.h"
#include "rdf_utf8_build.h"

namespace {

constexpr uint32_t kValidBit = 0x80000000u;   // of a row's note (aux)

__device__ __forceinline__ bool bit_at(const uint8_t* b, int64_t i) { return (b[i >> 3] >> (i & 7)) & 1; }

// last entry <= x of a prefix held in a strided table (empty chunks share the start of the next one and are skipped by this rule)
template <typename F>
__device__ __forceinline__ int64_t last_start_le(F start, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (start(mid) <= x) lo = mid + 1; else hi = mid;
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

// ---- the wave's forms of the row functions.  Every argument is the same in all 64 lanes, and so is the result.
__device__ int wave_count_code_points(const uint8_t* b, int len, int lane) {
    int c = 0;
    for (int off = lane * kPiece; off < len; off += kStep) c += (int)utf8_count_code_points(b + off, min(kPiece, len - off));
    return wave_sum(c);
}
// the byte offset of the start of code point number k (from 0) of [b, b + len); len if the row has no more than k
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
    return len;
}
// the start of the count-th (count >= 1) occurrence of d[0 .. m) in [b, b + len), counted from the left (fwd) or from the
// right; -1: the row has fewer.  Start position q (from the end the search begins at) is bit j of lane l in step s.
__device__ int wave_nth_match(const uint8_t* b, int len, const uint8_t* d, int m, int64_t count, bool fwd, int lane) {
    const int last = len - m;   // the last start
    for (int base = 0; base <= last; base += kStep) {
        uint32_t hits = 0;
        const int q0 = base + lane * kPiece;
        for (int j = 0; j < kPiece; ++j) {
            const int q = q0 + j;
            if (q > last) break;
            const uint8_t* p = b + (fwd ? q : last - q);
            if (*p == d[0] && utf8_bytes_at(p, d, m)) hits |= 1u << j;
        }
        const int cnt = __popc(hits);
        const int incl = wave_inclusive_scan(cnt, lane);
        const int total = __shfl(incl, 63);
        if (count <= total) {
            const bool mine = incl >= count && incl - cnt < count;
            int at = -1;
            if (mine) {
                uint32_t h = hits;
                for (int k = (int)count - (incl - cnt); k > 1; --k) h &= h - 1;   // drop the set bits before the wanted one
                const int q = q0 + __builtin_ctz(h);
                at = fwd ? q : last - q;
            }
            return __shfl(at, first_lane(__ballot(mine)));
        }
        count -= total;
    }
    return -1;
}

// a row's span, clamped into the bytes the host checked
__device__ __forceinline__ void row_span(const Utf8Chunk& c, int64_t r, int32_t& o0, int32_t& o1) {
    o0 = c.offs[r];
    o1 = c.offs[r + 1];
    o0 = min(max(o0, c.lo), c.hi);
    o1 = min(max(o1, o0), c.hi);
}
__device__ __forceinline__ bool row_valid(const Utf8Chunk& c, int64_t r) { return !c.valid || bit_at(c.valid, c.valid_off + r); }

constexpr bool op_is_pad(int op) { return op == U8B_LPAD || op == U8B_RPAD; }

// ---- 1. size
template <int OP>
__global__ __launch_bounds__(kUtf8PredThreads) void utf8_build_size_kernel(Utf8BuildArgs a) {
    __shared__ uint8_t s_lit[kUtf8PatternMax];
    __shared__ int s_nulls[kUtf8PredThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (op_is_pad(OP) || OP == U8B_SUBSTRING_INDEX)
        for (int i = threadIdx.x; i < a.lit_bytes; i += kUtf8PredThreads) s_lit[i] = a.lit[i];
    __syncthreads();
    const int m = a.lit_bytes;
    for (int64_t t = blockIdx.x; t < a.nsize_tiles; t += gridDim.x) {
        const int64_t c = last_start_le([&](int64_t i) { return a.tile_start[i]; }, a.nchunks, t);
        const Utf8Chunk& sh = a.shape[c];
        const int64_t r0 = (t - a.tile_start[c]) * kUtf8PredThreads + (int64_t)w * 64;
        const int64_t left = sh.rows - r0;
        const int nrows = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        const int64_t r = r0 + lane;
        bool valid = false, is_long = false;
        int64_t out = 0;
        uint32_t aux = 0;
        int32_t o0 = 0, o1 = 0;
        if (lane < nrows) {
            if (OP == U8B_CONCAT || OP == U8B_CONCAT_WS) {
                uint32_t present = 0;
                int64_t sum = 0;
                bool all = true;
                for (int k = 0; k < a.nparts; ++k) {
                    const Utf8BuildPart pt = a.parts[k];
                    if (!pt.col) { present |= 1u << k; sum += pt.lit_bytes; continue; }
                    const Utf8Chunk& ch = pt.col[c];
                    if (!row_valid(ch, r)) { all = false; continue; }
                    row_span(ch, r, o0, o1);
                    present |= 1u << k;
                    sum += o1 - o0;
                }
                valid = OP == U8B_CONCAT_WS || all;
                if (valid) {
                    aux = present;
                    out = sum + (OP == U8B_CONCAT_WS ? utf8_concat_seps(present) * m : 0);
                }
            } else if (OP == U8B_COALESCE || OP == U8B_CASE_WHEN) {
                // the chosen part (rdf_select.h's rule: the first part that can decide the row); its index is the row's note
                int chosen = -1;
                if (OP == U8B_COALESCE) {
                    for (int k = 0; k < a.nparts && chosen < 0; ++k) {
                        const Utf8BuildPart pt = a.parts[k];
                        if (pt.col ? row_valid(pt.col[c], r) : pt.lit_bytes >= 0) chosen = k;
                    }
                } else {
                    chosen = a.nconds;   // `otherwise`
                    for (int k = 0; k < a.nconds; ++k) {
                        const Utf8BuildCond cc = a.conds[(int64_t)k * a.nchunks + c];
                        if ((!cc.validity || bit_at(cc.validity, cc.offset + r)) && bit_at(cc.values, cc.offset + r)) { chosen = k; break; }
                    }
                }
                if (chosen >= 0) {
                    const Utf8BuildPart pt = a.parts[chosen];
                    valid = pt.col ? row_valid(pt.col[c], r) : pt.lit_bytes >= 0;
                    if (valid) {
                        aux = (uint32_t)chosen;
                        if (pt.col) { row_span(pt.col[c], r, o0, o1); out = o1 - o0; }
                        else out = pt.lit_bytes;
                    }
                }
            } else {
                const Utf8Chunk& ch = a.parts[0].col[c];
                valid = row_valid(ch, r);
                if (valid) {
                    row_span(ch, r, o0, o1);
                    const uint8_t *b = ch.data + o0, *e = ch.data + o1;
                    const int len = o1 - o0;
                    if (OP == U8B_REPEAT) out = (int64_t)len * a.param;
                    else if (OP == U8B_REVERSE) out = len;
                    else if (op_is_pad(OP)) {
                        if (a.param <= 0) out = 0;
                        else if (len > kUtf8ShortRow) is_long = true;
                        else {
                            const Utf8PadPlan pl = utf8_pad_plan(b, e, a.param, s_lit, m, a.lit_cp);
                            aux = (uint32_t)pl.kept;
                            out = utf8_pad_bytes_out(pl, m);
                        }
                    } else {   // substring_index
                        if (m == 0 || a.param == 0) out = 0;
                        else if (len > kUtf8ShortRow) is_long = true;
                        else {
                            const uint8_t *s0 = b, *s1 = b;
                            utf8_substring_index_span(b, e, s_lit, m, a.param, &s0, &s1);
                            aux = (uint32_t)(s0 - b);
                            out = s1 - s0;
                        }
                    }
                }
            }
        }
        if (op_is_pad(OP) || OP == U8B_SUBSTRING_INDEX) {
            uint64_t longs = __ballot(is_long);
            while (longs) {   // wave-uniform
                const int l = first_lane(longs);
                longs &= longs - 1;
                const int32_t q0 = __shfl(o0, l), q1 = __shfl(o1, l);
                const uint8_t* b = a.parts[0].col[c].data + q0;
                const int len = q1 - q0;
                int64_t res;
                uint32_t note;
                if (op_is_pad(OP)) {
                    const int64_t n = wave_count_code_points(b, len, lane);
                    Utf8PadPlan pl = {len, 0, 0};
                    if (!utf8_pad_fill(n, a.param, s_lit, m, a.lit_cp, &pl.full, &pl.part) && n > a.param)
                        pl.kept = wave_skip_code_points(b, len, (int)a.param, lane);
                    note = (uint32_t)pl.kept;
                    res = utf8_pad_bytes_out(pl, m);
                } else {
                    const bool fwd = a.param > 0;
                    const int at = wave_nth_match(b, len, s_lit, m, fwd ? a.param : -a.param, fwd, lane);
                    note = at < 0 || fwd ? 0u : (uint32_t)(at + m);
                    res = at < 0 ? len : (fwd ? at : len - (at + m));
                }
                if (lane == l) { out = res; aux = note; }
            }
        }
        if (lane < nrows) {
            const int64_t g = sh.row_start + r;
            a.blen[g] = out > kUtf8BuildClamp ? kUtf8BuildClamp : out;
            a.aux[g] = aux | (valid ? kValidBit : 0u);
        }
        if (OP != U8B_CONCAT_WS) {   // (the same in every lane of the block: the barriers are uniform)
            const uint64_t vmask = __ballot(valid);
            if (lane == 0) s_nulls[w] = nrows - __popcll(vmask);
            __syncthreads();
            if (threadIdx.x == 0) {
                int n = 0;
                for (int k = 0; k < kUtf8PredThreads / 64; ++k) n += s_nulls[k];
                if (n) atomicAdd(&a.null_counts[c], (unsigned long long)n);
            }
            __syncthreads();
        }
    }
}

// ---- 2. per chunk totals (after the scan)
__global__ void utf8_build_totals_kernel(Utf8BuildArgs a) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.nchunks; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = a.shape[c].row_start, e = s + a.shape[c].rows;
        a.tot[2 * c] = a.bscan[e] - a.bscan[s];
        a.tot[2 * c + 1] = a.shape[c].rows;
    }
}

// ---- 3. write
// validity cleared, the closing offset of every output chunk (also of empty ones)
__global__ void utf8_build_prep_kernel(Utf8BuildArgs a) {
    for (int64_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
        const Utf8OutChunk& o = a.outs[c];
        if (threadIdx.x == 0) o.offs[o.rows] = (int32_t)o.bytes;
        if (o.valid)
            for (int64_t k = threadIdx.x; k < (o.rows + 7) / 8; k += blockDim.x) o.valid[k] = 0;
    }
}

__global__ void utf8_build_place_kernel(Utf8BuildArgs a) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.n; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = last_start_le([&](int64_t i) { return a.shape[i].row_start; }, a.nchunks, g);
        const Utf8OutChunk& o = a.outs[c];
        const int64_t r = g - o.row_start;
        const int64_t b0 = a.bscan[g] - o.byte_start, b1 = a.bscan[g + 1] - o.byte_start;
        o.offs[r] = (int32_t)b0;
        if (o.valid && (a.aux[g] & kValidBit)) atomicOr((unsigned int*)(o.valid + ((r >> 3) & ~(int64_t)3)), 1u << (r & 31));
        // the copy tiles that start inside this row learn their first row here, so no copy block has to search for it
        for (int64_t t = (b0 + kUtf8CopyTile - 1) / kUtf8CopyTile; t * kUtf8CopyTile < b1; ++t) a.tile_row[o.tile_start + t] = r;
    }
}

// output byte j of row r of chunk c (L output bytes, note aux): its source byte, and how many bytes from there are consecutive
template <int OP>
__device__ __forceinline__ const uint8_t* row_source(const Utf8BuildArgs& a, int64_t c, int64_t r, uint32_t aux, int64_t L, int64_t j, int64_t* run) {
    int k = 0;
    if (OP == U8B_CONCAT || OP == U8B_CONCAT_WS) {   // pieces [separator before part k][part k]
        return utf8_piece_at(
            [&](int i) -> Utf8Piece {
                const int part = i >> 1;
                if (!((aux >> part) & 1u)) return Utf8Piece{nullptr, 0, 1};
                if (!(i & 1)) {
                    const int64_t sep = utf8_concat_sep_before(aux, part) ? a.lit_bytes : 0;
                    return Utf8Piece{a.lit, sep, sep > 0 ? sep : 1};
                }
                const Utf8BuildPart pt = a.parts[part];
                if (!pt.col) return Utf8Piece{pt.lit, pt.lit_bytes, pt.lit_bytes > 0 ? pt.lit_bytes : 1};
                int32_t o0, o1;
                row_span(pt.col[c], r, o0, o1);
                return Utf8Piece{pt.col[c].data + o0, o1 - o0, o1 > o0 ? o1 - o0 : 1};
            },
            2 * a.nparts, j, &k, run);
    }
    if (OP == U8B_COALESCE || OP == U8B_CASE_WHEN) {   // one piece: the chosen part's row or literal, L bytes
        const Utf8BuildPart pt = a.parts[aux & 15u];
        const uint8_t* src = pt.lit;
        if (pt.col) {
            int32_t p0, p1;
            row_span(pt.col[c], r, p0, p1);
            src = pt.col[c].data + p0;
        }
        return utf8_piece_at([&](int) { return Utf8Piece{src, L, L > 0 ? L : 1}; }, 1, j, &k, run);
    }
    const Utf8Chunk& ch = a.parts[0].col[c];
    int32_t o0, o1;
    row_span(ch, r, o0, o1);
    const uint8_t* b = ch.data + o0;
    const int64_t len = o1 - o0;
    if (OP == U8B_REVERSE) return utf8_reverse_at(b, len, j, run);
    if (OP == U8B_REPEAT) return utf8_piece_at([&](int) { return Utf8Piece{b, L, len > 0 ? len : 1}; }, 1, j, &k, run);
    if (OP == U8B_SUBSTRING_INDEX) return utf8_piece_at([&](int) { return Utf8Piece{b + aux, L, L > 0 ? L : 1}; }, 1, j, &k, run);
    return utf8_piece_at([&](int i) { return utf8_pad_piece(i, OP == U8B_LPAD ? 0 : 1, b, (int64_t)aux, a.lit, a.lit_bytes, L); }, 2, j, &k, run);
}

// one block per kUtf8CopyTile output bytes of one output chunk; lane t owns bytes [lo + 16 t, lo + 16 t + 16)
template <int OP>
__global__ void __launch_bounds__(kUtf8CopyThreads) utf8_build_copy_kernel(Utf8BuildArgs a) {
    __shared__ int32_t s_off[kUtf8WindowRows + 1];
    __shared__ uint32_t s_aux[kUtf8WindowRows];
    __shared__ uint4 s_buf[kUtf8CopyThreads];
    __shared__ int64_t s_meta[5];
    const int64_t tile = blockIdx.x;
    const int t = threadIdx.x;
    if (t == 0) {
        const int64_t oc = last_start_le([&](int64_t i) { return a.outs[i].tile_start; }, a.nchunks, tile);
        const Utf8OutChunk& o = a.outs[oc];
        const int64_t lt = tile - o.tile_start, lo = lt * kUtf8CopyTile, hi = min(lo + (int64_t)kUtf8CopyTile, o.bytes);
        // rows r0 .. the row of the next tile's first byte (the chunk's last row for its last tile) hold the tile's bytes
        const int64_t r0 = a.tile_row[tile];
        const int64_t r1 = hi < o.bytes ? a.tile_row[tile + 1] : o.rows - 1;
        s_meta[0] = oc; s_meta[1] = lo; s_meta[2] = hi; s_meta[3] = r0; s_meta[4] = r1 - r0 + 1;
    }
    __syncthreads();
    const int64_t c = s_meta[0];
    const Utf8OutChunk& o = a.outs[c];
    const int64_t lo = s_meta[1], hi = s_meta[2];
    const int64_t r0 = s_meta[3], nwin = s_meta[4];
    const bool inwin = nwin <= kUtf8WindowRows;
    if (inwin) {
        for (int64_t k = t; k <= nwin; k += kUtf8CopyThreads) s_off[k] = o.offs[r0 + k];
        for (int64_t k = t; k < nwin; k += kUtf8CopyThreads) s_aux[k] = a.aux[o.row_start + r0 + k];
    }
    __syncthreads();
    const int64_t p0 = lo + 16 * (int64_t)t;
    if (p0 >= hi) return;
    const int64_t pend = min(p0 + 16, hi);
    uint8_t* mine = (uint8_t*)&s_buf[t];
    auto off_at = [&](int64_t k) -> int64_t { return inwin ? s_off[k] : o.offs[r0 + k]; };
    // window row holding p0
    int64_t l = 0, h = nwin + 1;
    while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if (off_at(mid) <= p0) l = mid + 1; else h = mid;
    }
    int64_t k = l - 1;
    int64_t p = p0;
    while (p < pend) {
        int64_t next = off_at(k + 1);
        while (next <= p) { ++k; next = off_at(k + 1); }
        const int64_t rb = off_at(k), re = min(next, pend);
        const uint32_t aux = (inwin ? s_aux[k] : a.aux[o.row_start + r0 + k]) & ~kValidBit;
        while (p < re) {
            int64_t run = 0;
            const uint8_t* src = row_source<OP>(a, c, r0 + k, aux, next - rb, p - rb, &run);
            if (run < 1) { mine[p - p0] = 0; ++p; continue; }   // (cannot happen while both passes see the same offsets; never spin)
            const int64_t nb = min(run, re - p);
            for (int64_t i = 0; i < nb; ++i) mine[p - p0 + i] = src[i];
            p += nb;
        }
    }
    uint8_t* dst = o.data + p0;
    if (pend - p0 == 16 && ((uintptr_t)dst & 15) == 0) *(uint4*)dst = s_buf[t];
    else for (int64_t q = 0; q < pend - p0; ++q) dst[q] = mine[q];
}

unsigned grid_for(int64_t n, int threads) {
    const int64_t b = (n + threads - 1) / threads;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

}  // namespace

#define UTF8_BUILD_DISPATCH(KERNEL, OPV, ...)                                                        \
    switch (OPV) {                                                                                   \
        case U8B_CONCAT: hipLaunchKernelGGL((KERNEL<U8B_CONCAT>), __VA_ARGS__); break;               \
        case U8B_CONCAT_WS: hipLaunchKernelGGL((KERNEL<U8B_CONCAT_WS>), __VA_ARGS__); break;         \
        case U8B_LPAD: hipLaunchKernelGGL((KERNEL<U8B_LPAD>), __VA_ARGS__); break;                   \
        case U8B_RPAD: hipLaunchKernelGGL((KERNEL<U8B_RPAD>), __VA_ARGS__); break;                   \
        case U8B_REPEAT: hipLaunchKernelGGL((KERNEL<U8B_REPEAT>), __VA_ARGS__); break;               \
        case U8B_REVERSE: hipLaunchKernelGGL((KERNEL<U8B_REVERSE>), __VA_ARGS__); break;             \
        case U8B_COALESCE: hipLaunchKernelGGL((KERNEL<U8B_COALESCE>), __VA_ARGS__); break;           \
        case U8B_CASE_WHEN: hipLaunchKernelGGL((KERNEL<U8B_CASE_WHEN>), __VA_ARGS__); break;         \
        default: hipLaunchKernelGGL((KERNEL<U8B_SUBSTRING_INDEX>), __VA_ARGS__); break;              \
    }

hipError_t launch_utf8_build_size(const Utf8BuildArgs& a, hipStream_t s) {
    if (a.nsize_tiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int64_t>(a.nsize_tiles, 256 * 16)), block(kUtf8PredThreads);
    UTF8_BUILD_DISPATCH(utf8_build_size_kernel, a.op, grid, block, 0, s, a)
    return hipGetLastError();
}
hipError_t launch_utf8_build_totals(const Utf8BuildArgs& a, hipStream_t s) {
    if (a.nchunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(utf8_build_totals_kernel, dim3(grid_for(a.nchunks, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_build_write(const Utf8BuildArgs& a, hipStream_t s) {
    if (a.nchunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(utf8_build_prep_kernel, dim3((unsigned)(a.nchunks < 65536 ? a.nchunks : 65536)), dim3(256), 0, s, a);
    if (a.n > 0) hipLaunchKernelGGL(utf8_build_place_kernel, dim3(grid_for(a.n, 256)), dim3(256), 0, s, a);
    if (a.ntiles > 0) {
        const dim3 grid((unsigned)a.ntiles), block(kUtf8CopyThreads);
        UTF8_BUILD_DISPATCH(utf8_build_copy_kernel, a.op, grid, block, 0, s, a)
    }
    return hipGetLastError();
}
