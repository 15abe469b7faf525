// rdf_member.hip — the kernels of rdf_member_mask (LEFT SEMI / LEFT ANTI / x IN (...)) and rdf_first_occurrence
// (drop_duplicates); host side: rdf_capi_member.inc, table sizes and routes: rdf_member_plan.h.
//
// One primitive: a set of key tuples goes into an open-addressing table (linear probing, in HBM), a column of tuples is
// streamed past it, and every row gives ONE bit.  All kernels walk the row layout of rdf_wavetile.hip.h: tiles of kCsTile
// rows that never cross a chunk, a wave on 512 rows of one chunk, so every output word has one writer and a frame of
// 1024-row batches is walked like one long chunk.  Phases are separate launches; no block waits on another.
//   member_prep_kernel     2..4 key columns: per row the columns' key words, the NULL bits and the tuple's 64-bit hash
//   member_build_kernel    the build side into the table: a key word by compare-and-swap on the slot, a tuple by
//                          compare-and-swap of its ROW on the slot (a reader never sees half a key); the free-marker key
//                          and "a build row is NULL" go into flags
//   member_probe_kernel    the probe side past the table -> mask words (one ballot per 64 rows, one store per wave tile),
//                          <true>: the block probes a copy of the table in LDS
//   member_fold_kernel     first occurrence: every row finds or claims its key's slot and folds its row number into the
//                          slot's smallest (tiles ascending) or largest (tiles descending) row: load, compare, and the
//                          atomic only when it can change the slot
//   member_first_kernel    first occurrence: row == smallest / row == largest / smallest == largest -> mask words
//   member_total_kernel    the per-block TRUE counts -> one number
// One key column: the slot holds the key word itself (the order-preserving key bits of sort_keys_kernel, floats made
// canonical: -0.0 = +0.0, every NaN one NaN).  Tuples: equal hashes are compared column by column through the slot's
// row; two different tuples with one hash are two keys and probing goes on.
#include "rdf_common.hip.h"
#include "rdf_hash.h"
#include "rdf_member.h"
#include "rdf_wavetile.hip.h"

#include <algorithm>

namespace rdfk {
namespace {

// key word of element e of a chunk; returns true when the element is NULL
__device__ __forceinline__ bool member_load(const DevChunkCol& cc, int dt, int64_t e, uint64_t& w) {
    if (dt == RDF_BOOL) w = (as_global<uint8_t>(cc.values)[e >> 3] >> (e & 7)) & 1u;
    else w = sort_key_canon(dt, sort_key_bits(cc, dt, e));
    return cc.validity && !((as_global<uint8_t>(cc.validity)[e >> 3] >> (e & 7)) & 1);
}

__device__ __forceinline__ uint64_t member_home(const MemberTable& t, uint64_t w) { return (w * kJoinMul) >> t.tshift; }

// ---- one key column: a table of key words
template <class P>
__device__ __forceinline__ bool member_find_word(P keys, const MemberTable& t, uint64_t w, uint64_t* slot) {
    uint64_t s = member_home(t, w);
    for (uint64_t step = 0; step <= t.mask; ++step) {
        const uint64_t k = keys[s];
        if (k == w) { *slot = s; return true; }
        if (k == kMemberEmpty) return false;
        s = (s + 1) & t.mask;
    }
    return false;
}
// the slot of w, claimed if nobody holds it yet; false: every slot is taken by another key
__device__ __forceinline__ bool member_insert_word(const MemberTable& t, uint64_t w, uint64_t* slot) {
    uint64_t s = member_home(t, w);
    for (uint64_t step = 0; step <= t.mask; ++step) {
        uint64_t k = __atomic_load_n(&t.keys[s], __ATOMIC_RELAXED);
        if (k == kMemberEmpty) {
            k = atomicCAS((unsigned long long*)&t.keys[s], (unsigned long long)kMemberEmpty, (unsigned long long)w);
            if (k == kMemberEmpty) k = w;
        }
        if (k == w) { *slot = s; return true; }
        s = (s + 1) & t.mask;
    }
    return false;
}

// ---- tuples: a table of representative rows, compared through the prepared columns
__device__ __forceinline__ bool member_same(const MemberSide& x, int64_t i, const MemberSide& y, int64_t j) {
    bool eq = x.hash[i] == y.hash[j] && x.nullbits[i] == y.nullbits[j];
    for (int k = 0; k < x.nkeys; ++k) eq = eq && x.bits[k][i] == y.bits[k][j];
    return eq;
}
__device__ __forceinline__ bool member_find_tuple(const MemberTable& t, const MemberSide& me, int64_t i, const MemberSide& held, uint64_t* slot) {
    uint64_t s = member_home(t, me.hash[i]);
    for (uint64_t step = 0; step <= t.mask; ++step) {
        const uint32_t r = __atomic_load_n(&t.lo[s], __ATOMIC_RELAXED);
        if (r == kMemberNoRow) return false;
        if (member_same(me, i, held, r)) { *slot = s; return true; }
        s = (s + 1) & t.mask;
    }
    return false;
}
// the slot of row i's tuple, claimed with row i if nobody holds the tuple yet; *seen = the row read in the slot
__device__ __forceinline__ bool member_insert_tuple(const MemberTable& t, const MemberSide& me, int64_t i, uint64_t* slot, uint32_t* seen) {
    uint64_t s = member_home(t, me.hash[i]);
    for (uint64_t step = 0; step <= t.mask; ++step) {
        uint32_t r = __atomic_load_n(&t.lo[s], __ATOMIC_RELAXED);
        if (r == kMemberNoRow) {
            r = atomicCAS(&t.lo[s], kMemberNoRow, (uint32_t)i);
            if (r == kMemberNoRow) r = (uint32_t)i;
        }
        if (r == (uint32_t)i || member_same(me, i, me, r)) { *slot = s; *seen = r; return true; }
        s = (s + 1) & t.mask;
    }
    return false;
}

// first global row of the wave's tile
__device__ __forceinline__ int64_t member_row0(const CsCol& col, const DtWave& m) { return as_const<int64_t>(col.row_start)[m.chunk] + m.r0; }

// per-wave TRUE counts -> partial[blockIdx.x]
__device__ __forceinline__ void member_block_count(unsigned long long mine, unsigned long long* partial) {
    __shared__ unsigned long long wave_true[kCsThreads / 64];
    if ((threadIdx.x & 63) == 0) wave_true[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kCsThreads / 64; ++w) t += wave_true[w];
        partial[blockIdx.x] = t;
    }
}
// the wave tile's words: lane k holds word k
__device__ __forceinline__ void member_store(const DtOut& o, const DtWave& m, int lane, uint64_t mine, uint64_t valid) {
    const int nwords = (m.rows + 63) >> 6;
    if (lane < nwords) {
        as_global_mut<uint64_t>(o.values)[(m.r0 >> 6) + lane] = mine;
        if (o.validity) as_global_mut<uint64_t>(o.validity)[(m.r0 >> 6) + lane] = valid;
    }
}

__global__ __launch_bounds__(kCsThreads) void member_prep_kernel(const MemberSide s, const int with_nulls) {
    const int lane = threadIdx.x & 63, w = wave_id();
    for (int64_t t = blockIdx.x; t < s.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(s.col, t, w);
        if (m.rows == 0) continue;
        const int64_t g0 = member_row0(s.col, m);
        DevChunkCol cc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) cc[k] = const_col(s.col.chunks, (int64_t)(k < s.nkeys ? k : 0) * s.col.nchunks + m.chunk);
        for (int r = lane; r < m.rows; r += 64) {
            uint64_t h = kJoinSeed;
            uint32_t nb = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= s.nkeys) break;
                uint64_t x;
                if (member_load(cc[k], s.dtype[k], cc[k].offset + m.r0 + r, x)) { nb |= 1u << k; x = 0; }
                s.bits[k][g0 + r] = x;
                h = join_tuple_step(h, x, k);
            }
            if (with_nulls) h = join_tuple_step(h, nb, s.nkeys);   // (NULL is a key value of its own: the flags are part of the tuple)
            s.hash[g0 + r] = h;
            s.nullbits[g0 + r] = (uint8_t)nb;
        }
    }
}

__global__ __launch_bounds__(kCsThreads) void member_build_kernel(const MemberArgs a) {
    const MemberSide& b = a.build;
    const int lane = threadIdx.x & 63, w = wave_id();
    const bool single = b.nkeys == 1;
    unsigned int flags = 0;
    for (int64_t t = blockIdx.x; t < b.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(b.col, t, w);
        if (m.rows == 0) continue;
        const int64_t g0 = member_row0(b.col, m);
        const DevChunkCol cc = const_col(b.col.chunks, m.chunk);
        for (int r = lane; r < m.rows; r += 64) {
            uint64_t slot;
            if (single) {
                uint64_t x;
                if (member_load(cc, b.dtype[0], cc.offset + m.r0 + r, x)) flags |= 1u << MEMBER_F_NULL;
                else if (x == kMemberEmpty) flags |= 1u << MEMBER_F_MARKER;
                else if (!member_insert_word(a.t, x, &slot)) flags |= 1u << MEMBER_F_OVERFLOW;
            } else {
                uint32_t seen;
                if (b.nullbits[g0 + r]) flags |= 1u << MEMBER_F_NULL;
                else if (!member_insert_tuple(a.t, b, g0 + r, &slot, &seen)) flags |= 1u << MEMBER_F_OVERFLOW;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) flags |= (unsigned int)__shfl_xor((int)flags, d);
    if (lane == 0)
        for (int f = 0; f < MEMBER_F_WORDS; ++f)
            if ((flags >> f) & 1u) atomicOr(&a.t.flags[f], 1u);
}

template <bool LDS>
__global__ __launch_bounds__(kCsThreads) void member_probe_kernel(const MemberArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t member_sm[];
    const MemberSide& p = a.probe;
    const int lane = threadIdx.x & 63, w = wave_id();
    const bool single = p.nkeys == 1;
    if (LDS) {
        for (uint64_t i = threadIdx.x; i <= a.t.mask; i += kCsThreads) member_sm[i] = as_global<uint64_t>(a.t.keys)[i];
        __syncthreads();
    }
    const ConstPtr<unsigned int> fl = as_const<unsigned int>(a.t.flags);
    const bool marker = fl[MEMBER_F_MARKER] != 0, build_null = fl[MEMBER_F_NULL] != 0, build_empty = a.build.col.n == 0;
    unsigned long long mine_true = 0;
    for (int64_t t = blockIdx.x; t < p.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(p.col, t, w);
        if (m.rows == 0) continue;
        const int64_t g0 = member_row0(p.col, m);
        const DevChunkCol cc = const_col(p.col.chunks, m.chunk);
        uint64_t word = 0, valid = 0;
        unsigned int nulls = 0;
        for (int q = 0; q * 64 < m.rows; ++q) {
            const int r = q * 64 + lane;
            const bool in = r < m.rows;
            bool isnull = false, hit = false;
            if (in) {
                uint64_t slot;
                if (single) {
                    uint64_t x;
                    isnull = member_load(cc, p.dtype[0], cc.offset + m.r0 + r, x);
                    if (!isnull) {
                        if (x == kMemberEmpty) hit = marker;
                        else if (LDS) hit = member_find_word((const uint64_t*)member_sm, a.t, x, &slot);
                        else hit = member_find_word(as_global<uint64_t>(a.t.keys), a.t, x, &slot);
                    }
                } else {
                    isnull = p.nullbits[g0 + r] != 0;
                    if (!isnull) hit = member_find_tuple(a.t, p, g0 + r, a.build, &slot);
                }
            }
            const uint64_t rows = __ballot(in), hits = __ballot(hit);
            uint64_t bits = hits, ok = rows;
            if (a.kind == RDF_MEMBER_ANTI) bits = rows & ~hits;
            else if (a.kind == RDF_MEMBER_IS_IN && !build_empty) ok = hits | (build_null ? 0ull : rows & ~__ballot(isnull));
            if (lane == q) { word = bits; valid = ok; }
            if (lane == 0) { mine_true += (unsigned long long)__popcll(bits); nulls += (unsigned int)__popcll(rows & ~ok); }
        }
        if (a.outs) member_store(dt_out(a.outs, m.chunk), m, lane, word, valid);
        if (lane == 0 && nulls) atomicAdd(&a.chunk_nulls[m.chunk], (unsigned long long)nulls);
    }
    member_block_count(mine_true, a.partial);
}

__global__ __launch_bounds__(kCsThreads) void member_fold_kernel(const MemberArgs a) {
    const MemberSide& p = a.probe;
    const int lane = threadIdx.x & 63, w = wave_id();
    const bool single = p.nkeys == 1, desc = a.descending != 0;
    unsigned int flags = 0;
    unsigned long long saved = 0;
    for (int64_t ti = blockIdx.x; ti < p.col.ntiles; ti += gridDim.x) {
        const int64_t t = desc ? p.col.ntiles - 1 - ti : ti;
        const DtWave m = dt_wave(p.col, t, desc ? kCsThreads / 64 - 1 - w : w);
        if (m.rows == 0) continue;
        const int64_t g0 = member_row0(p.col, m);
        const DevChunkCol cc = const_col(p.col.chunks, m.chunk);
        const int passes = (m.rows + 63) >> 6;
        for (int qi = 0; qi < passes; ++qi) {
            const int r = (desc ? passes - 1 - qi : qi) * 64 + lane;
            if (r >= m.rows) continue;
            const uint32_t row = (uint32_t)(g0 + r);
            uint64_t e = 0;
            bool have = true;
            if (single) {
                uint64_t x;
                if (member_load(cc, p.dtype[0], cc.offset + m.r0 + r, x)) e = a.t.mask + 2;
                else if (x == kMemberEmpty) e = a.t.mask + 1;
                else have = member_insert_word(a.t, x, &e);
            } else {
                uint32_t seen;
                have = member_insert_tuple(a.t, p, g0 + r, &e, &seen);
            }
            if (!have) { flags |= 1u << MEMBER_F_OVERFLOW; continue; }
            if (desc) {
                if (row > __atomic_load_n(&a.t.hi[e], __ATOMIC_RELAXED)) atomicMax(&a.t.hi[e], row); else ++saved;
            } else {
                if (row < __atomic_load_n(&a.t.lo[e], __ATOMIC_RELAXED)) atomicMin(&a.t.lo[e], row); else ++saved;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) flags |= (unsigned int)__shfl_xor((int)flags, d);
    if (lane == 0 && flags) atomicOr(&a.t.flags[MEMBER_F_OVERFLOW], 1u);
    if (a.skipped) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) saved += shfl_xor64(saved, d);
        if (lane == 0 && saved) atomicAdd(a.skipped, saved);
    }
}

__global__ __launch_bounds__(kCsThreads) void member_first_kernel(const MemberArgs a) {
    const MemberSide& p = a.probe;
    const int lane = threadIdx.x & 63, w = wave_id();
    const bool single = p.nkeys == 1;
    unsigned long long mine_true = 0;
    for (int64_t t = blockIdx.x; t < p.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(p.col, t, w);
        if (m.rows == 0) continue;
        const int64_t g0 = member_row0(p.col, m);
        const DevChunkCol cc = const_col(p.col.chunks, m.chunk);
        uint64_t word = 0, valid = 0;
        for (int q = 0; q * 64 < m.rows; ++q) {
            const int r = q * 64 + lane;
            const bool in = r < m.rows;
            bool bit = false;
            if (in) {
                const uint32_t row = (uint32_t)(g0 + r);
                uint64_t e = 0;
                bool have = true;
                if (single) {
                    uint64_t x;
                    if (member_load(cc, p.dtype[0], cc.offset + m.r0 + r, x)) e = a.t.mask + 2;
                    else if (x == kMemberEmpty) e = a.t.mask + 1;
                    else have = member_find_word(as_global<uint64_t>(a.t.keys), a.t, x, &e);
                } else have = member_find_tuple(a.t, p, g0 + r, p, &e);
                if (have) {
                    if (a.kind == RDF_KEEP_FIRST) bit = a.t.lo[e] == row;
                    else if (a.kind == RDF_KEEP_LAST) bit = a.t.hi[e] == row;
                    else bit = a.t.lo[e] == a.t.hi[e];
                }
            }
            const uint64_t bits = __ballot(bit), rows = __ballot(in);
            if (lane == q) { word = bits; valid = rows; }
            if (lane == 0) mine_true += (unsigned long long)__popcll(bits);
        }
        if (a.outs) member_store(dt_out(a.outs, m.chunk), m, lane, word, valid);
    }
    member_block_count(mine_true, a.partial);
}

__global__ __launch_bounds__(256) void member_total_kernel(const unsigned long long* partial, int n, unsigned long long* total) {
    __shared__ unsigned long long part[4];
    unsigned long long mine = 0;
    for (int i = threadIdx.x; i < n; i += 256) mine += partial[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += shfl_xor64(mine, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) *total = part[0] + part[1] + part[2] + part[3];
}

}  // namespace
}  // namespace rdfk

using namespace rdfk;

// one block per tile up to the persistent grid; the LDS form: two blocks per CU (each holds up to 64 KB of the 160 KB)
int member_grid(int64_t ntiles, bool lds) {
    const int64_t lim = lds ? std::max(1, eval_grid_limit() / 4) : eval_grid_limit();
    return (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, lim));
}
hipError_t launch_member_prep(const MemberSide& s, int with_nulls, hipStream_t st) {
    if (s.nkeys < 2 || s.nkeys > 4 || !s.hash || !s.nullbits) return hipErrorInvalidValue;
    if (s.col.ntiles > 0) hipLaunchKernelGGL(member_prep_kernel, dim3(member_grid(s.col.ntiles, false)), dim3(kCsThreads), 0, st, s, with_nulls);
    return hipGetLastError();
}
hipError_t launch_member_build(const MemberArgs& a, hipStream_t s) {
    if (a.build.col.ntiles > 0) hipLaunchKernelGGL(member_build_kernel, dim3(member_grid(a.build.col.ntiles, false)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_member_probe(const MemberArgs& a, int grid, size_t lds_bytes, hipStream_t s) {
    if (grid < 1 || !a.partial) return hipErrorInvalidValue;
    if (lds_bytes) {
        if (lds_bytes > (size_t)kMemberLdsBudget || lds_bytes != 8 * (size_t)(a.t.mask + 1) || a.probe.nkeys != 1) return hipErrorInvalidValue;
        (void)hipFuncSetAttribute((const void*)member_probe_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL(member_probe_kernel<true>, dim3(grid), dim3(kCsThreads), lds_bytes, s, a);
    } else hipLaunchKernelGGL(member_probe_kernel<false>, dim3(grid), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_member_fold(const MemberArgs& a, hipStream_t s) {
    if (a.probe.col.ntiles > 0) hipLaunchKernelGGL(member_fold_kernel, dim3(member_grid(a.probe.col.ntiles, false)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_member_first(const MemberArgs& a, int grid, hipStream_t s) {
    if (grid < 1 || !a.partial) return hipErrorInvalidValue;
    hipLaunchKernelGGL(member_first_kernel, dim3(grid), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_member_total(const unsigned long long* partial, int n, unsigned long long* total, hipStream_t s) {
    hipLaunchKernelGGL(member_total_kernel, dim3(1), dim3(256), 0, s, partial, n, total);
    return hipGetLastError();
}
