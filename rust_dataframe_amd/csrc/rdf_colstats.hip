// rdf_colstats.hip — the kernels of Column::hist and Column::uniques (src/table.rs:244-341; host side:
// rdf_capi_colstats.inc, argument blocks: rdf_colstats.h).
//
//   hist      one streaming pass.  A value's bucket is estimated with one multiplication and then corrected against the
//             edges, so the comparisons decide and the estimate's rounding does not matter.  Counters: 16-bit fields of the
//             lane's own registers up to 16 buckets; 32-bit words in LDS while the buckets fit (a copy per wave up to 1024
//             buckets: four waves never meet on a word; one copy per block up to 4096), folded into the 64-bit global
//             counts once per block; beyond that global atomics.  Before any add the wave counts the lanes that share a
//             bucket with its first open lane and carries that bucket's count in registers from row group to row group —
//             a constant or one-hot column costs one add per wave, not 64 serialised ones per row group.
//   distinct  numeric keys normalised to 64 bits; a block keeps the keys it has met in an LDS open-addressing set and only
//             forwards keys new to the block to the insert-only table in HBM, which gives up (the host then takes the
//             sort route) when it has taken the keys it was sized for.
//   runs      the sort route: rows in sorted order, the first row of every run of equal keys is kept.
//   utf8      hash every valid row's bytes to 64 bits (a lane per row below 512 bytes, a wave per longer row — the same
//             function either way), insert (hash -> smallest row), then verify every row's bytes against its hash's
//             representative; a mismatch sends the call to the exact route (sorted order, neighbours compared).
//   dict      rdf_utf8_dictionary_encode on the utf8 passes: the verify pass's sibling keeps every row's representative
//             (the exact route: the first row of every sorted run, spread over the run), an exclusive scan of "is its own
//             representative" ranks the first occurrences, and the codes pass writes rank[rep[row]] and whole validity
//             bytes per output chunk.
// Every byte of a Utf8 row is read inside the chunk's value-offset range the host checked.
#include <algorithm>

#include "rdf_colstats.h"
#include "rdf_common.hip.h"

using namespace rdfk;

namespace {

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// Places in a list for a block of kCsThreads: thread t wants `mine` consecutive ones; ONE atomic per block (a same-address
// atomic costs ~12 ns: one per wave was 3 ms for a table of 2^24 slots).  Called by all threads of the block.
struct CsBlockScan { unsigned int wave[kCsThreads / 64]; unsigned long long base; };
__device__ __forceinline__ unsigned long long block_reserve(unsigned int mine, unsigned long long* ctr, CsBlockScan& sc) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int o = (unsigned int)__shfl_up((int)incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) sc.wave[w] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int tot = 0;
        for (int i = 0; i < kCsThreads / 64; ++i) tot += sc.wave[i];
        sc.base = tot ? atomicAdd(ctr, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    unsigned long long pos = sc.base + (incl - mine);
    for (int i = 0; i < w; ++i) pos += sc.wave[i];
    __syncthreads();
    return pos;
}

// ---------------------------------------------------------------- tiles of a chunked 8-byte column

struct CsTileView { GlobalPtr<uint64_t> v; const uint8_t* valid; int64_t bit0; int rows; };

__device__ __forceinline__ CsTileView cs_tile(const CsCol& col, int64_t t) {
    const ConstPtr<int64_t> ts = as_const<int64_t>(col.tile_start);
    const ConstPtr<int64_t> rs = as_const<int64_t>(col.row_start);
    const int64_t c = find_chunk_tile(ts, col.nchunks, t);
    const DevChunkCol ch = const_col(col.chunks, c);
    const int64_t r0 = (t - ts[c]) * kCsTile;
    const int64_t left = rs[c + 1] - rs[c] - r0;
    CsTileView tv;
    tv.v = as_global<uint64_t>(ch.values) + ch.offset + r0;
    tv.valid = ch.validity;
    tv.bit0 = ch.offset + r0;
    tv.rows = left < kCsTile ? (left < 0 ? 0 : (int)left) : kCsTile;
    return tv;
}

// the tile's rows of this lane: row threadIdx.x + k * 256; ok = the row exists and is not NULL
__device__ __forceinline__ void cs_load(const CsTileView& tv, uint64_t (&v)[kCsRowsPerLane], bool (&ok)[kCsRowsPerLane]) {
#pragma unroll
    for (int k = 0; k < kCsRowsPerLane; ++k) {
        const int i = (int)threadIdx.x + k * kCsThreads;
        ok[k] = i < tv.rows;
        v[k] = ok[k] ? tv.v[i] : 0;
    }
    if (tv.valid) {
#pragma unroll
        for (int k = 0; k < kCsRowsPerLane; ++k) {
            const int64_t bit = tv.bit0 + (int)threadIdx.x + k * kCsThreads;
            if (ok[k]) ok[k] = (tv.valid[bit >> 3] >> (bit & 7)) & 1;
        }
    }
}

// ---------------------------------------------------------------- histogram

// LDS: the block's counters live in LDS (nbins <= kCsHistLdsBins); INT: Int64 values; SMALL: nbins <= kCsHistRegBins — every lane
// counts in 16-bit fields of its own registers and touches LDS every 65 535 rows and when the kernel ends.
constexpr int kCsHistRegBins = 16;
template <bool LDS, bool INT, bool SMALL>
__global__ __launch_bounds__(kCsThreads) void cs_hist_kernel(CsHistArgs a) {
    __shared__ unsigned int lc[LDS ? kCsHistLdsBins : 1];
    const int lane = threadIdx.x & 63;
    const int nb = (int)a.nbins;
    int copies = 1;
    unsigned int* mine = lc;
    if (LDS) {
        copies = nb <= kCsHistWaveBins ? kCsThreads / 64 : 1;
        for (int i = threadIdx.x; i < nb * copies; i += kCsThreads) lc[i] = 0;
        if (copies > 1) mine = lc + wave_id() * nb;
        __syncthreads();
    }
    unsigned long long cnt = 0;
    // the bucket the wave's first open lane fell into last, and the rows counted for it but not added yet (wave-uniform):
    // a constant or one-hot column adds once per wave, not once per 64 rows
    int pend_j = -1;
    unsigned int pend_c = 0;
    unsigned long long wc[SMALL ? kCsHistRegBins / 4 : 1] = {};
    int since_flush = 0;
    auto flush_small = [&]() {   // the lane's packed counters -> the wave's LDS counters
#pragma unroll
        for (int b = 0; b < kCsHistRegBins; ++b) {
            const unsigned int c = (unsigned int)(wc[b >> 2] >> (16 * (b & 3))) & 0xFFFFu;
            if (b < nb && c) atomicAdd(&mine[b], c);
        }
#pragma unroll
        for (int q = 0; q < kCsHistRegBins / 4; ++q) wc[q] = 0;
    };
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        if (SMALL && ++since_flush == 65535 / kCsRowsPerLane) { flush_small(); since_flush = 0; }   // (16-bit counters)
        const CsTileView tv = cs_tile(a.col, t);
        uint64_t v[kCsRowsPerLane];
        bool ok[kCsRowsPerLane];
        cs_load(tv, v, ok);
        if (pend_c >= 0x40000000u) {   // (keeps the pending count inside 32 bits)
            if (lane == 0) { if (LDS) atomicAdd(&mine[pend_j], pend_c); else atomicAdd(&a.counts[pend_j], (unsigned long long)pend_c); }
            pend_c = 0;
        }
#pragma unroll
        for (int k = 0; k < kCsRowsPerLane; ++k) {
            const double x = INT ? (double)(int64_t)v[k] : u2d(v[k]);
            const bool in = ok[k] && x >= a.lo && x <= a.hi;   // (NaN fails both)
            int j = 0;
            if (in) {
                double e = (x - a.lo) * a.scale;
                e = fmin(fmax(e, 0.0), (double)(nb - 1));
                j = (int)e;
                ++cnt;
            }
            // the estimate is right or one off almost always: one straight-line test, and only a wave in which a lane
            // has to move goes through the loops that finish the correction
            const double e0 = cs_edge(a.lo, a.hi, a.step, nb, j), e1 = cs_edge(a.lo, a.hi, a.step, nb, j + 1);
            const int d = !in ? 0 : (x >= e1 && j < nb - 1) ? 1 : (x < e0 && j > 0) ? -1 : 0;
            if (__ballot(d != 0)) {
                if (d) {
                    j += d;
                    while (j > 0 && x < cs_edge(a.lo, a.hi, a.step, nb, j)) --j;
                    while (j < nb - 1 && x >= cs_edge(a.lo, a.hi, a.step, nb, j + 1)) ++j;
                }
            }
            if (SMALL) {   // four 16-bit counters per 64-bit word, private to the lane
                const unsigned long long inc = in ? 1ull << (16 * (j & 3)) : 0ull;
#pragma unroll
                for (int q = 0; q < kCsHistRegBins / 4; ++q) wc[q] += (j >> 2) == q ? inc : 0ull;
                continue;
            }
            unsigned long long open = __ballot(in);
            for (int p = 0; p < a.peels && open; ++p) {
                const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)open) - 1);
                const int jb = __builtin_amdgcn_readlane(j, leader);
                const unsigned long long same = __ballot(in && j == jb) & open;
                const unsigned int c = (unsigned int)__popcll(same);
                if (p == 0) {
                    if (jb == pend_j) pend_c += c;
                    else {
                        if (pend_c && lane == 0) { if (LDS) atomicAdd(&mine[pend_j], pend_c); else atomicAdd(&a.counts[pend_j], (unsigned long long)pend_c); }
                        pend_j = jb;
                        pend_c = c;
                    }
                } else if (lane == leader) {
                    if (LDS) atomicAdd(&mine[jb], c);
                    else atomicAdd(&a.counts[jb], (unsigned long long)c);
                }
                open &= ~same;
            }
            if ((open >> lane) & 1) {
                if (LDS) atomicAdd(&mine[j], 1u);
                else atomicAdd(&a.counts[j], 1ull);
            }
        }
    }
    if (pend_c && lane == 0) { if (LDS) atomicAdd(&mine[pend_j], pend_c); else atomicAdd(&a.counts[pend_j], (unsigned long long)pend_c); }
    if (SMALL) flush_small();
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < nb; b += kCsThreads) {
            unsigned long long sum = 0;
            for (int c = 0; c < copies; ++c) sum += lc[c * nb + b];
            if (sum) atomicAdd(&a.counts[b], sum);
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += shfl_xor64(cnt, m);
    if (lane == 0 && cnt) atomicAdd(a.counted, cnt);
}

__global__ void cs_fill64_kernel(uint64_t* p, int64_t n, uint64_t v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

// ---------------------------------------------------------------- the insert-only set in HBM

// -> the key's slot, or -1 when the table has taken the keys it was sized for (CS_G_OVERFLOW is raised).  fresh = the key
// was new: the caller adds the wave's new keys to CS_G_COUNT with ONE atomic (wave_count) — a same-address atomic per new
// key costs ~12 ns each, 12 ms per million distinct values.
__device__ int64_t set_insert(const CsSetArgs& a, uint64_t key, uint64_t h, bool& fresh) {
    uint64_t s = (h >> 20) & a.mask;
    for (uint64_t probe = 0; probe <= a.mask; ++probe) {
        uint64_t cur = __atomic_load_n(&a.table[s], __ATOMIC_RELAXED);
        if (cur == key) return (int64_t)s;
        if (cur == kCsEmpty) {
            if (__atomic_load_n(&a.g[CS_G_COUNT], __ATOMIC_RELAXED) >= a.max_fill) break;
            cur = atomicCAS((unsigned long long*)&a.table[s], (unsigned long long)kCsEmpty, (unsigned long long)key);
            if (cur == kCsEmpty) { fresh = true; return (int64_t)s; }
            if (cur == key) return (int64_t)s;
        }
        s = (s + 1) & a.mask;
    }
    __atomic_store_n(&a.g[CS_G_OVERFLOW], 1ull, __ATOMIC_RELAXED);
    return -1;
}

// all lanes of the wave: the wave's count of new keys grows by the lanes with `fresh`, and goes to CS_G_COUNT in lots of
// kCsCountLot or more (flush = whatever is left, at the end of the kernel).  The table's "full" test reads a count that
// lags by less than 2 * kCsCountLot keys per resident wave; its probe loop is bounded by the table whatever the count says.
constexpr unsigned int kCsCountLot = 256;
__device__ __forceinline__ void wave_count(bool fresh, unsigned int& pending, unsigned long long* ctr, bool flush = false) {
    pending += (unsigned int)__popcll(__ballot(fresh));
    if ((pending >= kCsCountLot || (flush && pending)) ) {
        if ((threadIdx.x & 63) == 0) atomicAdd(ctr, (unsigned long long)pending);
        pending = 0;
    }
}

__device__ __forceinline__ uint64_t norm_f64(uint64_t b) {
    const double x = u2d(b);
    if (x != x) return 0x7FF8000000000000ull;   // every NaN is one value
    if (x == 0.0) return 0;                     // -0.0 and +0.0 are one value, +0.0
    return b;
}

__device__ __forceinline__ void cs_distinct_row(const CsSetArgs& a, unsigned long long* lset, unsigned int* lcount, bool ok, uint64_t bits, bool& fresh) {
    if (!ok) return;
    const uint64_t key = a.is_f64 ? norm_f64(bits) : bits;
    if (key == kCsEmpty) { __atomic_store_n(&a.g[CS_G_SPECIAL], 1ull, __ATOMIC_RELAXED); return; }
    const uint64_t h = mix64(key);
    int s = (int)(h & (kCsLdsSetSlots - 1));
    for (int probe = 0; probe < 8; ++probe) {
        unsigned long long cur = __atomic_load_n(&lset[s], __ATOMIC_RELAXED);
        if (cur == key) return;
        if (cur == kCsEmpty) {
            if (__atomic_load_n(lcount, __ATOMIC_RELAXED) >= kCsLdsSetSlots / 2) break;
            cur = atomicCAS(&lset[s], (unsigned long long)kCsEmpty, (unsigned long long)key);
            if (cur == kCsEmpty) { atomicAdd(lcount, 1u); break; }   // new to the block: goes on to the table
            if (cur == key) return;
        }
        s = (s + 1) & (kCsLdsSetSlots - 1);
    }
    (void)set_insert(a, key, h, fresh);
}

__global__ __launch_bounds__(kCsThreads) void cs_distinct_kernel(CsSetArgs a) {
    __shared__ unsigned long long lset[kCsLdsSetSlots];
    __shared__ unsigned int lcount;
    for (int i = threadIdx.x; i < kCsLdsSetSlots; i += kCsThreads) lset[i] = kCsEmpty;
    if (threadIdx.x == 0) lcount = 0;
    __syncthreads();
    unsigned int pending = 0;
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        if (__atomic_load_n(&a.g[CS_G_OVERFLOW], __ATOMIC_RELAXED)) break;
        const CsTileView tv = cs_tile(a.col, t);
        uint64_t v[kCsRowsPerLane];
        bool ok[kCsRowsPerLane];
        cs_load(tv, v, ok);
#pragma unroll
        for (int k = 0; k < kCsRowsPerLane; ++k) {
            bool fresh = false;
            cs_distinct_row(a, lset, &lcount, ok[k], v[k], fresh);
            wave_count(fresh, pending, &a.g[CS_G_COUNT]);
        }
    }
    wave_count(false, pending, &a.g[CS_G_COUNT], true);
}

constexpr int kCsEmitSlots = 16;   // table slots per thread and trip of the emit pass (128 contiguous bytes)
__global__ __launch_bounds__(kCsThreads) void cs_emit_kernel(CsSetArgs a) {
    __shared__ CsBlockScan sc;
    const int64_t slots = (int64_t)a.mask + 1, per = (int64_t)kCsThreads * kCsEmitSlots;
    for (int64_t i0 = (int64_t)blockIdx.x * per; i0 < slots; i0 += (int64_t)gridDim.x * per) {
        const int64_t first = i0 + (int64_t)threadIdx.x * kCsEmitSlots;
        uint64_t key[kCsEmitSlots];
        unsigned int mine = 0;
#pragma unroll
        for (int k = 0; k < kCsEmitSlots; ++k) {
            key[k] = first + k < slots ? a.table[first + k] : kCsEmpty;
            mine += key[k] != kCsEmpty;
        }
        unsigned long long pos = block_reserve(mine, &a.g[CS_G_EMITTED], sc);
#pragma unroll
        for (int k = 0; k < kCsEmitSlots; ++k) {
            if (key[k] == kCsEmpty) continue;
            if (a.out64) a.out64[pos] = key[k];
            else a.out32[pos] = a.rep[first + k];
            ++pos;
        }
    }
}

// ---------------------------------------------------------------- the sort route of the numeric distinct

__device__ __forceinline__ bool cs_key_at(const CsCol& col, int is_f64, uint32_t row, double inv, uint64_t& key) {
    const int64_t c = find_chunk_row(col.row_start, col.nchunks, (int64_t)row, inv);
    const DevChunkCol ch = col.chunks[c];
    const int64_t e = ch.offset + ((int64_t)row - col.row_start[c]);
    if (ch.validity && !((ch.validity[e >> 3] >> (e & 7)) & 1)) return false;
    const uint64_t b = ((const uint64_t*)ch.values)[e];
    key = is_f64 ? norm_f64(b) : b;
    return true;
}

// NaNs (the sort puts the negative ones first, the others after +inf) are not runs: they raise CS_G_SPECIAL, the host adds one
__global__ __launch_bounds__(kCsThreads) void cs_runs_kernel(CsRunArgs a) {
    __shared__ CsBlockScan sc;
    const double inv = chunk_lookup_scale(a.col.row_start, a.col.nchunks);
    const uint64_t nan = 0x7FF8000000000000ull;
    for (int64_t i0 = (int64_t)blockIdx.x * kCsThreads; i0 < a.col.n; i0 += (int64_t)gridDim.x * kCsThreads) {
        const int64_t i = i0 + threadIdx.x;
        bool first = false;
        uint64_t key = 0;
        if (i < a.col.n && cs_key_at(a.col, a.is_f64, a.perm[i], inv, key)) {
            if (a.is_f64 && key == nan) __atomic_store_n(&a.g[CS_G_SPECIAL], 1ull, __ATOMIC_RELAXED);
            else {
                uint64_t pk = 0;
                first = i == 0 || !cs_key_at(a.col, a.is_f64, a.perm[i - 1], inv, pk) || (a.is_f64 && pk == nan) || pk != key;
            }
        }
        const unsigned long long pos = block_reserve(first ? 1u : 0u, &a.g[CS_G_EMITTED], sc);
        if (first && a.out64) a.out64[pos] = key;
    }
}

// ---------------------------------------------------------------- Utf8

struct CsRow { const uint8_t* p; int32_t len; bool valid; };

__device__ int64_t cs_find_chunk(const Utf8Chunk* ch, int64_t nch, int64_t row) {
    int64_t lo = 0, hi = nch;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ch[mid].row_start <= row) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
__device__ __forceinline__ CsRow cs_row(const CsUtf8Args& a, int64_t row) {
    const Utf8Chunk& c = a.chunks[a.nchunks > 1 ? cs_find_chunk(a.chunks, a.nchunks, row) : 0];
    const int64_t e = row - c.row_start;
    int32_t b = c.offs[e], en = c.offs[e + 1];
    b = b < c.lo ? c.lo : (b > c.hi ? c.hi : b);
    en = en < b ? b : (en > c.hi ? c.hi : en);
    CsRow r;
    r.p = c.data + b;
    r.len = en - b;
    r.valid = !c.valid || ((c.valid[(c.valid_off + e) >> 3] >> ((c.valid_off + e) & 7)) & 1);
    return r;
}

// cs_word / cs_term / cs_stream / cs_hash_close, the hash of a row: rdf_hash.h

// need: this lane wants ra == rb decided.  Called by all lanes of the wave (long rows are compared by the whole wave).
__device__ bool cs_rows_equal(bool need, const CsRow& ra, const CsRow& rb) {
    const int lane = threadIdx.x & 63;
    bool eq = true, lng = false;
    if (need) {
        if (ra.len != rb.len) eq = false;
        else if (ra.len >= kCsLongRow) lng = true;
        else {
            const int32_t nw = (ra.len + 7) >> 3;
            for (int32_t w = 0; w < nw && eq; ++w) eq = cs_word(ra.p, ra.len, w) == cs_word(rb.p, rb.len, w);
        }
    }
    unsigned long long m = __ballot(lng);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const uint8_t* pa = (const uint8_t*)(uintptr_t)shfl64((uint64_t)(uintptr_t)ra.p, src);
        const uint8_t* pb = (const uint8_t*)(uintptr_t)shfl64((uint64_t)(uintptr_t)rb.p, src);
        const int32_t len = __shfl(ra.len, src);
        const int32_t nw = (len + 7) >> 3;
        bool diff = false;
        for (int32_t w0 = 0; w0 < nw; w0 += 64) {
            const int32_t w = w0 + lane;
            diff = w < nw && cs_word(pa, len, w) != cs_word(pb, len, w);
            if (__ballot(diff)) { diff = true; break; }
        }
        const bool any = __ballot(diff) != 0;
        if (lane == src) eq = !any;
    }
    return eq;
}

__global__ __launch_bounds__(kCsThreads) void cs_utf8_hash_kernel(CsUtf8Args a) {
    const int lane = threadIdx.x & 63;
    unsigned int pending = 0;
    for (int64_t i0 = (int64_t)blockIdx.x * kCsThreads; i0 < a.n; i0 += (int64_t)gridDim.x * kCsThreads) {
        const int64_t i = i0 + threadIdx.x;
        CsRow r{nullptr, 0, false};
        if (i < a.n) r = cs_row(a, i);
        const bool lng = r.valid && r.len >= kCsLongRow;
        uint64_t acc = 0;
        if (r.valid && !lng) {
            const int32_t nw = (r.len + 7) >> 3;
            for (int32_t w = 0; w < nw; ++w) acc += cs_term(0, cs_word(r.p, r.len, w), w);
        }
        unsigned long long m = __ballot(lng);
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint8_t* p = (const uint8_t*)(uintptr_t)shfl64((uint64_t)(uintptr_t)r.p, src);
            const int32_t len = __shfl(r.len, src);
            static_assert(kCsStreams == 64, "one stream per lane of the wave");
            uint64_t st = cs_stream(p, len, lane);
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) st += shfl_xor64(st, x);
            if (lane == src) acc = st;
        }
        bool fresh = false;
        if (r.valid) {
            const uint64_t h = cs_hash_close(acc, r.len);
            a.hash[i] = h;
            if (!__atomic_load_n(&a.set.g[CS_G_OVERFLOW], __ATOMIC_RELAXED)) {
                const int64_t s = set_insert(a.set, h, h, fresh);
                if (s >= 0 && (uint32_t)i < __atomic_load_n(&a.set.rep[s], __ATOMIC_RELAXED)) atomicMin(&a.set.rep[s], (uint32_t)i);
            }
        }
        wave_count(fresh, pending, &a.set.g[CS_G_COUNT]);
    }
    wave_count(false, pending, &a.set.g[CS_G_COUNT], true);
}

__global__ __launch_bounds__(kCsThreads) void cs_utf8_verify_kernel(CsUtf8Args a) {
    for (int64_t i0 = (int64_t)blockIdx.x * kCsThreads; i0 < a.n; i0 += (int64_t)gridDim.x * kCsThreads) {
        const int64_t i = i0 + threadIdx.x;
        CsRow r{nullptr, 0, false}, q{nullptr, 0, false};
        if (i < a.n) r = cs_row(a, i);
        bool need = false, lost = false;
        if (r.valid) {
            const uint64_t h = a.hash[i];
            uint64_t s = (h >> 20) & a.set.mask;
            lost = true;
            for (uint64_t probe = 0; probe <= a.set.mask; ++probe) {
                const uint64_t cur = a.set.table[s];
                if (cur == h) { lost = false; break; }
                if (cur == kCsEmpty) break;
                s = (s + 1) & a.set.mask;
            }
            if (!lost) {
                const uint32_t rep = a.set.rep[s];
                if ((int64_t)rep >= a.n) lost = true;
                else if ((int64_t)rep != i) { need = true; q = cs_row(a, rep); }
            }
        }
        const bool eq = cs_rows_equal(need, r, q);
        if (lost || (need && !eq)) __atomic_store_n(&a.set.g[CS_G_MISMATCH], 1ull, __ATOMIC_RELAXED);
    }
}

// the exact route: rows in sorted order (NULL rows last), a row is kept when it differs from the row in front of it
__global__ __launch_bounds__(kCsThreads) void cs_utf8_runs_kernel(CsUtf8Args a) {
    __shared__ CsBlockScan sc;
    for (int64_t i0 = (int64_t)blockIdx.x * kCsThreads; i0 < a.n; i0 += (int64_t)gridDim.x * kCsThreads) {
        const int64_t i = i0 + threadIdx.x;
        CsRow r{nullptr, 0, false}, q{nullptr, 0, false};
        uint32_t row = 0;
        if (i < a.n) {
            row = a.perm[i];
            if ((int64_t)row < a.n) r = cs_row(a, row);
        }
        bool need = false;
        if (r.valid && i > 0) {
            const uint32_t prev = a.perm[i - 1];
            if ((int64_t)prev < a.n) q = cs_row(a, prev);
            need = q.valid;
        }
        const bool eq = cs_rows_equal(need, r, q);
        const bool first = r.valid && !(need && eq);
        const unsigned long long pos = block_reserve(first ? 1u : 0u, &a.set.g[CS_G_EMITTED], sc);
        if (first && a.out32) a.out32[pos] = row;
    }
}

// ---------------------------------------------------------------- Utf8 dictionary encoding

// The hash route: cs_utf8_verify_kernel's pass that also keeps what it finds — the representative of every row (the
// smallest row with the row's hash, compared byte for byte) and a flag where a row is its own representative.
__global__ __launch_bounds__(kCsThreads) void cs_dict_rep_kernel(CsDictArgs a) {
    const CsUtf8Args& u = a.u;
    for (int64_t i0 = (int64_t)blockIdx.x * kCsThreads; i0 < u.n; i0 += (int64_t)gridDim.x * kCsThreads) {
        const int64_t i = i0 + threadIdx.x;
        CsRow r{nullptr, 0, false}, q{nullptr, 0, false};
        if (i < u.n) r = cs_row(u, i);
        bool need = false, lost = false;
        uint32_t rep = kCsNoRow;
        if (r.valid) {
            const uint64_t h = u.hash[i];
            uint64_t s = (h >> 20) & u.set.mask;
            lost = true;
            for (uint64_t probe = 0; probe <= u.set.mask; ++probe) {
                const uint64_t cur = u.set.table[s];
                if (cur == h) { lost = false; break; }
                if (cur == kCsEmpty) break;
                s = (s + 1) & u.set.mask;
            }
            if (!lost) {
                rep = u.set.rep[s];
                if ((int64_t)rep >= u.n) { lost = true; rep = kCsNoRow; }
                else if ((int64_t)rep != i) { need = true; q = cs_row(u, rep); }
            }
        }
        const bool eq = cs_rows_equal(need, r, q);
        if (lost || (need && !eq)) __atomic_store_n(&u.set.g[CS_G_MISMATCH], 1ull, __ATOMIC_RELAXED);
        if (i < u.n) {
            a.rep[i] = rep;
            a.flags[i] = (int64_t)rep == i ? 1 : 0;
        }
    }
}

// The exact route, by sorted position (NULL rows last): flags[i] = 1 where position i starts a run of equal values; rep[]
// of the position's row says whether the row is NULL (kCsNoRow) or has a value (0, replaced by cs_dict_spread_kernel).
__global__ __launch_bounds__(kCsThreads) void cs_dict_heads_kernel(CsDictArgs a) {
    const CsUtf8Args& u = a.u;
    for (int64_t i0 = (int64_t)blockIdx.x * kCsThreads; i0 < u.n; i0 += (int64_t)gridDim.x * kCsThreads) {
        const int64_t i = i0 + threadIdx.x;
        CsRow r{nullptr, 0, false}, q{nullptr, 0, false};
        uint32_t row = kCsNoRow;
        if (i < u.n) {
            row = u.perm[i];
            if ((int64_t)row < u.n) r = cs_row(u, row);
        }
        bool need = false;
        if (r.valid && i > 0) {
            const uint32_t prev = u.perm[i - 1];
            if ((int64_t)prev < u.n) q = cs_row(u, prev);
            need = q.valid;
        }
        const bool eq = cs_rows_equal(need, r, q);
        if (i < u.n) {
            a.flags[i] = r.valid && !(need && eq) ? 1 : 0;
            if ((int64_t)row < u.n) a.rep[row] = r.valid ? 0u : kCsNoRow;
        }
    }
}

// phase 0: heads[run] = the row at the run's first position — the sort is stable, so that is the run's smallest row;
// phase 1: every row of a run gets the run's head as its representative, and flags[] (now by row) marks the heads.
template <int PHASE>
__global__ __launch_bounds__(kCsThreads) void cs_dict_spread_kernel(CsDictArgs a) {
    const int64_t n = a.u.n;
    for (int64_t i = (int64_t)blockIdx.x * kCsThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCsThreads) {
        const uint32_t row = a.u.perm[i];
        if ((int64_t)row >= n) continue;
        const int64_t before = a.scan[i], upto = a.scan[i + 1];   // run starts in front of / up to and including position i
        if (PHASE == 0) {
            if (upto != before) a.heads[before] = row;
        } else {
            uint32_t rep = kCsNoRow;
            if (a.rep[row] != kCsNoRow && upto > 0) rep = a.heads[upto - 1];
            a.rep[row] = rep;
            a.flags[row] = rep == row ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(kCsThreads) void cs_dict_firsts_kernel(CsDictArgs a) {
    const int64_t n = a.u.n;
    for (int64_t i = (int64_t)blockIdx.x * kCsThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCsThreads)
        if ((int64_t)a.rep[i] == i) a.firsts[a.scan[i]] = (uint32_t)i;
}

// code = rank of the representative's first occurrence.  A tile is kCsThreads rows of ONE output chunk starting at a
// multiple of kCsThreads, a wave's 64 rows make 8 whole validity bytes: no byte is written by two waves.  NULL rows are
// counted per wave and added to the chunk's counter when the wave moves to another chunk.
__global__ __launch_bounds__(kCsThreads) void cs_dict_codes_kernel(CsDictArgs a) {
    const int lane = threadIdx.x & 63;
    int64_t pend_c = -1;
    unsigned int pend = 0;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        int64_t lo = 0, hi = a.nouts;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.outs[mid].tile_start <= t) lo = mid + 1; else hi = mid;
        }
        const int64_t c = lo - 1;
        const CsDictOut o = a.outs[c];
        const int64_t e = (t - o.tile_start) * kCsThreads + threadIdx.x;
        const bool in = e < o.rows;
        bool valid = false;
        if (in) {
            const uint32_t rep = a.rep[o.row_start + e];
            valid = rep != kCsNoRow;
            o.codes[e] = valid ? (uint32_t)a.scan[rep] : 0u;
        }
        const unsigned long long vm = __ballot(valid);
        const unsigned int nulls = (unsigned int)__popcll(__ballot(in && !valid));
        const int64_t e0 = e - lane;   // the wave's first row: a multiple of 64
        if (o.valid && lane < 8 && e0 + lane * 8 < o.rows) o.valid[(e0 >> 3) + lane] = (uint8_t)(vm >> (8 * lane));
        if (c != pend_c) {
            if (pend && lane == 0) atomicAdd(&a.nulls[pend_c], (unsigned long long)pend);
            pend_c = c;
            pend = 0;
        }
        pend += nulls;
    }
    if (pend && lane == 0) atomicAdd(&a.nulls[pend_c], (unsigned long long)pend);
}

}  // namespace

int cs_grid(int64_t items) {
    const int64_t want = (items + kCsThreads - 1) / kCsThreads;
    const int64_t lim = (int64_t)eval_grid_limit();
    return (int)(want < 1 ? 1 : (want > lim ? lim : want));
}

hipError_t launch_cs_hist(const CsHistArgs& a, hipStream_t s) {
    if (a.col.ntiles <= 0) return hipSuccess;
    // 32-bit block counters: a block never counts 2^31 rows
    int64_t grid = std::min<int64_t>(a.col.ntiles, eval_grid_limit());
    grid = std::max<int64_t>(grid, (a.col.n >> 31) + 1);
    const dim3 g((unsigned)grid), b(kCsThreads);
    if (a.nbins <= kCsHistRegBins) {
        if (a.is_int) hipLaunchKernelGGL((cs_hist_kernel<true, true, true>), g, b, 0, s, a);
        else hipLaunchKernelGGL((cs_hist_kernel<true, false, true>), g, b, 0, s, a);
    } else if (a.nbins <= kCsHistLdsBins) {
        if (a.is_int) hipLaunchKernelGGL((cs_hist_kernel<true, true, false>), g, b, 0, s, a);
        else hipLaunchKernelGGL((cs_hist_kernel<true, false, false>), g, b, 0, s, a);
    } else {
        if (a.is_int) hipLaunchKernelGGL((cs_hist_kernel<false, true, false>), g, b, 0, s, a);
        else hipLaunchKernelGGL((cs_hist_kernel<false, false, false>), g, b, 0, s, a);
    }
    return hipGetLastError();
}
hipError_t launch_cs_fill64(uint64_t* p, int64_t n, uint64_t v, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cs_fill64_kernel, dim3(cs_grid(n)), dim3(kCsThreads), 0, s, p, n, v);
    return hipGetLastError();
}
hipError_t launch_cs_distinct(const CsSetArgs& a, hipStream_t s) {
    if (a.col.ntiles <= 0) return hipSuccess;
    const int64_t grid = std::min<int64_t>(a.col.ntiles, eval_grid_limit());
    hipLaunchKernelGGL(cs_distinct_kernel, dim3((unsigned)grid), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cs_emit(const CsSetArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(cs_emit_kernel, dim3(cs_grid(((int64_t)a.mask + kCsEmitSlots) / kCsEmitSlots)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cs_runs(const CsRunArgs& a, hipStream_t s) {
    if (a.col.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cs_runs_kernel, dim3(cs_grid(a.col.n)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cs_utf8_hash(const CsUtf8Args& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cs_utf8_hash_kernel, dim3(cs_grid(a.n)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cs_utf8_verify(const CsUtf8Args& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cs_utf8_verify_kernel, dim3(cs_grid(a.n)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cs_utf8_runs(const CsUtf8Args& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cs_utf8_runs_kernel, dim3(cs_grid(a.n)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cs_dict_rep(const CsDictArgs& a, hipStream_t s) {
    if (a.u.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cs_dict_rep_kernel, dim3(cs_grid(a.u.n)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cs_dict_heads(const CsDictArgs& a, hipStream_t s) {
    if (a.u.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cs_dict_heads_kernel, dim3(cs_grid(a.u.n)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cs_dict_spread(const CsDictArgs& a, hipStream_t s) {
    if (a.u.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cs_dict_spread_kernel<0>, dim3(cs_grid(a.u.n)), dim3(kCsThreads), 0, s, a);
    hipLaunchKernelGGL(cs_dict_spread_kernel<1>, dim3(cs_grid(a.u.n)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cs_dict_firsts(const CsDictArgs& a, hipStream_t s) {
    if (a.u.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cs_dict_firsts_kernel, dim3(cs_grid(a.u.n)), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cs_dict_codes(const CsDictArgs& a, hipStream_t s) {
    if (a.ntiles <= 0) return hipSuccess;
    const int64_t grid = std::min<int64_t>(a.ntiles, eval_grid_limit());
    hipLaunchKernelGGL(cs_dict_codes_kernel, dim3((unsigned)grid), dim3(kCsThreads), 0, s, a);
    return hipGetLastError();
}
