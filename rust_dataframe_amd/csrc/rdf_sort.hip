// rdf_sort.hip — the radix passes of DataFrame::sort (-> arrow::compute::lexsort_to_indices, src/dataframe.rs:194-214) and of
// every other sort on the device (join build side, window partitions, uniques): ONE kernel per 8-bit digit that reads the
// (key, row) pairs once and writes them once.
//   os_hist_kernel     one read of the keys builds the digit histograms of EVERY pass of the column at once
//   os_bases_kernel    their exclusive scans = where each digit's run starts in every pass
//   os_scatter_kernel  per pass: a block takes the next tile (ticket), ranks it with per-WAVE digit counters (a wave's lanes
//                      that share a digit are found with 8 ballots; the run's first lane bumps the counter — no atomics),
//                      publishes the tile's digit counts, finds its global offsets by DECOUPLED LOOK-BACK over the tiles
//                      before it (each digit's thread walks back until it meets a tile whose inclusive prefix is published),
//                      and writes the locally sorted tile out in digit runs.
//   os_bounds_kernel, os_bucket_max_kernel, os_local_kernel, os_local_wide_kernel
//                      the finish of the most-significant-digits-first order: after passes over the top bits, one wave sorts
//                      each bucket of rows that share them in LDS
//   os_sample_kernel   a sample of the keys for the host's value-bucket plan of f64 columns
// Stable: tiles are ticketed in index order and a tile's offsets are the prefix over lower-numbered tiles only.
// This is the only digit pass.  Three other forms of it were built, held to the oracle, measured slower and removed — scanner
// blocks instead of the look-back, K tiles per ticket, static tile ranges per block: profiles/r06_sort_digit_pass_ab.jsonl,
// r06_sort_super_tiles_ab.jsonl and r06_sort_super_tiles_unrolled_sweep_ab.jsonl hold what they measured.  (The histogram ->
// scan -> scatter kernels of rdf_kernels.hip, the first sort here, now serve the GROUP BY's radix partitioning only.)
//
// Cross-XCD visibility: the per-XCD L2s are not coherent, so a tile's state word is ONE naturally aligned 8-byte
// {sequence | flag | value} granule written and read with agent-scope atomics (write-through / L2-bypassing on gfx950,
// MI355X_MICROARCH.md "Workgroup dispatch, XCD placement & inter-workgroup visibility": an 8-byte granule needs no further
// ordering).  The sequence field makes words of earlier passes read as "not published", so the state array is zeroed once
// per sort, not once per pass.
#include "rdf_common.hip.h"

namespace rdfk {

// Phase timers of os_scatter_kernel (build with -DRDF_SORT_TIMERS, run with RDF_DEBUG_SORT=1): reading the clock drains the
// memory counters, so the timed build is ~8 % slower and is not the one that ships.
#ifdef RDF_SORT_TIMERS
#define OS_TIMERS_DECL unsigned long long tph[6] = {0, 0, 0, 0, 0, 0}
#define OS_TICK(c) const unsigned long long c = __builtin_readcyclecounter()
#define OS_TIMERS_ADD do { tph[0] += c1 - c0; tph[1] += c2 - c1; tph[2] += c3 - c2; tph[3] += c4 - c3; tph[4] += c5 - c4; tph[5] += 1; } while (0)
#define OS_TIMERS_FLUSH do { if (a.debug && threadIdx.x == 0) for (int i = 0; i < 6; ++i) atomicAdd(a.debug + i, tph[i]); } while (0)
#else
#define OS_TIMERS_DECL
#define OS_TICK(c)
#define OS_TIMERS_ADD
#define OS_TIMERS_FLUSH
#endif

constexpr int kOsWaves = kBlock / 64;
constexpr int kOsLook = 8;                  // predecessors read per look-back step
constexpr uint64_t kOsValueMask = (1ull << 48) - 1;
constexpr uint64_t kOsLocal = 1ull << 48, kOsInclusive = 2ull << 48;

__device__ __forceinline__ int os_digit(uint64_t key, uint64_t bias, int shift, int mask = 255) { return (int)(((key - bias) >> shift) & (uint64_t)mask); }
// every kernel that maps keys holds the plan's segment table (OsBucket::seg, rdf_sort_map.h) in LDS: as a dependent global load per
// key it cost the histogram and boundary kernels 0.1 - 0.15 ms each per 5e7 keys
__device__ __forceinline__ void os_load_segs(const OsBucket& f, uint2* lds) {      // whole block
    if (!f.seg || f.flat) return;
    for (int i = threadIdx.x; i < kOsSegs; i += blockDim.x) lds[i] = make_uint2(as_global<uint32_t>(f.seg)[2 * i], as_global<uint32_t>(f.seg)[2 * i + 1]);
    __syncthreads();
}
// the value bucket of an f64 key (OsBucket): order-preserving key bits -> the double -> os_map_value
__device__ __forceinline__ uint32_t os_value_bucket(uint64_t key, const OsBucket& f, const uint2* segs) {
    const uint64_t ord = f.flip ? ~key : key;
    const uint64_t b = (ord >> 63) ? (ord ^ 0x8000000000000000ull) : ~ord;
    const uint32_t k = os_map_value(u2d(b), (b >> 63) != 0, f, segs);
    return f.flip ? ((1u << f.bits) - 1) - k : k;
}

// Histograms of all `npass` digits of (key - bias) in one read of the keys (+ the NULL count for the nulls-last pass).
__global__ __launch_bounds__(kBlock) void os_hist_kernel(const OsHistArgs a) {
    __shared__ unsigned int h[9][256];
    __shared__ uint2 segs[kOsSegs];
    os_load_segs(a.fb, segs);
    for (int p = 0; p < 9; ++p) h[p][threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
        uint64_t k = __builtin_nontemporal_load(as_global<uint64_t>(a.keys) + i);
        k = a.fb.bits ? (uint64_t)os_value_bucket(k, a.fb, segs) : k - a.bias;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            if (p >= a.npass) break;
            const int d = a.generic ? (int)((k >> a.shift[p]) & (uint64_t)a.mask[p]) : (int)((k >> (8 * p)) & 255);
            // a wave whose rows all share the digit (the upper bytes of a narrow range, dictionary codes): one add, not 64 serialised ones
            const int d0 = __builtin_amdgcn_readfirstlane(d);
            const uint64_t same = __ballot(d == d0);
            if (same == __ballot(1)) { if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(same)) atomicAdd(&h[p][d0], (unsigned)__popcll(same)); }
            else atomicAdd(&h[p][d], 1u);
        }
        if (a.nullflags) { if (as_global<uint8_t>(a.nullflags)[i]) atomicAdd(&h[8][1], 1u); }
    }
    __syncthreads();
    for (int p = 0; p < a.npass; ++p) { const unsigned int c = h[p][threadIdx.x]; if (c) atomicAdd((unsigned long long*)&a.hist[p * 256 + threadIdx.x], (unsigned long long)c); }
    if (a.nullflags && threadIdx.x == 1 && h[8][1]) atomicAdd((unsigned long long*)&a.hist[8 * 256 + 1], (unsigned long long)h[8][1]);
}

// exclusive scan of each pass's 256 counts (block p = pass p; pass 8 = the nulls-last pass: bin 0 = n - nulls)
__global__ __launch_bounds__(256) void os_bases_kernel(int64_t* hist, int64_t n) {
    __shared__ int64_t s[256];
    const int p = blockIdx.x;
    int64_t c = hist[p * 256 + threadIdx.x];
    if (p == 8 && threadIdx.x == 0) c = n - hist[8 * 256 + 1];
    s[threadIdx.x] = c;
    __syncthreads();
    int64_t run = 0;
    for (int i = 0; i < (int)threadIdx.x; ++i) run += s[i];
    hist[p * 256 + threadIdx.x] = run;
}

template <int ITEMS>
__global__ __launch_bounds__(kBlock) void os_scatter_kernel(const OsPassArgs a) {
    constexpr int TILE = kBlock * ITEMS;
    __shared__ uint64_t lkeys[TILE];
    __shared__ uint32_t lidx[TILE];
    __shared__ uint8_t ldig[TILE];
    __shared__ unsigned int whist[kOsWaves][256];      // per-wave digit counts, then the wave's exclusive offset inside the digit's run
    __shared__ unsigned int dbase[256];                // tile-local start of each digit's run
    __shared__ int64_t gbase[256];                     // global start of this tile's part of each digit's run
    __shared__ unsigned int wsum[kOsWaves];
    __shared__ unsigned int thist[256];                // the tile's digit counts, taken before the ranking so that they can be published early
    __shared__ int64_t tile_s;
    __shared__ uint2 segs[kOsSegs];
    os_load_segs(a.fb, segs);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t seq = (uint64_t)a.seq << 50;
    OS_TIMERS_DECL;
    for (;;) {
        OS_TICK(c0);
        if (threadIdx.x == 0) tile_s = (int64_t)atomicAdd((unsigned long long*)a.ticket, 1ull);
#pragma unroll
        for (int w = 0; w < kOsWaves; ++w) whist[w][threadIdx.x] = 0;
        thist[threadIdx.x] = 0;
        __syncthreads();
        const int64_t tile = tile_s;
        if (tile >= a.ntiles) break;
        const int64_t base = tile * TILE;
        const int count = (int)((a.n - base) < (int64_t)TILE ? (a.n - base) : (int64_t)TILE);
        // ---- load (a wave owns ITEMS consecutive rows of 64 items) and rank inside the wave
        uint64_t key[ITEMS];
        uint32_t idx[ITEMS];
        int digit[ITEMS], rank[ITEMS];
        OS_TICK(c1);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int64_t i = base + (wave * ITEMS + j) * 64 + lane;
            const bool in = i < a.n;
            key[j] = in ? __builtin_nontemporal_load(as_global<uint64_t>(a.keys_in) + i) : 0;
            idx[j] = in ? (a.idx_in ? __builtin_nontemporal_load(as_global<uint32_t>(a.idx_in) + i) : (uint32_t)i) : 0;
        }
        // The tile's digit counts first, with plain LDS adds, and PUBLISHED at once: every tile ticketed after this one waits for
        // them in its look-back, and the ranking below (~6 us of dependent LDS round trips) then runs while this tile in turn
        // waits for the tiles before it, instead of in front of everybody's wait.
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int64_t i = base + (wave * ITEMS + j) * 64 + lane;
            int d = 0;
            if (i < a.n) {
                d = a.nullflags ? (int)as_global<uint8_t>(a.nullflags)[idx[j]]
                                : a.fb.bits ? (int)((os_value_bucket(key[j], a.fb, segs) >> a.shift) & (uint32_t)a.mask) : os_digit(key[j], a.bias, a.shift, a.mask);
                atomicAdd(&thist[d], 1u);
            }
            digit[j] = d;
        }
        __syncthreads();
        const unsigned int total_d = thist[threadIdx.x];
        unsigned long long* st = a.state + tile * 256 + threadIdx.x;
        if (tile > 0) __hip_atomic_store(st, seq | kOsLocal | total_d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // ranks inside the wave: the lanes of a row that share my digit (8 ballots); the run's first lane bumps the wave's counter
        // of the digit (plain read + write: the LDS serves a wave's instructions in order, rows are taken in order: stable).
        // (Measured alternatives, both slower on the whole sort: one returning LDS add per row issued back to back for all rows
        // — it keeps four more values per item live, 5.97 against 5.49 ms per 5e7 full-range keys — and 2048-pair tiles at
        // five blocks per CU, 996 against 653 us per pass: more tiles in flight, longer waits in the look-back.)
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int64_t i = base + (wave * ITEMS + j) * 64 + lane;
            const bool in = i < a.n;
            const int d = digit[j];
            uint64_t peers = __ballot(in);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const uint64_t m = __ballot((d >> b) & 1);
                peers &= ((d >> b) & 1) ? m : ~m;
            }
            const int leader = __builtin_ctzll(peers | (1ull << 63));
            unsigned int before = 0;
            if (in && lane == leader) { before = whist[wave][d]; whist[wave][d] = before + (unsigned)__popcll(peers); }
            before = __shfl(before, leader);
            rank[j] = (int)before + __popcll(peers & ((1ull << lane) - 1));
        }
        OS_TICK(c2);
        __syncthreads();
        OS_TICK(c3);
        // ---- thread d: the waves' counts of digit d -> their offsets inside the run
        {
            unsigned int run = 0;
#pragma unroll
            for (int w = 0; w < kOsWaves; ++w) { const unsigned int c = whist[w][threadIdx.x]; whist[w][threadIdx.x] = run; run += c; }
        }
        // look back for what lies before the tile
        unsigned int inc = total_d;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) { const unsigned int o = __shfl_up(inc, dd); if (lane >= dd) inc += o; }
        if (lane == 63) wsum[wave] = inc;
        // kOsLook predecessors are read at once (independent loads) and consumed nearest first
        int64_t excl = 0;
        for (int64_t t = tile - 1; t >= 0;) {
            unsigned long long w[kOsLook];
#pragma unroll
            for (int u = 0; u < kOsLook; ++u)
                w[u] = t - u >= 0 ? __hip_atomic_load(a.state + (t - u) * 256 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (seq | kOsInclusive);
            int used = 0;
            bool done = false, stalled = false;
#pragma unroll
            for (int u = 0; u < kOsLook; ++u) {
                if (done || stalled) continue;
                if ((w[u] >> 50) != (unsigned long long)a.seq) { stalled = true; continue; }   // not published yet in THIS pass
                excl += (int64_t)(w[u] & kOsValueMask);
                ++used;
                if (w[u] & kOsInclusive) done = true;
            }
            if (done) break;
            t -= used;
            if (stalled) __builtin_amdgcn_s_sleep(1);
        }
        __hip_atomic_store(st, seq | kOsInclusive | (unsigned long long)(excl + total_d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        gbase[threadIdx.x] = a.bases[threadIdx.x] + excl;
        OS_TICK(c4);
        __syncthreads();
        unsigned int wb = 0;
        for (int w = 0; w < wave; ++w) wb += wsum[w];
        dbase[threadIdx.x] = wb + inc - total_d;
        __syncthreads();
        // ---- local stable sort by digit into LDS
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int64_t i = base + (wave * ITEMS + j) * 64 + lane;
            if (i < a.n) {
                const int pos = (int)(dbase[digit[j]] + whist[wave][digit[j]]) + rank[j];
                lkeys[pos] = key[j];
                lidx[pos] = idx[j];
                ldig[pos] = (uint8_t)digit[j];
            }
        }
        __syncthreads();
        // ---- write-out: consecutive threads hold consecutive members of a digit run
        if (count == TILE) {
            // a full tile: all ITEMS rounds at once — the digit reads, then the two base reads that depend on them, then the pair
            // reads and the stores (one round at a time each store waited for a chain of three LDS round trips)
            int dd[ITEMS];
            int64_t dst[ITEMS];
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) dd[j] = ldig[threadIdx.x + j * kBlock];
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) dst[j] = gbase[dd[j]] + ((int)(threadIdx.x + j * kBlock) - (int)dbase[dd[j]]);
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                const int t = threadIdx.x + j * kBlock;
                __builtin_nontemporal_store(lkeys[t], as_global_mut<uint64_t>(a.keys_out) + dst[j]);
                __builtin_nontemporal_store(lidx[t], as_global_mut<uint32_t>(a.idx_out) + dst[j]);
            }
        } else {
            for (int t = threadIdx.x; t < count; t += kBlock) {
                const int d = ldig[t];
                const int64_t dst = gbase[d] + (t - (int)dbase[d]);
                __builtin_nontemporal_store(lkeys[t], as_global_mut<uint64_t>(a.keys_out) + dst);
                __builtin_nontemporal_store(lidx[t], as_global_mut<uint32_t>(a.idx_out) + dst);
            }
        }
        __syncthreads();
        OS_TICK(c5);
        OS_TIMERS_ADD;
    }
    OS_TIMERS_FLUSH;
}

hipError_t launch_os_hist(const OsHistArgs& a, hipStream_t s) {
    int64_t grid = (a.n + (int64_t)kBlock * 16 - 1) / ((int64_t)kBlock * 16);
    if (grid > eval_grid_limit()) grid = eval_grid_limit();
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL(os_hist_kernel, dim3((unsigned)grid), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(os_bases_kernel, dim3(9), dim3(256), 0, s, a.hist, a.n);
    return hipGetLastError();
}
int os_tile_items() { return kBlock * kOsItems; }
hipError_t launch_os_scatter(const OsPassArgs& a, hipStream_t s) {
    // every block must be RESIDENT (a ticketed tile waits for its predecessors): two blocks of 62 KB LDS per CU
    int64_t grid = (int64_t)(eval_grid_limit() / 8) * (kOsItems >= 16 ? 2 : 5);
    if (grid > a.ntiles) grid = a.ntiles;
    if (grid <= 0) return hipSuccess;
    OsPassArgs b = a;
    if (b.mask == 0) b.mask = 255;
    hipLaunchKernelGGL((os_scatter_kernel<kOsItems>), dim3((unsigned)grid), dim3(kBlock), 0, s, b);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The finish of the most-significant-digits-first order (see OsLocalArgs): bucket boundaries, then one block per bucket.

// bstart[b] = first row whose bucket is >= b (rows are sorted by bucket); thread i writes the entries of the buckets that END in
// front of row i — every entry of bstart[0 .. nbuckets] exactly once, empty buckets included
__global__ __launch_bounds__(kBlock) void os_bounds_kernel(const uint64_t* keys, int64_t n, uint64_t bias, int rbits, int nbuckets, const OsBucket fb, uint32_t* bstart) {
    __shared__ uint2 segs[kOsSegs];
    os_load_segs(fb, segs);
    auto bucket = [&](int64_t i) -> int64_t {
        const uint64_t k = as_global<uint64_t>(keys)[i];
        return fb.bits ? (int64_t)os_value_bucket(k, fb, segs) : (int64_t)((k - bias) >> rbits);
    };
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t cur = i < n ? bucket(i) : (int64_t)nbuckets;
        const int64_t prev = i > 0 ? bucket(i - 1) : -1;
        for (int64_t b = prev + 1; b <= cur; ++b) bstart[b] = (uint32_t)i;
    }
}
__global__ __launch_bounds__(kBlock) void os_bucket_max_kernel(const uint32_t* bstart, int nbuckets, unsigned int* out) {
    unsigned int m = 0;
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < nbuckets; b += (int64_t)gridDim.x * kBlock) {
        const unsigned int len = bstart[b + 1] - bstart[b];
        m = len > m ? len : m;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned int o = (unsigned int)__shfl_xor((int)m, d); m = o > m ? o : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// Bitonic network over P 64-bit words in LDS, ONE WAVE per bucket.  A word is (the key's low rbits) << 12 | (the row's place in
// the bucket): the places make the words distinct, so the order of equal keys is the order the rows came in — the sort is
// stable, which the column-by-column lexicographic order and the NULLs-last pass rely on.
// A lane takes 2^MB words whose indices differ in MB consecutive stride bits and runs the MB sub-stages of those strides in
// registers: one LDS round trip per four sub-stages (18 for 1024 words instead of 55 — the first version, one sub-stage per
// round trip and block barrier, was bound by LDS bandwidth: 1.04 ms per 5e7 rows), no block barrier at all.  Words are padded by
// one per 16 (a lane's 16 consecutive words would otherwise put all 64 lanes on the same banks).
__device__ __forceinline__ int os_pad(int i) { return i + (i >> 4); }
template <int MB>
__device__ __forceinline__ void os_chunk(uint64_t* s, int P, int k, int jl_log) {
    constexpr int E = 1 << MB;
    for (int q = threadIdx.x; q < (P >> MB); q += 64) {
        const int i = ((q >> jl_log) << (jl_log + MB)) | (q & ((1 << jl_log) - 1));
        uint64_t v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = s[os_pad(i | (e << jl_log))];
        const bool asc = (i & k) == 0;
#pragma unroll
        for (int b = MB - 1; b >= 0; --b) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (e & (1 << b)) continue;
                const uint64_t x = v[e], y = v[e | (1 << b)];
                const bool sw = (x > y) == asc;
                v[e] = sw ? y : x;
                v[e | (1 << b)] = sw ? x : y;
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) s[os_pad(i | (e << jl_log))] = v[e];
    }
}
// ... over (whole key, place) pairs: value buckets (f64 keys) — the rows of a bucket share no key bits
template <int MB>
__device__ __forceinline__ void os_chunk_wide(uint64_t* s, uint32_t* sp, int P, int k, int jl_log) {
    constexpr int E = 1 << MB;
    for (int q = threadIdx.x; q < (P >> MB); q += 64) {
        const int i = ((q >> jl_log) << (jl_log + MB)) | (q & ((1 << jl_log) - 1));
        uint64_t v[E];
        uint32_t w[E];
#pragma unroll
        for (int e = 0; e < E; ++e) { v[e] = s[os_pad(i | (e << jl_log))]; w[e] = sp[os_pad(i | (e << jl_log))]; }
        const bool asc = (i & k) == 0;
#pragma unroll
        for (int b = MB - 1; b >= 0; --b) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (e & (1 << b)) continue;
                const int f = e | (1 << b);
                const bool gt = v[e] > v[f] || (v[e] == v[f] && w[e] > w[f]);
                const bool sw = gt == asc;
                const uint64_t x = v[e], y = v[f];
                const uint32_t px = w[e], py = w[f];
                v[e] = sw ? y : x; v[f] = sw ? x : y;
                w[e] = sw ? py : px; w[f] = sw ? px : py;
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) { s[os_pad(i | (e << jl_log))] = v[e]; sp[os_pad(i | (e << jl_log))] = w[e]; }
    }
}
__global__ __launch_bounds__(64) void os_local_wide_kernel(const OsLocalArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t s[];
    const int64_t bucket = blockIdx.x;
    const uint32_t start = a.bstart[bucket], len = a.bstart[bucket + 1] - start;
    if (len <= a.len_lo || len > a.len_hi) return;
    if (len == 1) {
        if (threadIdx.x == 0) {
            as_global_mut<uint64_t>(a.keys_out)[start] = as_global<uint64_t>(a.keys_in)[start];
            as_global_mut<uint32_t>(a.idx_out)[start] = a.idx_in ? as_global<uint32_t>(a.idx_in)[start] : start;
        }
        return;
    }
    int P = 2, plog = 1;
    while (P < (int)len) { P <<= 1; ++plog; }
    uint32_t* sp = (uint32_t*)(s + os_pad(a.lds_items) + 1);
    for (int i = threadIdx.x; i < P; i += 64) {
        // padding sorts behind every row: the largest key with a place no row has
        s[os_pad(i)] = i < (int)len ? __builtin_nontemporal_load(as_global<uint64_t>(a.keys_in) + start + i) : ~0ull;
        sp[os_pad(i)] = i < (int)len ? (uint32_t)i : 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int ks = 1; ks <= plog; ++ks) {
        for (int jlog = ks - 1; jlog >= 0;) {
            const int mb = jlog + 1 < 3 ? jlog + 1 : 3;      // 8 pairs per lane: the registers of 16 words
            const int jl_log = jlog - mb + 1;
            switch (mb) {
                case 3: os_chunk_wide<3>(s, sp, P, 1 << ks, jl_log); break;
                case 2: os_chunk_wide<2>(s, sp, P, 1 << ks, jl_log); break;
                default: os_chunk_wide<1>(s, sp, P, 1 << ks, jl_log); break;
            }
            __syncthreads();
            jlog = jl_log - 1;
        }
    }
    for (int j = threadIdx.x; j < (int)len; j += 64) {
        const uint32_t from = start + sp[os_pad(j)];
        __builtin_nontemporal_store(s[os_pad(j)], as_global_mut<uint64_t>(a.keys_out) + start + j);
        __builtin_nontemporal_store(a.idx_in ? as_global<uint32_t>(a.idx_in)[from] : from, as_global_mut<uint32_t>(a.idx_out) + start + j);
    }
}
__global__ __launch_bounds__(64) void os_local_kernel(const OsLocalArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t s[];
    const int64_t bucket = blockIdx.x;
    const uint32_t start = a.bstart[bucket], len = a.bstart[bucket + 1] - start;
    if (len <= a.len_lo || len > a.len_hi) return;
    if (len == 1) {
        if (threadIdx.x == 0) {
            as_global_mut<uint64_t>(a.keys_out)[start] = as_global<uint64_t>(a.keys_in)[start];
            as_global_mut<uint32_t>(a.idx_out)[start] = a.idx_in ? as_global<uint32_t>(a.idx_in)[start] : start;
        }
        return;
    }
    int P = 2, plog = 1;
    while (P < (int)len) { P <<= 1; ++plog; }
    const uint64_t low = (1ull << a.rbits) - 1;
    for (int i = threadIdx.x; i < P; i += 64) {
        uint64_t w = ~0ull;
        if (i < (int)len) w = (((__builtin_nontemporal_load(as_global<uint64_t>(a.keys_in) + start + i) - a.bias) & low) << 12) | (uint64_t)i;
        s[os_pad(i)] = w;
    }
    __syncthreads();
    for (int ks = 1; ks <= plog; ++ks) {
        for (int jlog = ks - 1; jlog >= 0;) {
            const int mb = jlog + 1 < 4 ? jlog + 1 : 4;
            const int jl_log = jlog - mb + 1;
            switch (mb) {
                case 4: os_chunk<4>(s, P, 1 << ks, jl_log); break;
                case 3: os_chunk<3>(s, P, 1 << ks, jl_log); break;
                case 2: os_chunk<2>(s, P, 1 << ks, jl_log); break;
                default: os_chunk<1>(s, P, 1 << ks, jl_log); break;
            }
            __syncthreads();   // one wave: orders the LDS traffic for the compiler, costs nothing
            jlog = jl_log - 1;
        }
    }
    const uint64_t top = (uint64_t)bucket << a.rbits;
    for (int j = threadIdx.x; j < (int)len; j += 64) {
        const uint64_t w = s[os_pad(j)];
        const uint32_t from = start + (uint32_t)(w & 4095);
        __builtin_nontemporal_store((top | (w >> 12)) + a.bias, as_global_mut<uint64_t>(a.keys_out) + start + j);
        __builtin_nontemporal_store(a.idx_in ? as_global<uint32_t>(a.idx_in)[from] : from, as_global_mut<uint32_t>(a.idx_out) + start + j);
    }
}
// A sample of the keys for the host's bucket plan (value range without the outliers, densest region): one key from every stride,
// at a hashed place inside it (a column with a period would alias with fixed places).
__global__ __launch_bounds__(kBlock) void os_sample_kernel(const uint64_t* keys, int64_t n, int64_t stride, int nsamp, uint64_t* out) {
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= nsamp) return;
    uint64_t h = (uint64_t)i * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    int64_t pos = (int64_t)i * stride + (int64_t)(h % (uint64_t)stride);
    if (pos >= n) pos = n - 1;
    out[i] = as_global<uint64_t>(keys)[pos];
}
hipError_t launch_os_sample(const uint64_t* keys, int64_t n, int nsamp, uint64_t* out, hipStream_t s) {
    if (nsamp < 1 || n < 1) return hipSuccess;
    const int64_t stride = n / nsamp > 0 ? n / nsamp : 1;
    hipLaunchKernelGGL(os_sample_kernel, dim3((unsigned)((nsamp + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, keys, n, stride, nsamp, out);
    return hipGetLastError();
}
hipError_t launch_os_bounds(const uint64_t* keys, int64_t n, uint64_t bias, int rbits, int nbuckets, const OsBucket& fb, uint32_t* bstart, unsigned int* maxlen, hipStream_t s) {
    int64_t grid = (n + 1 + kBlock - 1) / kBlock;
    if (grid > eval_grid_limit()) grid = eval_grid_limit();
    hipLaunchKernelGGL(os_bounds_kernel, dim3((unsigned)grid), dim3(kBlock), 0, s, keys, n, bias, rbits, nbuckets, fb, bstart);
    int64_t g2 = ((int64_t)nbuckets + kBlock - 1) / kBlock;
    if (g2 > eval_grid_limit()) g2 = eval_grid_limit();
    hipLaunchKernelGGL(os_bucket_max_kernel, dim3((unsigned)g2), dim3(kBlock), 0, s, bstart, nbuckets, maxlen);
    return hipGetLastError();
}
static hipError_t launch_os_local_class(const OsLocalArgs& a, hipStream_t s);
hipError_t launch_os_local(const OsLocalArgs& a0, hipStream_t s) {
    // the LDS a block asks for decides how many blocks (of one wave) a CU holds: the few buckets beyond 1024 rows (tails,
    // outliers, a crowded value) get launches of their own (classes of <= 512, <= 1024, more rows) instead of setting the LDS
    // size of every bucket's block
    OsLocalArgs a = a0;
    a.len_lo = 0; a.len_hi = 0xFFFFFFFFu;
    if (a0.lds_items <= 512) return launch_os_local_class(a, s);
    a.lds_items = 512; a.len_hi = 512;
    hipError_t e = launch_os_local_class(a, s);
    if (e != hipSuccess) return e;
    if (a0.lds_items > 1024) {
        a.lds_items = 1024; a.len_lo = 512; a.len_hi = 1024;
        e = launch_os_local_class(a, s);
        if (e != hipSuccess) return e;
    }
    a.lds_items = a0.lds_items; a.len_lo = a0.lds_items > 1024 ? 1024 : 512; a.len_hi = 0xFFFFFFFFu;
    return launch_os_local_class(a, s);
}
static hipError_t launch_os_local_class(const OsLocalArgs& a, hipStream_t s) {
    const size_t words = (size_t)(a.lds_items + a.lds_items / 16 + 1);
    if (a.wide) {
        (void)hipFuncSetAttribute((const void*)os_local_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(words * 12 + 16));
        hipLaunchKernelGGL(os_local_wide_kernel, dim3((unsigned)a.nbuckets), dim3(64), words * 12 + 16, s, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(os_local_kernel, dim3((unsigned)a.nbuckets), dim3(64), words * 8, s, a);
    return hipGetLastError();
}

}  // namespace rdfk
