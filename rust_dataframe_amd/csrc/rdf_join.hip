// rdf_join.hip — the kernels of the equi-join (calc_equijoin_indices, src/functions/join.rs:19-137; host side: rdf_capi_join.inc).
// The reference hashes byte-encoded keys into HashMap<Vec<u8>, Vec<usize>> row lists; here the build side is radix-sorted (the
// sort kernels of rdf_sort.hip), every probe row finds the range of its partners among the sorted rows, and the pairs are written
// at offsets from an exclusive scan of the per-row match counts.  NULL keys never match.
//   join_combine_kernel      2..4 key columns: one 64-bit hash per row over the columns' key bits (join_verify compares the tuples)
//   join_place_kernel, join_place_scan_kernel, join_distinct_kernel
//                            one key column: the table of the distinct build keys, laid out by a scan (rdf_join_place.h)
//   join_buckets_kernel      every other join, and a table whose placement overflowed: the bucket index over the sorted build keys
//   join_count_kernel -> (launch_scan) -> join_write_kernel, join_append_kernel (FULL: the build rows nobody matched)
#include "rdf_common.hip.h"
#include "rdf_hash.h"
#include "rdf_join_place.h"

namespace rdfk {

// multi-column join keys: one 64-bit hash per row over the columns' order-preserving key bits (SplitMix64 finaliser per
// column, chained); rows with a NULL in any key column keep hash 0 and are excluded through nullflags
// (kJoinMul, join_mix and the chain over the columns: rdf_hash.h)
__global__ __launch_bounds__(kBlock) void join_combine_kernel(const JoinCombineArgs a) {
    uint64_t kmin = ~0ull, kmax = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
        const bool isnull = a.nullflags && a.nullflags[i];
        uint64_t h = kJoinSeed;
        for (int k = 0; k < a.nkeys; ++k) h = join_tuple_step(h, a.bits[k][i], k);
        if (isnull) h = 0;
        a.out[i] = h;
        if (!isnull) { kmin = h < kmin ? h : kmin; kmax = h > kmax ? h : kmax; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t x = shfl_xor64(kmin, m), y = shfl_xor64(kmax, m);
        kmin = x < kmin ? x : kmin; kmax = y > kmax ? y : kmax;
    }
    if ((threadIdx.x & 63) == 0) { atomicMin((unsigned long long*)&a.bit_stats[0], (unsigned long long)kmin); atomicMax((unsigned long long*)&a.bit_stats[1], (unsigned long long)kmax); }
}
__device__ __forceinline__ bool join_verify(const JoinProbeArgs& a, int64_t i, int64_t p) {   // hash match -> compare the key tuples
    const uint32_t r = a.ridx[p];
    bool eq = true;
    for (int k = 0; k < a.nkeys; ++k) eq = eq && a.pbits[k][i] == a.bbits[k][r];
    return eq;
}
__global__ __launch_bounds__(kBlock) void join_buckets_kernel(const JoinBucketArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.nrv; i += (int64_t)gridDim.x * kBlock) {
        const uint64_t b = (a.rkeys[i] - a.kmin) >> a.bucket_shift;
        if (i == 0 || ((a.rkeys[i - 1] - a.kmin) >> a.bucket_shift) != b) a.buckets[2 * b] = (uint32_t)i;
        if (i == a.nrv - 1 || ((a.rkeys[i + 1] - a.kmin) >> a.bucket_shift) != b) a.buckets[2 * b + 1] = (uint32_t)(i + 1);
    }
}
typedef uint64_t join_u64x2 __attribute__((ext_vector_type(2)));
// exclusive prefix of v over the block's threads (NT threads); total in *total
template <int NT>
__device__ __forceinline__ PlaceCM place_block_scan(PlaceCM v, PlaceCM* total) {
    __shared__ PlaceCM wtot[NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    PlaceCM inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        PlaceCM o; o.c = __shfl_up(inc.c, d); o.m = __shfl_up(inc.m, d);
        if (lane >= d) inc = place_join(o, inc);
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    PlaceCM ex; ex.c = __shfl_up(inc.c, 1); ex.m = __shfl_up(inc.m, 1);
    if (lane == 0) ex = place_empty();
    PlaceCM wp = place_empty();
    for (int w = 0; w < wave; ++w) wp = place_join(wp, wtot[w]);
    if (total) { PlaceCM t = wp; for (int w = wave; w < NT / 64; ++w) t = place_join(t, wtot[w]); *total = t; }
    __syncthreads();
    return place_join(wp, ex);
}
__global__ __launch_bounds__(1024) void join_place_scan_kernel(const JoinPlaceArgs a) {     // phase 1: one block
    const int64_t per = (a.ntiles + 1023) / 1024;
    const int64_t t0 = (int64_t)threadIdx.x * per, t1 = t0 + per < a.ntiles ? t0 + per : a.ntiles;
    PlaceCM acc = place_empty();
    for (int64_t t = t0; t < t1; ++t) { PlaceCM v; v.c = a.tiles[2 * t]; v.m = a.tiles[2 * t + 1]; acc = place_join(acc, v); }
    PlaceCM run = place_block_scan<1024>(acc, nullptr);
    for (int64_t t = t0; t < t1; ++t) {
        PlaceCM v; v.c = a.tiles[2 * t]; v.m = a.tiles[2 * t + 1];
        a.tiles[2 * t] = run.c; a.tiles[2 * t + 1] = run.m;
        run = place_join(run, v);
    }
}
__global__ __launch_bounds__(kBlock) void join_place_kernel(const JoinPlaceArgs a) {         // phases 0 and 2: one tile per block
    constexpr int kPer = kJoinPlaceTile / kBlock;                 // consecutive sorted rows per thread while the positions are computed
    constexpr int kPad = kJoinPlaceTile + kJoinPlaceTile / kPer + 1;     // one word of padding per thread's run: conflict-free in both access orders
    __shared__ uint64_t sk[kPad];
    __shared__ uint32_t spos[kPad], sgap[kPad];
    const int64_t base = (int64_t)blockIdx.x * kJoinPlaceTile;
    const int n = (int)(a.nrv - base < kJoinPlaceTile ? a.nrv - base : kJoinPlaceTile);
    for (int e = threadIdx.x; e < n; e += kBlock) sk[e + e / kPer] = a.rkeys[base + e];
    __syncthreads();
    const int e0 = threadIdx.x * kPer;
    const uint64_t before = e0 == 0 ? (base > 0 ? a.rkeys[base - 1] : 0) : sk[(e0 - 1) + (e0 - 1) / kPer];
    const bool no_prev = e0 == 0 && base == 0;
    uint64_t prev = before;
    PlaceCM loc = place_empty();
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int e = e0 + j;
        if (e >= n) break;
        const uint64_t h = sk[e + e / kPer];
        if ((j == 0 && no_prev) || h != prev) (void)place_push(loc, (long long)(h >> a.tshift));
        prev = h;
    }
    PlaceCM total;
    const PlaceCM ex = place_block_scan<kBlock>(loc, &total);
    if (a.phase == 0) {
        if (threadIdx.x == 0) { a.tiles[2 * blockIdx.x] = total.c; a.tiles[2 * blockIdx.x + 1] = total.m; }
        return;
    }
    PlaceCM carry; carry.c = a.tiles[2 * blockIdx.x]; carry.m = a.tiles[2 * blockIdx.x + 1];
    // this tile owns the slots from the one behind the previous tiles' last key up to its own last key (the last tile: up to the end):
    // it writes the empty ones too, so nobody clears the table beforehand and every line leaves whole
    const long long p0 = place_last(carry) + 1;
    PlaceCM run = place_join(carry, ex);        // {distinct keys before this thread's rows, max(home - index) over them}: absolute
    long long last = place_last(run);                          // slot of the distinct key before this thread's rows
    prev = before;
    bool too_far = false;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int e = e0 + j;
        if (e >= n) break;
        const uint64_t h = sk[e + e / kPer];
        uint32_t off = ~0u, gap = 0;
        if ((j == 0 && no_prev) || h != prev) {
            const long long pos = place_push(run, (long long)(h >> a.tshift));
            if (pos + 1 >= a.cap || pos - p0 >= 0xFFFFFFFFll) too_far = true;       // (the slot behind the last key stays empty: probes end there)
            else { off = (uint32_t)(pos - p0); gap = (uint32_t)(pos - last - 1); }
            last = pos;
        }
        spos[e + e / kPer] = off;
        sgap[e + e / kPer] = gap;
        prev = h;
    }
    if (too_far) atomicOr(a.flags, 1ull);
    __syncthreads();
    // consecutive lanes now take consecutive rows: their slots are neighbours, the stores of a wave fall into a few lines
    const join_u64x2 zero = {0, 0};
    for (int e = threadIdx.x; e < n; e += kBlock) {
        const uint32_t off = spos[e + e / kPer];
        if (off == ~0u) continue;
        const uint64_t h = sk[e + e / kPer];
        const long long pos = p0 + off;
        // the end of the run of equal keys that starts here: galloping, then a binary search (one lane walking a hot key's
        // millions of duplicates one dependent load at a time would hold its wave for as long)
        const int64_t i = base + e;
        int64_t jn = i + 1;
        if (jn < a.nrv && (e + 1 < n ? sk[(e + 1) + (e + 1) / kPer] : a.rkeys[jn]) == h) {
            int64_t step = 2;
            while (i + step < a.nrv && a.rkeys[i + step] == h) step <<= 1;
            int64_t l = i + (step >> 1), hh = i + step < a.nrv ? i + step : a.nrv;     // rkeys[l] == h; rkeys[hh] != h or hh == nrv
            while (l + 1 < hh) { const int64_t mid = l + ((hh - l) >> 1); if (a.rkeys[mid] == h) l = mid; else hh = mid; }
            jn = hh;
        }
        const uint32_t info = jn - i == 1 ? (0x80000000u | a.ridx[i]) : (uint32_t)(jn - i);
        join_u64x2 w; w[0] = h; w[1] = ((unsigned long long)i << 32) | info;
        *(join_u64x2*)(a.table + 2 * pos) = w;
        for (uint32_t g = 1, gap = sgap[e + e / kPer]; g <= gap; ++g) *(join_u64x2*)(a.table + 2 * (pos - g)) = zero;
    }
    if (blockIdx.x == gridDim.x - 1) {          // the slots behind the last key: empty up to the end of the table
        const long long end_of_keys = place_last(place_join(carry, total)) + 1;
        for (long long q = end_of_keys + threadIdx.x; q < a.cap; q += kBlock) *(join_u64x2*)(a.table + 2 * q) = zero;
    }
}
// sorted build positions [lo, hi) whose key equals probe row i's key; direct = the build row itself when the key occurs once (table path)
__device__ __forceinline__ void join_range(const JoinProbeArgs& a, int64_t i, int64_t& lo, int64_t& hi, uint32_t& direct) {
    lo = hi = 0;
    direct = 0;
    if (a.lnull && a.lnull[i]) return;
    const uint64_t k = a.lkeys[i];
    if (k < a.kmin || k > a.kmax) return;
    if (a.table) {
        const uint64_t want = k * kJoinMul;
        uint64_t s = want >> a.tshift;
        for (;;) {
            const join_u64x2 e = *(const join_u64x2*)(a.table + 2 * s);
            if (e[1] == 0) return;
            if (e[0] > want) return;     // the table holds its keys in hash order: a larger one ends the search
            if (e[0] == want) {
                const uint32_t info = (uint32_t)e[1];
                lo = (int64_t)(e[1] >> 32);
                if (info >> 31) { hi = lo + 1; direct = info; } else hi = lo + info;
                return;
            }
            s = s + 1;                   // no wrap-around: the last home slot's cluster ends inside the table's margin
        }
    }
    const uint64_t b = (k - a.kmin) >> a.bucket_shift;
    const uint2 se = *(const uint2*)(a.buckets + 2 * b);
    int64_t l = se.x, h = se.y;
    const int64_t e = h;
    while (l < h) { const int64_t m = (l + h) >> 1; if (a.rkeys[m] < k) l = m + 1; else h = m; }
    lo = l;
    h = e;
    while (l < h) { const int64_t m = (l + h) >> 1; if (a.rkeys[m] <= k) l = m + 1; else h = m; }
    hi = l;
}
__global__ __launch_bounds__(kBlock) void join_count_kernel(const JoinProbeArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.nl; i += (int64_t)gridDim.x * kBlock) {
        int64_t lo, hi;
        uint32_t direct;
        join_range(a, i, lo, hi, direct);
        int64_t c = hi - lo;
        if (a.nkeys > 1) {   // candidates share the tuple's hash: count (and mark) only the ones whose key tuples are equal
            c = 0;
            for (int64_t p = lo; p < hi; ++p)
                if (join_verify(a, i, p)) { ++c; if (a.matched) atomicOr(&a.matched[p >> 5], 1u << (p & 31)); }
        } else if (a.matched) for (int64_t p = lo; p < hi; ++p) atomicOr(&a.matched[p >> 5], 1u << (p & 31));
        a.counts[i] = (c == 0 && a.outer) ? 1 : c;
        a.first[i] = c == 0 ? ~0u : direct ? direct : (uint32_t)lo;   // the write phase does not search again (bit 31: not a position but the one build row itself)
        if (c == 0 && a.outer) atomicAdd(a.unmatched, 1ull);
    }
}
__global__ __launch_bounds__(kBlock) void join_write_kernel(const JoinProbeArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.nl; i += (int64_t)gridDim.x * kBlock) {
        int64_t o = a.offsets[i];
        const int64_t cnt = a.offsets[i + 1] - o;
        const uint32_t lo = a.first[i];
        if (lo == ~0u) {
            if (a.outer) {
                a.out_probe[o] = (uint32_t)i;
                a.out_build[o] = 0;
                atomicAnd(&a.out_build_validity[o >> 5], ~(1u << (o & 31)));
            }
            continue;
        }
        if (a.table && (lo >> 31)) {   // a key that occurs once on the build side: its row came with the table entry
            a.out_probe[o] = (uint32_t)i;
            a.out_build[o] = lo & 0x7FFFFFFFu;
            continue;
        }
        if (a.nkeys > 1) {   // walk the hash range again and emit the verified pairs (cnt of them, in sorted-position order)
            int64_t left = cnt;
            for (int64_t p = lo; left > 0; ++p)
                if (join_verify(a, i, p)) { a.out_probe[o] = (uint32_t)i; a.out_build[o] = a.ridx[p]; ++o; --left; }
            continue;
        }
        for (int64_t p = lo; p < (int64_t)lo + cnt; ++p, ++o) {
            a.out_probe[o] = (uint32_t)i;
            a.out_build[o] = a.ridx[p];
        }
    }
}
__global__ __launch_bounds__(kBlock) void join_append_kernel(const JoinAppendArgs a) {
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < a.nr; p += (int64_t)gridDim.x * kBlock) {
        const bool un = p >= a.nrv || !((a.matched[p >> 5] >> (p & 31)) & 1);
        if (!un) continue;
        const unsigned long long o = atomicAdd(a.cursor, 1ull);
        if (a.count_only) continue;
        a.out_probe[o] = 0;
        a.out_build[o] = a.ridx[p];
        atomicAnd(&a.out_probe_validity[o >> 5], ~(1u << (o & 31)));
    }
}
// distinct values of a SORTED key array (equal keys are neighbours): rows whose key differs from the row in front of them
__global__ __launch_bounds__(kBlock) void join_distinct_kernel(const uint64_t* keys, int64_t n, unsigned long long* out) {
    __shared__ unsigned int part[kBlock / 64];
    unsigned int mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const uint64_t k = __builtin_nontemporal_load(as_global<uint64_t>(keys) + i);
        const uint64_t p = i > 0 ? as_global<uint64_t>(keys)[i - 1] : ~k;
        mine += k != p ? 1u : 0u;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine += (unsigned int)__shfl_xor((int)mine, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += part[w];
        if (t) atomicAdd(out, t);
    }
}

static int join_rows_grid(int64_t n) {
    int64_t g = (n + kBlock - 1) / kBlock;
    if (g > eval_grid_limit()) g = eval_grid_limit();
    return g < 1 ? 1 : (int)g;
}
hipError_t launch_join_buckets(const JoinBucketArgs& a, hipStream_t s) {
    if (a.nrv > 0) hipLaunchKernelGGL(join_buckets_kernel, dim3(join_rows_grid(a.nrv)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_join_distinct(const uint64_t* keys, int64_t n, unsigned long long* out, hipStream_t s) {     // *out zeroed by the caller
    if (n > 0) hipLaunchKernelGGL(join_distinct_kernel, dim3(join_rows_grid(n)), dim3(kBlock), 0, s, keys, n, out);
    return hipGetLastError();
}
hipError_t launch_join_place(JoinPlaceArgs a, hipStream_t s) {
    if (a.nrv <= 0) return hipSuccess;
    a.phase = 0;
    hipLaunchKernelGGL(join_place_kernel, dim3((unsigned)a.ntiles), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(join_place_scan_kernel, dim3(1), dim3(1024), 0, s, a);
    a.phase = 2;
    hipLaunchKernelGGL(join_place_kernel, dim3((unsigned)a.ntiles), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_join_combine(const JoinCombineArgs& a, hipStream_t s) {
    if (a.n > 0) hipLaunchKernelGGL(join_combine_kernel, dim3(join_rows_grid(a.n)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_join_count(const JoinProbeArgs& a, hipStream_t s) {
    if (a.nl > 0) hipLaunchKernelGGL(join_count_kernel, dim3(join_rows_grid(a.nl)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_join_write(const JoinProbeArgs& a, hipStream_t s) {
    if (a.nl > 0) hipLaunchKernelGGL(join_write_kernel, dim3(join_rows_grid(a.nl)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_join_append(const JoinAppendArgs& a, hipStream_t s) {
    if (a.nr > 0) hipLaunchKernelGGL(join_append_kernel, dim3(join_rows_grid(a.nr)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace rdfk
