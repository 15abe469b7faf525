// rdf_collect.hip — the kernels of collect_list / collect_set per group and of explode (host side: rdf_capi_collect.inc,
// argument blocks: rdf_collect.h).
//
// COLLECT.  The window front has sorted the rows by the grouping keys (LIST: the stable sort leaves every group in row
// order; the items are the n sorted positions) or by (grouping keys, value) (SET: the items are the D heads, one per
// distinct (group, value) pair, each the smallest row of its pair).  An item is LIVE when the value at its row is not NULL.
// The result is the compaction of the live items, cut where a group starts:
//   count   one live count per fixed tile of kCollectTile items                    (skipped when no value chunk has validity)
//   (scan)  launch_scan over the tile counts                                       (skipped likewise)
//   emit    a tile recomputes its flags and ranks its live items — a ballot and a popcount inside every 64-item run, the
//           runs' totals through LDS — then writes child_rows[base + rank] and the gathered value; an item that starts a
//           group writes offsets[g] = base + (live items before it), NULL items included, so a group without a live item
//           gets an empty list by construction; the last item writes offsets[G].
// Every item is read once by one thread whatever the group boundaries: one group, one group per row, or all live items in
// one tile cost the same.  No atomics: every output word has one writer, fixed by (the item list, the validity).
//
// EXPLODE is driven by the output: count per list row, launch_scan, then a tile of kCollectTile OUTPUT rows finds its range
// of list rows by two binary searches over start[], stages that range in LDS when it holds at most kExplodeWindow rows, and
// every output row j takes as parent the LARGEST r with start[r] <= j — a row without output shares its start with the next
// one and is stepped over by that rule.  A range beyond the window (thousands of empty rows inside one tile) is searched
// in global memory.  O(rows + outputs) whatever the lengths.  (The one atomic is the integer count of NULL outputs.)
#include "rdf_collect.h"
#include "rdf_common.hip.h"

using namespace rdfk;

namespace {

struct ColItem { uint32_t row, group; bool starts; };

__device__ __forceinline__ ColItem col_item(const CollectArgs& a, int64_t i) {
    const int64_t j = a.gstart ? (int64_t)a.gstart[i] : i;
    ColItem it;
    it.row = a.perm ? a.perm[j] : (uint32_t)j;
    if (a.scan) {
        const uint64_t ex = (uint64_t)a.scan[j], inc = (uint64_t)a.scan[j + 1];
        it.starts = (inc >> 32) != (ex >> 32);
        it.group = (uint32_t)(inc >> 32) - 1;
    } else {
        it.starts = i == 0;
        it.group = 0;
    }
    return it;
}

// Is the value of `row` not NULL; *values / *e: where it lies (numeric chunks).
__device__ __forceinline__ bool col_live(const CollectArgs& a, double inv, int64_t row, const void** values, int64_t* e) {
    int64_t c = 0, start = 0;
    if (a.nchunks > 1) { c = find_chunk_row(a.row_start, a.nchunks, row, inv); start = a.row_start[c]; }
    if (a.vutf8) {
        const Utf8Chunk& u = a.vutf8[c];
        const int64_t b = u.valid_off + row - start;
        *values = nullptr;
        *e = 0;
        return u.valid ? ((u.valid[b >> 3] >> (b & 7)) & 1) != 0 : true;
    }
    const DevChunkCol cc = a.vchunks[c];
    *values = cc.values;
    *e = cc.offset + row - start;
    return cc.validity ? ((cc.validity[*e >> 3] >> (*e & 7)) & 1) != 0 : true;
}

__device__ __forceinline__ void col_store_value(const CollectArgs& a, const void* values, int64_t e, int64_t at) {
    switch (a.esize) {
        case 1: as_global_mut<uint8_t>(a.values)[at] = as_global<uint8_t>(values)[e]; break;
        case 2: as_global_mut<uint16_t>(a.values)[at] = as_global<uint16_t>(values)[e]; break;
        case 4: {
            uint32_t b = as_global<uint32_t>(values)[e];
            if (a.canon == 4) b = (b & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000u : (b == 0x80000000u ? 0u : b);
            as_global_mut<uint32_t>(a.values)[at] = b;
            break;
        }
        default: {
            uint64_t b = as_global<uint64_t>(values)[e];
            if (a.canon == 8) b = (b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull ? 0x7FF8000000000000ull : (b == 0x8000000000000000ull ? 0ull : b);
            as_global_mut<uint64_t>(a.values)[at] = b;
        }
    }
}

__global__ __launch_bounds__(kCollectThreads) void collect_count_kernel(const CollectArgs a) {
    __shared__ int wcnt[kCollectThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inv = chunk_lookup_scale(a.row_start, a.nchunks);
    const int64_t ntiles = collect_tiles(a.m);
    const int64_t m = a.m_dev ? (int64_t)(uint32_t)(uint64_t)*a.m_dev : a.m;   // (<= a.m: the heads are at most the rows)
    if (blockIdx.x == 0 && tid == 0 && a.front_total_out) *a.front_total_out = a.front_total ? *a.front_total : 0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < kCollectPer; ++k) {
            const int64_t i = tile * kCollectTile + k * kCollectThreads + tid;
            bool live = false;
            if (i < m && i < a.m) {
                const int64_t j = a.gstart ? (int64_t)a.gstart[i] : i;
                const void* vp;
                int64_t e;
                live = col_live(a, inv, a.perm ? (int64_t)a.perm[j] : j, &vp, &e);
            }
            cnt += __popcll(__ballot(live));               // (wave-uniform)
        }
        if (lane == 0) wcnt[wave] = cnt;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < kCollectThreads / 64; ++w) t += wcnt[w];
            a.tile_counts[tile] = t;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kCollectThreads) void collect_emit_kernel(const CollectArgs a) {
    __shared__ int segcnt[kCollectSegs];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inv = chunk_lookup_scale(a.row_start, a.nchunks);
    const int64_t ntiles = collect_tiles(a.m);
    const bool locate = a.nullable || a.values;            // the value's place is needed for its validity or its bits
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = a.tile_base ? a.tile_base[tile] : tile * kCollectTile;
        ColItem it[kCollectPer];
        const void* vp[kCollectPer];
        int64_t ve[kCollectPer];
        bool live[kCollectPer];
        int lrank[kCollectPer];
#pragma unroll
        for (int k = 0; k < kCollectPer; ++k) {
            const int64_t i = tile * kCollectTile + k * kCollectThreads + tid;
            live[k] = false;
            vp[k] = nullptr;
            ve[k] = 0;
            it[k] = ColItem{0, 0, false};
            if (i < a.m) {
                it[k] = col_item(a, i);
                live[k] = locate ? col_live(a, inv, (int64_t)it[k].row, &vp[k], &ve[k]) : true;
            }
            const unsigned long long b = __ballot(live[k]);
            lrank[k] = __popcll(b & ((1ull << lane) - 1));
            if (lane == 0) segcnt[k * (kCollectThreads / 64) + wave] = __popcll(b);
        }
        __syncthreads();
        int before = 0, sb[kCollectPer] = {};              // live items of the runs in front of this thread's run k
#pragma unroll
        for (int sgm = 0; sgm < kCollectSegs; ++sgm) {
#pragma unroll
            for (int k = 0; k < kCollectPer; ++k)
                if (sgm == k * (kCollectThreads / 64) + wave) sb[k] = before;
            before += segcnt[sgm];
        }
#pragma unroll
        for (int k = 0; k < kCollectPer; ++k) {
            const int64_t i = tile * kCollectTile + k * kCollectThreads + tid;
            if (i >= a.m) continue;
            const int64_t at = base + sb[k] + lrank[k];    // live items in front of item i
            if (live[k]) {
                if (a.child_rows) a.child_rows[at] = it[k].row;
                if (a.values) col_store_value(a, vp[k], ve[k], at);
            }
            if (it[k].starts && (int64_t)it[k].group < a.groups) {
                if (a.offsets) a.offsets[it[k].group] = (int32_t)at;
                if (a.group_rows) a.group_rows[it[k].group] = it[k].row;
            }
            if (i == a.m - 1 && a.offsets) a.offsets[a.groups] = (int32_t)(at + (live[k] ? 1 : 0));
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- explode

__device__ __forceinline__ bool exp_row(const ExplodeArgs& a, int64_t r, int32_t* first, int32_t* len) {
    const GlobalPtr<int32_t> offs = as_global<int32_t>(a.offsets.values) + a.offsets.offset;
    const int32_t b = offs[r], e = offs[r + 1];
    const int64_t bit = a.offsets.offset + r;
    const bool valid = a.offsets.validity ? ((a.offsets.validity[bit >> 3] >> (bit & 7)) & 1) != 0 : true;
    *first = b;
    *len = e > b ? e - b : 0;
    return valid && e > b;                                 // the row carries elements
}

__global__ __launch_bounds__(kCollectThreads) void explode_count_kernel(const ExplodeArgs a) {
    for (int64_t r = (int64_t)blockIdx.x * kCollectThreads + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * kCollectThreads) {
        int32_t first, len;
        const bool has = exp_row(a, r, &first, &len);
        a.counts[r] = has ? (int64_t)len : (a.outer ? 1 : 0);
    }
}

// largest x in [0, cnt) with s[x] <= j; s[0] <= j is given
template <class P> __device__ __forceinline__ int64_t exp_search(P s, int64_t cnt, int64_t j) {
    int64_t lo = 0, hi = cnt;                              // s[lo] <= j < s[hi] (s[cnt] = +inf)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (s[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kCollectThreads) void explode_expand_kernel(const ExplodeArgs a) {
    __shared__ int64_t win[kExplodeWindow];
    __shared__ int64_t ends[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t ntiles = collect_tiles(a.rows);
    unsigned int nulls = 0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t j0 = tile * kCollectTile, j1 = a.rows - j0 < kCollectTile ? a.rows : j0 + kCollectTile;
        if (tid < 2) ends[tid] = exp_search(a.start, a.n, tid == 0 ? j0 : j1 - 1);
        __syncthreads();
        const int64_t r_lo = ends[0], cnt = ends[1] - ends[0] + 1;
        const bool staged = cnt <= kExplodeWindow;
        if (staged)
            for (int64_t x = tid; x < cnt; x += kCollectThreads) win[x] = a.start[r_lo + x];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kCollectPer; ++k) {
            const int64_t j = j0 + k * kCollectThreads + tid;
            bool null_out = false;
            if (j < j1) {
                const int64_t x = staged ? exp_search((const int64_t*)win, cnt, j) : exp_search(a.start + r_lo, cnt, j);
                const int64_t r = r_lo + x, kk = j - (staged ? win[x] : a.start[r]);
                int32_t first, len;
                const bool has = exp_row(a, r, &first, &len);
                null_out = !has;
                if (a.parent_rows) a.parent_rows[j] = (uint32_t)r;
                if (a.child_index) a.child_index[j] = has ? (uint32_t)(first + (int32_t)kk) : 0u;
                if (a.pos) a.pos[j] = has ? (int32_t)kk : 0;
                if (a.vbytes) a.vbytes[j] = has ? 1 : 0;
            }
            nulls += null_out ? 1u : 0u;
        }
        __syncthreads();
    }
    if (a.nulls) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) nulls += (unsigned int)__shfl_xor((int)nulls, m);
        if (lane == 0 && nulls) atomicAdd(a.nulls, (unsigned long long)nulls);
    }
}

int collect_grid(int64_t blocks) {
    const int64_t lim = (int64_t)eval_grid_limit();
    return (int)(blocks < 1 ? 1 : (blocks > lim ? lim : blocks));
}

}  // namespace

hipError_t launch_collect_count(const CollectArgs& a, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(collect_count_kernel, dim3(collect_grid(collect_tiles(a.m))), dim3(kCollectThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_collect_emit(const CollectArgs& a, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(collect_emit_kernel, dim3(collect_grid(collect_tiles(a.m))), dim3(kCollectThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_explode_count(const ExplodeArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(explode_count_kernel, dim3(collect_grid((a.n + kCollectThreads - 1) / kCollectThreads)), dim3(kCollectThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_explode_expand(const ExplodeArgs& a, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(explode_expand_kernel, dim3(collect_grid(collect_tiles(a.rows))), dim3(kCollectThreads), 0, s, a);
    return hipGetLastError();
}
