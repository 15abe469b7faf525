// rdf_group_sorted.hip — the fold of the sorted GROUP BY (count_distinct, sum_distinct, first, last per group; host side:
// rdf_capi_group_sorted.inc, argument blocks: rdf_group_sorted.h).
//
// The window front has ordered the rows by (grouping keys, value): a group is a partition, a distinct (group, value) pair
// is a peer group, and gstart[h] is the first sorted position of pair h — its HEAD.  Ties keep ascending row order, so
// perm[gstart[h]] / perm[gstart[h + 1] - 1] are the smallest / largest row of pair h, and NULL values sort last in their
// partition, so a group's NULL run is its last pair or absent.  Everything asked per group is therefore a reduction over
// the group's heads, D of them in G groups, never over the n rows.
//
// The fold is a segmented reduction whose time does not depend on where the segment boundaries fall:
//   - the item list is walked in fixed tiles of kGrpTile items, one per thread; the segment of an item is its group;
//   - inside a tile: a segmented inclusive scan by lane shuffles, then the waves' tails joined in wave order through LDS;
//     the last item of every segment holds the segment's value over the tile;
//   - a segment that neither is the tile's first nor its last is complete and is written straight to the outputs;
//   - the tile's first and last segment go to part[tile][0 / 1] (a tile of one segment fills [1] with the neutral state),
//     and that table, 2 * tiles items whose segments are again ascending, is the item list of the next level;
//   - the level that fits one tile writes everything.  5e7 heads take four launches: 5e7 -> 390626 -> 3052 -> 24.
// Which states are joined, and in which order, is fixed by (D, G, the segment boundaries) alone: no atomics on values, no
// dependence on the grid, the dispatch order or the memory kind, so equal inputs give equal bytes — Float64 sums included.
// (The one atomic is an integer count of NULL results.)  Float32 values are widened to double before they are added.
#include "rdf_group_sorted.h"
#include "rdf_common.hip.h"

using namespace rdfk;

namespace {

__device__ __forceinline__ GrpState grp_neutral(uint32_t seg) {
    GrpState s;
    s.sum = 0;          // +0.0 as a double: x + 0.0 == x for every x the fold meets (zeros enter as +0.0)
    s.cnt = 0;
    s.lo_all = kGrpNone; s.hi_all = 0;
    s.lo_val = kGrpNone; s.hi_val = 0;
    s.seg = seg;
    return s;
}

// l lies before r in the item list; both belong to r.seg
__device__ __forceinline__ GrpState grp_join(const GrpState& l, const GrpState& r, bool isf) {
    GrpState s;
    s.sum = isf ? (uint64_t)__double_as_longlong(__longlong_as_double((long long)l.sum) + __longlong_as_double((long long)r.sum)) : l.sum + r.sum;
    s.cnt = l.cnt + r.cnt;
    s.lo_all = l.lo_all < r.lo_all ? l.lo_all : r.lo_all;
    s.hi_all = l.hi_all > r.hi_all ? l.hi_all : r.hi_all;
    s.lo_val = l.lo_val < r.lo_val ? l.lo_val : r.lo_val;
    s.hi_val = l.hi_val > r.hi_val ? l.hi_val : r.hi_val;
    s.seg = r.seg;
    return s;
}

__device__ __forceinline__ GrpState grp_shfl_up(const GrpState& v, int d) {
    GrpState o;
    o.sum = ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(v.sum >> 32), d) << 32) | (uint32_t)__shfl_up((int)(uint32_t)v.sum, d);
    o.cnt = (uint32_t)__shfl_up((int)v.cnt, d);
    o.lo_all = (uint32_t)__shfl_up((int)v.lo_all, d);
    o.hi_all = (uint32_t)__shfl_up((int)v.hi_all, d);
    o.lo_val = (uint32_t)__shfl_up((int)v.lo_val, d);
    o.hi_val = (uint32_t)__shfl_up((int)v.hi_val, d);
    o.seg = (uint32_t)__shfl_up((int)v.seg, d);
    return o;
}

// The value of `row`: is it NULL, and what it adds to a sum (a double's bits, zeros as +0.0, or a 64-bit integer).
__device__ __forceinline__ uint64_t grp_value(const GrpFoldArgs& a, double inv, int64_t row, bool* isnull) {
    int64_t c = 0, start = 0;
    if (a.nchunks > 1) { c = find_chunk_row(a.row_start, a.nchunks, row, inv); start = a.row_start[c]; }
    if (a.vutf8) {
        const Utf8Chunk& u = a.vutf8[c];
        const int64_t e = u.valid_off + row - start;
        *isnull = u.valid ? !((u.valid[e >> 3] >> (e & 7)) & 1) : false;
        return 0;
    }
    const DevChunkCol cc = a.vchunks[c];
    const int64_t e = cc.offset + row - start;
    *isnull = cc.validity ? !((cc.validity[e >> 3] >> (e & 7)) & 1) : false;
    if (*isnull) return 0;
    switch (a.vdtype) {
        case RDF_I8: return (uint64_t)(int64_t)as_global<int8_t>(cc.values)[e];
        case RDF_I16: return (uint64_t)(int64_t)as_global<int16_t>(cc.values)[e];
        case RDF_I32: return (uint64_t)(int64_t)as_global<int32_t>(cc.values)[e];
        case RDF_U8: return as_global<uint8_t>(cc.values)[e];
        case RDF_U16: return as_global<uint16_t>(cc.values)[e];
        case RDF_U32: return as_global<uint32_t>(cc.values)[e];
        case RDF_F32: {
            const double d = (double)as_global<float>(cc.values)[e];
            return d == 0.0 ? 0ull : (uint64_t)__double_as_longlong(d);
        }
        case RDF_F64: {
            const double d = as_global<double>(cc.values)[e];
            return d == 0.0 ? 0ull : (uint64_t)__double_as_longlong(d);
        }
        default: return as_global<uint64_t>(cc.values)[e];
    }
}

__device__ __forceinline__ GrpState grp_head(const GrpFoldArgs& a, double inv, int64_t h) {
    const int64_t j0 = a.gstart[h], j1 = (int64_t)a.gstart[h + 1] - 1;
    const uint32_t r0 = a.perm ? a.perm[j0] : (uint32_t)j0, r1 = a.perm ? a.perm[j1] : (uint32_t)j1;
    GrpState s;
    s.seg = (uint32_t)((uint64_t)a.scan[j0 + 1] >> 32) - 1;
    bool isnull = false;
    s.sum = (a.vchunks || a.vutf8) ? grp_value(a, inv, (int64_t)r0, &isnull) : 0;
    s.cnt = isnull ? 0u : 1u;
    s.lo_all = r0;
    s.hi_all = r1;
    s.lo_val = isnull ? kGrpNone : r0;
    s.hi_val = isnull ? 0u : r1 + 1;
    return s;
}

__global__ __launch_bounds__(kGrpThreads) void grp_fold_kernel(const GrpFoldArgs a) {
    __shared__ GrpState wtot[kGrpThreads / 64];
    __shared__ uint32_t sseg[kGrpTile + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool isf = a.vdtype == RDF_F32 || a.vdtype == RDF_F64;
    const bool final_level = a.part == nullptr;
    const double inv = a.level == 0 ? chunk_lookup_scale(a.row_start, a.nchunks) : 0.0;
    const int64_t ntiles = (a.m + kGrpTile - 1) / kGrpTile;
    unsigned int nulls[RDF_GROUP_MAX_CALLS];
#pragma unroll
    for (int c = 0; c < RDF_GROUP_MAX_CALLS; ++c) nulls[c] = 0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = tile * kGrpTile, i = base + tid;
        const bool in = i < a.m;
        GrpState st = grp_neutral(kGrpNone);
        if (in) st = a.level == 0 ? grp_head(a, inv, i) : a.in[i];
        sseg[tid] = st.seg;
        if (tid == 0) sseg[kGrpTile] = kGrpNone;
        // ---- the segment's value up to and including this item: inside the wave, then the tails of the waves before
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const GrpState o = grp_shfl_up(st, d);
            if (lane >= d && o.seg == st.seg) st = grp_join(o, st, isf);
        }
        if (lane == 63) wtot[wave] = st;
        __syncthreads();
        {
            GrpState acc = grp_neutral(st.seg);
            bool any = false;
            for (int w = 0; w < wave; ++w)
                if (wtot[w].seg == st.seg) { acc = any ? grp_join(acc, wtot[w], isf) : wtot[w]; any = true; }
            if (any) st = grp_join(acc, st, isf);
        }
        // ---- the last item of a segment holds its value over the tile
        const int last = (int)((a.m - base < kGrpTile ? a.m - base : kGrpTile) - 1);
        const uint32_t first_seg = sseg[0], last_seg = sseg[last];
        if (in && sseg[tid + 1] != st.seg) {
            if (!final_level && st.seg == first_seg) a.part[tile * 2] = st;
            else if (!final_level && st.seg == last_seg) a.part[tile * 2 + 1] = st;
            else if ((int64_t)st.seg < a.groups) {
                const int64_t g = st.seg;
                if (a.group_rows) a.group_rows[g] = st.lo_all;
#pragma unroll
                for (int c = 0; c < RDF_GROUP_MAX_CALLS; ++c) {
                    if (c >= a.ncalls) break;
                    const GrpCallOut& o = a.calls[c];
                    switch (o.fn) {
                        case RDF_GRP_COUNT_DISTINCT: as_global_mut<int64_t>(o.values)[g] = (int64_t)st.cnt; break;
                        case RDF_GRP_SUM_DISTINCT: as_global_mut<uint64_t>(o.values)[g] = st.sum; break;
                        default: {
                            const bool first = o.fn == RDF_GRP_FIRST;
                            const bool ok = !o.ignore_nulls || st.cnt > 0;
                            uint32_t v = first ? st.lo_all : st.hi_all;
                            if (o.ignore_nulls) v = !ok ? 0u : first ? st.lo_val : st.hi_val - 1;
                            as_global_mut<uint32_t>(o.values)[g] = v;
                            if (o.vbytes) o.vbytes[g] = ok ? 1 : 0;
                            nulls[c] += ok ? 0u : 1u;
                        }
                    }
                }
            }
            if (!final_level && tid == last && st.seg == first_seg) a.part[tile * 2 + 1] = grp_neutral(first_seg);
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < RDF_GROUP_MAX_CALLS; ++c) {
        if (c >= a.ncalls) break;
        if (a.calls[c].fn < RDF_GRP_FIRST || !a.calls[c].ignore_nulls) continue;   // (uniform: the same for every lane)
        unsigned int v = nulls[c];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += (unsigned int)__shfl_xor((int)v, m);
        if (lane == 0 && v) atomicAdd(&a.nulls[c], (unsigned long long)v);
    }
}

}  // namespace

hipError_t launch_grp_fold(const GrpFoldArgs& a, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    const int64_t want = grp_tiles(a.m), lim = (int64_t)eval_grid_limit();
    hipLaunchKernelGGL(grp_fold_kernel, dim3((unsigned)(want > lim ? lim : want)), dim3(kGrpThreads), 0, s, a);
    return hipGetLastError();
}
