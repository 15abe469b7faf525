// rdf_group_moments.hip — the kernels of rdf_groupby_moments: one moment state per group, then the statistics (host side:
// rdf_capi_group_moments.inc, argument blocks: rdf_group_moments.h, the tile step, the merge and the statistic formulas:
// rdf_moments_math.h; the level plan and the piece finish: rdf_group_moments_plan.h).
//
// The window front has ordered the rows by the grouping keys alone: a group is a partition, its rows are neighbours in the
// permutation in ascending row order, and the high word of the front's scan numbers the groups 0, 1, 2 ... along the sorted
// positions.  The value columns took no part in the sort; they are gathered at perm[position].
//
// Level 0 walks the n sorted positions in fixed tiles of kGmTile, one position per thread.  A PIECE is the run of one group
// inside one tile, and every piece is one application of rdf_moments' tile step to at most kGmTile rows:
//   1. a segmented scan of (sum x, count, first counted value, all equal to it) gives the piece's centre at its last item:
//      c = sum x / n, or the common value itself when the counted values are all equal — so a constant group has every
//      d = 0 and M2 = 0 exactly, whatever its size;
//   2. the centres go back to the piece's items through LDS (groups are numbered consecutively, so seg - first_seg < tile);
//   3. d = x - c, ONE rounding relative to d however large c is;
//   4. a segmented scan of the power sums of d (pairs: dx, dy, dx^2, dy^2, dx dy);
//   5. mo_tile_state / mo_cotile_state at the piece's last item.  sum x^2 is never formed.
// A piece that neither is the tile's first nor its last is a whole group and is written at once; the first and the last
// piece go to part[tile][0 / 1] (a tile of one piece fills [1] with the empty state), and that table, 2 * tiles states
// whose groups again ascend, is the item list of the next level.  Levels >= 1 are the same segmented scan over states with
// mo_merge / mo_comerge as the join, in item order, the waves' tails joined in wave order; every level is a launch of its
// own, and the level that fits one tile writes everything that is left.
//
// Which values are added and which states are merged, and in which order, is fixed by (n, the group boundaries) alone: the
// tiles are fixed positions, a block's loop over tiles only deals them out.  No float atomics, no block waits for another,
// nothing depends on the grid, the dispatch order or the memory kind, so equal inputs give equal bytes.  (The one atomic is
// an integer count of NULL results in the finish kernel.)
#include <type_traits>

#include "rdf_group_moments.h"
#include "rdf_common.hip.h"

using namespace rdfk;

namespace {

template <class V>
__device__ __forceinline__ V gm_shfl_up(const V& v, int d) {
    static_assert(sizeof(V) % 4 == 0, "whole words");
    uint32_t w[sizeof(V) / 4];
    __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
    for (size_t k = 0; k < sizeof(V) / 4; ++k) w[k] = (uint32_t)__shfl_up((int)w[k], d);
    V o;
    __builtin_memcpy(&o, w, sizeof(V));
    return o;
}

// The inclusive segmented scan over a tile, one item per thread: st <- the join of the items of st's segment from the
// segment's first item inside the tile through this one, in item order.  Inside the wave by lane shuffles, then the tails
// of the waves before joined in wave order through LDS.  Segments are runs of equal `seg`.  Every thread of the block
// calls it (it holds a barrier).
template <class V, class Join>
__device__ __forceinline__ void gm_seg_scan(V& st, uint32_t seg, V* wtot, uint32_t* wseg, Join join) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const V o = gm_shfl_up(st, d);
        const uint32_t os = (uint32_t)__shfl_up((int)seg, d);
        if (lane >= d && os == seg) st = join(o, st);
    }
    if (lane == 63) { wtot[wave] = st; wseg[wave] = seg; }
    __syncthreads();
    V acc = st;
    bool any = false;
    for (int w = 0; w < wave; ++w)
        if (wseg[w] == seg) { acc = any ? join(acc, wtot[w]) : wtot[w]; any = true; }
    if (any) st = join(acc, st);
}

// phase 1 of a piece: s sum, f the first counted value, bit k of same: every counted value of column k equals f[k]
template <int NV> struct GmP1 { double s[NV], f[NV]; uint32_t cnt, same; };
template <int NV>
__device__ __forceinline__ GmP1<NV> gm_join1(const GmP1<NV>& l, const GmP1<NV>& r) {
    if (l.cnt == 0) return r;
    if (r.cnt == 0) return l;
    GmP1<NV> o;
    uint32_t eq = 0;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        o.s[k] = l.s[k] + r.s[k];
        o.f[k] = l.f[k];
        eq |= l.f[k] == r.f[k] ? 1u << k : 0u;
    }
    o.cnt = l.cnt + r.cnt;
    o.same = l.same & r.same & eq;
    return o;
}
// phase 2: the power sums about the centre
template <int NS> struct GmP2 { double s[NS]; };
template <int NS>
__device__ __forceinline__ GmP2<NS> gm_join2(const GmP2<NS>& l, const GmP2<NS>& r) {
    GmP2<NS> o;
#pragma unroll
    for (int k = 0; k < NS; ++k) o.s[k] = l.s[k] + r.s[k];
    return o;
}

__device__ __forceinline__ rdf_moments_state gm_merged(const rdf_moments_state& l, const rdf_moments_state& r) {
    rdf_moments_state o = l;
    mo_merge(o, r);
    return o;
}
__device__ __forceinline__ rdf_comoments_state gm_merged(const rdf_comoments_state& l, const rdf_comoments_state& r) {
    rdf_comoments_state o = l;
    mo_comerge(o, r);
    return o;
}

// element e of a chunk `as f64`
__device__ __forceinline__ double gm_load(const DevChunkCol& cc, int dt, int64_t e) {
    switch (dt) {
        case RDF_I8: return (double)as_global<int8_t>(cc.values)[e];
        case RDF_I16: return (double)as_global<int16_t>(cc.values)[e];
        case RDF_I32: return (double)as_global<int32_t>(cc.values)[e];
        case RDF_I64: return (double)as_global<int64_t>(cc.values)[e];
        case RDF_U8: return (double)as_global<uint8_t>(cc.values)[e];
        case RDF_U16: return (double)as_global<uint16_t>(cc.values)[e];
        case RDF_U32: return (double)as_global<uint32_t>(cc.values)[e];
        case RDF_U64: return (double)as_global<uint64_t>(cc.values)[e];
        case RDF_F32: return (double)as_global<float>(cc.values)[e];
        default: return as_global<double>(cc.values)[e];
    }
}
__device__ __forceinline__ bool gm_valid(const DevChunkCol& cc, int64_t e) {
    return cc.validity ? ((cc.validity[e >> 3] >> (e & 7)) & 1) != 0 : true;
}

// The last item of a segment inside the tile holds the segment's state over the tile: where it goes.
template <class State>
__device__ __forceinline__ void gm_emit(const GmFoldArgs& a, int64_t tile, int tid, int last, uint32_t seg, uint32_t first_seg,
                                        uint32_t last_seg, const State& st) {
    using Item = GmItem<State>;
    Item* part = (Item*)a.part;
    Item it;
    it.st = st; it.seg = seg; it.pad = 0;
    if (part && seg == first_seg) part[tile * 2] = it;
    else if (part && seg == last_seg) part[tile * 2 + 1] = it;
    else if ((int64_t)seg < a.groups) ((State*)a.states)[seg] = st;
    if (part && tid == last && seg == first_seg) {   // a tile of one segment: its second slot is the empty state
        Item z = {};
        z.seg = first_seg;
        part[tile * 2 + 1] = z;
    }
}

template <bool PAIR>
__global__ __launch_bounds__(kGmThreads) void gm_level0_kernel(const GmFoldArgs a) {
    constexpr int NV = PAIR ? 2 : 1, NS = PAIR ? 5 : 4;
    using State = typename std::conditional<PAIR, rdf_comoments_state, rdf_moments_state>::type;
    __shared__ GmP1<NV> w1[kGmThreads / 64];
    __shared__ GmP2<NS> w2[kGmThreads / 64];
    __shared__ uint32_t wseg[kGmThreads / 64];
    __shared__ uint32_t sseg[kGmTile + 1];
    __shared__ double cen[NV][kGmTile];
    const int tid = threadIdx.x;
    const double inv = chunk_lookup_scale(a.row_start, a.nchunks);
    const int64_t ntiles = gm_tiles(a.m);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = tile * kGmTile, i = base + tid;
        const bool in = i < a.m;
        uint32_t seg = kGmNone;
        bool ok = false;
        double v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = 0.0;
        if (in) {
            seg = (uint32_t)((uint64_t)a.scan[i + 1] >> 32) - 1;
            const int64_t row = a.perm ? (int64_t)a.perm[i] : i;
            int64_t c = 0, start = 0;
            if (a.nchunks > 1) { c = find_chunk_row(a.row_start, a.nchunks, row, inv); start = a.row_start[c]; }
            const DevChunkCol cx = a.x[c];
            const int64_t ex = cx.offset + row - start;
            ok = gm_valid(cx, ex);
            if (PAIR) {
                const DevChunkCol cy = a.y[c];
                const int64_t ey = cy.offset + row - start;
                ok = ok && gm_valid(cy, ey);
                if (ok) v[NV - 1] = gm_load(cy, a.dt_y, ey);
            }
            if (ok) v[0] = gm_load(cx, a.dt_x, ex);
        }
        sseg[tid] = seg;
        if (tid == 0) sseg[kGmTile] = kGmNone;
        // ---- 1. the piece's sum, count and whether its counted values are all one value: its centre
        GmP1<NV> p;
#pragma unroll
        for (int k = 0; k < NV; ++k) p.s[k] = p.f[k] = v[k];
        p.cnt = ok ? 1u : 0u;
        p.same = (1u << NV) - 1;
        gm_seg_scan(p, seg, w1, wseg, [](const GmP1<NV>& l, const GmP1<NV>& r) { return gm_join1<NV>(l, r); });
        const int last = (int)((a.m - base < kGmTile ? a.m - base : kGmTile) - 1);
        const uint32_t first_seg = sseg[0], last_seg = sseg[last];
        const bool seg_end = in && sseg[tid + 1] != seg;
        const uint32_t n_piece = p.cnt;
        const uint32_t piece = (seg - first_seg) & (kGmTile - 1);   // groups are numbered consecutively: < the tile without the mask
        if (seg_end) {
#pragma unroll
            for (int k = 0; k < NV; ++k) cen[k][piece] = gm_piece_centre(n_piece, (p.same >> k) & 1, p.f[k], p.s[k]);
        }
        __syncthreads();
        // ---- 2 .. 4. d = x - c and its power sums over the piece
        double c[NV];
        GmP2<NS> q;
#pragma unroll
        for (int k = 0; k < NS; ++k) q.s[k] = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) c[k] = in ? cen[k][piece] : 0.0;
        if (ok) {
            if (PAIR) {
                const double dx = v[0] - c[0], dy = v[NV - 1] - c[NV - 1];
                q.s[0] = dx; q.s[1] = dy; q.s[2] = dx * dx; q.s[3] = dy * dy; q.s[NS - 1] = dx * dy;
            } else {
                const double d = v[0] - c[0], d2 = d * d;
                q.s[0] = d; q.s[1] = d2; q.s[2] = d2 * d; q.s[3] = d2 * d2;
            }
        }
        gm_seg_scan(q, seg, w2, wseg, [](const GmP2<NS>& l, const GmP2<NS>& r) { return gm_join2<NS>(l, r); });
        // ---- 5. the piece's state at its last item
        if (seg_end) {
            State st;
            if constexpr (PAIR) st = gm_piece_costate(n_piece, c[0], c[1], q.s);
            else st = gm_piece_state(n_piece, c[0], q.s);
            gm_emit(a, tile, tid, last, seg, first_seg, last_seg, st);
        }
        __syncthreads();
    }
}

template <class State>
__global__ __launch_bounds__(kGmThreads) void gm_fold_kernel(const GmFoldArgs a) {
    using Item = GmItem<State>;
    __shared__ State wtot[kGmThreads / 64];
    __shared__ uint32_t wseg[kGmThreads / 64];
    __shared__ uint32_t sseg[kGmTile + 1];
    const int tid = threadIdx.x;
    const Item* items = (const Item*)a.in;
    const int64_t ntiles = gm_tiles(a.m);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = tile * kGmTile, i = base + tid;
        const bool in = i < a.m;
        State st = {};
        uint32_t seg = kGmNone;
        if (in) { const Item it = items[i]; st = it.st; seg = it.seg; }
        sseg[tid] = seg;
        if (tid == 0) sseg[kGmTile] = kGmNone;
        gm_seg_scan(st, seg, wtot, wseg, [](const State& l, const State& r) { return gm_merged(l, r); });
        const int last = (int)((a.m - base < kGmTile ? a.m - base : kGmTile) - 1);
        if (in && sseg[tid + 1] != seg) gm_emit(a, tile, tid, last, seg, sseg[0], sseg[last], st);
        __syncthreads();
    }
}

// One thread per (group, call): the statistic, its validity byte and the NULL count; the threads of call 0 also write the
// group's count and its first row.  The calls are walked one after the other and the groups of a call in a grid-stride
// loop, so that a thread counts its NULL results of the call in a register and a wave adds them to the call's counter ONCE:
// 5e7 one-row groups make 5e7 NULL var_samp results, and one atomic per wave and 64 results on one address was the whole
// call's time.
__global__ __launch_bounds__(kGmThreads) void gm_finish_kernel(const GmFinishArgs a) {
    const int lane = threadIdx.x & 63;
    const int ncalls = a.ncalls > 0 ? a.ncalls : 1;
    for (int c = 0; c < ncalls; ++c) {
        const int32_t stat = a.ncalls > 0 ? a.calls[c].stat : 0;
        unsigned int nulls = 0;
        for (int64_t g = (int64_t)blockIdx.x * kGmThreads + threadIdx.x; g < a.groups; g += (int64_t)gridDim.x * kGmThreads) {
            double v = 0.0;
            bool some = false;
            int64_t count = 0;
            if (!a.states) {
                // the key tuples alone: nothing is read off a state
            } else if (a.pair) {
                const rdf_comoments_state s = ((const rdf_comoments_state*)a.states)[g];
                count = s.count;
                if (a.ncalls > 0) some = mo_costat(s, stat, &v);
            } else {
                const rdf_moments_state s = ((const rdf_moments_state*)a.states)[g];
                count = s.count;
                if (a.ncalls > 0) some = mo_stat(s, stat, &v);
            }
            if (c == 0) {
                if (a.counts) a.counts[g] = count;
                if (a.group_rows) { const uint32_t j = a.pstart[g]; a.group_rows[g] = a.perm ? a.perm[j] : j; }
            }
            if (a.ncalls > 0) {
                a.calls[c].values[g] = some ? v : 0.0;
                a.calls[c].vbytes[g] = some ? 1 : 0;
                nulls += some ? 0u : 1u;
            }
        }
        if (a.ncalls > 0) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) nulls += (unsigned int)__shfl_xor((int)nulls, m);
            if (lane == 0 && nulls) atomicAdd(&a.nulls[c], (unsigned long long)nulls);
        }
    }
}

unsigned gm_grid(int64_t m) {
    const int64_t want = gm_tiles(m), lim = (int64_t)eval_grid_limit();
    return (unsigned)(want > lim ? lim : want);
}

}  // namespace

hipError_t launch_gm_level0(const GmFoldArgs& a, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    if (a.y) hipLaunchKernelGGL(gm_level0_kernel<true>, dim3(gm_grid(a.m)), dim3(kGmThreads), 0, s, a);
    else hipLaunchKernelGGL(gm_level0_kernel<false>, dim3(gm_grid(a.m)), dim3(kGmThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gm_fold(const GmFoldArgs& a, bool pair, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    if (pair) hipLaunchKernelGGL(gm_fold_kernel<rdf_comoments_state>, dim3(gm_grid(a.m)), dim3(kGmThreads), 0, s, a);
    else hipLaunchKernelGGL(gm_fold_kernel<rdf_moments_state>, dim3(gm_grid(a.m)), dim3(kGmThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gm_finish(const GmFinishArgs& a, hipStream_t s) {
    if (a.groups <= 0) return hipSuccess;
    hipLaunchKernelGGL(gm_finish_kernel, dim3(gm_grid(a.groups)), dim3(kGmThreads), 0, s, a);
    return hipGetLastError();
}
