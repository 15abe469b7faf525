// rdf_window_range.hip — the kernels that turn RANGE frame offsets in key units into positions (rdf_window_range_agg; host
// side: rdf_capi_window_range.inc, rules and sizes: rdf_window_range.h).  rdf_window's front has ordered the rows; the scans
// and the emit are rdf_window_agg.hip's.  What is here:
//   keys     one gather of the order key through the permutation into a contiguous sorted array (the only random read the
//            feature adds), with a class byte per position: ordinary, LOW (NaN of a descending order), HIGH (NaN ascending, NULL)
//   window   both bounds are monotone in the position inside a partition, so every key the searches of a tile can read lies in
//            [x, y): x = the least bound position of the tile's first row, y = the greatest of its last row.  One wave per
//            tile finds them, a lane per (row, bound), searching global memory.
//   bounds   a block owns a tile of kWRangeTile positions.  When y - x <= kWRangeLdsKeys it stages keys and classes of [x, y)
//            into LDS with coalesced loads and every lane searches there, inside [max(ps, x), min(pe, y)) of its row's
//            partition [ps, pe); neighbouring lanes land on neighbouring keys.  A tile whose window does not fit is left to
//            wrange_bounds_global_kernel, whose lanes search the whole partition in the global array: the same predicate, the
//            same answers, and no use of the window argument.  A NULL / NaN row takes its peer group's ends.
// No atomics, no scratch; every output word is written by one lane from its own inputs, so chunking, memory kind and
// repetition change no byte.
#include "rdf_window_range.h"
#include "rdf_common.hip.h"

using namespace rdfk;

namespace {

constexpr uint64_t kSignBit = 0x8000000000000000ull;
constexpr uint64_t kInfBits = 0x7FF0000000000000ull;

__global__ __launch_bounds__(kWinThreads) void wrange_keys_kernel(const WRangeKeyArgs a) {
    const double inv = chunk_lookup_scale(a.row_start, a.nchunks);
    for (int64_t j = (int64_t)blockIdx.x * kWinThreads + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * kWinThreads) {
        const int64_t row = a.perm ? (int64_t)a.perm[j] : j;
        int64_t c = 0, start = 0;
        if (a.nchunks > 1) { c = find_chunk_row(a.row_start, a.nchunks, row, inv); start = a.row_start[c]; }
        const DevChunkCol cc = a.chunks[c];
        const int64_t e = cc.offset + row - start;
        const bool valid = cc.validity ? ((cc.validity[e >> 3] >> (e & 7)) & 1) : true;
        uint64_t bits = 0;
        int cls = WR_HIGH;
        if (valid) {
            bits = a.dtype == RDF_I32 ? (uint64_t)(int64_t)as_global<int32_t>(cc.values)[e] : as_global<uint64_t>(cc.values)[e];
            const bool nan = a.dtype == RDF_F64 && (bits & ~kSignBit) > kInfBits;
            cls = nan ? (a.desc ? WR_LOW : WR_HIGH) : WR_ORDINARY;
        }
        a.skey[j] = bits;
        a.scls[j] = (uint8_t)cls;
    }
}

struct GlobalKeys {
    const uint64_t* k;
    const uint8_t*  c;
    __device__ __forceinline__ uint64_t key(int64_t j) const { return k[j]; }
    __device__ __forceinline__ int cls(int64_t j) const { return c[j]; }
};
struct LdsKeys {
    const uint64_t* k;                  // the window's keys and classes, position x first
    const uint8_t*  c;
    int64_t         x;
    __device__ __forceinline__ uint64_t key(int64_t j) const { return k[j - x]; }
    __device__ __forceinline__ int cls(int64_t j) const { return c[j - x]; }
};

__device__ __forceinline__ int64_t wr_shfl_xor64(int64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(uint64_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), m);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// One wave per tile: lanes 0 .. nbounds - 1 resolve the bounds of the tile's first row, the next nbounds lanes those of its
// last row.  A first row that is not ordinary bounds the window by its own position (every ordinary row after it resolves
// behind it), a last row that is not ordinary by the position after it.
__global__ __launch_bounds__(kWinThreads) void wrange_window_kernel(const WRangeBoundsArgs a, int64_t ntiles) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * (kWinThreads / 64) + (threadIdx.x >> 6);
    if (t >= ntiles) return;                                   // (wave-uniform)
    const int64_t j0 = t * kWRangeTile, j1 = (j0 + kWRangeTile < a.n ? j0 + kWRangeTile : a.n) - 1;
    int64_t x = INT64_MAX, y = 0;
    if (lane < 2 * a.nbounds) {
        const bool last = lane >= a.nbounds;
        const int64_t j = last ? j1 : j0;
        int64_t r = last ? j + 1 : j;
        if (a.scls[j] == WR_ORDINARY) {
            const uint32_t pid = (uint32_t)((uint64_t)a.scan[j + 1] >> 32) - 1;
            const GlobalKeys g{a.skey, a.scls};
            r = wr_first(g, (int64_t)a.pstart[pid], (int64_t)a.pstart[(int64_t)pid + 1],
                         wr_probe(a.bounds[last ? lane - a.nbounds : lane], a.f64 != 0, a.desc != 0, a.skey[j]));
        }
        if (last) y = r; else x = r;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int64_t ox = wr_shfl_xor64(x, m), oy = wr_shfl_xor64(y, m);
        x = ox < x ? ox : x;
        y = oy > y ? oy : y;
    }
    if (lane == 0) {
        if (y < x) y = x;
        a.window[t] = make_uint2((uint32_t)x, (uint32_t)y);
        const bool lds = a.route != WR_ROUTE_GLOBAL && y - x <= kWRangeLdsKeys;
        a.used[lds ? 0 : 1] = 1u;                              // (every writer stores the same word)
    }
}

template <bool kLds, class K>
__device__ __forceinline__ void wrange_tile(const WRangeBoundsArgs& a, const K& keys, int64_t j0, int64_t x, int64_t y) {
#pragma unroll
    for (int q = 0; q < kWRangePer; ++q) {
        const int64_t j = j0 + q * kWRangeThreads + threadIdx.x;
        if (j >= a.n) break;
        const uint64_t inc = (uint64_t)a.scan[j + 1];
        const uint32_t pid = (uint32_t)(inc >> 32) - 1;
        const int64_t ps = (int64_t)a.pstart[pid], pe = (int64_t)a.pstart[(int64_t)pid + 1];
        if (a.scls[j] == WR_ORDINARY) {
            const uint64_t o = a.skey[j];
            const int64_t lo = kLds ? (ps > x ? ps : x) : ps, hi = kLds ? (pe < y ? pe : y) : pe;
            for (int b = 0; b < a.nbounds; ++b)
                a.out[b][j] = (uint32_t)(wr_first(keys, lo, hi, wr_probe(a.bounds[b], a.f64 != 0, a.desc != 0, o)) - ps);
        } else {                                               // a NULL / NaN row: its own peer group
            const uint32_t gid = (uint32_t)inc - 1;
            const int64_t f = (int64_t)a.gstart[gid], l1 = (int64_t)a.gstart[(int64_t)gid + 1];
            for (int b = 0; b < a.nbounds; ++b) a.out[b][j] = (uint32_t)((a.bounds[b].is_end ? l1 : f) - ps);
        }
    }
}

__global__ __launch_bounds__(kWRangeThreads) void wrange_bounds_lds_kernel(const WRangeBoundsArgs a) {
    __shared__ uint64_t lk[kWRangeLdsKeys];
    __shared__ uint8_t lc[kWRangeLdsKeys];
    const uint2 w = a.window[blockIdx.x];
    const int64_t x = w.x, y = w.y;
    if (a.route == WR_ROUTE_GLOBAL || y - x > kWRangeLdsKeys) return;   // (block-uniform) the global kernel's tile
    for (int64_t i = threadIdx.x; i < y - x; i += kWRangeThreads) {     // y - x <= kWRangeLdsKeys, x + i < y <= n
        lk[i] = a.skey[x + i];
        lc[i] = a.scls[x + i];
    }
    __syncthreads();
    wrange_tile<true>(a, LdsKeys{lk, lc, x}, (int64_t)blockIdx.x * kWRangeTile, x, y);
}

__global__ __launch_bounds__(kWRangeThreads) void wrange_bounds_global_kernel(const WRangeBoundsArgs a) {
    const uint2 w = a.window[blockIdx.x];
    if (a.route != WR_ROUTE_GLOBAL && (int64_t)w.y - (int64_t)w.x <= kWRangeLdsKeys) return;   // the LDS kernel's tile
    wrange_tile<false>(a, GlobalKeys{a.skey, a.scls}, (int64_t)blockIdx.x * kWRangeTile, 0, 0);
}

}  // namespace

hipError_t launch_wrange_keys(const WRangeKeyArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int64_t want = (a.n + kWinThreads - 1) / kWinThreads, lim = (int64_t)eval_grid_limit();
    hipLaunchKernelGGL(wrange_keys_kernel, dim3((unsigned)(want > lim ? lim : want)), dim3(kWinThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_wrange_bounds(const WRangeBoundsArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.nbounds <= 0) return hipSuccess;
    const int64_t ntiles = (a.n + kWRangeTile - 1) / kWRangeTile;   // < 2^22: n < 2^32
    constexpr int per = kWinThreads / 64;
    hipLaunchKernelGGL(wrange_window_kernel, dim3((unsigned)((ntiles + per - 1) / per)), dim3(kWinThreads), 0, s, a, ntiles);
    if (a.route != WR_ROUTE_GLOBAL) hipLaunchKernelGGL(wrange_bounds_lds_kernel, dim3((unsigned)ntiles), dim3(kWRangeThreads), 0, s, a);
    hipLaunchKernelGGL(wrange_bounds_global_kernel, dim3((unsigned)ntiles), dim3(kWRangeThreads), 0, s, a);
    return hipGetLastError();
}
