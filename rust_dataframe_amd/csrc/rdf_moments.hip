// rdf_moments.hip — the kernels of rdf_moments / rdf_comoments (host side: rdf_capi_moments.inc, argument block and the
// merge formulas: rdf_moments.h).
//
// One pass.  A block walks the tiles of CsCol (kCsTile rows of one chunk) it is dealt statically, each of its four waves
// takes a quarter of the tile — 64 lanes x 8 rows, held in registers — and keeps a running state of its own:
//
//   which rows count   validity, mask validity and mask bits are 64-bit windows fetched with scalar loads and ANDed on the
//                      scalar unit; their population count is the tile's n
//   centre             c = (sum x) / n by a wave butterfly — any double near the tile mean will do; a tile whose counted
//                      values are all equal takes that value, so that a constant column has every d = 0 exactly
//   power sums         d = x - c per row (ONE rounding, relative to d however large c is), sum d, d^2, d^3, d^4 per lane,
//                      four butterflies
//   tile state         mo_tile_state: the true mean is c + (sum d) / n, kept as two doubles; M2..M4 by the binomial shift
//   fold               mo_merge into the wave's running state — the host's merge, the same code
//
// The four wave states are folded in wave order through LDS and every block writes ONE state with plain stores; the host
// folds the blocks' states in block order.  No atomics, no waiting between blocks, nothing depends on arrival order: the
// same input gives the same bytes.  sum x^2 is never formed.
#include <algorithm>

#include "rdf_moments.h"
#include "rdf_common.hip.h"

using namespace rdfk;

namespace {

constexpr int R = kMoRowsPerLane;

struct MoTile { int64_t chunk, r0; int rows; };   // this wave's rows [r0, r0 + rows) of the chunk

__device__ __forceinline__ MoTile mo_tile(const CsCol& col, int64_t t, int w) {
    const ConstPtr<int64_t> ts = as_const<int64_t>(col.tile_start);
    const ConstPtr<int64_t> rs = as_const<int64_t>(col.row_start);
    MoTile m;
    m.chunk = find_chunk_tile(ts, col.nchunks, t);
    m.r0 = (t - ts[m.chunk]) * kCsTile + (int64_t)w * kMoWaveTile;
    const int64_t left = rs[m.chunk + 1] - rs[m.chunk] - m.r0;
    m.rows = left < kMoWaveTile ? (left < 0 ? 0 : (int)left) : kMoWaveTile;
    return m;
}

// ok[k] bit l = row k * 64 + l of the wave's tile exists
__device__ __forceinline__ void mo_rows(int rows, uint64_t (&ok)[R]) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int left = rows - 64 * k;
        ok[k] = left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1));
    }
}
// ... and its bit in the bitmap (nullptr = all set) is set
__device__ __forceinline__ void mo_and(const uint8_t* bitmap, int64_t bit0, int rows, uint64_t (&ok)[R]) {
    if (!bitmap) return;
    uint64_t w[R];
    load_windows_s<R>(bitmap, bit0, rows, w);
#pragma unroll
    for (int k = 0; k < R; ++k) ok[k] &= w[k];
}

template <int ES> struct MoRaw;
template <> struct MoRaw<1> { using T = uint8_t; };
template <> struct MoRaw<2> { using T = uint16_t; };
template <> struct MoRaw<4> { using T = uint32_t; };
template <> struct MoRaw<8> { using T = uint64_t; };

// the lane's rows lane + 64 k of the wave's tile `as f64` (rows that do not exist: 0); dt is the same in every lane
template <int ES>
__device__ __forceinline__ void mo_load(const DevChunkCol& ch, int dt, const MoTile& m, int lane, double (&x)[R]) {
    using T = typename MoRaw<ES>::T;
    const GlobalPtr<T> p = as_global<T>(ch.values) + (ch.offset + m.r0);
    T raw[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int i = k * 64 + lane;
        raw[k] = i < m.rows ? p[i] : (T)0;
    }
    if (ES == 8) {
        if (dt == RDF_F64) {
#pragma unroll
            for (int k = 0; k < R; ++k) x[k] = u2d((uint64_t)raw[k]);
        } else if (dt == RDF_I64) {
#pragma unroll
            for (int k = 0; k < R; ++k) x[k] = (double)(int64_t)raw[k];
        } else {
#pragma unroll
            for (int k = 0; k < R; ++k) x[k] = (double)(uint64_t)raw[k];
        }
    } else if (ES == 4) {
        if (dt == RDF_F32) {
#pragma unroll
            for (int k = 0; k < R; ++k) x[k] = (double)__uint_as_float((uint32_t)raw[k]);
        } else if (dt == RDF_I32) {
#pragma unroll
            for (int k = 0; k < R; ++k) x[k] = (double)(int32_t)raw[k];
        } else {
#pragma unroll
            for (int k = 0; k < R; ++k) x[k] = (double)(uint32_t)raw[k];
        }
    } else {
        const bool sgn = dt_is_signed(dt);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int32_t u = (int32_t)raw[k], s = ES == 2 ? (int32_t)(int16_t)raw[k] : (int32_t)(int8_t)raw[k];
            x[k] = (double)(sgn ? s : u);
        }
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += u2d(shfl_xor64(d2u(v), m));
    return v;
}

// rows that do not count become 0; -> true when every counted value equals the first one (then x0 is that value)
__device__ __forceinline__ bool mo_select(const uint64_t (&ok)[R], int lane, double (&x)[R], double& x0) {
    bool found = false;
    x0 = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (!found && ok[k]) {
            const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)ok[k]) - 1);
            const uint64_t b = d2u(x[k]);
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, src);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), src);
            x0 = u2d(((uint64_t)hi << 32) | lo);
            found = true;
        }
    }
    bool differs = false;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const bool on = (ok[k] >> lane) & 1;
        x[k] = on ? x[k] : 0.0;
        differs |= on && x[k] != x0;
    }
    return __ballot(differs) == 0;
}

__device__ __forceinline__ int mo_count(const uint64_t (&ok)[R]) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < R; ++k) n += __popcll(ok[k]);
    return __builtin_amdgcn_readfirstlane(n);
}

template <int ES>
__global__ __launch_bounds__(kCsThreads) void mo_moments_kernel(MoArgs a) {
    __shared__ rdf_moments_state ws[kCsThreads / 64];
    const int lane = threadIdx.x & 63, w = wave_id();
    rdf_moments_state run = {0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        const MoTile m = mo_tile(a.col, t, w);
        if (m.rows == 0) continue;
        const DevChunkCol ch = const_col(a.col.chunks, m.chunk);
        double x[R];
        mo_load<ES>(ch, a.dt_x, m, lane, x);
        uint64_t ok[R];
        mo_rows(m.rows, ok);
        mo_and(ch.validity, ch.offset + m.r0, m.rows, ok);
        if (a.mask) {
            const DevChunkCol mk = const_col(a.mask, m.chunk);
            mo_and(mk.validity, mk.offset + m.r0, m.rows, ok);
            mo_and((const uint8_t*)mk.values, mk.offset + m.r0, m.rows, ok);
        }
        const int n = mo_count(ok);
        if (n == 0) continue;
        double x0;
        const bool same = mo_select(ok, lane, x, x0);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) s += x[k];
        const double c = same ? x0 : wave_sum(s) / (double)n;
        double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const double d = (ok[k] >> lane) & 1 ? x[k] - c : 0.0;
            const double d2 = d * d;
            s1 += d; s2 += d2; s3 += d2 * d; s4 += d2 * d2;
        }
        s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); s4 = wave_sum(s4);
        mo_merge(run, mo_tile_state(n, c, s1, s2, s3, s4));
    }
    if (lane == 0) ws[w] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        rdf_moments_state tot = ws[0];
        for (int i = 1; i < kCsThreads / 64; ++i) mo_merge(tot, ws[i]);
        ((rdf_moments_state*)a.out)[blockIdx.x] = tot;
    }
}

template <int ESX, int ESY>
__global__ __launch_bounds__(kCsThreads) void mo_comoments_kernel(MoArgs a) {
    __shared__ rdf_comoments_state ws[kCsThreads / 64];
    const int lane = threadIdx.x & 63, w = wave_id();
    rdf_comoments_state run = {0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        const MoTile m = mo_tile(a.col, t, w);
        if (m.rows == 0) continue;
        const DevChunkCol cx = const_col(a.col.chunks, m.chunk), cy = const_col(a.y, m.chunk);
        double x[R], y[R];
        mo_load<ESX>(cx, a.dt_x, m, lane, x);
        mo_load<ESY>(cy, a.dt_y, m, lane, y);
        uint64_t ok[R];
        mo_rows(m.rows, ok);
        mo_and(cx.validity, cx.offset + m.r0, m.rows, ok);
        mo_and(cy.validity, cy.offset + m.r0, m.rows, ok);
        if (a.mask) {
            const DevChunkCol mk = const_col(a.mask, m.chunk);
            mo_and(mk.validity, mk.offset + m.r0, m.rows, ok);
            mo_and((const uint8_t*)mk.values, mk.offset + m.r0, m.rows, ok);
        }
        const int n = mo_count(ok);
        if (n == 0) continue;
        double x0, y0;
        const bool samex = mo_select(ok, lane, x, x0), samey = mo_select(ok, lane, y, y0);
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) { sx += x[k]; sy += y[k]; }
        const double ccx = samex ? x0 : wave_sum(sx) / (double)n, ccy = samey ? y0 : wave_sum(sy) / (double)n;
        double dx1 = 0.0, dy1 = 0.0, dxx = 0.0, dyy = 0.0, dxy = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const bool on = (ok[k] >> lane) & 1;
            const double dx = on ? x[k] - ccx : 0.0, dy = on ? y[k] - ccy : 0.0;
            dx1 += dx; dy1 += dy; dxx += dx * dx; dyy += dy * dy; dxy += dx * dy;
        }
        dx1 = wave_sum(dx1); dy1 = wave_sum(dy1); dxx = wave_sum(dxx); dyy = wave_sum(dyy); dxy = wave_sum(dxy);
        mo_comerge(run, mo_cotile_state(n, ccx, ccy, dx1, dy1, dxx, dyy, dxy));
    }
    if (lane == 0) ws[w] = run;
    __syncthreads();
    if (threadIdx.x == 0) {
        rdf_comoments_state tot = ws[0];
        for (int i = 1; i < kCsThreads / 64; ++i) mo_comerge(tot, ws[i]);
        ((rdf_comoments_state*)a.out)[blockIdx.x] = tot;
    }
}

int mo_es(int dt) {
    switch (dt) {
        case RDF_I8: case RDF_U8: return 1;
        case RDF_I16: case RDF_U16: return 2;
        case RDF_I32: case RDF_U32: case RDF_F32: return 4;
        default: return 8;
    }
}

template <int ESX>
void mo_launch_co(const MoArgs& a, int esy, dim3 g, dim3 b, hipStream_t s) {
    switch (esy) {
        case 1: hipLaunchKernelGGL((mo_comoments_kernel<ESX, 1>), g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL((mo_comoments_kernel<ESX, 2>), g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL((mo_comoments_kernel<ESX, 4>), g, b, 0, s, a); break;
        default: hipLaunchKernelGGL((mo_comoments_kernel<ESX, 8>), g, b, 0, s, a); break;
    }
}

}  // namespace

// every block has at least one tile, so every one of the grid's states is written
int mo_grid(int64_t ntiles) { return (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, eval_grid_limit())); }

hipError_t launch_mo_moments(const MoArgs& a, int grid, hipStream_t s) {
    if (a.col.ntiles <= 0 || grid <= 0 || grid > a.col.ntiles) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(kCsThreads);
    switch (mo_es(a.dt_x)) {
        case 1: hipLaunchKernelGGL(mo_moments_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(mo_moments_kernel<2>, g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL(mo_moments_kernel<4>, g, b, 0, s, a); break;
        default: hipLaunchKernelGGL(mo_moments_kernel<8>, g, b, 0, s, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_mo_comoments(const MoArgs& a, int grid, hipStream_t s) {
    if (a.col.ntiles <= 0 || grid <= 0 || grid > a.col.ntiles || !a.y) return hipErrorInvalidValue;
    const dim3 g((unsigned)grid), b(kCsThreads);
    switch (mo_es(a.dt_x)) {
        case 1: mo_launch_co<1>(a, mo_es(a.dt_y), g, b, s); break;
        case 2: mo_launch_co<2>(a, mo_es(a.dt_y), g, b, s); break;
        case 4: mo_launch_co<4>(a, mo_es(a.dt_y), g, b, s); break;
        default: mo_launch_co<8>(a, mo_es(a.dt_y), g, b, s); break;
    }
    return hipGetLastError();
}
