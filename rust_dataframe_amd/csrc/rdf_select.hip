// rdf_select.hip — the kernels of rdf_null_test / rdf_coalesce / rdf_case_when / rdf_extremum / rdf_nanvl (host side:
// rdf_capi_select.inc; what is decided about one row and the argument block: rdf_select.h; the row layout: rdf_wavetile.hip.h).
//
// One streaming launch per call, in the row layout of rdf_datetime.hip: a wave takes 512 rows of one chunk in passes of
// 64 lanes x V consecutive rows, V = 16 / (element bytes), at most 8 (1-byte types move 8 bytes per lane, so that a pass
// never exceeds the wave's tile): 128 / 256 / 512 / 512 rows for 8 / 4 / 2 / 1-byte elements.
//
//   alignment  every part, every condition and the output has its own element and bit offset, so whether a wave tile moves
//              by vector loads is decided per part: that part's first element on a vector boundary and a full tile.
//   choice     validity and condition windows are wave-uniform 64-bit words.  coalesce / case_when walk the parts in order
//              and keep the rows still `undecided`: taken = undecided & can(k), undecided &= ~can(k), all on the scalar
//              unit; values are merged per lane under the taken words.  A literal comes with its slot's table entry: no load per row.
//   skipping   a pass loads part k only when a row of its 64 V rows takes part k (a wave-uniform branch on the words), and
//              the walk ends when no row of the tile is undecided: parts behind the first never-NULL part are never read.
//              The loads of one part's passes are all issued before the first is merged.
//   NULLs      NULL rows hold 0; every wave stores the number of NULL rows of its tile and dt_nulls_kernel adds them up.
//              No atomics, no LDS, no block waits for another: the same input gives the same bytes.
#include <string.h>

#include <algorithm>

#include "rdf_select.h"
#include "rdf_wavetile.hip.h"

using namespace rdfk;

namespace {

// The A/B of skipping the parts no row of a pass takes: built with -DRDF_SELECT_READ_ALL every pass of every
// part is loaded.  Not part of the product build.
#ifdef RDF_SELECT_READ_ALL
constexpr bool kSelReadAll = true;
#else
constexpr bool kSelReadAll = false;
#endif

template <int ES> struct SelShape { static constexpr int V = ES == 1 ? 8 : 16 / ES, P = 8 / V; };

__device__ __forceinline__ uint64_t sel_or8(const uint64_t (&w)[8]) { return w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]; }
template <int V>
__device__ __forceinline__ uint64_t sel_or_pass(const uint64_t (&w)[8], int p) {
    uint64_t r = 0;
#pragma unroll
    for (int i = 0; i < V; ++i) r |= w[p * V + i];
    return r;
}

// The lane's V bits of pass p (dt_lane_bits), as an OR of masked words: inside the loop over the parts a chain of selects between
// the words is folded into ONE load behind a selected address, which keeps the words in scratch (or LDS) instead of SGPRs.
template <int V>
__device__ __forceinline__ uint32_t sel_lane_bits(const uint64_t (&ok)[8], int p, int lane) {
    const int q = (lane * V) >> 6;
    uint64_t w = 0;
#pragma unroll
    for (int i = 0; i < V; ++i) w |= q == i ? ok[p * V + i] : 0ull;
    return (uint32_t)(w >> ((lane * V) & 63)) & ((1u << V) - 1u);
}

// the wave's validity words and its NULL count
__device__ __forceinline__ void sel_finish(const SelArgs& a, const DtOut& o, const DtWave& m, int64_t t, int w, int lane, const uint64_t (&ok)[8]) {
    uint64_t mine = 0;
    int nvalid = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        mine = lane == k ? ok[k] : mine;
        nvalid += __popcll(ok[k]);
    }
    const int nwords = (m.rows + 63) >> 6;
    if (o.validity && lane < nwords) as_global_mut<uint64_t>(o.validity)[(m.r0 >> 6) + lane] = mine;
    if (a.wave_nulls && lane == 0) a.wave_nulls[t * (kCsThreads / 64) + w] = (uint32_t)(m.rows - nvalid);
}
__device__ __forceinline__ void sel_empty(const SelArgs& a, int64_t t, int w, int lane) {
    if (a.wave_nulls && lane == 0) a.wave_nulls[t * (kCsThreads / 64) + w] = 0u;
}

// slot k of the call in the wave's chunk: a column's chunk, or the literal
struct SelSlot { DevChunkCol ch; const DevChunkCol* cond; uint64_t lit; bool column; bool null_literal; };
__device__ __forceinline__ SelSlot sel_slot(const SelArgs& a, int k, int64_t chunk) {
    const ConstPtr<SelSlotDesc> t = as_const<SelSlotDesc>(a.slots);
    SelSlot s;
    s.ch = DevChunkCol{nullptr, nullptr, 0};
    const DevChunkCol* col = t[k].col;
    s.cond = t[k].cond;
    s.lit = t[k].lit;
    s.column = col != nullptr;
    s.null_literal = !s.column && t[k].lit_null != 0;
    if (s.column) s.ch = const_col(col, chunk);
    return s;
}
// v &= the rows of the tile in which the slot's value is not NULL
__device__ __forceinline__ void sel_valid(const SelSlot& s, const DtWave& m, uint64_t (&v)[8]) {
    if (s.column) dt_and(s.ch.validity, s.ch.offset + m.r0, m.rows, v);
    else if (s.null_literal) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0;
    }
}

// ---------------------------------------------------------------- coalesce / case_when: copy bits, by element size
template <int ES>
__global__ __launch_bounds__(kCsThreads) void sel_choose_kernel(SelArgs a) {
    using U = typename SelBits<ES>::U;
    constexpr int V = SelShape<ES>::V, P = SelShape<ES>::P;
    const int lane = threadIdx.x & 63, w = wave_id();
    const bool cw = a.kind == SEL_K_CASE_WHEN;
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(a.col, t, w);
        if (m.rows == 0) { sel_empty(a, t, w, lane); continue; }
        const DtOut o = dt_out(a.outs, m.chunk);
        const bool full = m.rows == kDtWaveTile;
        uint64_t undecided[8], ok[8];
        dt_rows(m.rows, undecided);
#pragma unroll
        for (int i = 0; i < 8; ++i) ok[i] = 0;
        U y[P][V];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int j = 0; j < V; ++j) y[p][j] = (U)0;
        for (int k = 0; k < a.nparts; ++k) {
            const SelSlot s = sel_slot(a, k, m.chunk);
            // can: the rows slot k can decide; val: the undecided rows it takes (sel_take), then those of them whose value is not NULL
            uint64_t val[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) val[i] = ~0ull;
            if (cw) {
                if (s.cond) {         // a branch: its condition is valid AND true (the last slot, `otherwise`, takes what is left)
                    const DevChunkCol cc = const_col(s.cond, m.chunk);
                    dt_and(cc.validity, cc.offset + m.r0, m.rows, val);
                    dt_and((const uint8_t*)cc.values, cc.offset + m.r0, m.rows, val);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) val[i] = sel_take(undecided[i], val[i]);
                sel_valid(s, m, val);
            } else {                  // coalesce: a part decides where it is not NULL
                sel_valid(s, m, val);
#pragma unroll
                for (int i = 0; i < 8; ++i) val[i] = sel_take(undecided[i], val[i]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) ok[i] |= val[i];
            if (s.column) {
                const U* src = (const U*)s.ch.values + (s.ch.offset + m.r0);
                const bool vin = full && dt_aligned<U, V>(src);
                bool need[P];
                U xs[P][V];
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    need[p] = kSelReadAll || sel_or_pass<V>(val, p) != 0;
                    if (need[p]) dt_load<U, V>(src, m.rows, p, lane, vin, xs[p]);
                }
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    if (!need[p]) continue;
                    const uint32_t bits = sel_lane_bits<V>(val, p, lane);
#pragma unroll
                    for (int j = 0; j < V; ++j) y[p][j] = (bits >> j) & 1u ? xs[p][j] : y[p][j];
                }
            } else if (sel_or8(val) != 0) {
                const U lit = (U)s.lit;
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const uint32_t bits = sel_lane_bits<V>(val, p, lane);
#pragma unroll
                    for (int j = 0; j < V; ++j) y[p][j] = (bits >> j) & 1u ? lit : y[p][j];
                }
            }
            if (!kSelReadAll && sel_or8(undecided) == 0) break;
        }
        U* dst = (U*)o.values + m.r0;
        const bool vout = full && dt_aligned<U, V>(dst);
#pragma unroll
        for (int p = 0; p < P; ++p) dt_store<U, V>(dst, m.rows, p, lane, vout, y[p]);
        sel_finish(a, o, m, t, w, lane, ok);
    }
}

// ---------------------------------------------------------------- greatest / least: the left-to-right fold, by class and size
template <int CLS, int ES>
__global__ __launch_bounds__(kCsThreads) void sel_extremum_kernel(SelArgs a) {
    using U = typename SelBits<ES>::U;
    constexpr int V = SelShape<ES>::V, P = SelShape<ES>::P;
    const int lane = threadIdx.x & 63, w = wave_id();
    const bool greatest = a.op != 0;
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(a.col, t, w);
        if (m.rows == 0) { sel_empty(a, t, w, lane); continue; }
        const DtOut o = dt_out(a.outs, m.chunk);
        const bool full = m.rows == kDtWaveTile;
        uint64_t ok[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ok[i] = 0;
        U acc[P][V];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int j = 0; j < V; ++j) acc[p][j] = (U)0;
        for (int k = 0; k < a.nparts; ++k) {
            const SelSlot s = sel_slot(a, k, m.chunk);
            uint64_t val[8];
            dt_rows(m.rows, val);
            sel_valid(s, m, val);
            const U* src = (const U*)s.ch.values + (s.ch.offset + m.r0);
            const bool vin = s.column && full && dt_aligned<U, V>(src);
            const U lit = (U)s.lit;
            bool need[P];
            U xs[P][V];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                need[p] = sel_or_pass<V>(val, p) != 0;     // a group in which the part is NULL throughout is not read
                if (need[p] && s.column) dt_load<U, V>(src, m.rows, p, lane, vin, xs[p]);
            }
#pragma unroll
            for (int p = 0; p < P; ++p) {
                if (!need[p]) continue;
                const uint32_t vb = sel_lane_bits<V>(val, p, lane), hb = sel_lane_bits<V>(ok, p, lane);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    bool have = (hb >> j) & 1u;
                    sel_fold<CLS, ES>(greatest, s.column ? xs[p][j] : lit, (vb >> j) & 1u, acc[p][j], have);
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) ok[i] |= val[i];
        }
        U* dst = (U*)o.values + m.r0;
        const bool vout = full && dt_aligned<U, V>(dst);
#pragma unroll
        for (int p = 0; p < P; ++p) dt_store<U, V>(dst, m.rows, p, lane, vout, acc[p]);
        sel_finish(a, o, m, t, w, lane, ok);
    }
}

// ---------------------------------------------------------------- nanvl: Float32 / Float64
template <int ES>
__global__ __launch_bounds__(kCsThreads) void sel_nanvl_kernel(SelArgs a) {
    using U = typename SelBits<ES>::U;
    constexpr int V = SelShape<ES>::V, P = SelShape<ES>::P;
    const int lane = threadIdx.x & 63, w = wave_id();
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(a.col, t, w);
        if (m.rows == 0) { sel_empty(a, t, w, lane); continue; }
        const DtOut o = dt_out(a.outs, m.chunk);
        const bool full = m.rows == kDtWaveTile;
        const SelSlot sa = sel_slot(a, 0, m.chunk), sb = sel_slot(a, 1, m.chunk);
        uint64_t ok[8], vb[8];
        dt_rows(m.rows, ok);
        dt_rows(m.rows, vb);
        sel_valid(sa, m, ok);
        sel_valid(sb, m, vb);
        const bool b_nullable = sb.column ? sb.ch.validity != nullptr : sb.null_literal;
        const U* pa = (const U*)sa.ch.values + (sa.ch.offset + m.r0);
        const U* pb = (const U*)sb.ch.values + (sb.ch.offset + m.r0);
        const bool va = sa.column && full && dt_aligned<U, V>(pa), vbv = sb.column && full && dt_aligned<U, V>(pb);
        const U la = (U)sa.lit, lb = (U)sb.lit;
        U xs[P][V], zs[P][V];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (sa.column) dt_load<U, V>(pa, m.rows, p, lane, va, xs[p]);
            if (sb.column) dt_load<U, V>(pb, m.rows, p, lane, vbv, zs[p]);
        }
        U y[P][V];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const uint32_t ab = sel_lane_bits<V>(ok, p, lane), bb = sel_lane_bits<V>(vb, p, lane);
            uint32_t good = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                bool valid;
                sel_nanvl<ES>(sa.column ? xs[p][j] : la, (ab >> j) & 1u, sb.column ? zs[p][j] : lb, (bb >> j) & 1u, y[p][j], valid);
                good |= (uint32_t)valid << j;
            }
            if (b_nullable) dt_drop<V>(ok, p, lane, good);   // a is NaN where b is NULL: a NULL row
        }
        U* dst = (U*)o.values + m.r0;
        const bool vout = full && dt_aligned<U, V>(dst);
#pragma unroll
        for (int p = 0; p < P; ++p) dt_store<U, V>(dst, m.rows, p, lane, vout, y[p]);
        sel_finish(a, o, m, t, w, lane, ok);
    }
}

// ---------------------------------------------------------------- is_null / is_not_null / is_nan: a mask, never NULL
// Row k * 64 + lane of the tile in lane `lane`: a wave's ballot is word k of the mask.  ES == 0: the values are not read.
template <int ES>
__global__ __launch_bounds__(kCsThreads) void sel_null_test_kernel(SelArgs a) {
    const int lane = threadIdx.x & 63, w = wave_id();
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(a.col, t, w);
        if (m.rows == 0) continue;
        const DevChunkCol ch = const_col(a.col.chunks, m.chunk);
        const DtOut o = dt_out(a.outs, m.chunk);
        uint64_t rows[8], res[8];
        dt_rows(m.rows, rows);
#pragma unroll
        for (int i = 0; i < 8; ++i) res[i] = rows[i];
        dt_and(ch.validity, ch.offset + m.r0, m.rows, res);
        if constexpr (ES == 0) {
            if (a.op == SEL_IS_NULL) {
#pragma unroll
                for (int i = 0; i < 8; ++i) res[i] = rows[i] & ~res[i];
            }
        } else {
            using U = typename SelBits<ES == 0 ? 4 : ES>::U;
            const GlobalPtr<U> src = as_global<U>((const U*)ch.values + (ch.offset + m.r0));
            U x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = i * 64 + lane < m.rows ? src[i * 64 + lane] : (U)0;
#pragma unroll
            for (int i = 0; i < 8; ++i) res[i] &= uniform64(__ballot(sel_is_nan<SEL_FLOAT, ES == 0 ? 4 : ES>(x[i])));
        }
        uint64_t mine = 0, all = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            mine = lane == i ? res[i] : mine;
            all = lane == i ? rows[i] : all;
        }
        const int nwords = (m.rows + 63) >> 6;
        if (lane < nwords) {
            as_global_mut<uint64_t>(o.values)[(m.r0 >> 6) + lane] = mine;
            if (o.validity) as_global_mut<uint64_t>(o.validity)[(m.r0 >> 6) + lane] = all;
        }
    }
}

int sel_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(n, eval_grid_limit())); }

}  // namespace

hipError_t launch_select(const SelArgs& a, hipStream_t s) {
    if (a.col.ntiles <= 0 || a.col.nchunks <= 0 || !a.outs || (a.kind != SEL_K_NULL_TEST && !a.slots) || (a.wave_nulls == nullptr) != (a.chunk_nulls == nullptr)) return hipErrorInvalidValue;
    const dim3 g((unsigned)sel_grid(a.col.ntiles)), b(kCsThreads);
    const bool size_ok = a.es == 1 || a.es == 2 || a.es == 4 || a.es == 8;
    const bool float_ok = a.cls == SEL_FLOAT && (a.es == 4 || a.es == 8);
    switch (a.kind) {
        case SEL_K_NULL_TEST:
            if (a.op < 0 || a.op >= SEL_NTESTS || !a.col.chunks || a.wave_nulls) return hipErrorInvalidValue;
            if (a.op != SEL_IS_NAN) hipLaunchKernelGGL((sel_null_test_kernel<0>), g, b, 0, s, a);
            else if (!float_ok) return hipErrorInvalidValue;
            else if (a.es == 4) hipLaunchKernelGGL((sel_null_test_kernel<4>), g, b, 0, s, a);
            else hipLaunchKernelGGL((sel_null_test_kernel<8>), g, b, 0, s, a);
            return hipGetLastError();
        case SEL_K_COALESCE:
        case SEL_K_CASE_WHEN: {
            const bool cw = a.kind == SEL_K_CASE_WHEN;
            if (!size_ok || a.nparts < 1 || a.nparts > (cw ? kSelSlots : kSelMaxParts) || (cw ? a.nconds != a.nparts - 1 || a.nconds < 1 : a.nconds != 0)) return hipErrorInvalidValue;
            switch (a.es) {
                case 1: hipLaunchKernelGGL((sel_choose_kernel<1>), g, b, 0, s, a); break;
                case 2: hipLaunchKernelGGL((sel_choose_kernel<2>), g, b, 0, s, a); break;
                case 4: hipLaunchKernelGGL((sel_choose_kernel<4>), g, b, 0, s, a); break;
                default: hipLaunchKernelGGL((sel_choose_kernel<8>), g, b, 0, s, a); break;
            }
            break;
        }
        case SEL_K_EXTREMUM:
            if (!size_ok || a.nparts < 2 || a.nparts > kSelMaxParts || (a.cls == SEL_FLOAT && !float_ok) || a.cls < SEL_SIGNED || a.cls > SEL_FLOAT) return hipErrorInvalidValue;
#define SEL_EXT(CLS)                                                                              \
    switch (a.es) {                                                                               \
        case 1: hipLaunchKernelGGL((sel_extremum_kernel<CLS, 1>), g, b, 0, s, a); break;          \
        case 2: hipLaunchKernelGGL((sel_extremum_kernel<CLS, 2>), g, b, 0, s, a); break;          \
        case 4: hipLaunchKernelGGL((sel_extremum_kernel<CLS, 4>), g, b, 0, s, a); break;          \
        default: hipLaunchKernelGGL((sel_extremum_kernel<CLS, 8>), g, b, 0, s, a); break;         \
    }
            if (a.cls == SEL_FLOAT) {
                if (a.es == 4) hipLaunchKernelGGL((sel_extremum_kernel<SEL_FLOAT, 4>), g, b, 0, s, a);
                else hipLaunchKernelGGL((sel_extremum_kernel<SEL_FLOAT, 8>), g, b, 0, s, a);
            } else if (a.cls == SEL_SIGNED) {
                SEL_EXT(SEL_SIGNED)
            } else {
                SEL_EXT(SEL_UNSIGNED)
            }
#undef SEL_EXT
            break;
        case SEL_K_NANVL:
            if (!float_ok || a.nparts != 2) return hipErrorInvalidValue;
            if (a.es == 4) hipLaunchKernelGGL((sel_nanvl_kernel<4>), g, b, 0, s, a);
            else hipLaunchKernelGGL((sel_nanvl_kernel<8>), g, b, 0, s, a);
            break;
        default:
            return hipErrorInvalidValue;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.wave_nulls) return e;
    DtArgs n;
    memset(&n, 0, sizeof n);
    n.col = a.col;
    n.wave_nulls = a.wave_nulls;
    n.chunk_nulls = a.chunk_nulls;
    n.null_split = a.null_split;
    return launch_dt_nulls(n, s);
}
