// rdf_datetime.hip — the kernels of rdf_datetime_fields / rdf_datetime_trunc / rdf_date_shift / rdf_date_diff (host side:
// rdf_capi_datetime.inc; the calendar arithmetic and the argument block: rdf_datetime.h; the row layout: rdf_wavetile.hip.h).
//
// One pass, nothing but streaming.  A block walks the tiles of CsCol (kCsTile = 2048 rows of one chunk) it is dealt
// statically; each of its four waves takes 512 rows, in passes of 64 lanes x V consecutive rows with V = 16 / (bytes of the
// storage type): a lane's rows of a pass are one 16-byte load and its results one vector store.
//
//   loads      16-byte vector loads when the wave's 512 rows all exist and the chunk's first element (values + offset) sits
//              on a 16-byte boundary; a chunk behind an odd offset and the last, partial wave tile of a chunk take the same
//              rows with element loads and a bound check each.  Outputs alike.
//   validity   the wave's eight 64-bit windows of the input bitmap(s) are fetched with scalar loads (any bit offset), ANDed
//              on the scalar unit and written as the output's words r0 / 64 ..: a wave starts on a multiple of 512 rows of
//              its chunk, so no word has two writers; rows past the chunk's length are 0 bits.  NULL rows hold 0.
//   NULL count every wave stores the number of NULL rows of its tile; dt_nulls_kernel adds them up per chunk slice.  No atomics,
//              no block waits for another, the same input gives the same bytes.
#include <algorithm>

#include "rdf_datetime.h"
#include "rdf_wavetile.hip.h"

using namespace rdfk;

namespace {

template <int ES> struct DtInt;
template <> struct DtInt<4> { using T = int32_t; };
template <> struct DtInt<8> { using T = int64_t; };

// the wave's validity words and its NULL count; nout outputs share the words
__device__ __forceinline__ void dt_finish(const DtArgs& a, const DtWave& m, int64_t t, int w, int lane, int nout, const uint64_t (&ok)[8]) {
    uint64_t mine = 0;
    int nvalid = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        mine = lane == k ? ok[k] : mine;
        nvalid += __popcll(ok[k]);
    }
    const int nwords = (m.rows + 63) >> 6;
    for (int f = 0; f < nout; ++f) {
        const DtOut o = dt_out(a.outs, (int64_t)f * a.col.nchunks + m.chunk);
        if (o.validity && lane < nwords) as_global_mut<uint64_t>(o.validity)[(m.r0 >> 6) + lane] = mine;
    }
    if (a.wave_nulls && lane == 0) a.wave_nulls[t * (kCsThreads / 64) + w] = (uint32_t)(m.rows - nvalid);
}
__device__ __forceinline__ void dt_empty(const DtArgs& a, int64_t t, int w, int lane) {
    if (a.wave_nulls && lane == 0) a.wave_nulls[t * (kCsThreads / 64) + w] = 0u;
}

// ---------------------------------------------------------------- fields: one read of the column, up to 8 Int32 outputs
template <int ES, int UNIT>
__global__ __launch_bounds__(kCsThreads) void dt_fields_kernel(DtArgs a) {
    using T = typename DtInt<ES>::T;
    constexpr int V = 16 / ES, P = 8 / V;
    const int lane = threadIdx.x & 63, w = wave_id();
    const bool civil = (a.need & DT_NEED_CIVIL) != 0, tod = (a.need & DT_NEED_TIME) != 0;
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(a.col, t, w);
        if (m.rows == 0) { dt_empty(a, t, w, lane); continue; }
        const DevChunkCol ch = const_col(a.col.chunks, m.chunk);
        uint64_t ok[8];
        dt_rows(m.rows, ok);
        dt_and(ch.validity, ch.offset + m.r0, m.rows, ok);
        const bool full = m.rows == kDtWaveTile;
        const T* src = (const T*)ch.values + (ch.offset + m.r0);
        const bool vin = full && dt_aligned<T, V>(src);
        T xs[P][V];   // every pass's rows are asked for before the first is used: P loads in flight per lane
#pragma unroll
        for (int p = 0; p < P; ++p) dt_load<T, V>(src, m.rows, p, lane, vin, xs[p]);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const T (&x)[V] = xs[p];
            const uint32_t bits = ch.validity ? dt_lane_bits<V>(ok, p, lane) : ~0u;
            int32_t day[V];
            uint32_t sod[V];
            DtCivil c[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                uint64_t rem;
                dt_split<UNIT>((int64_t)x[j], day[j], rem);
                sod[j] = 0;
                c[j] = DtCivil{0, 0, 0, 0, 0, 0, false};
                if (tod) sod[j] = dt_second_of_day<UNIT>(rem);
                if (civil) c[j] = dt_civil_from_days(day[j]);
            }
            for (int f = 0; f < a.nfields; ++f) {
                const DtOut o = dt_out(a.outs, (int64_t)f * a.col.nchunks + m.chunk);
                int32_t* dst = (int32_t*)o.values + m.r0;
                const int field = a.fields[f];
                int32_t y[V];
#pragma unroll
                for (int j = 0; j < V; ++j) y[j] = (bits >> j) & 1u ? dt_field(field, day[j], c[j], sod[j]) : 0;
                dt_store<int32_t, V>(dst, m.rows, p, lane, full && dt_aligned<int32_t, V>(dst), y);
            }
        }
        dt_finish(a, m, t, w, lane, a.nfields, ok);
    }
}

// ---------------------------------------------------------------- trunc: same storage type and unit out
template <int ES, int UNIT>
__global__ __launch_bounds__(kCsThreads) void dt_trunc_kernel(DtArgs a) {
    using T = typename DtInt<ES>::T;
    constexpr int V = 16 / ES, P = 8 / V;
    const int lane = threadIdx.x & 63, w = wave_id();
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(a.col, t, w);
        if (m.rows == 0) { dt_empty(a, t, w, lane); continue; }
        const DevChunkCol ch = const_col(a.col.chunks, m.chunk);
        const DtOut o = dt_out(a.outs, m.chunk);
        uint64_t ok[8];
        dt_rows(m.rows, ok);
        dt_and(ch.validity, ch.offset + m.r0, m.rows, ok);
        const bool full = m.rows == kDtWaveTile;
        const T* src = (const T*)ch.values + (ch.offset + m.r0);
        T* dst = (T*)o.values + m.r0;
        const bool vin = full && dt_aligned<T, V>(src), vout = full && dt_aligned<T, V>(dst);
        T xs[P][V];
#pragma unroll
        for (int p = 0; p < P; ++p) dt_load<T, V>(src, m.rows, p, lane, vin, xs[p]);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const T (&x)[V] = xs[p];
            T y[V];
            const uint32_t bits = ch.validity ? dt_lane_bits<V>(ok, p, lane) : ~0u;
#pragma unroll
            for (int j = 0; j < V; ++j) y[j] = (bits >> j) & 1u ? (T)dt_trunc<UNIT>((int64_t)x[j], a.op) : (T)0;
            dt_store<T, V>(dst, m.rows, p, lane, vout, y);
        }
        dt_finish(a, m, t, w, lane, 1, ok);
    }
}

// ---------------------------------------------------------------- shift: any unit in, Int32 days out; amounts per call or per row
template <int ES, int UNIT>
__global__ __launch_bounds__(kCsThreads) void dt_shift_kernel(DtArgs a) {
    using T = typename DtInt<ES>::T;
    constexpr int V = 16 / ES, P = 8 / V;
    const int lane = threadIdx.x & 63, w = wave_id();
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(a.col, t, w);
        if (m.rows == 0) { dt_empty(a, t, w, lane); continue; }
        const DevChunkCol ch = const_col(a.col.chunks, m.chunk);
        const DtOut o = dt_out(a.outs, m.chunk);
        DevChunkCol am = {nullptr, nullptr, 0};
        if (a.b) am = const_col(a.b, m.chunk);
        uint64_t ok[8];
        dt_rows(m.rows, ok);
        dt_and(ch.validity, ch.offset + m.r0, m.rows, ok);
        dt_and(am.validity, am.offset + m.r0, m.rows, ok);
        const bool full = m.rows == kDtWaveTile;
        const T* src = (const T*)ch.values + (ch.offset + m.r0);
        const int32_t* asrc = (const int32_t*)am.values + (am.offset + m.r0);
        int32_t* dst = (int32_t*)o.values + m.r0;
        const bool vin = full && dt_aligned<T, V>(src), vam = full && dt_aligned<int32_t, V>(asrc), vout = full && dt_aligned<int32_t, V>(dst);
        int32_t y[P][V];
        T xs[P][V];
        int32_t ks[P][V];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            dt_load<T, V>(src, m.rows, p, lane, vin, xs[p]);
            if (a.b) dt_load<int32_t, V>(asrc, m.rows, p, lane, vam, ks[p]);
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const T (&x)[V] = xs[p];
            const int32_t (&k)[V] = ks[p];
            uint32_t good = 0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                int32_t day;
                uint64_t rem;
                bool fine;
                dt_split<UNIT>((int64_t)x[j], day, rem);
                y[p][j] = dt_shift(a.op, day, a.b ? k[j] : a.amount, &fine);
                good |= (uint32_t)fine << j;
            }
            if (a.b && a.op == DT_SHIFT_NEXT_DAY) dt_drop<V>(ok, p, lane, good);   // a weekday outside 1..7: a NULL row
        }
        const bool nullable = ch.validity || am.validity || (a.b && a.op == DT_SHIFT_NEXT_DAY);
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const uint32_t bits = nullable ? dt_lane_bits<V>(ok, p, lane) : ~0u;
#pragma unroll
            for (int j = 0; j < V; ++j) y[p][j] = (bits >> j) & 1u ? y[p][j] : 0;
            dt_store<int32_t, V>(dst, m.rows, p, lane, vout, y[p]);
        }
        dt_finish(a, m, t, w, lane, 1, ok);
    }
}

// ---------------------------------------------------------------- diff: day(end) - day(start), each with its own storage and unit
template <int ESA, int ESB>
__global__ __launch_bounds__(kCsThreads) void dt_diff_kernel(DtArgs a) {
    using TA = typename DtInt<ESA>::T;
    using TB = typename DtInt<ESB>::T;
    constexpr int V = 16 / ESA, P = 8 / V;
    const int lane = threadIdx.x & 63, w = wave_id();
    for (int64_t t = blockIdx.x; t < a.col.ntiles; t += gridDim.x) {
        const DtWave m = dt_wave(a.col, t, w);
        if (m.rows == 0) { dt_empty(a, t, w, lane); continue; }
        const DevChunkCol ca = const_col(a.col.chunks, m.chunk), cb = const_col(a.b, m.chunk);
        const DtOut o = dt_out(a.outs, m.chunk);
        uint64_t ok[8];
        dt_rows(m.rows, ok);
        dt_and(ca.validity, ca.offset + m.r0, m.rows, ok);
        dt_and(cb.validity, cb.offset + m.r0, m.rows, ok);
        const bool full = m.rows == kDtWaveTile;
        const TA* sa = (const TA*)ca.values + (ca.offset + m.r0);
        const TB* sb = (const TB*)cb.values + (cb.offset + m.r0);
        int32_t* dst = (int32_t*)o.values + m.r0;
        const bool va = full && dt_aligned<TA, V>(sa), vb = full && dt_aligned<TB, V>(sb), vout = full && dt_aligned<int32_t, V>(dst);
        const bool nullable = ca.validity || cb.validity;
        TA xs[P][V];
        TB zs[P][V];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            dt_load<TA, V>(sa, m.rows, p, lane, va, xs[p]);
            dt_load<TB, V>(sb, m.rows, p, lane, vb, zs[p]);
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const TA (&x)[V] = xs[p];
            const TB (&z)[V] = zs[p];
            int32_t y[V];
            const uint32_t bits = nullable ? dt_lane_bits<V>(ok, p, lane) : ~0u;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                int32_t de, ds;
                uint64_t rem;
                dt_split_rt((int64_t)x[j], a.unit, de, rem);
                dt_split_rt((int64_t)z[j], a.unit_b, ds, rem);
                y[j] = (bits >> j) & 1u ? dt_sub32(de, ds) : 0;
            }
            dt_store<int32_t, V>(dst, m.rows, p, lane, vout, y);
        }
        dt_finish(a, m, t, w, lane, 1, ok);
    }
}

// NULL rows of chunk c: block (s, c) adds up slice s of the chunk's wave counts, in one fixed order; the host adds the
// null_split partial sums of a chunk (one block per chunk would walk the 488 281 counts of a 2.5e8-row chunk alone)
__global__ __launch_bounds__(kCsThreads) void dt_nulls_kernel(DtArgs a) {
    __shared__ unsigned long long part[kCsThreads];
    const ConstPtr<int64_t> ts = as_const<int64_t>(a.col.tile_start);
    const int64_t S = a.null_split, sl = blockIdx.x;
    for (int64_t c = blockIdx.y; c < a.col.nchunks; c += gridDim.y) {
        const int64_t first = ts[c] * (kCsThreads / 64), n = (ts[c + 1] - ts[c]) * (kCsThreads / 64);
        const int64_t lo = first + n * sl / S, hi = first + n * (sl + 1) / S;
        unsigned long long s = 0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += kCsThreads) s += a.wave_nulls[i];
        part[threadIdx.x] = s;
        __syncthreads();
        for (int k = kCsThreads / 2; k >= 1; k >>= 1) {
            if ((int)threadIdx.x < k) part[threadIdx.x] += part[threadIdx.x + k];
            __syncthreads();
        }
        if (threadIdx.x == 0) a.chunk_nulls[c * S + sl] = (int64_t)part[0];
        __syncthreads();
    }
}

int dt_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(n, eval_grid_limit())); }

bool dt_args_ok(const DtArgs& a) {
    return a.col.ntiles > 0 && a.col.nchunks > 0 && a.outs && (a.es == 4 || a.es == 8) && a.unit >= DT_UNIT_S && a.unit <= DT_UNIT_DAY &&
           !(a.unit == DT_UNIT_DAY && a.es != 4) && (a.wave_nulls == nullptr) == (a.chunk_nulls == nullptr);
}

hipError_t dt_count_nulls(const DtArgs& a, hipStream_t s) {
    if (a.wave_nulls) {
        if (a.null_split < 1 || a.null_split > kDtMaxNullSplit) return hipErrorInvalidValue;
        hipLaunchKernelGGL(dt_nulls_kernel, dim3((unsigned)a.null_split, (unsigned)std::min<int64_t>(a.col.nchunks, 65535)), dim3(kCsThreads), 0, s, a);
    }
    return hipGetLastError();
}

// KERNEL<ES, UNIT> for the call's storage width and unit (RDF_TIME_DAY is Int32 only)
#define DT_LAUNCH(KERNEL)                                                                                     \
    const dim3 g((unsigned)dt_grid(a.col.ntiles)), b(kCsThreads);                                            \
    if (a.es == 4) switch (a.unit) {                                                                          \
        case DT_UNIT_S: hipLaunchKernelGGL((KERNEL<4, DT_UNIT_S>), g, b, 0, s, a); break;                     \
        case DT_UNIT_MS: hipLaunchKernelGGL((KERNEL<4, DT_UNIT_MS>), g, b, 0, s, a); break;                   \
        case DT_UNIT_US: hipLaunchKernelGGL((KERNEL<4, DT_UNIT_US>), g, b, 0, s, a); break;                   \
        case DT_UNIT_NS: hipLaunchKernelGGL((KERNEL<4, DT_UNIT_NS>), g, b, 0, s, a); break;                   \
        default: hipLaunchKernelGGL((KERNEL<4, DT_UNIT_DAY>), g, b, 0, s, a); break;                          \
    } else switch (a.unit) {                                                                                  \
        case DT_UNIT_S: hipLaunchKernelGGL((KERNEL<8, DT_UNIT_S>), g, b, 0, s, a); break;                     \
        case DT_UNIT_MS: hipLaunchKernelGGL((KERNEL<8, DT_UNIT_MS>), g, b, 0, s, a); break;                   \
        case DT_UNIT_US: hipLaunchKernelGGL((KERNEL<8, DT_UNIT_US>), g, b, 0, s, a); break;                   \
        default: hipLaunchKernelGGL((KERNEL<8, DT_UNIT_NS>), g, b, 0, s, a); break;                           \
    }                                                                                                         \
    const hipError_t e = hipGetLastError();                                                                   \
    return e != hipSuccess ? e : dt_count_nulls(a, s)

}  // namespace

// the NULL counts alone, for the families that share the row layout and fill wave_nulls themselves (col, wave_nulls, chunk_nulls, null_split)
hipError_t launch_dt_nulls(const DtArgs& a, hipStream_t s) { return dt_count_nulls(a, s); }

hipError_t launch_dt_fields(const DtArgs& a, hipStream_t s) {
    if (!dt_args_ok(a) || a.nfields < 1 || a.nfields > kDtMaxFields) return hipErrorInvalidValue;
    DT_LAUNCH(dt_fields_kernel);
}

hipError_t launch_dt_trunc(const DtArgs& a, hipStream_t s) {
    if (!dt_args_ok(a) || !dt_trunc_level_ok(a.unit, a.op)) return hipErrorInvalidValue;
    DT_LAUNCH(dt_trunc_kernel);
}

hipError_t launch_dt_shift(const DtArgs& a, hipStream_t s) {
    if (!dt_args_ok(a) || a.op < 0 || a.op >= DT_NSHIFTS) return hipErrorInvalidValue;
    DT_LAUNCH(dt_shift_kernel);
}

hipError_t launch_dt_diff(const DtArgs& a, hipStream_t s) {
    if (!dt_args_ok(a) || !a.b || (a.es_b != 4 && a.es_b != 8) || a.unit_b < DT_UNIT_S || a.unit_b > DT_UNIT_DAY || (a.unit_b == DT_UNIT_DAY && a.es_b != 4))
        return hipErrorInvalidValue;
    const dim3 g((unsigned)dt_grid(a.col.ntiles)), b(kCsThreads);
    if (a.es == 4) {
        if (a.es_b == 4) hipLaunchKernelGGL((dt_diff_kernel<4, 4>), g, b, 0, s, a);
        else hipLaunchKernelGGL((dt_diff_kernel<4, 8>), g, b, 0, s, a);
    } else {
        if (a.es_b == 4) hipLaunchKernelGGL((dt_diff_kernel<8, 4>), g, b, 0, s, a);
        else hipLaunchKernelGGL((dt_diff_kernel<8, 8>), g, b, 0, s, a);
    }
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : dt_count_nulls(a, s);
}
