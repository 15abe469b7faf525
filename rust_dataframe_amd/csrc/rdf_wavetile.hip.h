// rdf_wavetile.hip.h — the row layout of the stand-alone streaming families (rdf_datetime.hip, rdf_select.hip), device side.
//
// A block walks the tiles of CsCol (kCsTile = 2048 rows of one chunk) it is dealt statically; each of its four waves takes
// kDtWaveTile = 512 rows, in passes of 64 lanes x V consecutive rows with V = 16 / (bytes of the storage type): a lane's rows
// of a pass are one 16-byte load and its results one vector store.  The wave's eight 64-bit windows of a bitmap come through
// scalar loads at any bit offset; a wave starts on a multiple of 512 rows of its chunk, so no output word has two writers.
#pragma once
#include "rdf_datetime.h"
#include "rdf_common.hip.h"

namespace rdfk {

struct DtWave { int64_t chunk, r0; int rows; };   // this wave's rows [r0, r0 + rows) of the chunk

__device__ __forceinline__ DtWave dt_wave(const CsCol& col, int64_t t, int w) {
    const ConstPtr<int64_t> ts = as_const<int64_t>(col.tile_start);
    const ConstPtr<int64_t> rs = as_const<int64_t>(col.row_start);
    DtWave m;
    m.chunk = find_chunk_tile(ts, col.nchunks, t);
    m.r0 = (t - ts[m.chunk]) * kCsTile + (int64_t)w * kDtWaveTile;
    const int64_t left = rs[m.chunk + 1] - rs[m.chunk] - m.r0;
    m.rows = left < kDtWaveTile ? (left < 0 ? 0 : (int)left) : kDtWaveTile;
    return m;
}

__device__ __forceinline__ DtOut dt_out(const DtOut* table, int64_t i) {
    const ConstPtr<DtOut> t = as_const<DtOut>(table);
    DtOut o;
    o.values = t[i].values; o.validity = t[i].validity;
    return o;
}

// ok[k] bit l = row k * 64 + l of the wave's tile exists ...
__device__ __forceinline__ void dt_rows(int rows, uint64_t (&ok)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int left = rows - 64 * k;
        ok[k] = left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1));
    }
}
// ... and its bit in the bitmap (nullptr = all set) is set
__device__ __forceinline__ void dt_and(const uint8_t* bitmap, int64_t bit0, int rows, uint64_t (&ok)[8]) {
    if (!bitmap) return;
    uint64_t w[8];
    load_windows_s<8>(bitmap, bit0, rows, w);
#pragma unroll
    for (int k = 0; k < 8; ++k) ok[k] &= w[k];
}

// The lane's rows of pass p are p * 64 V + lane * V + j, j < V.  Their V bits of ok:
template <int V>
__device__ __forceinline__ uint32_t dt_lane_bits(const uint64_t (&ok)[8], int p, int lane) {
    const int q = (lane * V) >> 6;
    uint64_t w = ok[p * V];
#pragma unroll
    for (int i = 1; i < V; ++i) w = q == i ? ok[p * V + i] : w;
    return (uint32_t)(w >> ((lane * V) & 63)) & ((1u << V) - 1u);
}

// V elements of T are moved as NL pieces of LB = min(V sizeof(T), 16) bytes
template <class T, int V> struct DtVec {
    static constexpr int B = V * (int)sizeof(T), LB = B < 16 ? B : 16, NL = B / LB, EPL = LB / (int)sizeof(T);
    typedef T type __attribute__((ext_vector_type(EPL)));
};
template <class T, int V>
__device__ __forceinline__ bool dt_aligned(const void* p) { return ((uintptr_t)p & (uintptr_t)(DtVec<T, V>::LB - 1)) == 0; }

// x[j] = base[p * 64 V + lane * V + j]; rows that do not exist: 0.  vec (the same in every lane): all rows of the wave's
// tile exist and base is dt_aligned
template <class T, int V>
__device__ __forceinline__ void dt_load(const T* base, int rows, int p, int lane, bool vec, T (&x)[V]) {
    using VT = typename DtVec<T, V>::type;
    constexpr int NL = DtVec<T, V>::NL, EPL = DtVec<T, V>::EPL;
    const int row0 = (p * 64 + lane) * V;
    if (vec) {
        const GlobalPtr<VT> q = (GlobalPtr<VT>)as_global<T>(base + row0);
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const VT v = q[i];
#pragma unroll
            for (int e = 0; e < EPL; ++e) x[i * EPL + e] = v[e];
        }
    } else {
        const GlobalPtr<T> q = as_global<T>(base);
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = row0 + j < rows ? q[row0 + j] : (T)0;
    }
}
template <class T, int V>
__device__ __forceinline__ void dt_store(T* base, int rows, int p, int lane, bool vec, const T (&x)[V]) {
    using VT = typename DtVec<T, V>::type;
    constexpr int NL = DtVec<T, V>::NL, EPL = DtVec<T, V>::EPL;
    const int row0 = (p * 64 + lane) * V;
    if (vec) {
        const GlobalMutPtr<VT> q = (GlobalMutPtr<VT>)as_global_mut<T>(base + row0);
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            VT v;
#pragma unroll
            for (int e = 0; e < EPL; ++e) v[e] = x[i * EPL + e];
            __builtin_nontemporal_store(v, q + i);
        }
    } else {
        const GlobalMutPtr<T> q = as_global_mut<T>(base);
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (row0 + j < rows) __builtin_nontemporal_store(x[j], q + row0 + j);
    }
}

__device__ __forceinline__ uint64_t dt_wave_or(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v |= shfl_xor64(v, m);
    return uniform64(v);
}
// rows whose bit of `good` (V bits per lane, pass p) is clear leave ok
template <int V>
__device__ __forceinline__ void dt_drop(uint64_t (&ok)[8], int p, int lane, uint32_t good) {
    const int q = (lane * V) >> 6;
    const uint64_t bad = (uint64_t)(~good & ((1u << V) - 1u)) << ((lane * V) & 63);
#pragma unroll
    for (int i = 0; i < V; ++i) ok[p * V + i] &= ~dt_wave_or(q == i ? bad : 0ull);
}

}  // namespace rdfk
