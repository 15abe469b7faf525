// rdf_window.hip — the kernels of the window functions (row_number, rank, dense_rank, percent_rank, cume_dist, ntile,
// lag, lead over partitions; host side: rdf_capi_window.inc, argument blocks: rdf_window.h).
//
// sort_core has ordered the rows by (partition keys, order keys).  From its permutation:
//   flags   a lane per sorted position compares the row with the one before it, key by key: does a partition start here
//           (P), does a peer group start here (G)?  A numeric key is gathered once per row — the neighbour's comes over a
//           lane shuffle, only lane 0 of a wave reads two rows; Utf8 keys compare lengths, then bytes as 8-byte words, a
//           whole wave on a row of kWinLongRow bytes or more.  Floats compare canonically (-0.0 == +0.0, one NaN).
//   (scan)  launch_scan over the packed flags numbers partitions and peer groups at every position
//   starts  the first position of every partition and peer group goes into two tables (the last entry = n)
//   emit    a lane per sorted position reads its numbers and the two tables' entries around it — k, n, f, l, d in
//           registers — and writes every requested call's answer to out[row]; lag / lead read the permutation o places away
//   pack    the valid bytes of a lag / lead output become its bitmap (a ballot per 64 rows: no atomics on bitmap words)
// No kernel waits on another block: there is no look-back to stall.
#include "rdf_window.h"
#include "rdf_common.hip.h"

using namespace rdfk;

namespace {

__device__ __forceinline__ uint64_t win_shfl_up64(uint64_t v) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t win_shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// The bits two rows of a numeric key are compared by: the value itself, floats canonical.  *isnull: the row is NULL.
__device__ __forceinline__ uint64_t win_num_bits(const WinKey& key, const int64_t* row_start, int64_t nchunks, double inv, int64_t row, bool* isnull) {
    int64_t c = 0, start = 0;
    if (nchunks > 1) { c = find_chunk_row(row_start, nchunks, row, inv); start = row_start[c]; }
    const DevChunkCol cc = key.chunks[c];
    const int64_t e = cc.offset + row - start;
    *isnull = cc.validity ? !((cc.validity[e >> 3] >> (e & 7)) & 1) : false;
    switch (key.dtype) {
        case RDF_I8: case RDF_U8: return as_global<uint8_t>(cc.values)[e];
        case RDF_I16: case RDF_U16: return as_global<uint16_t>(cc.values)[e];
        case RDF_I32: case RDF_U32: return as_global<uint32_t>(cc.values)[e];
        case RDF_F32: {
            const uint32_t b = as_global<uint32_t>(cc.values)[e];
            if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC00000u;
            return b == 0x80000000u ? 0u : b;
        }
        case RDF_F64: {
            const uint64_t b = as_global<uint64_t>(cc.values)[e];
            if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return 0x7FF8000000000000ull;
            return b == 0x8000000000000000ull ? 0ull : b;
        }
        default: return as_global<uint64_t>(cc.values)[e];
    }
}

struct WinRow { const uint8_t* p; int32_t len; bool valid; };
// last chunk whose first row is <= row (empty chunks share the first row of the next one and are skipped by this rule)
__device__ int64_t win_find_chunk(const Utf8Chunk* ch, int64_t nch, int64_t row) {
    int64_t lo = 0, hi = nch;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ch[mid].row_start <= row) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
// every byte read is clamped into the chunk's value-offset range the host checked
__device__ __forceinline__ WinRow win_row(const Utf8Chunk* chunks, int64_t nchunks, int64_t row) {
    const Utf8Chunk& c = chunks[nchunks > 1 ? win_find_chunk(chunks, nchunks, row) : 0];
    const int64_t e = row - c.row_start;
    int32_t b = c.offs[e], en = c.offs[e + 1];
    b = b < c.lo ? c.lo : (b > c.hi ? c.hi : b);
    en = en < b ? b : (en > c.hi ? c.hi : en);
    WinRow r;
    r.p = c.data + b;
    r.len = en - b;
    r.valid = !c.valid || ((c.valid[(c.valid_off + e) >> 3] >> ((c.valid_off + e) & 7)) & 1);
    return r;
}
// bytes [8w, 8w + 8) of a row as a little-endian word, zero beyond the row's end (nothing past the row is read)
__device__ __forceinline__ uint64_t win_word(const uint8_t* p, int32_t len, int32_t w) {
    const int32_t o = w * 8;
    uint64_t x = 0;
    if (o + 8 <= len) { __builtin_memcpy(&x, p + o, 8); return x; }
    for (int b = 0; o + b < len; ++b) x |= (uint64_t)p[o + b] << (8 * b);
    return x;
}
// need: this lane wants "ra and rb hold the same bytes" decided.  Called by all lanes of the wave.
__device__ bool win_rows_equal(bool need, const WinRow& ra, const WinRow& rb) {
    const int lane = threadIdx.x & 63;
    bool eq = true, lng = false;
    if (need) {
        if (ra.len != rb.len) eq = false;
        else if (ra.len >= kWinLongRow) lng = true;
        else {
            const int32_t nw = (ra.len + 7) >> 3;
            for (int32_t w = 0; w < nw && eq; ++w) eq = win_word(ra.p, ra.len, w) == win_word(rb.p, rb.len, w);
        }
    }
    unsigned long long m = __ballot(lng);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const uint8_t* pa = (const uint8_t*)(uintptr_t)win_shfl64((uint64_t)(uintptr_t)ra.p, src);
        const uint8_t* pb = (const uint8_t*)(uintptr_t)win_shfl64((uint64_t)(uintptr_t)rb.p, src);
        const int32_t len = __shfl(ra.len, src);
        const int32_t nw = (len + 7) >> 3;
        bool any = false;
        for (int32_t w0 = 0; w0 < nw && !any; w0 += 64) {
            const int32_t w = w0 + lane;
            const bool diff = w < nw && win_word(pa, len, w) != win_word(pb, len, w);
            any = __ballot(diff) != 0;
        }
        if (lane == src) eq = !any;
    }
    return eq;
}

__global__ __launch_bounds__(kWinThreads) void win_flags_kernel(const WinFlagArgs a) {
    const int lane = threadIdx.x & 63;
    const double inv = chunk_lookup_scale(a.row_start, a.nchunks);
    for (int64_t j0 = (int64_t)blockIdx.x * kWinThreads; j0 < a.n; j0 += (int64_t)gridDim.x * kWinThreads) {
        const int64_t j = j0 + threadIdx.x;
        const bool in = j < a.n;
        const bool cmp = in && j > 0;                       // there is a row before this one
        const uint32_t r1 = in ? (a.perm ? a.perm[j] : (uint32_t)j) : 0u;
        uint32_t r0 = (uint32_t)__shfl_up((int)r1, 1);
        if (lane == 0 && cmp) r0 = a.perm ? a.perm[j - 1] : (uint32_t)(j - 1);
        bool dp = false, dg = false;                        // differs on a partition key / on any key
        for (int k = 0; k < a.nkeys; ++k) {
            const WinKey& key = a.keys[k];
            bool differ;
            if (key.chunks) {
                bool n1 = false, n0;
                const uint64_t b1 = in ? win_num_bits(key, a.row_start, a.nchunks, inv, (int64_t)r1, &n1) : 0;
                uint64_t b0 = win_shfl_up64(b1);
                n0 = __shfl_up((int)n1, 1) != 0;
                if (lane == 0 && cmp) b0 = win_num_bits(key, a.row_start, a.nchunks, inv, (int64_t)r0, &n0);
                differ = n1 != n0 || (!n1 && b1 != b0);
            } else {
                const bool need = cmp && !dg;               // a peer-group start is decided already: spare the bytes
                WinRow ra{nullptr, 0, true}, rb{nullptr, 0, true};
                if (need) { ra = win_row(key.utf8, a.nchunks, (int64_t)r1); rb = win_row(key.utf8, a.nchunks, (int64_t)r0); }
                const bool both = need && ra.valid && rb.valid;
                const bool eq = win_rows_equal(both, ra, rb);
                differ = need && (ra.valid != rb.valid || (both && !eq));
            }
            if (cmp && differ) { dg = true; if (!key.order) dp = true; }
        }
        // a row that differs from its predecessor on an order key only stays in its partition; one that differs on a
        // partition key starts both.  (Keys after the first difference are still compared for numeric columns — their
        // gather is the cost, not the compare — and dp needs every partition key looked at anyway.)
        if (in) {
            const bool p = j == 0 || dp, g = p || dg;
            a.flags[j] = (int64_t)((p ? kWinFlagP : 0) | (g ? kWinFlagG : 0));
        }
    }
}

__global__ __launch_bounds__(kWinThreads) void win_starts_kernel(const WinStartArgs a) {
    for (int64_t j = (int64_t)blockIdx.x * kWinThreads + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * kWinThreads) {
        const uint64_t ex = (uint64_t)a.scan[j], inc = (uint64_t)a.scan[j + 1];
        const uint32_t pid = (uint32_t)(inc >> 32) - 1, gid = (uint32_t)inc - 1;
        if ((inc >> 32) != (ex >> 32)) a.pstart[pid] = (uint32_t)j;
        if ((uint32_t)inc != (uint32_t)ex) a.gstart[gid] = (uint32_t)j;
        if (j == a.n - 1) { a.pstart[(int64_t)pid + 1] = (uint32_t)a.n; a.gstart[(int64_t)gid + 1] = (uint32_t)a.n; }
    }
}

__global__ __launch_bounds__(kWinThreads) void win_emit_kernel(const WinEmitArgs a) {
    unsigned int nulls[RDF_WINDOW_MAX_CALLS];
#pragma unroll
    for (int c = 0; c < RDF_WINDOW_MAX_CALLS; ++c) nulls[c] = 0;
    for (int64_t j = (int64_t)blockIdx.x * kWinThreads + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * kWinThreads) {
        const uint64_t inc = (uint64_t)a.scan[j + 1];
        const uint32_t pid = (uint32_t)(inc >> 32) - 1, gid = (uint32_t)inc - 1;
        const uint32_t ps = a.pstart[pid], pe = a.pstart[(int64_t)pid + 1];
        const uint32_t gs = a.gstart[gid], ge = a.gstart[(int64_t)gid + 1];
        const uint32_t gid_ps = (uint32_t)(uint64_t)a.scan[(int64_t)ps + 1] - 1;   // the peer group the partition starts with
        const uint32_t k = (uint32_t)j - ps, n = pe - ps, f = gs - ps, l = ge - 1 - ps, d = gid - gid_ps;
        const int64_t row = a.perm ? (int64_t)a.perm[j] : j;
#pragma unroll
        for (int c = 0; c < RDF_WINDOW_MAX_CALLS; ++c) {
            if (c >= a.ncalls) break;
            const WinCallOut& o = a.calls[c];
            switch (o.fn) {
                case RDF_WIN_ROW_NUMBER: as_global_mut<int64_t>(o.values)[row] = (int64_t)k + 1; break;
                case RDF_WIN_RANK: as_global_mut<int64_t>(o.values)[row] = (int64_t)f + 1; break;
                case RDF_WIN_DENSE_RANK: as_global_mut<int64_t>(o.values)[row] = (int64_t)d + 1; break;
                case RDF_WIN_PERCENT_RANK: as_global_mut<double>(o.values)[row] = n == 1 ? 0.0 : (double)f / (double)(n - 1); break;
                case RDF_WIN_CUME_DIST: as_global_mut<double>(o.values)[row] = (double)(l + 1) / (double)n; break;
                case RDF_WIN_NTILE: {
                    int64_t t = (int64_t)k + 1;                                     // more buckets than rows: one row each
                    if (o.param <= (uint64_t)n) {
                        const uint32_t b = (uint32_t)o.param, q = n / b, r = n % b, big = r * (q + 1);   // big <= n: no overflow
                        t = k < big ? (int64_t)(k / (q + 1)) + 1 : (int64_t)r + (int64_t)((k - big) / q) + 1;
                    }
                    as_global_mut<int64_t>(o.values)[row] = t;
                    break;
                }
                default: {   // LAG / LEAD: the row o.param places before / after, inside [ps, pe)
                    const bool lag = o.fn == RDF_WIN_LAG;
                    const bool ok = lag ? o.param <= (uint64_t)k : o.param < (uint64_t)(n - k);
                    uint32_t v = 0;
                    if (ok) { const int64_t jj = lag ? j - (int64_t)o.param : j + (int64_t)o.param; v = a.perm ? a.perm[jj] : (uint32_t)jj; }
                    as_global_mut<uint32_t>(o.values)[row] = v;
                    if (o.vbytes) o.vbytes[row] = ok ? 1 : 0;
                    nulls[c] += ok ? 0u : 1u;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < RDF_WINDOW_MAX_CALLS; ++c) {
        if (c >= a.ncalls) break;
        if (a.calls[c].fn < RDF_WIN_LAG) continue;          // (uniform: the same for every lane)
        unsigned int v = nulls[c];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += (unsigned int)__shfl_xor((int)v, m);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&a.nulls[c], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kWinThreads) void win_pack_kernel(const uint8_t* vbytes, int64_t n, uint64_t* words) {
    for (int64_t i0 = (int64_t)blockIdx.x * kWinThreads; i0 < n; i0 += (int64_t)gridDim.x * kWinThreads) {
        const int64_t i = i0 + threadIdx.x;
        const unsigned long long b = __ballot(i < n && vbytes[i] != 0);
        if ((threadIdx.x & 63) == 0 && i < n) words[i >> 6] = b;
    }
}

int win_grid(int64_t items) {
    const int64_t want = (items + kWinThreads - 1) / kWinThreads;
    const int64_t lim = (int64_t)eval_grid_limit();
    return (int)(want < 1 ? 1 : (want > lim ? lim : want));
}

}  // namespace

hipError_t launch_win_flags(const WinFlagArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(win_flags_kernel, dim3(win_grid(a.n)), dim3(kWinThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_win_starts(const WinStartArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(win_starts_kernel, dim3(win_grid(a.n)), dim3(kWinThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_win_emit(const WinEmitArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(win_emit_kernel, dim3(win_grid(a.n)), dim3(kWinThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_win_pack(const uint8_t* vbytes, int64_t n, uint64_t* words, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(win_pack_kernel, dim3(win_grid(n)), dim3(kWinThreads), 0, s, vbytes, n, words);
    return hipGetLastError();
}
