// rdf_utf8_sort.hip — the kernels of a sort by a Utf8 criterion (DataFrame::sort over a StringArray column; host side:
// rdf_capi_sort_utf8.inc, argument block: rdf_utf8.h).
//
// A criterion refines the incoming row order in rounds; the digit passes themselves are the 64-bit radix passes every
// sort column takes (rdf_sort.hip).  Per round:
//   lcp    (rounds >= 1) a wave per row compares the row with its segment's first row from the segment's depth on, and
//          the segment's depth jumps past the prefix all its rows share: a run of identical long strings costs one pass
//          over their bytes, and every round after round 0 splits every segment it is given
//   keys   a lane per row writes the row's word (7 bytes + end code) — the row read through the permutation
//   (sort) stable passes over the words, then over the segment numbers
//   mark   the rows in sorted order go back into the slots of their segment; a row goes on when a neighbour in its
//          segment holds the same word and the row has bytes past it
//   next   a scan of those flags numbers the next round's rows and segments
// Every byte read is clamped into the chunk's value-offset range the host checked: offsets inside it are not trusted.
#include "rdf_utf8.h"

namespace {

__device__ __forceinline__ int64_t gsx() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ int64_t gstride() { return (int64_t)gridDim.x * blockDim.x; }

// last chunk whose first row is <= row (empty chunks share the first row of the next one and are skipped by this rule)
__device__ int64_t us_find_chunk(const Utf8Chunk* ch, int64_t nch, int64_t row) {
    int64_t lo = 0, hi = nch;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ch[mid].row_start <= row) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

struct UsRow { const uint8_t* p; int32_t len; bool valid; };
__device__ __forceinline__ UsRow us_row(const Utf8SortArgs& a, uint32_t row) {
    const Utf8Chunk& c = a.chunks[a.nchunks > 1 ? us_find_chunk(a.chunks, a.nchunks, row) : 0];
    const int64_t e = (int64_t)row - c.row_start;
    int32_t b = c.offs[e], en = c.offs[e + 1];
    b = b < c.lo ? c.lo : (b > c.hi ? c.hi : b);
    en = en < b ? b : (en > c.hi ? c.hi : en);
    UsRow r;
    r.p = c.data + b;
    r.len = en - b;
    r.valid = !c.valid || ((c.valid[(c.valid_off + e) >> 3] >> ((c.valid_off + e) & 7)) & 1);
    return r;
}

__global__ void us_init_kernel(Utf8SortArgs a) {
    for (int64_t i = gsx(); i < a.n; i += gstride()) a.perm[i] = a.order_in ? a.order_in[i] : (uint32_t)i;
}

// one wave per round row; the first row of a segment has nothing to compare
__global__ __launch_bounds__(256) void us_lcp_kernel(Utf8SortArgs a) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = (gsx() >> 6); j < a.m; j += (gstride() >> 6)) {
        const uint32_t s = a.useg[j], f = a.sfirst[s];
        if ((uint32_t)j == f) continue;
        const UsRow r = us_row(a, a.perm[a.upos[j]]), q = us_row(a, a.perm[a.upos[f]]);
        const int32_t d = a.sdepth[s];
        int32_t cap = r.len - d;
        cap = q.len - d < cap ? q.len - d : cap;
        const int32_t known = __atomic_load_n(&a.slcp[s], __ATOMIC_RELAXED);
        cap = known < cap ? known : cap;
        if (cap < 0) cap = 0;
        int32_t lcp = cap;
        for (int32_t k = 0; k < cap; k += 64) {
            const int32_t i = k + lane;
            const bool diff = i < cap && r.p[d + i] != q.p[d + i];
            const unsigned long long b = __ballot(diff);
            if (b) { lcp = k + __ffsll((long long)b) - 1; break; }
        }
        if (lane == 0 && lcp < known) atomicMin(&a.slcp[s], lcp);
    }
}
__global__ void us_fold_kernel(Utf8SortArgs a) {
    for (int64_t s = gsx(); s < a.nseg; s += gstride()) {
        const int32_t l = a.slcp[s];
        if (l != kUtf8SortNoLcp) a.sdepth[s] += l;
    }
}

__global__ __launch_bounds__(256) void us_keys_kernel(Utf8SortArgs a) {
    uint64_t kmin = ~0ull, kmax = 0;
    for (int64_t j = gsx(); j < a.m; j += gstride()) {
        const UsRow r = us_row(a, a.perm[a.round0 ? (uint32_t)j : a.upos[j]]);
        const int32_t d = a.round0 ? 0 : a.sdepth[a.useg[j]];
        uint64_t w = 0;
        if (r.valid) {
            const int32_t left = r.len - d > 0 ? r.len - d : 0;
            const int32_t take = left < kUtf8SortWordBytes ? left : kUtf8SortWordBytes;
            for (int i = 0; i < take; ++i) w |= (uint64_t)r.p[d + i] << (56 - 8 * i);
            w |= (uint64_t)(left < 8 ? left : 8);
            if (a.descending) w = ~w;
            kmin = w < kmin ? w : kmin;
            kmax = w > kmax ? w : kmax;
        }
        a.word[j] = w;
        a.keys[j] = w;
        if (a.nullflags) a.nullflags[j] = r.valid ? 0 : 1;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t x = __shfl_xor(kmin, m, 64), y = __shfl_xor(kmax, m, 64);
        kmin = x < kmin ? x : kmin;
        kmax = y > kmax ? y : kmax;
    }
    if ((threadIdx.x & 63) == 0 && kmin <= kmax) {
        atomicMin((unsigned long long*)&a.bit_stats[0], (unsigned long long)kmin);
        atomicMax((unsigned long long*)&a.bit_stats[1], (unsigned long long)kmax);
    }
}

__global__ void us_seg_keys_kernel(Utf8SortArgs a) {
    for (int64_t t = gsx(); t < a.m; t += gstride()) a.keys[t] = a.useg[a.order ? a.order[t] : (uint32_t)t];
}

__global__ void us_gather_kernel(Utf8SortArgs a) {
    for (int64_t t = gsx(); t < a.m; t += gstride()) {
        const uint32_t j = a.order ? a.order[t] : (uint32_t)t;
        a.trow[t] = a.perm[a.round0 ? j : a.upos[j]];
        a.tword[t] = a.word[j];
        a.tseg[t] = a.round0 ? 0u : a.useg[j];
        a.tnull[t] = a.nullflags ? a.nullflags[j] : 0;
    }
}

__device__ __forceinline__ bool us_head(const Utf8SortArgs& a, int64_t t) {
    return t == 0 || a.tseg[t] != a.tseg[t - 1] || a.tword[t] != a.tword[t - 1] || a.tnull[t] != a.tnull[t - 1];
}
__global__ void us_mark_kernel(Utf8SortArgs a) {
    for (int64_t t = gsx(); t < a.m; t += gstride()) {
        a.perm[a.round0 ? (uint32_t)t : a.upos[t]] = a.trow[t];
        const uint64_t w = a.descending ? ~a.tword[t] : a.tword[t];
        const bool head = us_head(a, t);
        const bool alone = head && (t + 1 == a.m || us_head(a, t + 1));
        const bool go_on = !a.tnull[t] && (w & 0xFF) == 8 && !alone;
        a.fu[t] = go_on;
        a.fh[t] = go_on && head;
    }
}

__global__ void us_next_kernel(Utf8SortArgs a) {
    for (int64_t t = gsx(); t < a.m; t += gstride()) {
        if (!a.fu[t]) continue;
        const int64_t jn = a.su[t];
        const int64_t sn = a.fh[t] ? a.sh[t] : a.sh[t] - 1;
        a.nupos[jn] = a.round0 ? (uint32_t)t : a.upos[t];
        a.nuseg[jn] = (uint32_t)sn;
        if (a.fh[t]) {
            a.nsfirst[sn] = (uint32_t)jn;
            a.nsdepth[sn] = (a.round0 ? 0 : a.sdepth[a.tseg[t]]) + kUtf8SortWordBytes;
            a.slcp[sn] = kUtf8SortNoLcp;
        }
    }
}

unsigned us_grid(int64_t n, int threads) {
    const int64_t b = (n + threads - 1) / threads;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

}  // namespace

hipError_t launch_utf8_sort_init(const Utf8SortArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(us_init_kernel, dim3(us_grid(a.n, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_sort_lcp(const Utf8SortArgs& a, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(us_lcp_kernel, dim3(us_grid(a.m, 4)), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(us_fold_kernel, dim3(us_grid(a.nseg, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_sort_keys(const Utf8SortArgs& a, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(us_keys_kernel, dim3(us_grid(a.m, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_sort_seg_keys(const Utf8SortArgs& a, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(us_seg_keys_kernel, dim3(us_grid(a.m, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_sort_mark(const Utf8SortArgs& a, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(us_gather_kernel, dim3(us_grid(a.m, 256)), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(us_mark_kernel, dim3(us_grid(a.m, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_utf8_sort_next(const Utf8SortArgs& a, hipStream_t s) {
    if (a.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(us_next_kernel, dim3(us_grid(a.m, 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
