// rdf_window_agg.hip — the kernels of the window frame aggregates (sum / min / max / count / avg / first_value / last_value
// over rows_between and range_between; host side: rdf_capi_window_agg.inc, argument blocks: rdf_window_agg.h).
//
// rdf_window's front has ordered the rows and numbered partitions and peer groups (rdf_window.hip).  On top of it:
//   scan   one segmented inclusive scan per (value column, payload): a lane gathers its four consecutive sorted positions'
//          values THROUGH the permutation — the one random 8-byte read per row and column — and the scan runs over the
//          (restart flag, payload) monoid  (f1,p1) o (f2,p2) = (f1|f2, f2 ? p2 : p1 (+) p2).  Three launches like launch_scan:
//          every block scans a 4096-position segment, one block folds the segments' aggregates, a third pass adds the fold of
//          the segments before to the positions ahead of a segment's first restart.  No block waits on another.
//          A backward scan is the same scan over the mirrored index (position n - 1 - i), restarting at the ends.
//   emit   a lane per sorted position has k, n, f, l from rdf_window's scan words and start tables, resolves every call's
//          frame [a, b], reads the scans at the two positions and writes value and valid byte to out[row].
// Float64 sums are carried as double-doubles.  The error-free transformations below (TwoSum, FastTwoSum) are only error-free
// when every operation is one IEEE operation in the order written: the library is built with -ffp-contract=off and without
// fast-math (see the Makefile), and must stay so.
#include "rdf_window_agg.h"
#include "rdf_common.hip.h"

using namespace rdfk;

namespace {

constexpr uint64_t kSign = 0x8000000000000000ull;
constexpr uint64_t kQuietNaN = 0x7FF8000000000000ull;
constexpr uint64_t kInfBits = 0x7FF0000000000000ull;

template <int K> struct Pay { uint64_t w[wagg_words(K)]; };

__device__ __forceinline__ double bits_f64(uint64_t b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ uint64_t f64_bits(double d) { return (uint64_t)__double_as_longlong(d); }

// Knuth's TwoSum: s + e == a + b exactly, s = fl(a + b).  Dekker's FastTwoSum needs |a| >= |b| (or a == 0).
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
__device__ __forceinline__ void fast_two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    e = b - (s - a);
}
// The "accurate" double-word addition (TwoSum on both words, two renormalisations): relative error <= 3u^2 + 13u^3, u = 2^-53.
__device__ __forceinline__ void dd_add(double xh, double xl, double yh, double yl, double& zh, double& zl) {
    double sh, sl, th, tl, vh, vl;
    two_sum(xh, yh, sh, sl);
    two_sum(xl, yl, th, tl);
    const double c = sl + th;
    fast_two_sum(sh, c, vh, vl);
    const double w = tl + vl;
    fast_two_sum(vh, w, zh, zl);
}

template <int K> __device__ __forceinline__ Pay<K> identity(int ismax) {
    Pay<K> p;
#pragma unroll
    for (int i = 0; i < wagg_words(K); ++i) p.w[i] = 0;
    if (K == kWaggExt && !ismax) p.w[0] = ~0ull;
    return p;
}
// left (+) right, left the earlier positions in scan order
template <int K> __device__ __forceinline__ Pay<K> combine(const Pay<K>& l, const Pay<K>& r, int ismax) {
    Pay<K> o;
    if constexpr (K == kWaggSumF) {
        double zh, zl;
        dd_add(bits_f64(l.w[0]), bits_f64(l.w[1]), bits_f64(r.w[0]), bits_f64(r.w[1]), zh, zl);
        o.w[0] = f64_bits(zh);
        o.w[1] = f64_bits(zl);
        o.w[2] = l.w[2] + r.w[2];
        o.w[3] = l.w[3] + r.w[3];
    } else if constexpr (K == kWaggSumI) {
        o.w[0] = l.w[0] + r.w[0];
        o.w[1] = l.w[1] + r.w[1];
    } else {
        o.w[0] = ismax ? (l.w[0] > r.w[0] ? l.w[0] : r.w[0]) : (l.w[0] < r.w[0] ? l.w[0] : r.w[0]);
    }
    return o;
}
template <int K> __device__ __forceinline__ Pay<K> shfl_up_pay(const Pay<K>& p, int d) {
    Pay<K> o;
#pragma unroll
    for (int i = 0; i < wagg_words(K); ++i) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)p.w[i], d), hi = (uint32_t)__shfl_up((int)(uint32_t)(p.w[i] >> 32), d);
        o.w[i] = ((uint64_t)hi << 32) | lo;
    }
    return o;
}

// The order-preserving image of a value: IEEE total order for Float64 (-0.0 < +0.0), two's complement order for Int64.
__device__ __forceinline__ uint64_t ext_image(uint64_t bits, int f64) {
    if (f64 && (bits & kSign)) return ~bits;
    return bits ^ kSign;
}
__device__ __forceinline__ uint64_t ext_value(uint64_t image, int f64) {
    if (f64 && !(image & kSign)) return ~image;
    return image ^ kSign;
}
// An absent row is the fold's identity.  A Float64 NaN is the word next to it — every non-NaN image lies strictly between
// 0x000FFFFFFFFFFFFF (-inf) and 0xFFF0000000000000 (+inf) — so a frame of NaNs only is told from a frame of NULLs only.
__device__ __forceinline__ uint64_t ext_nan(int ismax) { return ismax ? 1ull : ~0ull - 1; }

// The payload of sorted position j.
template <int K> __device__ __forceinline__ Pay<K> wagg_load(const WaggScanArgs& a, double inv, int64_t j) {
    const int64_t row = a.perm ? (int64_t)a.perm[j] : j;
    int64_t c = 0, start = 0;
    if (a.nchunks > 1) { c = find_chunk_row(a.row_start, a.nchunks, row, inv); start = a.row_start[c]; }
    const DevChunkCol cc = a.chunks[c];
    const int64_t e = cc.offset + row - start;
    const bool valid = cc.validity ? ((cc.validity[e >> 3] >> (e & 7)) & 1) : true;
    Pay<K> p = identity<K>(a.ismax);
    if (!valid) return p;
    const uint64_t bits = as_global<uint64_t>(cc.values)[e];
    if constexpr (K == kWaggSumF) {
        const double x = a.f64 ? bits_f64(bits) : (double)(int64_t)bits;
        const uint64_t xb = f64_bits(x), mag = xb & ~kSign;
        p.w[2] = 1ull << 32;
        if (mag > kInfBits) p.w[2] |= 1;                       // NaN
        else if (mag == kInfBits) p.w[3] = (xb & kSign) ? 1ull : 1ull << 32;
        else p.w[0] = xb;
    } else if constexpr (K == kWaggSumI) {
        p.w[0] = bits;
        p.w[1] = 1ull << 32;
    } else {
        const bool nan = a.f64 && (bits & ~kSign) > kInfBits;
        p.w[0] = nan ? ext_nan(a.ismax) : ext_image(bits, a.f64);
    }
    return p;
}

// Does the scan restart at sorted position j (a backward scan: is j the last position of its run)?
__device__ __forceinline__ bool wagg_flag(const WaggScanArgs& a, int64_t j) {
    const uint64_t ex = (uint64_t)a.scan[j], inc = (uint64_t)a.scan[j + 1];
    if (a.restart == kWaggRestartPeer) return (uint32_t)inc != (uint32_t)ex;
    if (a.restart == kWaggRestartPartition) {
        if (!a.backward) return (inc >> 32) != (ex >> 32);
        return j == a.n - 1 || ((uint64_t)a.scan[j + 2] >> 32) != (inc >> 32);
    }
    const uint32_t pid = (uint32_t)(inc >> 32) - 1;
    const uint32_t ps = a.pstart[pid], k = (uint32_t)j - ps;
    if (!a.backward) return k % a.w == 0;
    return k % a.w == a.w - 1 || (uint32_t)j == a.pstart[(int64_t)pid + 1] - 1;
}

// Inclusive segmented scan of one (flag, payload) per thread over the block.  Returns the EXCLUSIVE result of the thread
// (flag false and the identity for thread 0) and the fold of the whole block in (tf, tp).
template <int K> __device__ __forceinline__ void block_seg_scan(bool f, const Pay<K>& p, int ismax, bool* lds_f, Pay<K>* lds_p,
                                                                bool& ef, Pay<K>& ep, bool& tf, Pay<K>& tp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool fi = f;
    Pay<K> pi = p;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const bool of = __shfl_up((int)fi, d) != 0;
        const Pay<K> op = shfl_up_pay<K>(pi, d);
        if (lane >= d) {
            if (!fi) pi = combine<K>(op, pi, ismax);
            fi = fi || of;
        }
    }
    __syncthreads();                                           // the arrays may still be read from a call before
    if (lane == 63) { lds_f[wave] = fi; lds_p[wave] = pi; }
    __syncthreads();
    bool wf = false;                                           // the fold of the waves before this one, and of all of them
    Pay<K> wp = identity<K>(ismax);
    tf = false;
    tp = identity<K>(ismax);
    for (int w = 0; w < kWaggThreads / 64; ++w) {
        const bool xf = lds_f[w];
        const Pay<K> xp = lds_p[w];
        tp = xf ? xp : combine<K>(tp, xp, ismax);
        tf = tf || xf;
        if (w + 1 == wave) { wf = tf; wp = tp; }
    }
    bool lf = __shfl_up((int)fi, 1) != 0;                      // the lanes before this one, inside the wave
    Pay<K> lp = shfl_up_pay<K>(pi, 1);
    if (lane == 0) { lf = false; lp = identity<K>(ismax); }
    ef = lf || wf;
    ep = lf ? lp : combine<K>(wp, lp, ismax);
}

template <int K> __global__ __launch_bounds__(kWaggThreads) void wagg_scan_segments_kernel(const WaggScanArgs a) {
    __shared__ bool lds_f[kWaggThreads / 64];
    __shared__ Pay<K> lds_p[kWaggThreads / 64];
    __shared__ uint32_t first;
    if (threadIdx.x == 0) first = kWaggSeg;
    __syncthreads();
    const double inv = chunk_lookup_scale(a.row_start, a.nchunks);
    const int64_t base = (int64_t)blockIdx.x * kWaggSeg + (int64_t)threadIdx.x * kWaggPer;
    bool fl[kWaggPer], seen = false;
    Pay<K> r[kWaggPer];
    Pay<K> run = identity<K>(a.ismax);
    uint32_t myfirst = kWaggSeg;
#pragma unroll
    for (int q = 0; q < kWaggPer; ++q) {
        const int64_t i = base + q;
        fl[q] = false;
        r[q] = run;
        if (i < a.n) {
            const int64_t j = a.backward ? a.n - 1 - i : i;
            const bool f = wagg_flag(a, j);
            const Pay<K> p = wagg_load<K>(a, inv, j);
            run = f ? p : combine<K>(run, p, a.ismax);
            if (f && !seen) myfirst = (uint32_t)(threadIdx.x * kWaggPer + q);
            seen = seen || f;
            fl[q] = seen;
            r[q] = run;
        }
    }
    if (myfirst < kWaggSeg) atomicMin(&first, myfirst);
    bool ef, tf;
    Pay<K> ep, tp;
    block_seg_scan<K>(seen, run, a.ismax, lds_f, lds_p, ef, ep, tf, tp);
#pragma unroll
    for (int q = 0; q < kWaggPer; ++q) {
        const int64_t i = base + q;
        if (i >= a.n) break;
        const int64_t j = a.backward ? a.n - 1 - i : i;
        const Pay<K> v = fl[q] ? r[q] : combine<K>(ep, r[q], a.ismax);
#pragma unroll
        for (int x = 0; x < wagg_words(K); ++x) a.out[x][j] = v.w[x];
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int x = 0; x < wagg_words(K); ++x) a.seg[x][blockIdx.x] = tp.w[x];
        a.seg_first[blockIdx.x] = first;                       // (block_seg_scan's barriers order every atomicMin before this read)
    }
}

// seg[s] becomes the fold of the segments 0 .. s under the same monoid: what segment s + 1 carries in.
template <int K> __global__ __launch_bounds__(kWaggThreads) void wagg_scan_totals_kernel(const WaggScanArgs a, int64_t nseg) {
    __shared__ bool lds_f[kWaggThreads / 64];
    __shared__ Pay<K> lds_p[kWaggThreads / 64];
    Pay<K> carry = identity<K>(a.ismax);
    for (int64_t b = 0; b < nseg; b += kWaggThreads) {
        const int64_t s = b + threadIdx.x;
        bool f = false;
        Pay<K> p = identity<K>(a.ismax);
        if (s < nseg) {
            f = a.seg_first[s] < (uint32_t)kWaggSeg;
#pragma unroll
            for (int x = 0; x < wagg_words(K); ++x) p.w[x] = a.seg[x][s];
        }
        bool ef, tf;
        Pay<K> ep, tp;
        block_seg_scan<K>(f, p, a.ismax, lds_f, lds_p, ef, ep, tf, tp);
        if (s < nseg) {
            Pay<K> v = f ? p : combine<K>(ep, p, a.ismax);     // inclusive inside this round
            if (!(f || ef)) v = combine<K>(carry, v, a.ismax);
#pragma unroll
            for (int x = 0; x < wagg_words(K); ++x) a.seg[x][s] = v.w[x];
        }
        carry = tf ? tp : combine<K>(carry, tp, a.ismax);
    }
}

template <int K> __global__ __launch_bounds__(kWaggThreads) void wagg_scan_add_kernel(const WaggScanArgs a) {
    const int64_t s = (int64_t)blockIdx.x + 1;                 // segment 0 carries nothing in
    const uint32_t first = a.seg_first[s];
    const uint32_t local = threadIdx.x * kWaggPer;
    if (local >= first) return;
    Pay<K> carry;
#pragma unroll
    for (int x = 0; x < wagg_words(K); ++x) carry.w[x] = a.seg[x][s - 1];
#pragma unroll
    for (int q = 0; q < kWaggPer; ++q) {
        const int64_t i = s * kWaggSeg + local + q;
        if (local + q >= first || i >= a.n) break;
        const int64_t j = a.backward ? a.n - 1 - i : i;
        Pay<K> v;
#pragma unroll
        for (int x = 0; x < wagg_words(K); ++x) v.w[x] = a.out[x][j];
        v = combine<K>(carry, v, a.ismax);
#pragma unroll
        for (int x = 0; x < wagg_words(K); ++x) a.out[x][j] = v.w[x];
    }
}

// One call's answer for the row at sorted position j (k of n in its partition, peers f .. l).  -> the result is valid.
// kBounds: the frame's offset ends are not positions but were resolved from the order key's values into rb's arrays
// (rdf_window_range.hip): start[j] the first position of the frame, endx[j] one past its last, both inside the partition.
template <bool kBounds>
__device__ __forceinline__ bool wagg_emit_call(const WaggEmitArgs& a, const WaggCallOut& o, const uint32_t* rstart, const uint32_t* rendx,
                                               int64_t ps, int64_t k, int64_t n, int64_t f, int64_t l, int64_t row) {
    int64_t fa, fb;                                     // the frame [fa, fb] in positions of the partition
    if constexpr (kBounds) {
        fa = rstart ? (int64_t)rstart[ps + k] : o.start_kind == RDF_BOUND_UNBOUNDED_PRECEDING ? 0 : f;
        fb = rendx ? (int64_t)rendx[ps + k] - 1 : o.end_kind == RDF_BOUND_UNBOUNDED_FOLLOWING ? n - 1 : l;
    } else {
        const bool range = o.unit == RDF_FRAME_RANGE;
        switch (o.start_kind) {
            case RDF_BOUND_UNBOUNDED_PRECEDING: fa = 0; break;
            case RDF_BOUND_PRECEDING: fa = k - o.start; break;
            case RDF_BOUND_CURRENT_ROW: fa = range ? f : k; break;
            default: fa = k + o.start;
        }
        switch (o.end_kind) {
            case RDF_BOUND_UNBOUNDED_FOLLOWING: fb = n - 1; break;
            case RDF_BOUND_PRECEDING: fb = k - o.end; break;
            case RDF_BOUND_CURRENT_ROW: fb = range ? l : k; break;
            default: fb = k + o.end;
        }
        fa = fa < 0 ? 0 : fa;
        fb = fb > n - 1 ? n - 1 : fb;
    }
    const bool some = fa <= fb;
    const int64_t ja = (int64_t)ps + fa, jb = (int64_t)ps + fb;   // read only when `some`
    // the frame's packed counts: valid << 32 | NaN, +inf << 32 | -inf (differences of prefixes of one partition:
    // no half ever borrows)
    uint64_t c1 = 0, c2 = 0;
    if (some && o.sum[2]) {
        c1 = o.sum[2][jb] - (fa > 0 ? o.sum[2][ja - 1] : 0);
        if (o.sum[3]) c2 = o.sum[3][jb] - (fa > 0 ? o.sum[3][ja - 1] : 0);
    }
    const uint32_t cnt = (uint32_t)(c1 >> 32);
    bool ok = true;
    switch (o.fn) {
        case RDF_WAGG_COUNT:
            as_global_mut<int64_t>(o.values)[row] = o.sum[2] ? (int64_t)cnt : (some ? fb - fa + 1 : 0);
            break;
        case RDF_WAGG_FIRST_VALUE: case RDF_WAGG_LAST_VALUE: {
            ok = some;
            uint32_t v = 0;
            if (ok) { const int64_t jj = o.fn == RDF_WAGG_FIRST_VALUE ? ja : jb; v = a.perm ? a.perm[jj] : (uint32_t)jj; }
            as_global_mut<uint32_t>(o.values)[row] = v;
            break;
        }
        case RDF_WAGG_SUM: case RDF_WAGG_AVG: {
            ok = cnt > 0;
            uint64_t out = 0;
            if (ok && o.sum[1]) {                       // the double-double path
                const uint32_t nan = (uint32_t)c1, pinf = (uint32_t)(c2 >> 32), ninf = (uint32_t)c2;
                double s;
                if (nan || (pinf && ninf)) s = bits_f64(kQuietNaN);
                else if (pinf || ninf) s = bits_f64(pinf ? kInfBits : kInfBits | kSign);
                else {
                    double zh = bits_f64(o.sum[0][jb]), zl = bits_f64(o.sum[1][jb]);
                    if (fa > 0) dd_add(zh, zl, -bits_f64(o.sum[0][ja - 1]), -bits_f64(o.sum[1][ja - 1]), zh, zl);
                    s = zh == 0.0 ? 0.0 : zh;           // normalised: zh is the one rounding of the pair; a zero is +0.0
                }
                if (o.fn == RDF_WAGG_AVG) s = s / (double)cnt;
                out = f64_bits(s);
            } else if (ok) {
                out = o.sum[0][jb] - (fa > 0 ? o.sum[0][ja - 1] : 0);
            }
            as_global_mut<uint64_t>(o.values)[row] = out;
            break;
        }
        default: {                                      // MIN / MAX
            const int ismax = o.fn == RDF_WAGG_MAX;
            uint64_t m = ismax ? 0ull : ~0ull;
            if (some) {
                if (o.ext_mode == kWaggExtForward) m = o.fwd[jb];
                else if (o.ext_mode == kWaggExtBackward) m = o.bwd[ja];
                else if (fa / o.w != fb / o.w) {
                    const uint64_t x = o.fwd[jb], y = o.bwd[ja];
                    m = ismax ? (x > y ? x : y) : (x < y ? x : y);
                } else m = fa % o.w == 0 ? o.fwd[jb] : o.bwd[ja];
            }
            uint64_t out = 0;
            if (o.f64) {
                ok = m != (ismax ? 0ull : ~0ull);
                if (ok) out = m == ext_nan(ismax) ? kQuietNaN : ext_value(m, 1);
            } else {
                ok = cnt > 0;                           // a genuine INT64_MAX / INT64_MIN equals the identity: the count decides
                if (ok) out = ext_value(m, 0);
            }
            as_global_mut<uint64_t>(o.values)[row] = out;
        }
    }
    if (o.vbytes) o.vbytes[row] = ok ? 1 : 0;
    return ok;
}

template <bool kBounds, int C>
__device__ __forceinline__ void wagg_emit_calls(const WaggEmitArgs& a, const WaggRangeBounds* rb, int64_t ps, int64_t k, int64_t n, int64_t f, int64_t l,
                                                int64_t row, unsigned int (&nulls)[RDF_WINDOW_MAX_CALLS]) {
    if constexpr (C < RDF_WINDOW_MAX_CALLS) {
        if (C >= a.ncalls) return;
        const uint32_t* rstart = nullptr;
        const uint32_t* rendx = nullptr;
        if constexpr (kBounds) { rstart = rb->start[C]; rendx = rb->endx[C]; }
        nulls[C] += wagg_emit_call<kBounds>(a, a.calls[C], rstart, rendx, ps, k, n, f, l, row) ? 0u : 1u;
        wagg_emit_calls<kBounds, C + 1>(a, rb, ps, k, n, f, l, row, nulls);
    }
}
template <int C> __device__ __forceinline__ void wagg_emit_nulls(const WaggEmitArgs& a, const unsigned int (&nulls)[RDF_WINDOW_MAX_CALLS]) {
    if constexpr (C < RDF_WINDOW_MAX_CALLS) {
        if (C >= a.ncalls) return;
        unsigned int v = nulls[C];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += (unsigned int)__shfl_xor((int)v, m);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&a.nulls[C], (unsigned long long)v);
        wagg_emit_nulls<C + 1>(a, nulls);
    }
}

template <bool kBounds> __device__ __forceinline__ void wagg_emit_rows(const WaggEmitArgs& a, const WaggRangeBounds* rb) {
    unsigned int nulls[RDF_WINDOW_MAX_CALLS] = {};
    for (int64_t j = (int64_t)blockIdx.x * kWinThreads + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * kWinThreads) {
        const uint64_t inc = (uint64_t)a.scan[j + 1];
        const uint32_t pid = (uint32_t)(inc >> 32) - 1, gid = (uint32_t)inc - 1;
        const uint32_t ps = a.pstart[pid], pe = a.pstart[(int64_t)pid + 1];
        const uint32_t gs = a.gstart[gid], ge = a.gstart[(int64_t)gid + 1];
        const int64_t row = a.perm ? (int64_t)a.perm[j] : j;
        wagg_emit_calls<kBounds, 0>(a, rb, (int64_t)ps, (int64_t)j - ps, (int64_t)pe - ps, (int64_t)gs - ps, (int64_t)ge - 1 - ps, row, nulls);
    }
    wagg_emit_nulls<0>(a, nulls);
}
__global__ __launch_bounds__(kWinThreads) void wagg_emit_kernel(const WaggEmitArgs a) { wagg_emit_rows<false>(a, nullptr); }
// rdf_window_range_agg's form: frames whose offset ends come from the bounds arrays
__global__ __launch_bounds__(kWinThreads) void wagg_emit_range_kernel(const WaggEmitArgs a, const WaggRangeBounds rb) { wagg_emit_rows<true>(a, &rb); }

template <int K> hipError_t launch_scan_kind(const WaggScanArgs& a, hipStream_t s) {
    const int64_t nseg = (a.n + kWaggSeg - 1) / kWaggSeg;
    hipLaunchKernelGGL(wagg_scan_segments_kernel<K>, dim3((unsigned)nseg), dim3(kWaggThreads), 0, s, a);
    if (nseg > 1) {
        hipLaunchKernelGGL(wagg_scan_totals_kernel<K>, dim3(1), dim3(kWaggThreads), 0, s, a, nseg);
        hipLaunchKernelGGL(wagg_scan_add_kernel<K>, dim3((unsigned)(nseg - 1)), dim3(kWaggThreads), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_wagg_scan(int kind, const WaggScanArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    switch (kind) {
        case kWaggSumF: return launch_scan_kind<kWaggSumF>(a, s);
        case kWaggSumI: return launch_scan_kind<kWaggSumI>(a, s);
        default: return launch_scan_kind<kWaggExt>(a, s);
    }
}
hipError_t launch_wagg_emit(const WaggEmitArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int64_t want = (a.n + kWinThreads - 1) / kWinThreads, lim = (int64_t)eval_grid_limit();
    hipLaunchKernelGGL(wagg_emit_kernel, dim3((unsigned)(want > lim ? lim : want)), dim3(kWinThreads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_wagg_emit_range(const WaggEmitArgs& a, const WaggRangeBounds& rb, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int64_t want = (a.n + kWinThreads - 1) / kWinThreads, lim = (int64_t)eval_grid_limit();
    hipLaunchKernelGGL(wagg_emit_range_kernel, dim3((unsigned)(want > lim ? lim : want)), dim3(kWinThreads), 0, s, a, rb);
    return hipGetLastError();
}
