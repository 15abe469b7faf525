// rdf_window_range.h — what rdf_window_range_agg decides about ONE frame bound: the tile and window sizes, the frame checks,
// the bound arithmetic (Int64 and Float64 keys, ascending and descending) and the two searches over a partition's sorted
// keys (kernels: rdf_window_range.hip, host side: rdf_capi_window_range.inc).  ONE definition, __host__ __device__ inline:
// hipcc compiles it into the kernels, plain g++ compiles it into tests/cpp/test_window_range_host.cpp.  It includes nothing
// of HIP.
//
// A partition's sorted positions fall into three classes, in this order: LOW (NaN keys of a DESCENDING order: they sort
// before +inf), ORDINARY (a key that is neither NULL nor NaN), HIGH (NaN keys of an ascending order, then the NULLs).  A
// bound of an ordinary row with key o is the VALUE v = o + sgn * s (sgn = +1: the bound lies later in the sort direction's
// own key order, see wr_probe) and resolves to a position:
//   start   the first position that is HIGH or whose ordinary key is not before v in the sort direction
//   end     ONE PAST the last ordinary position whose key is not after v = the first position that is HIGH or whose
//           ordinary key is after v
// Both are "the first position where a predicate holds" and the predicate is monotone over the partition (LOW: false,
// HIGH: true), so both are one binary search that never needs the ordinary run's own ends: a start with no such key comes
// out one past the run, an end with none at the run's first position (an empty frame, representable at position 0).
// Integer bounds are compared exactly (no wrap): v itself is never formed, the unsigned distance of two ordered keys is
// compared with s.  Float64 bounds are ONE IEEE operation, fl(o - s) or fl(o + s), compared by IEEE < / > (-0.0 == +0.0);
// build with -ffp-contract=off.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RDF_WR_HD __host__ __device__ inline
#else
#define RDF_WR_HD inline
#endif

// Sizes (mirrored by _abi.WINDOW_RANGE_TILE / WINDOW_RANGE_LDS_KEYS).  A block of kWRangeThreads lanes owns kWRangeTile
// consecutive sorted positions.  A staged window holds kWRangeLdsKeys keys and class bytes: 4096 * 9 B = 36 KiB of the CU's
// 160 KiB of LDS, four blocks = 16 waves per CU, 4 per SIMD; the searches are latency bound, so waves matter more than a
// wider window (a window of 4 tiles covers every frame whose two ends lie within 1.5 tiles of the row on either side).
constexpr int kWRangeThreads = 256;
constexpr int kWRangePer = 4;
constexpr int kWRangeTile = kWRangeThreads * kWRangePer;   // 1024
constexpr int kWRangeLdsKeys = 4096;
constexpr int kWRangeMaxBounds = 16;                       // 8 calls, two ends each

enum : int { WR_ORDINARY = 0, WR_LOW = 1, WR_HIGH = 2 };   // class of a sorted position
enum : int { WR_ROUTE_AUTO = 0, WR_ROUTE_LDS = 1, WR_ROUTE_GLOBAL = 2 };   // (AUTO decides as LDS does today: a window that fits was never slower)

// rdf_frame_bound of include/rdf_mi355x.h, restated so that this header stands alone (rdf_capi_window_range.inc static_asserts)
enum : int { WR_UNBOUNDED_PRECEDING = 0, WR_PRECEDING = 1, WR_CURRENT_ROW = 2, WR_FOLLOWING = 3, WR_UNBOUNDED_FOLLOWING = 4 };

// ---------------------------------------------------------------- frame checks
enum : int { WR_FRAME_OK = 0, WR_FRAME_KIND, WR_FRAME_START_UF, WR_FRAME_END_UP, WR_FRAME_NEGATIVE, WR_FRAME_NOT_FINITE, WR_FRAME_ORDER };
RDF_WR_HD const char* wr_frame_error(int e) {
    switch (e) {
        case WR_FRAME_KIND: return "unknown frame bound";
        case WR_FRAME_START_UF: return "a frame cannot start at UNBOUNDED FOLLOWING";
        case WR_FRAME_END_UP: return "a frame cannot end at UNBOUNDED PRECEDING";
        case WR_FRAME_NEGATIVE: return "a frame offset cannot be negative";
        case WR_FRAME_NOT_FINITE: return "a Float64 frame offset must be finite";
        case WR_FRAME_ORDER: return "the frame starts after its end";
        default: return "";
    }
}
RDF_WR_HD bool wr_is_offset(int kind) { return kind == WR_PRECEDING || kind == WR_FOLLOWING; }
// The static rules of a frame.  Offsets are read only where the kind is PRECEDING / FOLLOWING: the integer pair for
// Int32 / Int64 order keys, the double pair for Float64 ones.
RDF_WR_HD int wr_check_frame(int start_kind, int end_kind, int64_t start_i, int64_t end_i, double start_f, double end_f, bool f64) {
    if (start_kind < WR_UNBOUNDED_PRECEDING || start_kind > WR_UNBOUNDED_FOLLOWING || end_kind < WR_UNBOUNDED_PRECEDING || end_kind > WR_UNBOUNDED_FOLLOWING)
        return WR_FRAME_KIND;
    if (start_kind == WR_UNBOUNDED_FOLLOWING) return WR_FRAME_START_UF;
    if (end_kind == WR_UNBOUNDED_PRECEDING) return WR_FRAME_END_UP;
    const bool so = wr_is_offset(start_kind), eo = wr_is_offset(end_kind);
    if (f64) {
        // (x - x != 0 for NaN and the infinities alone)
        if ((so && !(start_f - start_f == 0.0)) || (eo && !(end_f - end_f == 0.0))) return WR_FRAME_NOT_FINITE;
        if ((so && start_f < 0.0) || (eo && end_f < 0.0)) return WR_FRAME_NEGATIVE;
    } else if ((so && start_i < 0) || (eo && end_i < 0)) return WR_FRAME_NEGATIVE;
    if (start_kind > end_kind) return WR_FRAME_ORDER;
    if (start_kind == end_kind && so) {
        const bool less = f64 ? start_f < end_f : start_i < end_i, more = f64 ? start_f > end_f : start_i > end_i;
        if ((start_kind == WR_PRECEDING && less) || (start_kind == WR_FOLLOWING && more)) return WR_FRAME_ORDER;
    }
    return WR_FRAME_OK;
}

// ---------------------------------------------------------------- bound arithmetic
// One distinct offset bound of a request.
struct WRBound {
    int32_t  is_end;       // 0: a frame start, 1: a frame end (resolved one past)
    int32_t  following;    // 0: PRECEDING s, 1: FOLLOWING s
    uint64_t s_i;          // the offset of an integer key, >= 0
    double   s_f;          // the offset of a Float64 key, finite and >= 0
};
// What one row asks of the keys: the bound of `b` for the row whose key has the bits `o`.
struct WRProbe {
    int32_t  f64, desc, is_end, up;   // up: v lies above o in KEY order (FOLLOWING ascending, PRECEDING descending)
    uint64_t o, s;                    // integer keys: o's bits and the offset
    double   v;                       // Float64 keys: fl(o + s) or fl(o - s)
};
RDF_WR_HD double wr_f64_of(uint64_t bits) { union { uint64_t u; double d; } x; x.u = bits; return x.d; }
RDF_WR_HD uint64_t wr_bits_of(double d) { union { uint64_t u; double d; } x; x.d = d; return x.u; }
RDF_WR_HD WRProbe wr_probe(const WRBound& b, bool f64, bool desc, uint64_t o) {
    WRProbe p;
    p.f64 = f64;
    p.desc = desc;
    p.is_end = b.is_end;
    p.up = (b.following != 0) != desc;
    p.o = o;
    p.s = b.s_i;
    p.v = 0.0;
    if (f64) p.v = p.up ? wr_f64_of(o) + b.s_f : wr_f64_of(o) - b.s_f;   // one IEEE operation
    return p;
}
// The sign of key - v in exact arithmetic.  Integer keys: two's complement bits; v = o + s or o - s is never formed.
RDF_WR_HD int wr_cmp_int(uint64_t key, uint64_t o, bool up, uint64_t s) {
    const bool below = (int64_t)key < (int64_t)o;
    if (up) {                                         // v = o + s >= o
        if (below) return -1;
        const uint64_t d = key - o;                   // key >= o: the distance, exact in 64 unsigned bits
        return d < s ? -1 : d > s ? 1 : 0;
    }
    if (!below && key != o) return 1;                 // v = o - s <= o < key
    const uint64_t d = o - key;                       // key <= o
    return d < s ? 1 : d > s ? -1 : 0;
}
RDF_WR_HD int wr_cmp(const WRProbe& p, uint64_t key) {
    if (p.f64) { const double k = wr_f64_of(key); return k < p.v ? -1 : k > p.v ? 1 : 0; }
    return wr_cmp_int(key, p.o, p.up != 0, p.s);
}
// Does the predicate of the bound hold at a position of class `cls` with key bits `key`?
RDF_WR_HD bool wr_holds(const WRProbe& p, int cls, uint64_t key) {
    if (cls != WR_ORDINARY) return cls == WR_HIGH;
    const int c = p.desc ? -wr_cmp(p, key) : wr_cmp(p, key);   // > 0: the key lies after v in the sort direction
    return p.is_end ? c > 0 : c >= 0;
}

// ---------------------------------------------------------------- the searches
// The first position of [lo, hi) where the predicate holds, hi when it holds nowhere.  `K` answers cls(j) and key(j) for
// lo <= j < hi and nothing else is read.
template <class K> RDF_WR_HD int64_t wr_first(const K& keys, int64_t lo, int64_t hi, const WRProbe& p) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (wr_holds(p, keys.cls(mid), keys.key(mid))) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// A frame START of the row: the first position of the partition [ps, pe) that is not before the bound.
template <class K> RDF_WR_HD int64_t wr_search_start(const K& keys, int64_t ps, int64_t pe, const WRBound& b, bool f64, bool desc, uint64_t o) {
    WRBound s = b;
    s.is_end = 0;
    return wr_first(keys, ps, pe, wr_probe(s, f64, desc, o));
}
// A frame END of the row, ONE PAST: the first position of [ps, pe) that is after the bound.
template <class K> RDF_WR_HD int64_t wr_search_end(const K& keys, int64_t ps, int64_t pe, const WRBound& b, bool f64, bool desc, uint64_t o) {
    WRBound e = b;
    e.is_end = 1;
    return wr_first(keys, ps, pe, wr_probe(e, f64, desc, o));
}

// ---------------------------------------------------------------- argument blocks and launchers (hipcc only)
#if defined(__HIPCC__)
#include "rdf_window.h"

// The sorted key pass: skey[j] / scls[j] = key bits (Int32 sign-extended) and class of sorted position j.
struct WRangeKeyArgs {
    const uint32_t* perm;               // sorted position -> row (nullptr = identity)
    const rdfk::DevChunkCol* chunks;    // the order key, one descriptor per chunk
    const int64_t*  row_start;          // [nchunks + 1]
    int64_t         nchunks, n;
    int32_t         dtype, desc;        // RDF_I32 / RDF_I64 / RDF_F64; the order is descending
    uint64_t*       skey;               // [n]
    uint8_t*        scls;               // [n]
};
// The bounds pass: out[b][j] = the position bound b resolves to for sorted position j, relative to the partition's start
// (ends ONE PAST).  window[t] = the sorted positions [x, y) the searches of tile t can read; used[0] / used[1] become 1 when
// a tile takes the LDS / the global route.
struct WRangeBoundsArgs {
    const int64_t*  scan;
    const uint32_t* pstart;
    const uint32_t* gstart;
    const uint64_t* skey;
    const uint8_t*  scls;
    int64_t         n;
    int32_t         f64, desc, nbounds, route;
    WRBound         bounds[kWRangeMaxBounds];
    uint32_t*       out[kWRangeMaxBounds];
    uint2*          window;             // [tiles]
    uint32_t*       used;               // [2], zeroed
};
hipError_t launch_wrange_keys(const WRangeKeyArgs& a, hipStream_t s);
hipError_t launch_wrange_bounds(const WRangeBoundsArgs& a, hipStream_t s);   // window pass, LDS-route tiles, global-route tiles
#endif
