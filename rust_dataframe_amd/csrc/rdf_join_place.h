// rdf_join_place.h — where the distinct build keys of an equi-join land in the probe table when the build side arrives sorted by
// hash (rdf_join.hip: join_place_kernel / join_place_scan_kernel; rdf_capi_join.inc: rdf_equijoin_indices_multi).  Linear probing
// over keys that come in home-slot order is a scan: slot(r) = max(home(r), slot(r - 1) + 1) = r + max over q <= r of (home(q) - q).
// A run of consecutive distinct keys is summarised by {c = how many, m = max(home(q) - q) with q counted from the run's start};
// two adjacent runs combine associatively, so tiles are summarised independently, one block scans the tiles' summaries, and every
// tile places its keys from the prefix in front of it.  Shared by the kernels and a CPU test (tests/cpp/test_join_place.cpp) that
// holds the combination to the sequential rule it replaces.  No HIP types in here.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RDF_PLACE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RDF_PLACE_HD inline
#endif

namespace rdfk {

constexpr long long kPlaceNone = -(1ll << 62);             // m of an empty run
struct PlaceCM { long long c, m; };
RDF_PLACE_HD PlaceCM place_empty() { PlaceCM r; r.c = 0; r.m = kPlaceNone; return r; }
// run a, then run b: b's keys are counted from a.c on, so their (home - index) values drop by a.c
RDF_PLACE_HD PlaceCM place_join(PlaceCM a, PlaceCM b) { PlaceCM r; r.c = a.c + b.c; const long long bm = b.m - a.c; r.m = a.m > bm ? a.m : bm; return r; }
// one more distinct key with home slot `home` behind run a; returns the slot it takes
RDF_PLACE_HD long long place_push(PlaceCM& a, long long home) {
    const long long g = home - a.c;
    a.m = g > a.m ? g : a.m;
    return a.c++ + a.m;
}
// slot of the last key of a non-empty prefix a (absolute: a counted from the first key of all)
RDF_PLACE_HD long long place_last(PlaceCM a) { return a.c > 0 ? a.c - 1 + a.m : -1; }

// ---- how large the host makes the two lookups (rdf_capi_join.inc), over `rows` sorted non-NULL build keys in [kmin, kmax] ----
// The table holds the DISTINCT build keys: no more of them than rows, and no more than the key range spans — a build side of 1e8
// rows over a few dozen dictionary codes gets a table of 1024 slots, not 2e8 whose empty stretches a few lanes would have to write
// one slot after another (the placement fills the gaps in front of its keys itself).
constexpr int       kJoinTableMinBits = 10;
constexpr long long kJoinTableMargin  = 1ll << 16;   // no wrap-around: the last home slot's cluster runs into the margin
constexpr long long kJoinCountFrom    = 65536;       // build rows from which a wide key range has its distinct keys counted
RDF_PLACE_HD bool join_range_bounds_keys(long long rows, uint64_t kmin, uint64_t kmax) { return kmax >= kmin && kmax - kmin < (uint64_t)rows; }
// ... and a few keys spread over a WIDE range (hashed identifiers, 37 of them over 3e6 rows): the sorted build side is read once
// more to COUNT its distinct keys (join_distinct_kernel) — sized from the rows, the few lanes in front of such keys wrote millions
// of empty slots one by one
RDF_PLACE_HD bool join_table_counts_keys(long long rows, uint64_t kmin, uint64_t kmax) { return !join_range_bounds_keys(rows, kmin, kmax) && rows >= kJoinCountFrom; }
struct JoinTablePlan { long long nd; int tbits; long long cap; };     // distinct keys at most, 2^tbits home slots, slots in all
// counted = the distinct keys join_distinct_kernel found, 0 = not counted; load <= 0.5: tbits = the smallest >= 10 with 2^tbits >= 2 nd
RDF_PLACE_HD JoinTablePlan join_table_plan(long long rows, uint64_t kmin, uint64_t kmax, uint64_t counted) {
    JoinTablePlan p;
    p.nd = rows;
    if (join_range_bounds_keys(rows, kmin, kmax)) p.nd = (long long)(kmax - kmin) + 1;
    else if (counted > 0 && (long long)counted < p.nd) p.nd = (long long)counted;
    p.tbits = kJoinTableMinBits;
    while ((1ll << p.tbits) < 2 * p.nd) ++p.tbits;
    p.cap = (1ll << p.tbits) + kJoinTableMargin;
    return p;
}
// bucket index: about one bucket per build row (a power of two, 2^24 at most), on the top bits of (key - kmin): the smallest shift
// that brings kmax - kmin below the bucket count.  One bucket over the whole 64-bit range would need a shift of 64, which is what this
// returns without shifting by it; the host never asks for that (one bucket = at most one key = a range of 0).  kmax < kmin: no keys.
constexpr long long kJoinMaxBuckets = 1ll << 24;
struct JoinBucketPlan { long long nbuckets; int shift; };
RDF_PLACE_HD JoinBucketPlan join_bucket_plan(long long rows, uint64_t kmin, uint64_t kmax) {
    JoinBucketPlan p;
    p.nbuckets = 1;
    while (p.nbuckets < rows && p.nbuckets < kJoinMaxBuckets) p.nbuckets <<= 1;
    p.shift = 0;
    if (kmax >= kmin) while (p.shift < 64 && ((kmax - kmin) >> p.shift) >= (uint64_t)p.nbuckets) ++p.shift;
    return p;
}

}  // namespace rdfk
