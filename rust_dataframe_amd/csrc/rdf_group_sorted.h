// rdf_group_sorted.h — argument blocks and launchers of the sorted GROUP BY's fold (kernels: rdf_group_sorted.hip, host
// side: rdf_capi_group_sorted.inc).  The window front (rdf_window.h) has sorted the rows by (grouping keys, value) and left
// the permutation, the scan of its partition / peer flags and the two start tables; what is here folds the HEAD LIST —
// one entry per distinct (group, value) pair — into one output row per group.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdf_device.h"
#include "rdf_utf8.h"

constexpr int kGrpThreads = 256;
constexpr int kGrpTile = RDF_GROUP_SORTED_TILE;     // items of one block's tile: one per thread
static_assert(kGrpTile == kGrpThreads, "one item per thread");

// What the fold carries per item and per segment.  A head is the state of its one pair; + joins two neighbours of a group:
//   cnt           distinct non-NULL values
//   sum           their sum: the bits of a double (Float32 / Float64 values) or of a wrapping 64-bit integer
//   lo_all        smallest row index;  hi_all  largest row index
//   lo_val        smallest row index whose value is not NULL, kGrpNone when there is none
//   hi_val        1 + the largest such row index, 0 when there is none  (rows < 2^32 - 1 keep both encodings apart)
struct GrpState {
    uint64_t sum;
    uint32_t cnt, lo_all, hi_all, lo_val, hi_val;
    uint32_t seg;        // the group the state belongs to
};
constexpr uint32_t kGrpNone = 0xFFFFFFFFu;

struct GrpCallOut { int32_t fn, ignore_nulls; void* values; uint8_t* vbytes; };

struct GrpFoldArgs {
    // level 0: the head list, read through the front's tables
    const int64_t*           scan;       // [n + 1] exclusive scan of the flags
    const uint32_t*          gstart;     // [D + 1] first sorted position of every pair, then n
    const uint32_t*          perm;       // sorted position -> row (nullptr = identity)
    const rdfk::DevChunkCol* vchunks;    // the value column's numeric chunks, or nullptr
    const Utf8Chunk*         vutf8;      // the value column's Utf8 chunks (validity only is read), or nullptr
    const int64_t*           row_start;  // [nchunks + 1]
    int64_t                  nchunks;
    int32_t                  vdtype;     // numeric value: rdf_dtype
    int32_t                  level;      // 0 = items are heads; > 0 = items are `in`
    // level > 0: the partials of the level below
    const GrpState*          in;         // [m]
    int64_t                  m;          // items of this level (level 0: D)
    GrpState*                part;       // [tiles][2] out: the tile's first and last segment; nullptr on the final level
    int64_t                  groups;     // G: no group index beyond it is written
    uint32_t*                group_rows; // [G] or nullptr
    int32_t                  ncalls, pad;
    GrpCallOut               calls[RDF_GROUP_MAX_CALLS];   // values: [G]; vbytes (FIRST / LAST with ignore_nulls): [G] 1 = valid
    unsigned long long*      nulls;      // [RDF_GROUP_MAX_CALLS], zeroed
};

// One level of the fold over a.m items; the caller chains levels (m -> 2 * ceil(m / kGrpTile)) until one tile is left.
hipError_t launch_grp_fold(const GrpFoldArgs& a, hipStream_t s);
inline int64_t grp_tiles(int64_t m) { return (m + kGrpTile - 1) / kGrpTile; }
