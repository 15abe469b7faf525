// rdf_collect.h — argument blocks and launchers of collect_list / collect_set per group and of explode (kernels:
// rdf_collect.hip, host side: rdf_capi_collect.inc).  Collect compacts an ITEM LIST the window front (rdf_window.h) has
// laid out — the n sorted rows for LIST, the D heads of the distinct (group, value) pairs for SET — into one list row per
// group; explode expands a List column back into one row per element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdf_device.h"
#include "rdf_utf8.h"

constexpr int kCollectThreads = 256;
constexpr int kCollectTile = RDF_COLLECT_TILE;                  // items (collect) / output rows (explode) of one block's tile
constexpr int kCollectPer = kCollectTile / kCollectThreads;     // per thread: item k of a thread is tile base + k * threads + tid
constexpr int kCollectSegs = kCollectPer * (kCollectThreads / 64);   // 64-item runs of a tile, in item order
static_assert(kCollectTile % kCollectThreads == 0, "a whole number of items per thread");
constexpr int kExplodeWindow = 2048;                            // list rows whose starts one explode tile stages in LDS (16 KiB)

struct CollectArgs {
    // the item list
    int64_t                  m;          // items: n (LIST) or D (SET)
    const int64_t*           m_dev;      // count pass, SET: the front's total on the device, whose low word is D; `m` is
                                         // then only the bound (n) the tiles are numbered by.  nullptr: m is the count
    const uint32_t*          gstart;     // SET: [D] sorted position of every head; LIST: nullptr, item i is sorted position i
    const int64_t*           scan;       // [n + 1] the front's exclusive scan (partitions in the high word); nullptr = one group
    const uint32_t*          perm;       // sorted position -> row (nullptr = identity)
    // the value column: liveness (not NULL) and, if asked, the value itself
    const rdfk::DevChunkCol* vchunks;    // numeric chunks (also a Utf8 LIST value: its offsets as Int32, only validity is read)
    const Utf8Chunk*         vutf8;      // SET over a Utf8 value: the order key's chunks (validity only is read)
    const int64_t*           row_start;  // [nchunks + 1]
    int64_t                  nchunks;
    int32_t                  esize;      // bytes of one value (with `values`)
    int32_t                  canon;      // 0 raw bits, 4 / 8: Float32 / Float64 made canonical (+0.0, one quiet NaN)
    int32_t                  nullable;   // some value chunk carries validity; 0: every item is live
    int32_t                  pad;
    // compaction
    int64_t*                 tile_counts;  // count pass out: [tiles] live items per tile
    const int64_t*           tile_base;    // emit pass in: their exclusive scan; nullptr (fast path) = tile * kCollectTile
    const int64_t*           front_total;  // count pass: the front's grand total, copied to *front_total_out so that
    int64_t*                 front_total_out;   //         G, D and E come back in one copy (either may be nullptr)
    int64_t                  groups;     // G
    // outputs, each may be nullptr
    uint32_t*                group_rows; // [G] the row of the item that starts group g (LIST: the group's first row)
    int32_t*                 offsets;    // [G + 1]
    uint32_t*                child_rows; // [E]
    void*                    values;     // [E]
};

struct ExplodeArgs {
    rdfk::DevChunkCol offsets;           // Int32 value_offsets [n + 1]; its validity bits are the list rows' validity
    int64_t           n;                 // list rows
    int32_t           outer, pad;
    int64_t*          counts;            // count pass out: [n] output rows of every list row
    const int64_t*    start;             // expand pass in: [n + 1] their exclusive scan
    int64_t           rows;              // start[n]
    uint32_t*         parent_rows;       // [rows] or nullptr
    uint32_t*         child_index;       // [rows] or nullptr
    int32_t*          pos;               // [rows] or nullptr
    uint8_t*          vbytes;            // [rows] 1 = the row carries an element (outer only), or nullptr
    unsigned long long* nulls;           // outer: rows without an element, zeroed
};

__host__ __device__ inline int64_t collect_tiles(int64_t m) { return (m + kCollectTile - 1) / kCollectTile; }
hipError_t launch_collect_count(const CollectArgs& a, hipStream_t s);
hipError_t launch_collect_emit(const CollectArgs& a, hipStream_t s);
hipError_t launch_explode_count(const ExplodeArgs& a, hipStream_t s);
hipError_t launch_explode_expand(const ExplodeArgs& a, hipStream_t s);
