// rdf_group_moments.h — argument blocks and launchers of rdf_groupby_moments: variance, stddev, skewness, kurtosis, covar
// and corr per group (kernels: rdf_group_moments.hip, host side: rdf_capi_group_moments.inc, formulas: rdf_moments_math.h).  The
// window front (rdf_window.h) has sorted the rows by the grouping keys alone and left the permutation, the scan of its
// partition flags and the partition start table; what is here folds the n sorted rows into one moment state per group and
// reads the statistics off the states.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdf_device.h"
#include "rdf_moments.h"
#include "rdf_group_moments_plan.h"

constexpr int kGmThreads = 256;
static_assert(kGmTile == kGmThreads, "one item per thread");
constexpr uint32_t kGmNone = 0xFFFFFFFFu;

// An item of the levels >= 1: the state of a run of rows of group `seg`.  Two per tile of the level below.
template <class State> struct GmItem { State st; uint32_t seg, pad; };
using GmItem1 = GmItem<rdf_moments_state>;
using GmItem2 = GmItem<rdf_comoments_state>;

struct GmFoldArgs {
    // level 0: the sorted rows, read through the front's tables
    const int64_t*           scan;       // [n + 1] exclusive scan of the flags: the high word of scan[j + 1] is 1 + the group of position j
    const uint32_t*          perm;       // sorted position -> row (nullptr = identity)
    const rdfk::DevChunkCol* x;          // [nchunks]
    const rdfk::DevChunkCol* y;          // [nchunks] or nullptr
    const int64_t*           row_start;  // [nchunks + 1]
    int64_t                  nchunks;
    int32_t                  dt_x, dt_y; // rdf_dtype
    // levels >= 1: the partials of the level below (GmItem1 / GmItem2)
    const void*              in;         // [m]
    int64_t                  m;          // items of this level (level 0: n)
    void*                    part;       // [tiles][2] out: the tile's first and last segment; nullptr on the final level
    void*                    states;     // [G] rdf_moments_state / rdf_comoments_state
    int64_t                  groups;     // G: no group index beyond it is written
};

struct GmCallOut { int32_t stat, pad; double* values; uint8_t* vbytes; };

struct GmFinishArgs {
    const void*         states;          // [G], or nullptr: the key tuples alone
    int32_t             pair, ncalls;
    int64_t             groups;
    const uint32_t*     pstart;          // [G + 1] first sorted position of every group
    const uint32_t*     perm;            // nullptr = identity
    uint32_t*           group_rows;      // [G] or nullptr
    int64_t*            counts;          // [G] or nullptr
    GmCallOut           calls[RDF_GROUP_MOMENTS_MAX_CALLS];   // values: [G]; vbytes: [G] 1 = valid
    unsigned long long* nulls;           // [RDF_GROUP_MOMENTS_MAX_CALLS], zeroed
};

// Level 0 over a.m = n sorted rows, then the caller chains gm_fold levels (m -> 2 * gm_tiles(m), rdf_group_moments_plan.h) until one
// tile is left.
hipError_t launch_gm_level0(const GmFoldArgs& a, hipStream_t s);
hipError_t launch_gm_fold(const GmFoldArgs& a, bool pair, hipStream_t s);
hipError_t launch_gm_finish(const GmFinishArgs& a, hipStream_t s);
