// rdf_moments.h — rdf_moments / rdf_comoments (kernels: rdf_moments.hip, host side: rdf_capi_moments.inc): the argument
// block and the launchers.  The formulas — the merge of two moment states, the tile step's finish and the statistics — are
// in rdf_moments_math.h, ONE definition for the kernels, the host and rdf_moments_merge / rdf_moments_stat.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdf_colstats.h"
#include "rdf_moments_math.h"

// A wave's tile: 64 lanes x kMoRowsPerLane rows; the four waves of a block share one tile of CsCol (kCsTile rows of one chunk).
constexpr int kMoRowsPerLane = 8;
constexpr int kMoWaveTile = 64 * kMoRowsPerLane;
static_assert(kMoWaveTile * (kCsThreads / 64) == kCsTile, "a block's four wave tiles make one tile of CsCol");

struct MoArgs {
    CsCol    col;                   // x: chunks, row and tile prefix tables
    const rdfk::DevChunkCol* y;     // [nchunks] rdf_comoments, else nullptr
    const rdfk::DevChunkCol* mask;  // [nchunks] RDF_BOOL chunks (values = the bits), or nullptr
    int32_t  dt_x, dt_y;            // rdf_dtype
    void*    out;                   // [grid] rdf_moments_state / rdf_comoments_state, one per block
};

int        mo_grid(int64_t ntiles);
hipError_t launch_mo_moments(const MoArgs& a, int grid, hipStream_t s);
hipError_t launch_mo_comoments(const MoArgs& a, int grid, hipStream_t s);
