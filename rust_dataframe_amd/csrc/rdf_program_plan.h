// rdf_program_plan.h — the launch policy of the program path (rdf_capi_program.inc: run_program) as pure host code: the tile
// prefix tables and the reciprocal the kernels find a tile's batch with, the persistent grid and the tile walk of the specialised
// kernels (rdf_spec_kernel.hip.h) and of the grouped register-accumulator kernel (rdf_gspec_kernel.hip.h), the LDS copies of the
// interpreted grouped sink.  Plain integers in, plain structs out; the measurements behind every rule stand next to it.  Shared by
// the host engine and a CPU test (tests/cpp/test_program_plan.cpp) that holds the rules to the figures they were measured at.
// No HIP types in here.
#pragma once
#include <cstdint>

namespace rdfk {

// The constants of the device header (rdf_device.h) and of the C API the rules are written against; rdf_capi_program.inc asserts
// that they are the same.
constexpr int kPlanSinkStore = 0, kPlanSinkAgg = 1;
constexpr int kPlanCuBlocks = 8;                 // eval_grid_limit() = CUs x 8 resident blocks
constexpr int kPlanTmpSlotBytes = 4 * 256 * 8 + 256 * 4;   // one TMP slot of the interpreter's LDS spill area: kVPT * kBlock values + kBlock validity words

// Tile prefix of a batch list: out[c] = tiles in front of batch c, out[nchunks] = all of them (the return value).
inline int64_t tile_prefix(const int64_t* clen, int64_t nchunks, int rows_per_tile, int64_t* out) {
    out[0] = 0;
    for (int64_t c = 0; c < nchunks; ++c) out[c + 1] = out[c] + (clen[c] + rows_per_tile - 1) / rows_per_tile;
    return out[nchunks];
}

// 2^32 x (batches in front of the last) / (tiles in front of the last): a kernel's first guess of a tile's batch is
// (tile * this) >> 32, exact for equal batches and a step or two off otherwise.  0 = no guess (the kernel bisects).
inline uint64_t tile_reciprocal(int64_t nchunks, int64_t tiles_before_last_chunk) {
    if (!(nchunks > 1 && tiles_before_last_chunk > 0 && nchunks - 1 < ((int64_t)1 << 31))) return 0;
    return (uint64_t)(((unsigned __int128)(uint64_t)(nchunks - 1) << 32) / (unsigned __int128)(uint64_t)tiles_before_last_chunk);
}

struct SpecWalkIn {
    int     sink;             // kPlanSinkStore / kPlanSinkAgg
    bool    heavy;            // the program holds a libm-class operator (op_is_heavy)
    int64_t nchunks;
    int     ncols;            // program columns
    bool    any_bitmap;       // some program column carries a validity bitmap
    int64_t ntiles;           // wave-granular tiles (SpecArgs::ntiles)
    int     grid_limit;       // eval_grid_limit()
    int     waves_per_block;  // kBlock / 64
    int     spec_blocks_per_cu, spec_tile_rot, spec_xcd_swz, spec_grid_adj;   // rdf_set_option: 0 / -1 / -1 / 0 = by the program
};
struct WalkPlan { int grid; int64_t tile_rot; int xcd_swz; };

// Persistent grid and tile walk of spec_kernel.
//
// Resident blocks per CU of the persistent grid.  More is not always better on this part: a one-column filter -> aggregate
// over a column without a bitmap keeps 128 KB per CU in flight with eight blocks and runs at 0.826-0.844 of the HBM peak;
// with three (48 KB in flight) at 0.876-0.879, with four 0.866-0.868, with five 0.824-0.830 (bench.py, same box, three
// alternating rounds; tools/ubench_stream's bare loop shows the same: 4 blocks x 64 B per lane 0.86-0.88, 8 blocks 0.80).
// Aggregates over several columns follow it: a*b+c -> min / max / count over four columns (config C3) 0.824-0.840 with three
// against 0.786-0.813 with eight (two boxes, alternating rounds), `x > c AND y < d -> sum` 2.32 against 2.62 ms per 1e9
// rows; EVEN counts are the bad ones (four: 0.767 on C3, six: 0.770 — the strides between the blocks' tiles then line up
// with the memory channels' interleave).  Store sinks (new columns): seven — a + b 4.2-4.4 ms per 1e9 rows against 4.6-4.8
// with eight, with a validity bitmap 4.0-4.1 against 4.8-4.9, a*b+c 5.7-5.95 against 6.2-6.3 (two boxes).  Aggregates over
// columns with bitmaps measured best at eight (1.34 against 1.35 / 1.46 ms with seven / three) and keep it.  The same program over the readers' 1024-row batches (a descriptor per two tiles): four blocks 0.825-0.830,
// five 0.810, eight 0.788-0.796, three 0.764, six 0.740-0.745 (two boxes, alternating rounds).
// rdf_set_option("spec_blocks_per_cu", n) pins a value (A/B).
// Round 5 (tools/exp_tilewalk.py, three boxes, profiles/r05_tilewalk_*.jsonl): with the chunk tables in SGPRs and the
// full-tile bitmap path, aggregates run best with 48-64 KB per CU in flight — TWO blocks per CU for the one-column
// headline shape (0.886-0.894 against 0.869-0.877 with three), three where a bitmap or a batch table adds scalar work
// per tile (0.858-0.866 with 10 % NULLs, 0.76 in round 4; 1024-row batches 0.863-0.875, 0.82) — and with a tile walk that
// does not depend on the grid: XCD x takes the x-th contiguous eighth of every row of tiles (xcd_swz), rows rotated by
// one block per iteration where several columns or batches are walked (tile_rot).  The plain grid stride swung
// 0.78-0.83 from box to box on C3; rotated / swizzled walks and 8 rows per lane hold 0.827-0.842 on every grid tried.
inline WalkPlan spec_walk_plan(const SpecWalkIn& in) {
    const bool agg = in.sink == kPlanSinkAgg && !in.heavy;
    int blocks_per_cu = in.spec_blocks_per_cu;
    if (blocks_per_cu <= 0) {
        if (agg) blocks_per_cu = (in.nchunks == 1 && !in.any_bitmap) ? 2 : 3;
        else if (in.sink == kPlanSinkStore && in.nchunks == 1) blocks_per_cu = 7;
        else blocks_per_cu = 8;
    }
    blocks_per_cu = blocks_per_cu < 1 ? 1 : blocks_per_cu > kPlanCuBlocks ? kPlanCuBlocks : blocks_per_cu;
    const int walk_swz = in.spec_xcd_swz < 0 ? (agg ? 1 : 0) : in.spec_xcd_swz;
    const int walk_rot = in.spec_tile_rot < 0 ? (agg && (in.nchunks > 1 || in.ncols > 1) ? 1 : 0) : in.spec_tile_rot;
    const int64_t btiles = (in.ntiles + in.waves_per_block - 1) / in.waves_per_block;   // a block's waves take consecutive tiles
    const int64_t limit = (int64_t)(in.grid_limit / kPlanCuBlocks) * blocks_per_cu;
    int grid = (int)(btiles < limit ? btiles : limit);
    if (grid == limit && in.spec_grid_adj != 0) {   // (A/B of grids that are not a multiple of the CU count)
        grid += in.spec_grid_adj;
        if (grid > in.grid_limit) grid = in.grid_limit;
    }
    if (grid < 1) grid = 1;
    WalkPlan p;
    p.grid = grid;
    p.tile_rot = ((int64_t)walk_rot * in.waves_per_block) % ((int64_t)grid * in.waves_per_block);
    p.xcd_swz = walk_swz ? 1 : 0;
    return p;
}

// Grid cap and tile walk of gspec_kernel, from the interpreter's grid over the same tiles.
// The kernel keeps G x NV accumulators per lane (~220 VGPRs for Q1): two waves per SIMD = two blocks per CU are resident
// whatever is launched; launching just those keeps the grid persistent (one prologue / epilogue per block, and the
// next-tile prefetch of rdf_gspec_kernel.hip.h never runs dry at a block's end).
// The walks that help the ungrouped aggregates do not help here — Q1, same box: plain 0.769 of peak, swizzled 0.755,
// rotated 0.752, both 0.748 — so the grouped kernel keeps the plain grid stride unless an option asks.
inline WalkPlan gspec_walk_plan(int grid, int grid_limit, int gspec_blocks_per_cu, int spec_tile_rot, int spec_xcd_swz) {
    const int per_cu = gspec_blocks_per_cu > 0 ? gspec_blocks_per_cu : 2;
    const int64_t lim = (int64_t)(grid_limit / kPlanCuBlocks) * per_cu;
    if (grid > lim) grid = (int)lim;
    WalkPlan p;
    p.grid = grid;
    p.xcd_swz = spec_xcd_swz > 0 ? 1 : 0;
    p.tile_rot = (spec_tile_rot > 0 ? spec_tile_rot : 0) % (grid > 1 ? grid : 1);
    return p;
}

// LDS copies of the interpreted grouped sink's accumulator table (gwords 64-bit words): as many (power of two, <= 32) as fit
// in 32 KB, and in 64 KB together with the TMP spill area of a program with ntmp temporaries.
inline int group_replicas(int gwords, int ntmp) {
    const uint64_t tmp_bytes = (uint64_t)ntmp * kPlanTmpSlotBytes;
    int reps = 32;
    while (reps > 1 && ((uint64_t)reps * (uint64_t)gwords * 8 > 32768 || tmp_bytes + (uint64_t)reps * (uint64_t)gwords * 8 > 65536)) reps >>= 1;
    return reps;
}

}  // namespace rdfk
