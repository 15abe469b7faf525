// The launch policy of the program path (rust_dataframe_amd/csrc/rdf_program_plan.h) on the CPU: the persistent grid and the tile
// walk of the specialised kernels, the grouped kernel's grid cap, the LDS copies of the interpreted grouped sink, the tile prefix
// and its reciprocal.  The expected figures are written out from the rules as they were measured (blocks per CU x CUs, rotation
// in waves), not computed by a second copy of the code.
#include <cstdint>
#include <vector>

#include "mini_test.hpp"
#include "../../rust_dataframe_amd/csrc/rdf_program_plan.h"

using namespace rdfk;

namespace {

// an MI355X: 256 CUs x 8 resident blocks, 4 waves per block; every option left to the program
SpecWalkIn walk(int sink, bool heavy, int64_t nchunks, int ncols, bool any_bitmap, int64_t ntiles) {
    SpecWalkIn in;
    in.sink = sink; in.heavy = heavy; in.nchunks = nchunks; in.ncols = ncols; in.any_bitmap = any_bitmap; in.ntiles = ntiles;
    in.grid_limit = 2048; in.waves_per_block = 4;
    in.spec_blocks_per_cu = 0; in.spec_tile_rot = -1; in.spec_xcd_swz = -1; in.spec_grid_adj = 0;
    return in;
}
constexpr int64_t kMany = 1000000;   // tiles: far more than any grid

}  // namespace

TEST(aggregates_take_two_or_three_blocks_per_cu_and_the_swizzled_walk) {
    WalkPlan p = spec_walk_plan(walk(kPlanSinkAgg, false, 1, 1, false, kMany));     // the headline: one chunk, one column, no bitmap
    CHECK_EQ(p.grid, 512); CHECK_EQ(p.xcd_swz, 1); CHECK_EQ(p.tile_rot, 0);
    p = spec_walk_plan(walk(kPlanSinkAgg, false, 1, 1, true, kMany));               // ... with a bitmap
    CHECK_EQ(p.grid, 768); CHECK_EQ(p.xcd_swz, 1); CHECK_EQ(p.tile_rot, 0);
    p = spec_walk_plan(walk(kPlanSinkAgg, false, 977, 1, false, kMany));            // a batch table: three, rows rotated by one block
    CHECK_EQ(p.grid, 768); CHECK_EQ(p.xcd_swz, 1); CHECK_EQ(p.tile_rot, 4);
    p = spec_walk_plan(walk(kPlanSinkAgg, false, 1, 4, false, kMany));              // several columns: rotated too
    CHECK_EQ(p.grid, 512); CHECK_EQ(p.xcd_swz, 1); CHECK_EQ(p.tile_rot, 4);
}

TEST(heavy_and_store_programs_keep_the_plain_walk) {
    WalkPlan p = spec_walk_plan(walk(kPlanSinkAgg, true, 1, 1, false, kMany));      // libm-class operator: not bandwidth-bound
    CHECK_EQ(p.grid, 2048); CHECK_EQ(p.xcd_swz, 0); CHECK_EQ(p.tile_rot, 0);
    p = spec_walk_plan(walk(kPlanSinkStore, false, 1, 2, false, kMany));
    CHECK_EQ(p.grid, 1792); CHECK_EQ(p.xcd_swz, 0); CHECK_EQ(p.tile_rot, 0);
    p = spec_walk_plan(walk(kPlanSinkStore, false, 977, 2, false, kMany));
    CHECK_EQ(p.grid, 2048); CHECK_EQ(p.xcd_swz, 0); CHECK_EQ(p.tile_rot, 0);
}

TEST(small_inputs_take_a_block_per_four_tiles_and_at_least_one) {
    SpecWalkIn in = walk(kPlanSinkAgg, false, 1, 1, false, 37);
    CHECK_EQ(spec_walk_plan(in).grid, 10);
    in.spec_grid_adj = 3;                                   // the adjustment applies at the limit only
    CHECK_EQ(spec_walk_plan(in).grid, 10);
    in = walk(kPlanSinkAgg, false, 1, 1, false, 0);
    CHECK_EQ(spec_walk_plan(in).grid, 1); CHECK_EQ(spec_walk_plan(in).tile_rot, 0);
    in = walk(kPlanSinkAgg, false, 3, 2, false, 1);         // a rotation never leaves the grid's waves: 4 mod 4
    CHECK_EQ(spec_walk_plan(in).grid, 1); CHECK_EQ(spec_walk_plan(in).tile_rot, 0);
    in = walk(kPlanSinkAgg, false, 1, 1, false, 2048);      // exactly the limit's worth of tiles
    CHECK_EQ(spec_walk_plan(in).grid, 512);
    in.ntiles = 2047;
    CHECK_EQ(spec_walk_plan(in).grid, 512);
    in.ntiles = 2044;
    CHECK_EQ(spec_walk_plan(in).grid, 511);
}

TEST(options_pin_what_the_program_would_choose) {
    SpecWalkIn in = walk(kPlanSinkAgg, false, 1, 1, false, kMany);
    in.spec_grid_adj = 3;
    CHECK_EQ(spec_walk_plan(in).grid, 515);
    in.spec_grid_adj = -600;
    CHECK_EQ(spec_walk_plan(in).grid, 1);
    in = walk(kPlanSinkStore, false, 977, 1, false, kMany);
    in.spec_grid_adj = 3;                                   // never past the device's resident blocks
    CHECK_EQ(spec_walk_plan(in).grid, 2048);
    in = walk(kPlanSinkAgg, false, 1, 1, false, kMany);
    in.spec_blocks_per_cu = 5;
    CHECK_EQ(spec_walk_plan(in).grid, 1280);
    in.spec_blocks_per_cu = 12;
    CHECK_EQ(spec_walk_plan(in).grid, 2048);
    in = walk(kPlanSinkAgg, false, 977, 4, true, kMany);
    in.spec_tile_rot = 0; in.spec_xcd_swz = 0;
    CHECK_EQ(spec_walk_plan(in).grid, 768); CHECK_EQ(spec_walk_plan(in).xcd_swz, 0); CHECK_EQ(spec_walk_plan(in).tile_rot, 0);
    in = walk(kPlanSinkStore, false, 1, 1, false, kMany);
    in.spec_tile_rot = 2; in.spec_xcd_swz = 1;              // ... and the other way round: two blocks' worth of waves
    CHECK_EQ(spec_walk_plan(in).grid, 1792); CHECK_EQ(spec_walk_plan(in).xcd_swz, 1); CHECK_EQ(spec_walk_plan(in).tile_rot, 8);
}

TEST(another_cu_count_keeps_the_ratios) {
    SpecWalkIn in = walk(kPlanSinkAgg, false, 1, 1, false, kMany);
    in.grid_limit = 304 * 8;
    CHECK_EQ(spec_walk_plan(in).grid, 608);
    in.any_bitmap = true;
    CHECK_EQ(spec_walk_plan(in).grid, 912);
    in = walk(kPlanSinkStore, false, 1, 1, false, kMany);
    in.grid_limit = 304 * 8;
    CHECK_EQ(spec_walk_plan(in).grid, 2128);
    in.nchunks = 977;
    CHECK_EQ(spec_walk_plan(in).grid, 2432);
}

TEST(tile_reciprocal_is_the_128_bit_quotient_with_its_guards) {
    CHECK_EQ(tile_reciprocal(3, 10), (uint64_t)858993459);                  // floor(2 * 2^32 / 10)
    CHECK_EQ(tile_reciprocal(976563, 976562), (uint64_t)4294967296);       // a tile per batch: exactly 2^32
    CHECK_EQ(tile_reciprocal(1, 0), (uint64_t)0);
    CHECK_EQ(tile_reciprocal(1, 12345), (uint64_t)0);
    CHECK_EQ(tile_reciprocal(0, 0), (uint64_t)0);
    CHECK_EQ(tile_reciprocal(5, 0), (uint64_t)0);
    CHECK_EQ(tile_reciprocal(((int64_t)1 << 31) + 1, 7), (uint64_t)0);      // nchunks - 1 == 2^31: no guess
    CHECK_EQ(tile_reciprocal((int64_t)1 << 31, (int64_t)1 << 31), (uint64_t)4294967294);   // the last count that has one: floor((2^31 - 1) * 2^32 / 2^31)
}

TEST(tile_prefix_counts_the_tiles_in_front_of_every_batch) {
    const std::vector<int64_t> clen = {0, 1, 1024, 1025};
    std::vector<int64_t> ts(clen.size() + 1, -1);
    CHECK_EQ(tile_prefix(clen.data(), (int64_t)clen.size(), 1024, ts.data()), 4);
    CHECK(ts == (std::vector<int64_t>{0, 0, 1, 2, 4}));
    int64_t one = -1;
    CHECK_EQ(tile_prefix(nullptr, 0, 1024, &one), 0);                       // no batches: the one entry, zero
    CHECK_EQ(one, 0);
}

TEST(the_grouped_kernel_runs_two_blocks_per_cu_on_the_plain_stride) {
    WalkPlan p = gspec_walk_plan(2048, 2048, 0, -1, -1);
    CHECK_EQ(p.grid, 512); CHECK_EQ(p.xcd_swz, 0); CHECK_EQ(p.tile_rot, 0);
    p = gspec_walk_plan(100, 2048, 0, -1, -1);                               // fewer tiles than the cap: untouched
    CHECK_EQ(p.grid, 100);
    p = gspec_walk_plan(2048, 2048, 3, -1, -1);
    CHECK_EQ(p.grid, 768);
    p = gspec_walk_plan(2048, 304 * 8, 0, 0, 0);
    CHECK_EQ(p.grid, 608); CHECK_EQ(p.xcd_swz, 0); CHECK_EQ(p.tile_rot, 0);
    p = gspec_walk_plan(2048, 2048, 0, 1, 1);                                // only an option turns the walks on
    CHECK_EQ(p.grid, 512); CHECK_EQ(p.xcd_swz, 1); CHECK_EQ(p.tile_rot, 1);
    p = gspec_walk_plan(4, 2048, 0, 5, -1);                                  // rotation in blocks, inside the grid
    CHECK_EQ(p.grid, 4); CHECK_EQ(p.tile_rot, 1);
    p = gspec_walk_plan(1, 2048, 0, 1, -1);
    CHECK_EQ(p.grid, 1); CHECK_EQ(p.tile_rot, 0);
}

TEST(group_replicas_fill_32_kb_of_lds_and_leave_room_for_the_temporaries) {
    CHECK_EQ(kPlanTmpSlotBytes, 9216);
    CHECK_EQ(group_replicas(3, 0), 32);            // 24 bytes a copy
    CHECK_EQ(group_replicas(128, 0), 32);          // 1 KB a copy: 32 copies are exactly 32 KB
    CHECK_EQ(group_replicas(129, 0), 16);          // ... and a word more is past it
    CHECK_EQ(group_replicas(2048, 0), 2);          // 16 KB a copy
    CHECK_EQ(group_replicas(4096, 0), 1);
    CHECK_EQ(group_replicas(5000, 0), 1);          // never fewer than one
    CHECK_EQ(group_replicas(128, 4), 16);          // 36 KB of temporaries leave 28 KB of the 64
    CHECK_EQ(group_replicas(64, 7), 2);            // 63 KB of temporaries leave 1 KB: two copies of 512 bytes
    CHECK_EQ(group_replicas(128, 3), 32);          // 27 KB of temporaries: the 32 KB bound is still the tighter one
}

int main() { return run_all(); }
