// The scan that lays out the equi-join's table of distinct build keys (rust_dataframe_amd/csrc/rdf_join_place.h) on the CPU: the
// summaries {c, m} of runs of keys and their combination, held to the rule they replace — linear probing over keys that arrive in
// home-slot order, slot(r) = max(home(r), slot(r - 1) + 1) — for every way of cutting the key list into tiles and the tiles into
// threads' runs, the way join_place_kernel / join_place_scan_kernel do.
#include <algorithm>
#include <cstdint>
#include <random>
#include <vector>

#include "mini_test.hpp"
#include "../../rust_dataframe_amd/csrc/rdf_join_place.h"

using namespace rdfk;

namespace {

std::vector<long long> sequential(const std::vector<long long>& home) {
    std::vector<long long> pos(home.size());
    long long last = -1;
    for (size_t r = 0; r < home.size(); ++r) { pos[r] = std::max(home[r], last + 1); last = pos[r]; }
    return pos;
}

// the kernels' way: tiles of `tile` keys, cut into runs of `per` keys; summaries per run, exclusive prefixes over the runs of a tile
// and over the tiles, then every run places its keys from the prefix in front of it
std::vector<long long> tiled(const std::vector<long long>& home, size_t tile, size_t per) {
    const size_t n = home.size(), ntiles = (n + tile - 1) / tile;
    std::vector<PlaceCM> tsum(ntiles, place_empty());
    for (size_t t = 0; t < ntiles; ++t)
        for (size_t r0 = t * tile; r0 < std::min(n, (t + 1) * tile); r0 += per) {
            PlaceCM loc = place_empty();
            for (size_t r = r0; r < std::min({n, (t + 1) * tile, r0 + per}); ++r) (void)place_push(loc, home[r]);
            tsum[t] = place_join(tsum[t], loc);
        }
    std::vector<PlaceCM> carry(ntiles);
    PlaceCM run = place_empty();
    for (size_t t = 0; t < ntiles; ++t) { carry[t] = run; run = place_join(run, tsum[t]); }
    std::vector<long long> pos(n);
    for (size_t t = 0; t < ntiles; ++t) {
        PlaceCM ex = place_empty();                     // the runs of this tile in front of the current one
        for (size_t r0 = t * tile; r0 < std::min(n, (t + 1) * tile); r0 += per) {
            PlaceCM here = place_join(carry[t], ex), loc = place_empty();
            long long last = place_last(here);
            for (size_t r = r0; r < std::min({n, (t + 1) * tile, r0 + per}); ++r) {
                pos[r] = place_push(here, home[r]);
                CHECK(pos[r] > last);                   // (what the kernel's gap fill relies on)
                last = pos[r];
                (void)place_push(loc, home[r]);
            }
            ex = place_join(ex, loc);
        }
    }
    return pos;
}

std::vector<long long> homes(std::mt19937_64& g, size_t n, long long slots, int shape) {
    std::vector<long long> h(n);
    for (size_t i = 0; i < n; ++i) {
        switch (shape) {
            case 0: h[i] = (long long)(g() % (uint64_t)slots); break;                        // uniform hashes: load n / slots
            case 1: h[i] = (long long)(g() % 7); break;                                      // everything crowds on a few slots
            case 2: h[i] = slots - 1 - (long long)(g() % 3); break;                          // ... on the LAST slots (past the end: the margin's case)
            case 3: h[i] = (long long)((g() % (uint64_t)slots) & ~(uint64_t)0xFFF); break;   // clusters every 4096 slots
            default: h[i] = (long long)i * 3; break;                                         // no collisions at all
        }
    }
    std::sort(h.begin(), h.end());
    return h;
}

}  // namespace

TEST(join_of_runs_is_associative_and_has_an_identity) {
    std::mt19937_64 g(1);
    for (int it = 0; it < 20000; ++it) {
        PlaceCM a{(long long)(g() % 50), (long long)(g() % 1000) - 300}, b{(long long)(g() % 50), (long long)(g() % 1000) - 300}, c{(long long)(g() % 50), (long long)(g() % 1000) - 300};
        if (a.c == 0) a = place_empty();
        if (b.c == 0) b = place_empty();
        const PlaceCM l = place_join(place_join(a, b), c), r = place_join(a, place_join(b, c));
        CHECK(l.c == r.c);
        if (l.c > 0) CHECK(l.m == r.m);
        const PlaceCM e = place_join(place_empty(), a), f = place_join(a, place_empty());
        CHECK(e.c == a.c && f.c == a.c);
        if (a.c > 0) CHECK(e.m == a.m && f.m == a.m);
    }
}

TEST(tiles_place_what_linear_probing_places) {
    std::mt19937_64 g(2);
    for (int shape = 0; shape < 5; ++shape)
        for (size_t n : {(size_t)1, (size_t)2, (size_t)63, (size_t)2048, (size_t)2049, (size_t)40000}) {
            const long long slots = (long long)std::max<size_t>(4, 2 * n);
            const std::vector<long long> h = homes(g, n, slots, shape);
            const std::vector<long long> want = sequential(h);
            for (auto cut : {std::pair<size_t, size_t>{2048, 8}, {64, 4}, {7, 3}, {1, 1}, {100000, 100000}})
                CHECK(tiled(h, cut.first, cut.second) == want);
            // slots are distinct, in key order, never in front of a key's home
            for (size_t r = 0; r < n; ++r) { CHECK(want[r] >= h[r]); if (r) CHECK(want[r] > want[r - 1]); }
        }
}

TEST(a_probe_finds_every_key_by_walking_from_its_home) {
    std::mt19937_64 g(3);
    const size_t n = 5000;
    const long long slots = 16384;
    const std::vector<long long> h = homes(g, n, slots, 0);
    const std::vector<long long> pos = tiled(h, 2048, 8);
    std::vector<long long> table((size_t)slots + n + 1, -1);
    for (size_t r = 0; r < n; ++r) table[(size_t)pos[r]] = (long long)r;
    for (size_t r = 0; r < n; ++r) {
        long long s = h[r];
        while (table[(size_t)s] != (long long)r) { CHECK(table[(size_t)s] >= 0); ++s; }     // no empty slot between a key's home and the key
    }
}

// The sizes the host gives the two lookups.  Every expected value follows from the rules, none is measured: distinct keys nd =
// min(rows, key range + 1, counted distinct); tbits = the smallest value >= 10 with 2^tbits >= 2 nd; cap = 2^tbits + 2^16.
TEST(the_table_is_sized_from_the_distinct_keys) {
    // 3e6 rows over 37 dictionary codes: the range bounds the keys, nobody counts
    CHECK(join_range_bounds_keys(3000000, 100, 136) && !join_table_counts_keys(3000000, 100, 136));
    JoinTablePlan p = join_table_plan(3000000, 100, 136, 0);
    CHECK(p.nd == 37 && p.tbits == 10 && p.cap == 66560);
    // 37 hashed identifiers over 3e6 rows: the range says nothing (>= rows), the count does
    CHECK(!join_range_bounds_keys(3000000, 5, 5 + 3000000ull) && join_table_counts_keys(3000000, 5, 5 + 3000000ull));
    p = join_table_plan(3000000, 5, 5 + 3000000ull, 37);
    CHECK(p.nd == 37 && p.tbits == 10 && p.cap == 66560);
    p = join_table_plan(3000000, 0, ~0ull, 37);
    CHECK(p.nd == 37 && p.tbits == 10 && p.cap == 66560);
    // a range of exactly rows - 1 still bounds (rows keys at most either way)
    CHECK(join_range_bounds_keys(3000000, 0, 2999999) && !join_range_bounds_keys(3000000, 0, 3000000));
    // below 65 536 rows a wide range is not counted: sized from the rows
    CHECK(!join_table_counts_keys(65535, 0, ~0ull) && join_table_counts_keys(65536, 0, ~0ull));
    p = join_table_plan(65535, 0, ~0ull, 0);
    CHECK(p.nd == 65535 && p.tbits == 17 && p.cap == (1ll << 17) + 65536);
    // a count that is not below the rows changes nothing; a count of 0 means "not counted"
    p = join_table_plan(6000000, 0, ~0ull, 6000000);
    CHECK(p.nd == 6000000 && p.tbits == 24 && p.cap == (1ll << 24) + 65536);      // 2^23 < 1.2e7 <= 2^24
    p = join_table_plan(6000000, 0, ~0ull, 0);
    CHECK(p.nd == 6000000 && p.tbits == 24);
    // load <= 0.5 exactly at the power of two, one more bit one key later; never below 10 bits
    p = join_table_plan(512, 0, ~0ull, 0);
    CHECK(p.nd == 512 && p.tbits == 10 && p.cap == 1024 + 65536);
    p = join_table_plan(513, 0, ~0ull, 0);
    CHECK(p.nd == 513 && p.tbits == 11 && p.cap == 2048 + 65536);
    p = join_table_plan(1, 7, 7, 0);
    CHECK(p.nd == 1 && p.tbits == 10);
    // no keys at all (kmax < kmin): the range bounds nothing
    CHECK(!join_range_bounds_keys(10, 1, 0));
}

TEST(the_bucket_index_has_a_bucket_per_row_on_the_top_bits_of_the_range) {
    // nbuckets = the smallest power of two >= rows, 2^24 at most; shift = the smallest with (kmax - kmin) >> shift < nbuckets
    JoinBucketPlan b = join_bucket_plan(1, 42, 42);
    CHECK(b.nbuckets == 1 && b.shift == 0);
    b = join_bucket_plan(0, 1, 0);                      // no rows, an empty key range
    CHECK(b.nbuckets == 1 && b.shift == 0);
    b = join_bucket_plan(1000, 1, 0);                   // an empty key range, whatever the rows
    CHECK(b.nbuckets == 1024 && b.shift == 0);
    b = join_bucket_plan(1ll << 25, 0, (1ull << 25) - 1);
    CHECK(b.nbuckets == (1ll << 24) && b.shift == 1);
    b = join_bucket_plan(3, 10, 13);                    // range 3 < 4 buckets
    CHECK(b.nbuckets == 4 && b.shift == 0);
    b = join_bucket_plan(4, 10, 14);                    // range 4: one shift
    CHECK(b.nbuckets == 4 && b.shift == 1);
    b = join_bucket_plan(5, 10, 14);
    CHECK(b.nbuckets == 8 && b.shift == 0);
    b = join_bucket_plan(2, 0, ~0ull);                  // the whole 64-bit range over two buckets: the top bit
    CHECK(b.nbuckets == 2 && b.shift == 63);
    b = join_bucket_plan(1ll << 30, 0, ~0ull);
    CHECK(b.nbuckets == (1ll << 24) && b.shift == 40);
    // one bucket over the whole 64-bit range: the rule's answer is 64, reached without ever shifting by 64 (the loop this replaces
    // went on to evaluate range >> 64).  The host cannot ask for it: one bucket means one key at most, a range of 0.
    b = join_bucket_plan(1, 0, ~0ull);
    CHECK(b.nbuckets == 1 && b.shift == 64);
    // every plan keeps the largest key's bucket inside the array
    std::mt19937_64 g(4);
    for (int it = 0; it < 20000; ++it) {
        const long long rows = 1 + (long long)(g() % (1ull << (1 + g() % 27)));
        const uint64_t lo = g() >> (g() % 64), span = g() >> (g() % 64), hi = lo + span < lo ? ~0ull : lo + span;
        if (rows == 1 && hi != lo) continue;
        b = join_bucket_plan(rows, lo, hi);
        CHECK(b.shift < 64 && ((hi - lo) >> b.shift) < (uint64_t)b.nbuckets);
        if (b.shift > 0) CHECK(((hi - lo) >> (b.shift - 1)) >= (uint64_t)b.nbuckets);
    }
}

int main() { return run_all(); }
