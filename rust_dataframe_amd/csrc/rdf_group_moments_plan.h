// rdf_group_moments_plan.h — what rdf_groupby_moments decides apart from the GPU: the level plan of its fold, the finish of
// one PIECE (the run of one group inside one level-0 tile), and a serial emulation of the whole fold (kernels:
// rdf_group_moments.hip, host side: rdf_capi_group_moments.inc, executable model: tests/group_moments_ref.py).
// ONE definition: hipcc compiles the plan and the piece finish into the kernels and the host side, plain g++ compiles
// everything into tests/cpp/test_group_moments_host.cpp.  It includes nothing of HIP.
#pragma once
#include <stdint.h>

#include "rdf_moments_math.h"

constexpr int kGmTile = RDF_GROUP_MOMENTS_TILE;     // sorted rows (level 0) or partial states (levels >= 1) of one tile

// ---------------------------------------------------------------- the level plan: it depends on the row count alone
// m items -> 2 * gm_tiles(m) items (every tile hands on its first and its last segment), until one tile is left.
RDF_MO_HD int64_t gm_tiles(int64_t m) { return (m + kGmTile - 1) / kGmTile; }
RDF_MO_HD int gm_levels(int64_t n) {
    int levels = 1;
    for (int64_t m = n; m > kGmTile; m = 2 * gm_tiles(m)) ++levels;
    return levels;
}

// ---------------------------------------------------------------- one piece: rdf_moments' tile step
// The centre of a piece of n counted values with sum `sum`: any double near the mean will do; a piece whose counted values
// all equal `first` takes that value, so that a constant group has every d = 0 exactly.
RDF_MO_HD double gm_piece_centre(uint32_t n, bool same, double first, double sum) { return n == 0 ? 0.0 : same ? first : sum / (double)n; }
// The piece's state from its power sums about the centre (s: d, d^2, d^3, d^4; pairs: dx, dy, dx^2, dy^2, dx dy).  A piece
// without a counted value is the all-zero state.
RDF_MO_HD rdf_moments_state gm_piece_state(uint32_t n, double c, const double* s) {
    if (n == 0) return rdf_moments_state{0, 0.0, 0.0, 0.0, 0.0, 0.0};
    return mo_tile_state((int64_t)n, c, s[0], s[1], s[2], s[3]);
}
RDF_MO_HD rdf_comoments_state gm_piece_costate(uint32_t n, double cx, double cy, const double* s) {
    if (n == 0) return rdf_comoments_state{0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    return mo_cotile_state((int64_t)n, cx, cy, s[0], s[1], s[2], s[3], s[4]);
}

#if !defined(__HIPCC__) && !defined(__CUDACC__)
// ---------------------------------------------------------------- the fold, serially (tests)
// The states rdf_groupby_moments forms for one column, with every sum taken in item order: seg[j] is the group of sorted
// position j (0, 1, 2 ... ascending), ok[j] whether the row counts, x[j] its value.  Level 0 makes a piece per (tile,
// group), the levels above merge the handed-on states per tile in item order.  states[g] for g < groups is written once.
#include <vector>
struct GmSerialItem { rdf_moments_state st; uint32_t seg; };
inline void gm_serial_emit(std::vector<GmSerialItem>& tile_items, bool final_level, std::vector<GmSerialItem>& next, rdf_moments_state* states, int64_t groups) {
    const int nseg = (int)tile_items.size();
    for (int j = 0; j < nseg; ++j) {
        const GmSerialItem& it = tile_items[(size_t)j];
        if (!final_level && (j == 0 || j == nseg - 1)) next.push_back(it);   // a tile's first and last segment are handed on
        else if ((int64_t)it.seg < groups) states[it.seg] = it.st;            // the others are whole groups
    }
    if (!final_level && nseg == 1) next.push_back(GmSerialItem{rdf_moments_state{0, 0.0, 0.0, 0.0, 0.0, 0.0}, tile_items[0].seg});
    tile_items.clear();
}
inline void gm_serial_moments(const uint32_t* seg, const uint8_t* ok, const double* x, int64_t n, rdf_moments_state* states, int64_t groups) {
    std::vector<GmSerialItem> items, next, tile_items;
    const int levels = gm_levels(n);
    for (int64_t base = 0; base < n; base += kGmTile) {
        const int64_t end = base + kGmTile < n ? base + kGmTile : n;
        for (int64_t a = base; a < end;) {
            int64_t b = a;
            while (b < end && seg[b] == seg[a]) ++b;
            uint32_t cnt = 0;
            bool same = true;
            double first = 0.0, sum = 0.0;
            for (int64_t j = a; j < b; ++j) {
                if (!ok[j]) continue;
                if (cnt == 0) { first = x[j]; sum = x[j]; } else { sum = sum + x[j]; same = same && x[j] == first; }
                ++cnt;
            }
            const double c = gm_piece_centre(cnt, same, first, sum);
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            bool any = false;
            for (int64_t j = a; j < b; ++j) {
                if (!ok[j]) continue;
                const double d = x[j] - c, d2 = d * d, t[4] = {d, d2, d2 * d, d2 * d2};
                for (int k = 0; k < 4; ++k) s[k] = any ? s[k] + t[k] : t[k];
                any = true;
            }
            tile_items.push_back(GmSerialItem{gm_piece_state(cnt, c, s), seg[a]});
            a = b;
        }
        gm_serial_emit(tile_items, levels == 1, next, states, groups);
    }
    for (int level = 1; level < levels; ++level) {
        items.swap(next);
        next.clear();
        const int64_t m = (int64_t)items.size();
        for (int64_t base = 0; base < m; base += kGmTile) {
            const int64_t end = base + kGmTile < m ? base + kGmTile : m;
            for (int64_t j = base; j < end; ++j) {
                if (!tile_items.empty() && tile_items.back().seg == items[(size_t)j].seg) mo_merge(tile_items.back().st, items[(size_t)j].st);
                else tile_items.push_back(items[(size_t)j]);
            }
            gm_serial_emit(tile_items, level == levels - 1, next, states, groups);
        }
    }
}
#endif
