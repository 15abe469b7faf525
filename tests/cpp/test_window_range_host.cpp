// test_window_range_host.cpp — rust_dataframe_amd/csrc/rdf_window_range.h on the host: the bound arithmetic, the predicate and
// the two searches over the table tests/window_range_ref.py writes, and the frame checks.  Plain g++ with
// -fsanitize=address,undefined -ffp-contract=off; no HIP, no GPU.  A signed overflow in the integer bound arithmetic, or a
// probe outside [lo, hi), stops the program here.
//
// One line per search: f64 desc is_end following offset o nkeys key:class ... expect.  Float64 keys and offsets are the hex
// of their bits.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "../../rust_dataframe_amd/csrc/rdf_window_range.h"

namespace {

int g_failed = 0, g_checked = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        ++g_checked;                                                 \
        if (!(cond)) {                                               \
            ++g_failed;                                              \
            if (g_failed < 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                            \
    } while (0)

// Exactly [lo, hi) may be read: the vectors are sized to the partition, so AddressSanitizer sees anything else.
struct Keys {
    const std::vector<uint64_t>& k;
    const std::vector<uint8_t>& c;
    uint64_t key(int64_t j) const { return k.at((size_t)j); }
    int cls(int64_t j) const { return c.at((size_t)j); }
};

uint64_t parse_bits(const std::string& t, bool f64) {
    if (f64) return strtoull(t.c_str(), nullptr, 16);
    return (uint64_t)strtoll(t.c_str(), nullptr, 10);
}

void frame_checks() {
    const int UP = WR_UNBOUNDED_PRECEDING, P = WR_PRECEDING, C = WR_CURRENT_ROW, F = WR_FOLLOWING, UF = WR_UNBOUNDED_FOLLOWING;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int f64 = 0; f64 < 2; ++f64) {
        CHECK(wr_check_frame(UF, UF, 0, 0, 0, 0, f64) == WR_FRAME_START_UF, "start UF");
        CHECK(wr_check_frame(UP, UP, 0, 0, 0, 0, f64) == WR_FRAME_END_UP, "end UP");
        CHECK(wr_check_frame(C, P, 1, 1, 1, 1, f64) == WR_FRAME_ORDER && wr_check_frame(F, C, 1, 1, 1, 1, f64) == WR_FRAME_ORDER &&
              wr_check_frame(F, P, 1, 1, 1, 1, f64) == WR_FRAME_ORDER, "start kind > end kind");
        CHECK(wr_check_frame(P, P, 1, 2, 1, 2, f64) == WR_FRAME_ORDER, "1 PRECEDING .. 2 PRECEDING");
        CHECK(wr_check_frame(F, F, 3, 2, 3, 2, f64) == WR_FRAME_ORDER, "3 FOLLOWING .. 2 FOLLOWING");
        CHECK(wr_check_frame(P, P, 2, 1, 2, 1, f64) == WR_FRAME_OK && wr_check_frame(F, F, 2, 5, 2, 5, f64) == WR_FRAME_OK, "ordered offsets");
        CHECK(wr_check_frame(P, C, -1, 0, -1.0, 0, f64) == WR_FRAME_NEGATIVE && wr_check_frame(C, F, 0, -1, 0, -0.5, f64) == WR_FRAME_NEGATIVE, "negative offsets");
        for (int kind : {-1, 5, 77}) CHECK(wr_check_frame(kind, C, 0, 0, 0, 0, f64) == WR_FRAME_KIND && wr_check_frame(UP, kind, 0, 0, 0, 0, f64) == WR_FRAME_KIND, "kinds");
        CHECK(wr_check_frame(UP, UF, -5, -5, nan, nan, f64) == WR_FRAME_OK && wr_check_frame(C, C, -5, -5, -inf, nan, f64) == WR_FRAME_OK, "offsets are read for offset kinds only");
        CHECK(wr_check_frame(P, F, INT64_MAX, INT64_MAX, 1e308, 1e308, f64) == WR_FRAME_OK, "large offsets");
    }
    for (double bad : {inf, -inf, nan}) {
        CHECK(wr_check_frame(P, C, 0, 0, bad, 0, true) == WR_FRAME_NOT_FINITE && wr_check_frame(C, F, 0, 0, 0, bad, true) == WR_FRAME_NOT_FINITE, "non-finite offsets");
        CHECK(wr_check_frame(P, C, 0, 0, bad, 0, false) == WR_FRAME_OK, "the double pair is not read for integer keys");
    }
    CHECK(wr_check_frame(P, C, -1, 0, 1.0, 0, true) == WR_FRAME_OK, "the integer pair is not read for Float64 keys");
    for (int e = WR_FRAME_KIND; e <= WR_FRAME_ORDER; ++e) CHECK(strlen(wr_frame_error(e)) > 0, "message %d", e);
    // the integer comparison at the ends of the range: v = o + s and o - s are never formed
    const uint64_t mn = (uint64_t)INT64_MIN, mx = (uint64_t)INT64_MAX;
    CHECK(wr_cmp_int(mx, mn, true, mx) == 1 && wr_cmp_int(~0ull, mn, true, mx) == 0 && wr_cmp_int(0, mn, true, mx) == 1 && wr_cmp_int(mn, mn, true, mx) == -1, "MIN + (2^63 - 1) = -1");
    CHECK(wr_cmp_int(mn, mx, false, mx) == -1 && wr_cmp_int(0, mx, false, mx) == 0 && wr_cmp_int(1, mx, false, mx) == 1, "MAX - (2^63 - 1) = 0");
    CHECK(wr_cmp_int(mx, mx, true, 1) == -1 && wr_cmp_int(mn, mn, false, 1) == 1, "beyond both ends");
    CHECK(wr_cmp_int(mn, mx, true, 0) == -1 && wr_cmp_int(mx, mn, false, 0) == 1 && wr_cmp_int(5, 5, true, 0) == 0 && wr_cmp_int(5, 5, false, 0) == 0, "offset 0");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <table>\n", argv[0]); return 2; }
    static_assert(kWRangeTile == kWRangeThreads * kWRangePer && kWRangeLdsKeys >= kWRangeTile, "a window holds at least its own tile");
    static_assert(kWRangeLdsKeys * 9 <= 64 * 1024, "keys and class bytes fit a block's static LDS");
    frame_checks();
    FILE* fh = fopen(argv[1], "r");
    if (!fh) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    int64_t rows = 0;
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, fh)) {
        std::istringstream in(buf);
        int f64, desc, is_end, following;
        std::string soff, so;
        size_t nk;
        if (!(in >> f64 >> desc >> is_end >> following >> soff >> so >> nk)) continue;
        std::vector<uint64_t> keys(nk);
        std::vector<uint8_t> cls(nk);
        for (size_t i = 0; i < nk; ++i) {
            std::string t;
            in >> t;
            const size_t colon = t.rfind(':');
            keys[i] = parse_bits(t.substr(0, colon), f64 != 0);
            cls[i] = (uint8_t)atoi(t.c_str() + colon + 1);
        }
        int64_t want = -1;
        in >> want;
        WRBound b{is_end, following, 0, 0.0};
        if (f64) b.s_f = wr_f64_of(parse_bits(soff, true)); else b.s_i = parse_bits(soff, false);
        const uint64_t o = parse_bits(so, f64 != 0);
        const Keys K{keys, cls};
        const int64_t got = is_end ? wr_search_end(K, 0, (int64_t)nk, b, f64 != 0, desc != 0, o) : wr_search_start(K, 0, (int64_t)nk, b, f64 != 0, desc != 0, o);
        CHECK(got == want, "row %" PRId64 ": f64 %d desc %d end %d following %d offset %s o %s: got %" PRId64 " want %" PRId64, rows, f64, desc, is_end,
              following, soff.c_str(), so.c_str(), got, want);
        // the predicate is monotone over the partition, and the answer is where it turns
        const WRProbe p = wr_probe(b, f64 != 0, desc != 0, o);
        bool seen = false, mono = true;
        for (size_t i = 0; i < nk; ++i) {
            const bool h = wr_holds(p, cls[i], keys[i]);
            if (seen && !h) mono = false;
            seen = seen || h;
            if (h != ((int64_t)i >= want)) mono = false;
        }
        CHECK(mono, "row %" PRId64 ": the predicate is not monotone", rows);
        // a sub-range that holds the answer gives the same answer (what a tile's window relies on)
        const int64_t lo = want > 2 ? want - 2 : 0, hi = want + 2 < (int64_t)nk ? want + 2 : (int64_t)nk;
        CHECK(wr_first(K, lo, hi, p) == want, "row %" PRId64 ": clipped search", rows);
        ++rows;
    }
    fclose(fh);
    printf("rows: %" PRId64 "\n", rows);
    printf("%d checked, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
