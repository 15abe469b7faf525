// rust_dataframe_amd/csrc/rdf_group_moments_plan.h and rdf_moments_math.h under plain g++ with -fsanitize=address,undefined
// -ffp-contract=off: no HIP, no GPU, no Python in the process.  It reads the case table tests/group_moments_ref.py writes
// (tests/test_group_moments_host.py) and holds, bit for bit,
//   L  the level plan: gm_levels and the chain m -> 2 * gm_tiles(m)
//   S  mo_stat of a state, every rdf_stat: absent or the value's bits
//   Q  mo_costat of a state, every rdf_costat
//   M  mo_merge of two states
//   F  gm_serial_moments — level 0 pieces, the part tables, the levels of merges — over a table of (group, counts, value)
// to the model's restatement with its sums taken in item order.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rust_dataframe_amd/csrc/rdf_group_moments_plan.h"

static double d_of(uint64_t b) { double d; std::memcpy(&d, &b, 8); return d; }
static uint64_t b_of(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }
static int failed = 0;
static long rows[5] = {0, 0, 0, 0, 0};

static void fail(const char* what, long line) {
    if (failed++ < 20) std::printf("FAIL %s at table line %ld\n", what, line);
}
static bool read_state(FILE* f, rdf_moments_state& s) {
    uint64_t b[5];
    long long n;
    if (std::fscanf(f, "%lld %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &n, &b[0], &b[1], &b[2], &b[3], &b[4]) != 6) return false;
    s = rdf_moments_state{(int64_t)n, d_of(b[0]), d_of(b[1]), d_of(b[2]), d_of(b[3]), d_of(b[4])};
    return true;
}
static bool same_state(const rdf_moments_state& a, const rdf_moments_state& b) {
    return a.count == b.count && b_of(a.mean) == b_of(b.mean) && b_of(a.mean_lo) == b_of(b.mean_lo) && b_of(a.m2) == b_of(b.m2) &&
           b_of(a.m3) == b_of(b.m3) && b_of(a.m4) == b_of(b.m4);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s <case table>\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char kind[4];
    long line = 0;
    while (std::fscanf(f, "%3s", kind) == 1) {
        ++line;
        if (kind[0] == 'L') {                     // L n levels m0 m1 ...
            long long n; int levels;
            if (std::fscanf(f, "%lld %d", &n, &levels) != 2) { fail("L: short line", line); break; }
            bool ok = gm_levels(n) == levels;
            int64_t m = n;
            for (int l = 0; l < levels; ++l) {
                long long want;
                if (std::fscanf(f, "%lld", &want) != 1) { ok = false; break; }
                ok = ok && want == (long long)m && (l == levels - 1) == (m <= kGmTile);
                m = 2 * gm_tiles(m);
            }
            if (!ok) fail("L", line);
            ++rows[0];
        } else if (kind[0] == 'S') {              // S state stat is_some bits
            rdf_moments_state s; int stat, some; uint64_t bits;
            if (!read_state(f, s) || std::fscanf(f, "%d %d %" SCNx64, &stat, &some, &bits) != 3) { fail("S: short line", line); break; }
            double out = 0.0;
            const bool got = mo_stat(s, stat, &out);
            if (got != (some != 0) || (got && b_of(out) != bits)) fail("S", line);
            ++rows[1];
        } else if (kind[0] == 'Q') {              // Q count m2x m2y cxy stat is_some bits
            long long n; uint64_t b[3], bits; int stat, some;
            if (std::fscanf(f, "%lld %" SCNx64 " %" SCNx64 " %" SCNx64 " %d %d %" SCNx64, &n, &b[0], &b[1], &b[2], &stat, &some, &bits) != 7) { fail("Q: short line", line); break; }
            const rdf_comoments_state s{(int64_t)n, 0.0, 0.0, 0.0, 0.0, d_of(b[0]), d_of(b[1]), d_of(b[2])};
            double out = 0.0;
            const bool got = mo_costat(s, stat, &out);
            if (got != (some != 0) || (got && b_of(out) != bits)) fail("Q", line);
            ++rows[2];
        } else if (kind[0] == 'M') {              // M a b merged
            rdf_moments_state a, b, want;
            if (!read_state(f, a) || !read_state(f, b) || !read_state(f, want)) { fail("M: short line", line); break; }
            mo_merge(a, b);
            if (!same_state(a, want)) fail("M", line);
            ++rows[3];
        } else if (kind[0] == 'F') {              // F n groups, then n x (seg ok bits), then groups x state
            long long n, groups;
            if (std::fscanf(f, "%lld %lld", &n, &groups) != 2) { fail("F: short line", line); break; }
            std::vector<uint32_t> seg((size_t)n);
            std::vector<uint8_t> ok((size_t)n);
            std::vector<double> x((size_t)n);
            bool good = true;
            for (long long j = 0; j < n && good; ++j) {
                unsigned sg, o; uint64_t bits;
                good = std::fscanf(f, "%u %u %" SCNx64, &sg, &o, &bits) == 3;
                seg[(size_t)j] = sg; ok[(size_t)j] = (uint8_t)o; x[(size_t)j] = d_of(bits);
            }
            // one more state than there are groups: nothing may be written past the last group
            std::vector<rdf_moments_state> got((size_t)groups + 1, rdf_moments_state{-1, 0.0, 0.0, 0.0, 0.0, 0.0});
            if (good) gm_serial_moments(seg.data(), ok.data(), x.data(), n, got.data(), groups);
            for (long long g = 0; g < groups && good; ++g) {
                rdf_moments_state want;
                good = read_state(f, want);
                if (good && !same_state(got[(size_t)g], want)) { fail("F", line); break; }
            }
            if (!good) { fail("F: short case", line); break; }
            if (got[(size_t)groups].count != -1) fail("F: a state past the last group", line);
            ++rows[4];
        } else { fail("unknown line", line); break; }
    }
    std::fclose(f);
    std::printf("rows: L %ld S %ld Q %ld M %ld F %ld\n", rows[0], rows[1], rows[2], rows[3], rows[4]);
    std::printf("%ld checked, %d failed\n", rows[0] + rows[1] + rows[2] + rows[3] + rows[4], failed);
    return failed ? 1 : 0;
}
