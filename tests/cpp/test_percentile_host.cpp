// rust_dataframe_amd/csrc/rdf_percentile.h under a plain host compiler (g++ -std=c++17, no HIP): the functions the pick kernel
// runs for one group and one call — d(v), the rank rule, the DISC index, the interpolation, the test of p — and the select
// route's decisions — the ordered key of a value and the way back, the planner step on a digit histogram — over the table
// that tests/percentile_ref.py writes (argv[1]; the formats of its lines are described there).  Every double of the table is
// its bits in hex; counts and positions are decimal.
// Usage: test_percentile_host <percentile_cases.txt>.  Exit status 0 = everything agreed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rust_dataframe_amd/csrc/rdf_percentile.h"

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            if (++g_failed <= 20) { printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                  \
    } while (0)

static double dbl(uint64_t bits) { return __builtin_bit_cast(double, bits); }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <percentile_cases.txt>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    long rows[256] = {0};
    std::vector<char> line_buf(1 << 16);
    char* const buf = line_buf.data();
    long line = 0;
    while (fgets(buf, (int)line_buf.size(), f)) {
        ++line;
        const char kind = buf[0];
        const char* rest = buf + 1;
        bool parsed = false;
        if (kind == 'D') {
            int dtype; uint64_t raw, want;
            if ((parsed = sscanf(rest, "%d %" SCNx64 " %" SCNx64, &dtype, &raw, &want) == 3)) {
                const uint64_t got = pct_bits(pct_d(dtype, raw));
                CHECK(got == want, "line %ld: d(%d, %" PRIx64 ") = %016" PRIx64 ", the model has %016" PRIx64, line, dtype, raw, got, want);
            }
        } else if (kind == 'R') {
            long long m, lo, hi; uint64_t p, wlo, whi;
            if ((parsed = sscanf(rest, "%lld %" SCNx64 " %lld %lld %" SCNx64 " %" SCNx64, &m, &p, &lo, &hi, &wlo, &whi) == 6)) {
                const PctRank r = pct_rank(m, dbl(p));
                CHECK(r.lo == lo && r.hi == hi, "line %ld: m %lld: positions %lld %lld, the model has %lld %lld", line, m, (long long)r.lo, (long long)r.hi, lo, hi);
                CHECK(pct_bits(r.wlo) == wlo && pct_bits(r.whi) == whi, "line %ld: m %lld: weights %016" PRIx64 " %016" PRIx64, line, m, pct_bits(r.wlo), pct_bits(r.whi));
                CHECK(r.lo >= 0 && r.lo <= r.hi && r.hi <= m - 1 && r.hi - r.lo <= 1, "line %ld: m %lld: positions out of the group", line, m);
            }
        } else if (kind == 'K') {
            long long m, k; uint64_t p;
            if ((parsed = sscanf(rest, "%lld %" SCNx64 " %lld", &m, &p, &k) == 3)) {
                const int64_t got = pct_disc_index(m, dbl(p));
                CHECK(got == k, "line %ld: m %lld: index %lld, the model has %lld", line, m, (long long)got, k);
                CHECK(got >= 0 && got <= m - 1, "line %ld: m %lld: index out of the group", line, m);
            }
        } else if (kind == 'I') {
            long long m; uint64_t p, dlo, dhi, want; int peers;
            if ((parsed = sscanf(rest, "%lld %" SCNx64 " %" SCNx64 " %" SCNx64 " %d %" SCNx64, &m, &p, &dlo, &dhi, &peers, &want) == 6)) {
                const uint64_t got = pct_interpolate(pct_rank(m, dbl(p)), dbl(dlo), dbl(dhi), peers != 0);
                CHECK(got == want, "line %ld: m %lld: %016" PRIx64 ", the model has %016" PRIx64, line, m, got, want);
            }
        } else if (kind == 'P') {
            uint64_t p; int ok;
            if ((parsed = sscanf(rest, "%" SCNx64 " %d", &p, &ok) == 2))
                CHECK(pct_p_ok(dbl(p)) == (ok != 0), "line %ld: p %016" PRIx64, line, p);
        }
        else if (kind == 'Q') {
            int dtype; uint64_t raw, key, back;
            if ((parsed = sscanf(rest, "%d %" SCNx64 " %" SCNx64 " %" SCNx64, &dtype, &raw, &key, &back) == 4)) {
                const uint64_t got = pct_key(dtype, raw);
                CHECK(got == key, "line %ld: key(%d, %" PRIx64 ") = %" PRIx64 ", the model has %" PRIx64, line, dtype, raw, got, key);
                CHECK(pct_unkey(dtype, key) == back, "line %ld: unkey(%d, %" PRIx64 ") = %" PRIx64 ", the model has %" PRIx64, line, dtype, key, pct_unkey(dtype, key), back);
                CHECK(pct_key(dtype, pct_unkey(dtype, got)) == got, "line %ld: the key does not survive the round trip", line);
                const int bits = pct_key_bits(dtype);
                CHECK((bits == 8 || bits == 16 || bits == 32 || bits == 64) && (bits == 64 || (got >> bits) == 0), "line %ld: a key wider than its %d bits", line, bits);
                CHECK(pct_bits(pct_d(dtype, pct_unkey(dtype, got))) == pct_bits(pct_d(dtype, raw)), "line %ld: d() of the key's value differs from d() of the value", line);
            }
        } else if (kind == 'O') {
            int dtype, want; uint64_t ra, rb;
            if ((parsed = sscanf(rest, "%d %" SCNx64 " %" SCNx64 " %d", &dtype, &ra, &rb, &want) == 4)) {
                const uint64_t ka = pct_key(dtype, ra), kb = pct_key(dtype, rb);
                const int got = (ka > kb) - (ka < kb);
                CHECK(got == want, "line %ld: dtype %d: keys order %" PRIx64 " and %" PRIx64 " as %d, the values as %d", line, dtype, ra, rb, got, want);
            }
        } else if (kind == 'B') {
            int nb = 0, used = 0, want_bucket = 0; unsigned long long res = 0, want_res = 0;
            if (sscanf(rest, "%d %llu %d %llu%n", &nb, &res, &want_bucket, &want_res, &used) == 4 && nb > 0 && nb <= 4096) {
                std::vector<uint32_t> hist((size_t)nb);      // exactly nb counters: a step past them is the sanitizer's to find
                const char* at = rest + used;
                parsed = true;
                for (int b = 0; b < nb && parsed; ++b) {
                    char* end = nullptr;
                    const unsigned long long v = strtoull(at, &end, 10);
                    parsed = end != at && v <= 0xFFFFFFFFull;
                    hist[(size_t)b] = (uint32_t)v;
                    at = end;
                }
                if (parsed) {
                    uint64_t r = res;
                    const int got = pct_plan_bucket(hist.data(), nb, &r);
                    CHECK(got == want_bucket && r == want_res, "line %ld: rank %llu: bucket %d residual %llu, the model has %d %llu", line, res, got, (unsigned long long)r, want_bucket, want_res);
                    CHECK(got >= 0 && got < nb, "line %ld: a bucket outside the histogram", line);
                }
            }
        }
        if (!parsed) { fprintf(stderr, "line %ld: cannot read: %s", line, buf); fclose(f); return 2; }
        ++rows[(unsigned char)kind];
    }
    fclose(f);
    printf("rows: D %ld R %ld K %ld I %ld P %ld Q %ld O %ld B %ld\n", rows['D'], rows['R'], rows['K'], rows['I'], rows['P'], rows['Q'], rows['O'], rows['B']);
    printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
