// The top-bits decision of a numeric sort column (rust_dataframe_amd/csrc/rdf_sort_plan.h) on the CPU: the function
// os_column_passes calls.  Pass widths, the LDS word's bit budget, every threshold where the route flips — among them the third
// pass at 118 030 336 rows, which no GPU test can reach in seconds — and the top-digit limit.  Stand-alone: no library, no device.
#include <cstdint>
#include <initializer_list>

#include "mini_test.hpp"
#include "../../rust_dataframe_amd/csrc/rdf_sort_plan.h"

using namespace rdfk;

namespace {

// what holds for every eligible plan
void check_plan(const OsTopPlan& p, int sig) {
    CHECK(p.eligible == 1);
    CHECK(p.B >= 12 && p.B <= 24);
    CHECK_EQ(p.npass, (p.B + 7) / 8);
    CHECK(p.npass >= 2 && p.npass <= 3);
    int sum = 0, sh = p.R;
    for (int i = 0; i < p.npass; ++i) {
        int w = 0;
        for (int m = p.mask[i]; m; m >>= 1) { CHECK(m & 1); ++w; }      // a mask is 2^w - 1
        CHECK(w >= 1 && w <= 8);
        if (i > 0) CHECK_EQ(w, 8);                                      // pass 0 takes the remainder, the others whole bytes
        CHECK_EQ(p.shift[i], sh);                                       // the digits tile [R, R + B) from the bottom up
        sh += w; sum += w;
    }
    CHECK_EQ(sum, p.B);
    CHECK_EQ(8 * (p.npass - 1) + (p.B - 8 * (p.npass - 1)), p.B);
    CHECK(p.R >= 0 && p.R + 12 <= 64);                                  // the narrow LDS word: (R bits << 12) | place
    if (!p.value) CHECK_EQ(p.R + p.B, sig); else CHECK_EQ(p.R, 0);
    CHECK_EQ(p.wtop, p.npass == 1 ? p.B : 8);
    CHECK_EQ(p.top_limit, (int64_t)kOsPlanLocalMax << (p.B - p.wtop));
}

const int64_t kThird = (int64_t)1801 << 16;      // the first n with (n >> 16) > 1800

}  // namespace

TEST(every_eligible_plan_tiles_its_top_bits) {
    for (int64_t n : {(int64_t)65536, (int64_t)70001, (int64_t)200000, (int64_t)1 << 21, (int64_t)4000000, (int64_t)100000000, kThird - 1, kThird, (int64_t)1 << 30, ((int64_t)1 << 32) - 1})
        for (int sig = 25; sig <= 64; ++sig)
            for (int kind : {(int)OS_KEYS_INT, (int)OS_KEYS_F64, (int)OS_KEYS_F64_DESC}) {
                const OsTopPlan p = os_top_plan(n, sig, 8, kind, 0, false, true);
                if (p.eligible) check_plan(p, sig);
                if (kind == OS_KEYS_INT) CHECK_EQ(p.eligible, sig - p.B <= 52 && (sig + 7) / 8 >= (p.B + 7) / 8 + 2 ? 1 : 0);
                for (int vb = 12; vb <= 24; ++vb) {                      // value maps: sampled ones are taken at any rows per bucket
                    const OsTopPlan q = os_top_plan(n, sig, 8, OS_KEYS_F64, vb, true, true);
                    CHECK_EQ(q.B, vb);
                    CHECK_EQ(q.eligible, (sig + 7) / 8 >= (vb + 7) / 8 + 2 ? 1 : 0);
                    if (q.eligible) { check_plan(q, sig); CHECK(q.value == 1 && q.check_top == 0); }
                }
            }
}

TEST(eligibility_flips_at_65536_rows_and_at_25_bits) {
    CHECK_EQ(os_top_plan(65535, 64, 8, OS_KEYS_INT, 0, false, true).eligible, 0);
    CHECK_EQ(os_top_plan(65536, 64, 8, OS_KEYS_INT, 0, false, true).eligible, 1);
    CHECK_EQ(os_top_plan(65535, 25, 4, OS_KEYS_INT, 0, false, true).eligible, 0);
    CHECK_EQ(os_top_plan(65536, 25, 4, OS_KEYS_INT, 0, false, true).eligible, 1);
    CHECK_EQ(os_top_plan(65536, 24, 4, OS_KEYS_INT, 0, false, true).eligible, 0);
    CHECK_EQ(os_top_plan(65536, 24, 8, OS_KEYS_INT, 0, false, true).eligible, 0);
    CHECK_EQ(os_top_plan(200000, 24, 8, OS_KEYS_F64, 0, false, true).eligible, 0);
    CHECK_EQ(os_top_plan(200000, 25, 8, OS_KEYS_F64, 0, false, true).eligible, 1);
    for (int64_t n : {(int64_t)65536, (int64_t)4000000}) {
        CHECK_EQ(os_top_plan(n, 64, 8, OS_KEYS_INT, 0, false, false).eligible, 0);      // sort_msd = 0
        CHECK_EQ(os_top_plan(n, 32, 4, OS_KEYS_F32, 0, false, true).eligible, 0);        // 4-byte floats never
        CHECK_EQ(os_top_plan(n, 64, 8, OS_KEYS_F64, 12, true, false).eligible, 0);
    }
    CHECK_EQ(os_top_plan(((int64_t)1 << 32) - 1, 64, 8, OS_KEYS_INT, 0, false, true).eligible, 1);
    CHECK_EQ(os_top_plan((int64_t)1 << 32, 64, 8, OS_KEYS_INT, 0, false, true).eligible, 0);
    // sig is held to the bytes the dtype has
    CHECK_EQ(os_top_plan(65536, 64, 3, OS_KEYS_INT, 0, false, true).eligible, 0);
    const OsTopPlan p = os_top_plan(65536, 64, 4, OS_KEYS_INT, 0, false, true);
    CHECK(p.eligible == 1 && p.R == 20 && p.B == 12);
    CHECK_EQ(os_sig_bits(0, 8), 0);
    CHECK_EQ(os_sig_bits(1, 8), 1);
    CHECK_EQ(os_sig_bits(0xFFFFFF, 8), 24);
    CHECK_EQ(os_sig_bits(0x1000000, 8), 25);
    CHECK_EQ(os_sig_bits(~0ull, 8), 64);
    CHECK_EQ(os_sig_bits(~0ull, 4), 32);
}

TEST(raw_bits_leave_at_most_52_to_the_lds_finish) {
    // R + 12 <= 64: a 64-bit range at B = 12 is exactly the word; the plan never asks for more
    OsTopPlan p = os_top_plan(65536, 64, 8, OS_KEYS_INT, 0, false, true);
    CHECK(p.eligible == 1 && p.B == 12 && p.R == 52 && p.npass == 2);
    CHECK(p.shift[0] == 52 && p.mask[0] == 15 && p.shift[1] == 56 && p.mask[1] == 255);
    CHECK_EQ(p.top_limit, (int64_t)65536);       // 4096 << (12 - 8): cannot fire below 65 537 rows
    p = os_top_plan(65536, 25, 8, OS_KEYS_INT, 0, false, true);
    CHECK(p.eligible == 1 && p.R == 13 && p.shift[0] == 13 && p.shift[1] == 17);
    // a value map has no R and may take three passes at any row count
    p = os_top_plan(70001, 64, 8, OS_KEYS_F64, 24, true, true);
    CHECK(p.eligible == 1 && p.value == 1 && p.R == 0 && p.npass == 3 && p.check_top == 0);
    CHECK(p.shift[0] == 0 && p.shift[1] == 8 && p.shift[2] == 16 && p.mask[0] == 255);
    p = os_top_plan(70001, 64, 8, OS_KEYS_F64, 17, true, true);
    CHECK(p.eligible == 1 && p.npass == 3 && p.mask[0] == 1 && p.shift[1] == 1 && p.shift[2] == 9);
    // linear over [min, max] (sort_sample 0): a value map, but the top digit is still checked
    p = os_top_plan(70001, 64, 8, OS_KEYS_F64_DESC, 12, false, true);
    CHECK(p.eligible == 1 && p.value == 1 && p.R == 0 && p.check_top == 1 && p.B == 12);
}

TEST(bits_grow_with_the_rows_and_a_third_pass_starts_at_118030336) {
    // B = 12 while (n >> 12) <= 512: through 2^21 + 2^9 and up to 2^21 + 2^12 - 1 rows, 13 from there
    for (int64_t n : {(int64_t)65536, (int64_t)1 << 21, ((int64_t)1 << 21) + 511, ((int64_t)1 << 21) + 512, ((int64_t)513 << 12) - 1})
        for (int kind : {(int)OS_KEYS_INT, (int)OS_KEYS_F64}) CHECK_EQ(os_bits_by_rows(n, kind), 12);
    CHECK_EQ(os_bits_by_rows((int64_t)513 << 12, OS_KEYS_INT), 13);
    CHECK_EQ(os_bits_by_rows((int64_t)513 << 12, OS_KEYS_F64), 13);
    CHECK_EQ(os_bits_by_rows(4000000, OS_KEYS_INT), 13);
    int prev = 12;
    for (int64_t n = 65536; n < ((int64_t)1 << 32); n += n / 64) {
        const int b = os_bits_by_rows(n, OS_KEYS_INT);
        CHECK(b >= prev);
        prev = b;
        const OsTopPlan p = os_top_plan(n, 64, 8, OS_KEYS_INT, 0, false, true);
        CHECK(p.eligible == 1);                                         // an 8-byte integer column is always taken
        CHECK((n >> p.B) <= kOsRowsPerBucketInt);
        CHECK_EQ(p.npass, n < kThird ? 2 : 3);
        check_plan(p, 64);
    }
    CHECK_EQ(kThird, (int64_t)118030336);
    OsTopPlan p = os_top_plan(kThird - 1, 64, 8, OS_KEYS_INT, 0, false, true);
    CHECK(p.eligible == 1 && p.npass == 2 && p.B == 16 && p.R == 48);
    CHECK_EQ(p.top_limit, (int64_t)4096 << 8);
    p = os_top_plan(kThird, 64, 8, OS_KEYS_INT, 0, false, true);
    CHECK(p.eligible == 1 && p.npass == 3 && p.B == 18 && p.R == 46);
    CHECK(p.mask[0] == 3 && p.shift[0] == 46 && p.shift[1] == 48 && p.shift[2] == 56);
    CHECK_EQ(p.top_limit, (int64_t)4096 << 10);
    // three top passes and the finish must still save two byte passes: keys of 4 bytes keep the byte passes, 33 bits are taken
    CHECK_EQ(os_top_plan(kThird, 32, 8, OS_KEYS_INT, 0, false, true).eligible, 0);
    CHECK_EQ(os_top_plan(kThird, 33, 8, OS_KEYS_INT, 0, false, true).eligible, 1);
    // doubles on raw bits: ~512 per bucket, so the bits go on past 16
    CHECK_EQ(os_bits_by_rows(200000, OS_KEYS_F64), 12);
    CHECK_EQ(os_bits_by_rows(50000000, OS_KEYS_F64), 17);
    CHECK_EQ(os_bits_by_rows(((int64_t)1 << 32) - 1, OS_KEYS_F64), 23);
    p = os_top_plan(200000, 59, 8, OS_KEYS_F64, 0, false, true);
    CHECK(p.eligible == 1 && p.R == 47 && p.value == 0 && p.check_top == 1);
    CHECK_EQ(os_top_plan(200000, 64, 8, OS_KEYS_F64, 0, false, true).R, 52);
}

int main() { return run_all(); }
