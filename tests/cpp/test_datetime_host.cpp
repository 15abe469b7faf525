// rust_dataframe_amd/csrc/rdf_datetime.h under a plain host compiler (g++ -std=c++17, no HIP): the calendar arithmetic the
// kernels run, checked where it can be checked exhaustively —
//   round trip   days_from_civil(civil_from_days(d)) == d on every day of three whole eras (one negative, the one holding
//                1970, one far positive), on the 4096 days at each end of Int32 and on a stride-9973 walk across all of Int32;
//                along every run of consecutive days the civil date, the day of the year and the weekday step by one day
//   floor div    dt_floor_divmod against __int128 arithmetic at the ends of Int64 and around 0, every unit
//   the table    argv[1] = the table of tests/golden/datetime_cases.npz (tests/datetime_ref.py) as text:
//                unit value | 11 fields | 8 truncations | days months weekday | 4 shifts
// Usage: test_datetime_host <datetime_cases.txt>.  Exit status 0 = everything agreed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../rust_dataframe_amd/csrc/rdf_datetime.h"

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            if (++g_failed <= 20) { printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                  \
    } while (0)

static void round_trip(int64_t lo, int64_t hi, int64_t step) {
    DtCivil prev = {0, 0, 0, 0, 0, 0, false};
    bool have = false;
    for (int64_t z = lo; z <= hi; z += step) {
        const int32_t d = (int32_t)z;
        const DtCivil c = dt_civil_from_days(d);
        int32_t y; uint32_t m, dd;
        civil_from_days(d, y, m, dd);
        CHECK(y == c.year && m == c.month && dd == c.day, "day %d", d);
        CHECK(days_from_civil(c.year, c.month, c.day) == (int64_t)d, "day %d -> %d-%u-%u -> %lld", d, c.year, c.month, c.day, (long long)days_from_civil(c.year, c.month, c.day));
        CHECK(c.month >= 1 && c.month <= 12 && c.day >= 1 && c.day <= dt_last_day_of_month(c.year, c.month), "day %d -> %d-%u-%u", d, c.year, c.month, c.day);
        CHECK(c.wd == dt_weekday(d) && c.wd < 7, "day %d", d);
        CHECK(c.yday == (uint32_t)((int64_t)d - days_from_civil(c.year, 1, 1) + 1), "day %d: day of year %u", d, c.yday);
        const uint32_t wk = dt_iso_week(c);
        CHECK(wk >= 1 && wk <= 53, "day %d: week %u", d, wk);
        if (have && step == 1) {   // consecutive days: one step of the calendar
            const bool new_month = prev.day == dt_last_day_of_month(prev.year, prev.month);
            const bool new_year = new_month && prev.month == 12;
            CHECK(c.day == (new_month ? 1u : prev.day + 1), "day %d", d);
            CHECK(c.month == (new_year ? 1u : new_month ? prev.month + 1 : prev.month), "day %d", d);
            CHECK(c.year == prev.year + (new_year ? 1 : 0), "day %d", d);
            CHECK(c.wd == (prev.wd + 1) % 7, "day %d", d);
            CHECK(c.yday == (new_year ? 1u : prev.yday + 1), "day %d", d);
            const uint32_t pwk = dt_iso_week(prev);   // a week number changes on Mondays only: one more, or back to 1 after 52 / 53
            CHECK(c.wd == 0 ? (wk == pwk + 1 || (wk == 1 && pwk >= 52)) : wk == pwk, "day %d: week %u after %u", d, wk, pwk);
        }
        prev = c;
        have = true;
    }
}

template <uint64_t D>
static void floor_div_checks() {
    const int64_t probes[] = {INT64_MIN, INT64_MIN + 1, INT64_MIN + (int64_t)D, -(int64_t)D - 1, -(int64_t)D, -(int64_t)D + 1, -1, 0, 1,
                              (int64_t)D - 1, (int64_t)D, (int64_t)D + 1, INT64_MAX - (int64_t)D, INT64_MAX - 1, INT64_MAX};
    for (int64_t v : probes)
        for (int64_t k = -3; k <= 3; ++k) {
            const __int128 x = (__int128)v + k * 1000003;
            if (x < INT64_MIN || x > INT64_MAX) continue;
            int64_t q; uint64_t r;
            dt_floor_divmod<D>((int64_t)x, q, r);
            __int128 eq = x / (__int128)D, er = x % (__int128)D;
            if (er < 0) { er += D; eq -= 1; }
            CHECK((__int128)q == eq && (__int128)r == er, "floor_divmod<%llu>(%lld)", (unsigned long long)D, (long long)(int64_t)x);
            CHECK(dt_floor_div<D>((int64_t)x) == q && dt_floor_mod<D>((int64_t)x) == r, "floor_div / floor_mod");
        }
}

static int table(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { printf("cannot open %s\n", path); return 1; }
    char line[2048];
    long rows = 0;
    while (fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        long long x[2 + 11 + 8 + 3 + 4];
        int n = 0;
        for (char* tok = strtok(line, " \n"); tok && n < 28; tok = strtok(nullptr, " \n")) x[n++] = strtoll(tok, nullptr, 10);
        CHECK(n == 28, "%s: a line of %d numbers", path, n);
        if (n != 28) break;
        ++rows;
        const int unit = (int)x[0];
        const int64_t v = (int64_t)x[1];
        int32_t day; uint64_t rem;
        dt_split_rt(v, unit, day, rem);
        const DtCivil c = dt_civil_from_days(day);
        const uint32_t sod = dt_second_of_day_rt(rem, unit);
        for (int fld = 0; fld < DT_NFIELDS; ++fld)
            CHECK(dt_field(fld, day, c, sod) == (int32_t)x[2 + fld], "unit %d value %lld field %d: %d, expected %lld", unit, (long long)v, fld, dt_field(fld, day, c, sod), x[2 + fld]);
        for (int lv = 0; lv < DT_NLEVELS; ++lv) {
            if (!dt_trunc_level_ok(unit, lv)) { CHECK(unit == DT_UNIT_DAY && lv > DT_TRUNC_DAY, "level"); continue; }
            const uint64_t t = dt_trunc_rt(v, unit, lv);
            const int64_t got = unit == DT_UNIT_DAY ? (int64_t)(int32_t)(uint32_t)t : (int64_t)t;   // Date32 is Int32 storage
            CHECK(got == (int64_t)x[13 + lv], "unit %d value %lld trunc %d: %lld, expected %lld", unit, (long long)v, lv, (long long)got, x[13 + lv]);
        }
        const int32_t amounts[4] = {(int32_t)x[21], (int32_t)x[22], 0, (int32_t)x[23]};
        for (int op = 0; op < DT_NSHIFTS; ++op) {
            bool ok;
            const int32_t got = dt_shift(op, day, amounts[op], &ok);
            CHECK(ok && got == (int32_t)x[24 + op], "unit %d value %lld shift %d by %d: %d, expected %lld", unit, (long long)v, op, amounts[op], got, x[24 + op]);
        }
    }
    fclose(f);
    CHECK(rows >= 2000, "%s: only %ld rows", path, rows);
    printf("table: %ld rows\n", rows);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: %s <datetime_cases.txt>\n", argv[0]); return 2; }
    const int64_t era = kDtEraDays;
    round_trip(-719468 - 3000 * era, -719468 - 2999 * era - 1, 1);   // a negative era
    round_trip(-719468 + 4 * era, -719468 + 5 * era - 1, 1);         // 1600-03-01 .. 2000-02-29: holds 1970
    round_trip(-719468 + 14000 * era, -719468 + 14001 * era - 1, 1); // a far positive one
    round_trip(INT32_MIN, (int64_t)INT32_MIN + 4095, 1);
    round_trip((int64_t)INT32_MAX - 4095, INT32_MAX, 1);
    round_trip(INT32_MIN, INT32_MAX, 9973);
    floor_div_checks<86400ull>(); floor_div_checks<86400000ull>(); floor_div_checks<86400000000ull>(); floor_div_checks<86400000000000ull>();
    floor_div_checks<1ull>(); floor_div_checks<1000ull>(); floor_div_checks<1000000ull>(); floor_div_checks<1000000000ull>();
    bool ok;
    CHECK(dt_shift(DT_SHIFT_NEXT_DAY, 0, 0, &ok) == 0 && !ok, "next_day(0)");
    CHECK(dt_shift(DT_SHIFT_NEXT_DAY, 0, 8, &ok) == 0 && !ok, "next_day(8)");
    CHECK(dt_shift(DT_SHIFT_DAYS, INT32_MAX, 1, &ok) == INT32_MIN && ok, "date_add wraps");
    if (table(argv[1])) return 2;
    printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
