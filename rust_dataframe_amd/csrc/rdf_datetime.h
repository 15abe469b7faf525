// rdf_datetime.h — the calendar arithmetic of rdf_datetime_fields / rdf_datetime_trunc / rdf_date_shift / rdf_date_diff
// (kernels: rdf_datetime.hip, host side: rdf_capi_datetime.inc).  ONE definition, __host__ __device__ inline: hipcc compiles
// it into the kernels, plain g++ compiles it into tests/cpp/test_datetime_host.cpp.  It includes nothing of HIP.
//
// Rules kept throughout:
//   no UB       everything that can wrap is computed in unsigned types; signed values are only shifted right (arithmetic,
//               i.e. floor) or divided by positive constants
//   no tables   month lengths, weekday and week numbers are closed forms
//   constants   every divisor is a compile-time constant: the compiler turns it into a multiply-high
//   32 bits     one 64-bit floor division gives the day number and the remainder inside the day; from there on the
//               civil date, the weekday and (except for nanoseconds) the second of the day are 32-bit arithmetic
//
// The calendar is the proleptic Gregorian one with astronomical year numbering (year 0 = 1 BC), day 0 = 1970-01-01, a
// Thursday.  civil_from_days / days_from_civil are the era / day-of-era formulation (an era = 400 years = 146 097 days =
// 20 871 weeks), exact for EVERY Int32 day number: -5877641-06-23 .. 5881580-07-11.
//
// Domain rule ("integers wrap", as rdf_binary): the day number of a value is floor_div(value, units per day) in Int64,
// truncated to Int32 by wrapping — reached only by Int64 seconds / milliseconds beyond year +-5.8 million.  Time-of-day
// fields are exact for every Int64.  Nothing fails or becomes NULL because of a value's magnitude.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RDF_DT_HD __host__ __device__ inline
#else
#define RDF_DT_HD inline
#endif

// rdf_time_unit / rdf_datetime_field / rdf_trunc_level / rdf_date_shift_op of include/rdf_mi355x.h, restated so that this
// header stands alone (rdf_capi_datetime.inc static_asserts that they agree)
enum : int { DT_UNIT_S = 0, DT_UNIT_MS = 1, DT_UNIT_US = 2, DT_UNIT_NS = 3, DT_UNIT_DAY = 4 };
enum : int { DT_YEAR = 0, DT_QUARTER, DT_MONTH, DT_DAY_OF_MONTH, DT_DAY_OF_WEEK, DT_DAY_OF_YEAR, DT_WEEK_OF_YEAR, DT_HOUR, DT_MINUTE, DT_SECOND, DT_DATE, DT_NFIELDS };
enum : int { DT_TRUNC_YEAR = 0, DT_TRUNC_QUARTER, DT_TRUNC_MONTH, DT_TRUNC_WEEK, DT_TRUNC_DAY, DT_TRUNC_HOUR, DT_TRUNC_MINUTE, DT_TRUNC_SECOND, DT_NLEVELS };
enum : int { DT_SHIFT_DAYS = 0, DT_SHIFT_MONTHS, DT_SHIFT_LAST_DAY, DT_SHIFT_NEXT_DAY, DT_NSHIFTS };

constexpr uint32_t kDtEraDays = 146097;      // days of 400 Gregorian years; a multiple of 7
constexpr uint32_t kDtEpochShift = 719468;   // 0000-03-01 .. 1970-01-01
constexpr uint32_t kDtEraBias = 14695;       // eras added to a negative day number: 14695 * 146097 = 2 146 895 415

template <int UNIT> struct DtUnit;
template <> struct DtUnit<DT_UNIT_S>   { static constexpr uint64_t per_second = 1ull,          per_day = 86400ull; };
template <> struct DtUnit<DT_UNIT_MS>  { static constexpr uint64_t per_second = 1000ull,       per_day = 86400000ull; };
template <> struct DtUnit<DT_UNIT_US>  { static constexpr uint64_t per_second = 1000000ull,    per_day = 86400000000ull; };
template <> struct DtUnit<DT_UNIT_NS>  { static constexpr uint64_t per_second = 1000000000ull, per_day = 86400000000000ull; };
template <> struct DtUnit<DT_UNIT_DAY> { static constexpr uint64_t per_second = 0ull,          per_day = 1ull; };

constexpr int dt_ctz(uint64_t d) { return (d & 1) ? 0 : 1 + dt_ctz(d >> 1); }

// q = floor(v / D), r = v - q D in [0, D) for a positive constant D = 2^K M (M odd).  floor(v / D) = floor(floor(v / 2^K) / M);
// the inner floor is an arithmetic shift, the outer one an UNSIGNED division after adding a multiple of M that makes the
// operand non-negative (it is taken off the quotient again).  r is put together from the remainder by M and v's low K bits.
template <uint64_t D>
RDF_DT_HD void dt_floor_divmod(int64_t v, int64_t& q, uint64_t& r) {
    constexpr int K = dt_ctz(D);
    constexpr uint64_t M = D >> K;
    constexpr uint64_t QB = ((1ull << (63 - K)) + M - 1) / M;   // M QB >= 2^(63-K) > -floor(v / 2^K), and v / 2^K + M QB < 2^64
    const uint64_t t = (uint64_t)(v >> K) + M * QB;
    const uint64_t tq = t / M;
    q = (int64_t)(tq - QB);
    r = ((t - tq * M) << K) | ((uint64_t)v & ((1ull << K) - 1));
}
template <uint64_t D> RDF_DT_HD int64_t dt_floor_div(int64_t v) { int64_t q; uint64_t r; dt_floor_divmod<D>(v, q, r); return q; }
template <uint64_t D> RDF_DT_HD uint64_t dt_floor_mod(int64_t v) { int64_t q; uint64_t r; dt_floor_divmod<D>(v, q, r); return r; }

RDF_DT_HD int32_t dt_wrap32(int64_t v) { return (int32_t)(uint32_t)(uint64_t)v; }
RDF_DT_HD int32_t dt_add32(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
RDF_DT_HD int32_t dt_sub32(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }

// value -> (day number wrapped to Int32, units into the day).  RDF_TIME_DAY: the identity (the value is truncated to Int32).
template <int UNIT>
RDF_DT_HD void dt_split(int64_t v, int32_t& day, uint64_t& rem) {
    if (UNIT == DT_UNIT_DAY) { day = dt_wrap32(v); rem = 0; return; }
    int64_t q;
    dt_floor_divmod<DtUnit<UNIT>::per_day>(v, q, rem);
    day = dt_wrap32(q);
}
// ... -> the whole second of the day, 0..86399 (17 bits): the fraction is dropped by floor
template <int UNIT>
RDF_DT_HD uint32_t dt_second_of_day(uint64_t rem) {
    if (UNIT == DT_UNIT_S) return (uint32_t)rem;
    if (UNIT == DT_UNIT_MS) return (uint32_t)rem / 1000u;                 // rem < 86.4e6
    if (UNIT == DT_UNIT_US) return (uint32_t)(rem >> 6) / 15625u;         // 1e6 = 2^6 15625, rem >> 6 < 1.35e9
    if (UNIT == DT_UNIT_NS) return (uint32_t)(rem / 1000000000ull);       // rem < 2^47: the one other 64-bit division
    return 0;
}
// the same with the unit known only at run time (it is the same for every row of a call)
RDF_DT_HD void dt_split_rt(int64_t v, int unit, int32_t& day, uint64_t& rem) {
    switch (unit) {
        case DT_UNIT_S: dt_split<DT_UNIT_S>(v, day, rem); break;
        case DT_UNIT_MS: dt_split<DT_UNIT_MS>(v, day, rem); break;
        case DT_UNIT_US: dt_split<DT_UNIT_US>(v, day, rem); break;
        case DT_UNIT_NS: dt_split<DT_UNIT_NS>(v, day, rem); break;
        default: dt_split<DT_UNIT_DAY>(v, day, rem); break;
    }
}
RDF_DT_HD uint32_t dt_second_of_day_rt(uint64_t rem, int unit) {
    switch (unit) {
        case DT_UNIT_S: return dt_second_of_day<DT_UNIT_S>(rem);
        case DT_UNIT_MS: return dt_second_of_day<DT_UNIT_MS>(rem);
        case DT_UNIT_US: return dt_second_of_day<DT_UNIT_US>(rem);
        case DT_UNIT_NS: return dt_second_of_day<DT_UNIT_NS>(rem);
        default: return 0;
    }
}

// day number -> (era, day of era).  day + 719468 does not fit 32 bits at the top of the range and is negative at the bottom:
// a negative day number is moved up by 14695 whole eras first, then both halves fit an unsigned 32-bit word.
RDF_DT_HD void dt_era(int32_t day, int32_t& era, uint32_t& doe) {
    const bool neg = day < 0;
    const uint32_t z = (uint32_t)day + kDtEpochShift + (neg ? kDtEraBias * kDtEraDays : 0u);
    const uint32_t e = z / kDtEraDays;
    doe = z - e * kDtEraDays;
    era = (int32_t)e - (neg ? (int32_t)kDtEraBias : 0);
}

// floor(x / D) for 0 <= x <= XMAX as ONE multiplication of two numbers below 2^24 and a shift: 32 x 32-bit multiplications
// (v_mul_hi_u32, v_mul_lo_u32) issue at a quarter of the rate of the 24-bit ones on CDNA, and everything after the day of
// the era is small.  M = ceil(2^S / D); exact because XMAX (M D - 2^S) < 2^S (checked at compile time); the masks tell the
// compiler that both factors fit 24 bits.  Where the product fits 32 bits it is one instruction; with S >= 32 only its high word is needed.
template <uint32_t D, int S, uint32_t XMAX>
RDF_DT_HD uint32_t dt_div24(uint32_t x) {
    constexpr uint64_t M = ((1ull << S) + D - 1) / D;
    static_assert(M < (1ull << 24) && XMAX < (1u << 24), "24-bit factors");
    static_assert((uint64_t)XMAX * (M * D - (1ull << S)) < (1ull << S), "exact up to XMAX");
    if ((uint64_t)XMAX * M < (1ull << 32)) return ((x & 0xFFFFFFu) * (uint32_t)M) >> S;
    return (uint32_t)(((uint64_t)(x & 0xFFFFFFu) * (uint64_t)(uint32_t)M) >> S);
}

RDF_DT_HD bool dt_leap400(uint32_t yy) {   // is a year that is yy (0..400) modulo 400 a leap year
    return (yy & 3u) == 0 && (yy - 100u * dt_div24<100, 16, 400>(yy) != 0 || yy == 0 || yy == 400u);
}
RDF_DT_HD uint32_t dt_month_length(bool leap, uint32_t m) { return m == 2 ? (leap ? 29u : 28u) : 30u + ((m + (m >> 3)) & 1u); }

// weekday index, Monday = 0 .. Sunday = 6 (day 0 is a Thursday = 3).  An era is a whole number of weeks and
// 719468 = 1 (mod 7), so day + 3 = day of era + 2 (mod 7).
RDF_DT_HD uint32_t dt_weekday_of_doe(uint32_t doe) { return doe + 2u - 7u * dt_div24<7, 26, 146098>(doe + 2u); }
RDF_DT_HD uint32_t dt_weekday(int32_t day) { int32_t era; uint32_t doe; dt_era(day, era, doe); return dt_weekday_of_doe(doe); }

RDF_DT_HD bool dt_is_leap(int32_t y) { return (y & 3) == 0 && ((y % 25) != 0 || (y & 15) == 0); }
RDF_DT_HD uint32_t dt_last_day_of_month(int32_t y, uint32_t m) { return m == 2 ? (dt_is_leap(y) ? 29u : 28u) : 30u + ((m + (m >> 3)) & 1u); }

struct DtCivil {
    int32_t  year;
    uint32_t month, day;   // 1..12, 1..31
    uint32_t yday;         // 1..366
    uint32_t wd;           // Monday = 0 .. Sunday = 6
    uint32_t yy;           // the year modulo 400, 0..400 (400: January and February of a year that 400 divides)
    bool     leap;
};

RDF_DT_HD DtCivil dt_civil_from_days(int32_t z) {
    int32_t era;
    uint32_t doe;
    dt_era(z, era, doe);                                                              // doe < 146097 < 2^18
    const uint32_t t = doe - dt_div24<1460, 34, 146096>(doe) + dt_div24<36524, 39, 146096>(doe) - (doe == 146096u ? 1u : 0u);
    const uint32_t yoe = dt_div24<365, 32, 146096>(t);                                // [0, 399]
    const uint32_t c100 = dt_div24<100, 16, 400>(yoe);
    const uint32_t doy = doe - (365u * yoe + (yoe >> 2) - c100);                      // [0, 365], 0 = March 1
    const uint32_t mp = dt_div24<153, 18, 1832>(5u * doy + 2u);                       // [0, 11], 0 = March
    DtCivil c;
    c.day = doy - dt_div24<5, 16, 1687>(153u * mp + 2u) + 1u;
    c.month = mp < 10u ? mp + 3u : mp - 9u;
    const uint32_t yy = yoe + (mp >= 10u ? 1u : 0u);                                  // the year inside its 400: [0, 400]
    c.year = (int32_t)yy + era * 400;
    c.yy = yy;
    c.leap = dt_leap400(yy);                                                          // = dt_is_leap(c.year): 400 divides era * 400
    c.yday = mp < 10u ? doy + 60u + (c.leap ? 1u : 0u) : doy - 305u;
    c.wd = dt_weekday_of_doe(doe);
    return c;
}
RDF_DT_HD void civil_from_days(int32_t z, int32_t& year, uint32_t& month, uint32_t& day) {
    const DtCivil c = dt_civil_from_days(z);
    year = c.year; month = c.month; day = c.day;
}

// exact in Int64 for every |year| < 4e8 (add_months of an Int32 day number by an Int32 amount stays below 1.9e8)
RDF_DT_HD int64_t days_from_civil(int32_t y, uint32_t m, uint32_t d) {
    const uint32_t yb = (uint32_t)y - (m <= 2u ? 1u : 0u) + 400000000u;   // years since -400 000 000-03-01
    const uint32_t era = yb / 400u, yoe = yb - era * 400u;
    const uint32_t doy = (153u * (m > 2u ? m - 3u : m + 9u) + 2u) / 5u + d - 1u;
    const uint32_t doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;
    return ((int64_t)era - 1000000) * (int64_t)kDtEraDays + (int64_t)doe - (int64_t)kDtEpochShift;
}

// ISO-8601 week, 1..53: the week (Monday first) that holds the year's first Thursday is week 1
RDF_DT_HD uint32_t dt_iso_week(const DtCivil& c) {
    const uint32_t w = dt_div24<7, 16, 400>(c.yday + 9u - c.wd);   // (yday - iso weekday + 10) / 7
    if (w == 0) {                                            // the last week of the year before: that of its December 31st
        const uint32_t plen = 365u + (c.yy != 0 && dt_leap400(c.yy - 1u) ? 1u : 0u);   // (yy = 0: the year before is 399 mod 400)
        const uint32_t d = c.wd + 7u - c.yday, pwd = d >= 7u ? d - 7u : d;             // yday is 1..3 here
        return dt_div24<7, 16, 400>(plen + 9u - pwd);
    }
    if (w == 53) {                                           // week 1 of the next year when this week's Thursday lies there
        const uint32_t ylen = 365u + (c.leap ? 1u : 0u);
        if (c.yday + 3u > ylen + c.wd) return 1u;            // Thursday = this day + (3 - wd)
    }
    return w;
}

RDF_DT_HD bool dt_field_is_civil(int f) { return f <= DT_WEEK_OF_YEAR; }              // needs dt_civil_from_days
RDF_DT_HD bool dt_field_is_time(int f) { return f >= DT_HOUR && f <= DT_SECOND; }     // needs the second of the day

// one field (Spark 3): DAY_OF_WEEK 1 = Sunday .. 7 = Saturday, WEEK_OF_YEAR the ISO week, QUARTER 1..4, DATE the day number
RDF_DT_HD int32_t dt_field(int f, int32_t day, const DtCivil& c, uint32_t sod) {
    switch (f) {
        case DT_YEAR: return c.year;
        case DT_QUARTER: return (int32_t)dt_div24<3, 16, 16>(c.month + 2u);
        case DT_MONTH: return (int32_t)c.month;
        case DT_DAY_OF_MONTH: return (int32_t)c.day;
        case DT_DAY_OF_WEEK: return (int32_t)(c.wd == 6u ? 1u : c.wd + 2u);
        case DT_DAY_OF_YEAR: return (int32_t)c.yday;
        case DT_WEEK_OF_YEAR: return (int32_t)dt_iso_week(c);
        case DT_HOUR: return (int32_t)dt_div24<3600, 35, 86399>(sod);
        case DT_MINUTE: { const uint32_t m = dt_div24<60, 29, 86399>(sod); return (int32_t)(m - 60u * dt_div24<60, 16, 1439>(m)); }
        case DT_SECOND: return (int32_t)(sod - 60u * dt_div24<60, 29, 86399>(sod));
        default: return day;
    }
}

// days to take off `day` to reach the first day of its year / quarter / month or its Monday
RDF_DT_HD uint32_t dt_trunc_days_back(int level, const DtCivil& c) {
    switch (level) {
        case DT_TRUNC_YEAR: return c.yday - 1u;
        case DT_TRUNC_MONTH: return c.day - 1u;
        case DT_TRUNC_WEEK: return c.wd;
        default: {   // QUARTER: the day of the month plus the one or two months before it in the quarter
            const uint32_t k = (c.month - 1u) % 3u;
            uint32_t back = c.day - 1u;
            if (k >= 1u) back += dt_month_length(c.leap, c.month - 1u);
            if (k == 2u) back += dt_month_length(c.leap, c.month - 2u);
            return back;
        }
    }
}

// date_trunc: the value's bits after truncation, same unit, wrapping modulo 2^64 (the caller narrows Int32 storage).
// YEAR / QUARTER / MONTH / WEEK: (day number - days back) * units per day.  DAY and finer: v - floor_mod(v, step).
template <int UNIT>
RDF_DT_HD uint64_t dt_trunc(int64_t v, int level) {
    if (level <= DT_TRUNC_WEEK) {
        int32_t day;
        uint64_t rem;
        dt_split<UNIT>(v, day, rem);
        const DtCivil c = dt_civil_from_days(day);
        const uint64_t first = (uint64_t)((int64_t)day - (int64_t)dt_trunc_days_back(level, c));
        return first * DtUnit<UNIT>::per_day;
    }
    if (UNIT == DT_UNIT_DAY) return (uint64_t)v;
    int64_t q;
    uint64_t rem;
    dt_floor_divmod<DtUnit<UNIT>::per_day>(v, q, rem);
    if (level == DT_TRUNC_DAY) return (uint64_t)v - rem;
    const uint32_t sod = dt_second_of_day<UNIT>(rem);
    const uint64_t frac = rem - (uint64_t)sod * DtUnit<UNIT>::per_second;
    const uint32_t secs = level == DT_TRUNC_HOUR ? sod % 3600u : level == DT_TRUNC_MINUTE ? sod % 60u : 0u;
    return (uint64_t)v - ((uint64_t)secs * DtUnit<UNIT>::per_second + frac);
}
RDF_DT_HD uint64_t dt_trunc_rt(int64_t v, int unit, int level) {
    switch (unit) {
        case DT_UNIT_S: return dt_trunc<DT_UNIT_S>(v, level);
        case DT_UNIT_MS: return dt_trunc<DT_UNIT_MS>(v, level);
        case DT_UNIT_US: return dt_trunc<DT_UNIT_US>(v, level);
        case DT_UNIT_NS: return dt_trunc<DT_UNIT_NS>(v, level);
        default: return dt_trunc<DT_UNIT_DAY>(v, level);
    }
}
// a level is refused when its step is shorter than one unit: only the time-of-day levels on RDF_TIME_DAY
RDF_DT_HD bool dt_trunc_level_ok(int unit, int level) { return level >= 0 && level < DT_NLEVELS && !(unit == DT_UNIT_DAY && level > DT_TRUNC_DAY); }

// date_add / add_months / last_day / next_day on a day number; the result wraps to Int32.
// MONTHS keeps the day of the month, clamped to the target month's last day.  NEXT_DAY: amount = 1 (Sunday) .. 7 (Saturday),
// the first date strictly later on that weekday; *ok = false for any other amount (the row is NULL).
RDF_DT_HD int32_t dt_shift(int op, int32_t day, int32_t amount, bool* ok) {
    *ok = true;
    if (op == DT_SHIFT_DAYS) return dt_add32(day, amount);
    if (op == DT_SHIFT_NEXT_DAY) {
        if (amount < 1 || amount > 7) { *ok = false; return 0; }
        const uint32_t target = ((uint32_t)amount + 5u) % 7u;   // Monday = 0
        return dt_add32(day, (int32_t)((target + 6u - dt_weekday(day)) % 7u + 1u));
    }
    const DtCivil c = dt_civil_from_days(day);
    if (op == DT_SHIFT_LAST_DAY) return dt_add32(day, (int32_t)(dt_month_length(c.leap, c.month) - c.day));
    const int64_t total = (int64_t)c.year * 12 + (int64_t)(c.month - 1u) + (int64_t)amount;   // months since year 0, |total| < 2.3e9
    const uint64_t tb = (uint64_t)(total + 12ll * 400000000ll);
    const uint64_t yq = tb / 12u;
    const int32_t y = (int32_t)((int64_t)yq - 400000000ll);
    const uint32_t m = (uint32_t)(tb - yq * 12u) + 1u;
    const uint32_t last = dt_last_day_of_month(y, m);
    return dt_wrap32(days_from_civil(y, m, c.day < last ? c.day : last));
}

// ---------------------------------------------------------------------------------------------------------------------
// The kernels' argument block and launchers (hipcc only; everything above is plain C++).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "rdf_colstats.h"

// A wave's tile: 512 rows of one chunk; the four waves of a block share one tile of CsCol (kCsTile rows of one chunk), so a
// wave starts on a multiple of 512 rows of its chunk and no validity word of an output has two writers.
constexpr int kDtWaveTile = 512;
static_assert(kDtWaveTile * (kCsThreads / 64) == kCsTile, "a block's four wave tiles make one tile of CsCol");
constexpr int kDtMaxFields = 8;
constexpr int kDtMaxNullSplit = 256;
enum : int { DT_NEED_CIVIL = 1, DT_NEED_TIME = 2 };

struct DtOut { void* values; uint8_t* validity; };   // one output chunk (offset 0)

struct DtArgs {
    CsCol    col;                    // the column (date_diff: `end`)
    const rdfk::DevChunkCol* b;      // [nchunks] date_shift: the Int32 amounts, date_diff: `start`; else nullptr
    const DtOut* outs;               // [nout * nchunks], output f of chunk c at f * nchunks + c
    uint32_t* wave_nulls;            // [ntiles * 4] NULL rows of every wave's tile, or nullptr when nothing can be NULL
    int64_t*  chunk_nulls;           // [nchunks * null_split] their sums per slice of a chunk (dt_nulls_kernel); the host adds a chunk's
    int64_t   null_split;            // 1..kDtMaxNullSplit
    int32_t  es, es_b;               // bytes of the storage type of col / b
    int32_t  unit, unit_b;           // rdf_time_unit of col / b
    int32_t  op;                     // rdf_trunc_level / rdf_date_shift
    int32_t  amount;                 // date_shift without an amounts column
    int32_t  nfields, need;          // fields: their number, DT_NEED_* of the list
    int32_t  fields[kDtMaxFields];
};

hipError_t launch_dt_fields(const DtArgs& a, hipStream_t s);
hipError_t launch_dt_trunc(const DtArgs& a, hipStream_t s);
hipError_t launch_dt_shift(const DtArgs& a, hipStream_t s);
hipError_t launch_dt_diff(const DtArgs& a, hipStream_t s);
hipError_t launch_dt_nulls(const DtArgs& a, hipStream_t s);
#endif
