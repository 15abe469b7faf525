// rdf_textconv.h — everything that is decided about ONE row of rdf_utf8_parse / rdf_utf8_format (kernels: rdf_textconv.hip,
// host side: rdf_capi_textconv.inc).  ONE definition, __host__ __device__ inline: hipcc compiles it into the kernels, plain
// g++ compiles it into tests/cpp/test_textconv_host.cpp.  The executable model of the same rules is tests/textconv_ref.py.
//
//   textconv_compile       the datetime pattern compiler (host only): at most 32 tokens and 64 literal bytes
//   textconv_parse_*       a byte span [b, e) -> a value; false = the row is NULL
//   textconv_length_* / textconv_write_*   a value -> the length of its text / the text, into a window the caller sized
//
// Rules kept throughout:
//   calendar    rdf_datetime.h (DtCivil, days_from_civil, the floor divisions): there is no second calendar here
//   no tables   beyond the month and weekday names
//   no UB       magnitudes are accumulated in unsigned arithmetic and an overflow is detected before it happens
//   bounds      no byte outside [b, e) is read, none outside the window is written
//   registers   no run-time-indexed private array: digits are taken by division, high to low
#pragma once
#include <stdint.h>

#include "rdf_datetime.h"

#define RDF_TC_HD RDF_DT_HD

// rdf_text_kind of include/rdf_mi355x.h and the rdf_dtype codes used here, restated so that this header stands alone
// (rdf_capi_textconv.inc static_asserts that they agree)
enum : int { TC_BOOL = 0, TC_INT = 1, TC_DATE = 2, TC_TIMESTAMP = 3, TC_NKINDS = 4 };
enum : int { TC_DT_I8 = 0, TC_DT_I64 = 3, TC_DT_U8 = 4, TC_DT_U64 = 7, TC_DT_BOOL = 10 };

constexpr int kTcMaxTokens = 32;
constexpr int kTcMaxLiteral = 64;
constexpr int kTcMaxRowBytes = 256;   // of a formatted row

enum : uint8_t {
    TCT_LIT = 0,      // arg literal bytes, taken from lit[] in order
    TCT_YEAR4, TCT_YEAR2, TCT_MONTH, TCT_MONTH_NAME, TCT_DAY, TCT_DOY, TCT_HOUR, TCT_HOUR12, TCT_AMPM, TCT_MINUTE, TCT_SECOND,
    TCT_FRAC,         // arg = 1..9 digits
    TCT_WEEKDAY       // format only
};
// numeric tokens: arg = 1 (one letter: 1..2 digits when parsed, DOY 1..3; no padding when printed) or 2 (padded / exact width)
struct TcPattern {
    int32_t ntok, nlit;
    int32_t max_out;              // most bytes a formatted row can have
    int32_t pad_;
    uint8_t tok[kTcMaxTokens];
    uint8_t arg[kTcMaxTokens];
    uint8_t lit[kTcMaxLiteral];
};

enum : int { TC_OK = 0, TC_E_LETTER, TC_E_RUN, TC_E_QUOTE, TC_E_TOKENS, TC_E_LITERAL, TC_E_PARSE_ONLY_FORMAT, TC_E_NEEDS_AMPM, TC_E_TOO_LONG, TC_E_EMPTY };

RDF_TC_HD const char* textconv_compile_message(int err) {
    switch (err) {
        case TC_E_LETTER: return "a letter that is no pattern letter";
        case TC_E_RUN: return "a run length the letter does not take";
        case TC_E_QUOTE: return "a quote that is not closed";
        case TC_E_TOKENS: return "more than 32 tokens";
        case TC_E_LITERAL: return "more than 64 literal bytes";
        case TC_E_PARSE_ONLY_FORMAT: return "EEE is taken by format only";
        case TC_E_NEEDS_AMPM: return "a clock hour (h) needs 'a'";
        case TC_E_TOO_LONG: return "a row could pass 256 bytes";
        case TC_E_EMPTY: return "an empty pattern";
        default: return "ok";
    }
}

// ---- the pattern compiler (host only).  *pos: the offending byte position on failure.
inline int textconv_compile(const uint8_t* p, int64_t n, bool for_parse, TcPattern* out, int64_t* pos) {
    TcPattern& t = *out;
    t.ntok = t.nlit = t.max_out = t.pad_ = 0;
    for (int i = 0; i < kTcMaxTokens; ++i) t.tok[i] = t.arg[i] = 0;
    for (int i = 0; i < kTcMaxLiteral; ++i) t.lit[i] = 0;
    *pos = 0;
    if (n <= 0) return TC_E_EMPTY;
    bool last_lit = false;
    int64_t first_h = -1;
    bool has_a = false;
    auto push = [&](uint8_t tok, uint8_t arg, int width, int64_t at) -> int {
        if (t.ntok >= kTcMaxTokens) { *pos = at; return TC_E_TOKENS; }
        t.tok[t.ntok] = tok;
        t.arg[t.ntok] = arg;
        ++t.ntok;
        t.max_out += width;
        last_lit = false;
        return TC_OK;
    };
    auto push_lit = [&](uint8_t c, int64_t at) -> int {
        if (t.nlit >= kTcMaxLiteral) { *pos = at; return TC_E_LITERAL; }
        if (!last_lit) {
            if (t.ntok >= kTcMaxTokens) { *pos = at; return TC_E_TOKENS; }
            t.tok[t.ntok] = TCT_LIT;
            t.arg[t.ntok] = 0;
            ++t.ntok;
            last_lit = true;
        }
        t.lit[t.nlit++] = c;
        ++t.arg[t.ntok - 1];
        ++t.max_out;
        return TC_OK;
    };
    int64_t i = 0;
    while (i < n) {
        const uint8_t c = p[i];
        const bool letter = (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z');
        if (c == '\'') {
            if (i + 1 < n && p[i + 1] == '\'') {   // '' outside quotes: one quote
                if (int e = push_lit('\'', i)) return e;
                i += 2;
                continue;
            }
            const int64_t open = i++;
            bool closed = false;
            while (i < n) {
                if (p[i] == '\'') {
                    if (i + 1 < n && p[i + 1] == '\'') { if (int e = push_lit('\'', i)) return e; i += 2; continue; }
                    closed = true;
                    ++i;
                    break;
                }
                if (int e = push_lit(p[i], i)) return e;
                ++i;
            }
            if (!closed) { *pos = open; return TC_E_QUOTE; }
            continue;
        }
        if (!letter) {
            if (int e = push_lit(c, i)) return e;
            ++i;
            continue;
        }
        int64_t j = i;
        while (j < n && p[j] == c) ++j;
        const int run = (int)(j - i);
        int e = TC_OK;
        bool known = true, run_ok = true;
        switch (c) {
            case 'y': if (run == 4) e = push(TCT_YEAR4, 4, 13, i); else if (run == 2) e = push(TCT_YEAR2, 2, 2, i); else run_ok = false; break;
            case 'M': if (run <= 2) e = push(TCT_MONTH, (uint8_t)run, 2, i); else if (run == 3) e = push(TCT_MONTH_NAME, 3, 3, i); else run_ok = false; break;
            case 'd': if (run <= 2) e = push(TCT_DAY, (uint8_t)run, 2, i); else run_ok = false; break;
            case 'D': if (run == 1 || run == 3) e = push(TCT_DOY, (uint8_t)(run == 3 ? 2 : 1), 3, i); else run_ok = false; break;
            case 'H': if (run <= 2) e = push(TCT_HOUR, (uint8_t)run, 2, i); else run_ok = false; break;
            case 'h': if (run <= 2) { e = push(TCT_HOUR12, (uint8_t)run, 2, i); if (first_h < 0) first_h = i; } else run_ok = false; break;
            case 'a': if (run == 1) { e = push(TCT_AMPM, 1, 2, i); has_a = true; } else run_ok = false; break;
            case 'm': if (run <= 2) e = push(TCT_MINUTE, (uint8_t)run, 2, i); else run_ok = false; break;
            case 's': if (run <= 2) e = push(TCT_SECOND, (uint8_t)run, 2, i); else run_ok = false; break;
            case 'S': if (run <= 9) e = push(TCT_FRAC, (uint8_t)run, run, i); else run_ok = false; break;
            case 'E':
                if (run != 3) run_ok = false;
                else if (for_parse) { *pos = i; return TC_E_PARSE_ONLY_FORMAT; }
                else e = push(TCT_WEEKDAY, 3, 3, i);
                break;
            default: known = false; break;
        }
        if (!known) { *pos = i; return TC_E_LETTER; }
        if (!run_ok) { *pos = i; return TC_E_RUN; }
        if (e) return e;
        i = j;
    }
    if (first_h >= 0 && !has_a) { *pos = first_h; return TC_E_NEEDS_AMPM; }
    if (!for_parse && t.max_out > kTcMaxRowBytes) { *pos = n - 1; return TC_E_TOO_LONG; }
    return TC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- parse
RDF_TC_HD bool tc_is_ws(uint8_t c) { return (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x20); }
RDF_TC_HD bool tc_is_digit(uint8_t c) { return (uint32_t)c - (uint32_t)'0' <= 9u; }

// the CAST grammars' trim: 0x09-0x0D, 0x1C-0x20 from both ends
RDF_TC_HD void textconv_trim(const uint8_t*& b, const uint8_t*& e) {
    while (b < e && tc_is_ws(*b)) ++b;
    while (e > b && tc_is_ws(e[-1])) --e;
}

// does (neg ? -mag : mag) fit the integer dtype; its two's-complement bits
RDF_TC_HD bool tc_int_fits(uint64_t mag, bool neg, int dtype, uint64_t* bits) {
    const int w = 8 << (dtype & 3);
    const bool sgn = dtype < TC_DT_U8;
    const uint64_t maxpos = sgn ? ((1ull << (w - 1)) - 1ull) : (w == 64 ? ~0ull : ((1ull << w) - 1ull));
    if (!neg) {
        if (mag > maxpos) return false;
        *bits = mag;
        return true;
    }
    if (!sgn) {
        if (mag != 0) return false;
        *bits = 0;
        return true;
    }
    if (mag > maxpos + 1ull) return false;
    *bits = 0ull - mag;
    return true;
}
RDF_TC_HD bool tc_all_digits(const uint8_t* p, const uint8_t* e) {
    for (; p < e; ++p)
        if (!tc_is_digit(*p)) return false;
    return true;
}
// [p, e): what follows the sign (and, when had_digit, leading zeros the caller skipped).  *frac: the first byte after the
// '.', whose tail [*frac, e) the caller still has to find all digits; nullptr when there is no fraction.
RDF_TC_HD bool tc_int_core(const uint8_t* p, const uint8_t* e, bool neg, bool had_digit, int dtype, uint64_t* bits, const uint8_t** frac) {
    uint64_t mag = 0;
    *frac = nullptr;
    for (; p < e; ++p) {
        const uint32_t d = (uint32_t)*p - (uint32_t)'0';
        if (d > 9u) break;
        if (mag > (~0ull - d) / 10ull) return false;   // beyond UInt64: beyond every dtype, whatever follows
        mag = mag * 10ull + d;
        had_digit = true;
    }
    if (!had_digit) return false;
    if (p < e) {
        if (*p != '.') return false;
        *frac = p + 1;
    }
    return tc_int_fits(mag, neg, dtype, bits);
}
RDF_TC_HD bool textconv_parse_int(const uint8_t* b, const uint8_t* e, int dtype, uint64_t* bits) {
    textconv_trim(b, e);
    if (b == e) return false;
    bool neg = false;
    if (*b == '+' || *b == '-') { neg = *b == '-'; ++b; }
    const uint8_t* frac;
    if (!tc_int_core(b, e, neg, false, dtype, bits, &frac)) return false;
    return !frac || tc_all_digits(frac, e);
}

constexpr uint64_t tc_word(int n, uint64_t w) { return ((uint64_t)n << 56) | w; }
// (the _trimmed forms take a span the caller trimmed: the wave's long-row path of the parse kernel)
RDF_TC_HD bool textconv_parse_bool_trimmed(const uint8_t* b, const uint8_t* e, bool* v) {
    const int n = (int)(e - b);
    if (n < 1 || n > 5) return false;
    uint64_t key = 0;
    for (int i = 0; i < n; ++i) {
        uint8_t c = b[i];
        if (c >= 'A' && c <= 'Z') c |= 0x20;
        key |= (uint64_t)c << (8 * i);
    }
    key |= (uint64_t)n << 56;   // (the length too: a NUL byte adds nothing to the word)
    // little-endian words of the ten spellings, their length in the top byte
    if (key == tc_word(1, 0x74ull) || key == tc_word(4, 0x65757274ull) || key == tc_word(1, 0x79ull) || key == tc_word(3, 0x736579ull) || key == tc_word(1, 0x31ull)) { *v = true; return true; }
    if (key == tc_word(1, 0x66ull) || key == tc_word(5, 0x65736c6166ull) || key == tc_word(1, 0x6eull) || key == tc_word(2, 0x6f6eull) || key == tc_word(1, 0x30ull)) { *v = false; return true; }
    return false;
}
RDF_TC_HD bool textconv_parse_bool(const uint8_t* b, const uint8_t* e, bool* v) {
    textconv_trim(b, e);
    return textconv_parse_bool_trimmed(b, e, v);
}

// up to `most` digits, at least `least`, greedy; false when fewer
RDF_TC_HD bool tc_take_digits(const uint8_t*& p, const uint8_t* e, int least, int most, uint32_t* v) {
    uint32_t x = 0;
    int n = 0;
    while (p < e && n < most && tc_is_digit(*p)) { x = x * 10u + (uint32_t)(*p - '0'); ++p; ++n; }
    *v = x;
    return n >= least;
}

// the digits of a year: 4..most of them, and no digit after them
RDF_TC_HD bool tc_take_year(const uint8_t*& p, const uint8_t* e, int most, uint32_t* v) {
    if (!tc_take_digits(p, e, 4, most, v)) return false;
    return !(p < e && tc_is_digit(*p));
}

// [+-]? y{4,7} ( - m{1,2} ( - d{1,2} )? )?   stage: 1 = year, 2 = year-month, 3 = year-month-day.  The date is checked.
RDF_TC_HD bool tc_parse_date_part(const uint8_t*& p, const uint8_t* e, int32_t* year, uint32_t* month, uint32_t* day, int* stage) {
    bool neg = false;
    if (p < e && (*p == '+' || *p == '-')) { neg = *p == '-'; ++p; }
    uint32_t y;
    if (!tc_take_year(p, e, 7, &y)) return false;
    *year = neg ? -(int32_t)y : (int32_t)y;
    *month = 1;
    *day = 1;
    *stage = 1;
    if (p < e && *p == '-') {
        ++p;
        if (!tc_take_digits(p, e, 1, 2, month)) return false;
        *stage = 2;
        if (p < e && *p == '-') {
            ++p;
            if (!tc_take_digits(p, e, 1, 2, day)) return false;
            *stage = 3;
        }
    }
    if (*month < 1u || *month > 12u || *day < 1u || *day > dt_last_day_of_month(*year, *month)) return false;
    return true;
}
RDF_TC_HD bool tc_day_fits(int64_t days, int32_t* out) {
    if (days < -2147483648ll || days > 2147483647ll) return false;
    *out = (int32_t)days;
    return true;
}
RDF_TC_HD bool textconv_parse_date_trimmed(const uint8_t* b, const uint8_t* e, int32_t* out) {
    int32_t y;
    uint32_t m, d;
    int stage;
    if (!tc_parse_date_part(b, e, &y, &m, &d, &stage)) return false;
    if (b < e && !(stage == 3 && (*b == ' ' || *b == 'T'))) return false;
    return tc_day_fits(days_from_civil(y, m, d), out);
}
RDF_TC_HD bool textconv_parse_date(const uint8_t* b, const uint8_t* e, int32_t* out) {
    textconv_trim(b, e);
    return textconv_parse_date_trimmed(b, e, out);
}

RDF_TC_HD uint64_t tc_per_second(int unit) { return unit == DT_UNIT_S ? 1ull : unit == DT_UNIT_MS ? 1000ull : unit == DT_UNIT_US ? 1000000ull : 1000000000ull; }

// seconds since the epoch (|secs| < 2^50) + nanoseconds of the second -> the unit's Int64; false when it does not fit
RDF_TC_HD bool tc_compose(int64_t secs, uint32_t nanos, int unit, int64_t* out) {
    const uint64_t ps = tc_per_second(unit);
    const uint64_t frac = unit == DT_UNIT_S ? 0ull : unit == DT_UNIT_MS ? nanos / 1000000u : unit == DT_UNIT_US ? nanos / 1000u : nanos;
    if (secs >= 0) {
        const uint64_t u = (uint64_t)secs;
        if (u > (0x7fffffffffffffffull - frac) / ps) return false;
        *out = (int64_t)(u * ps + frac);
        return true;
    }
    const uint64_t m = 0ull - (uint64_t)secs;
    if (m > (0x8000000000000000ull + frac) / ps) return false;
    *out = (int64_t)(0ull - (m * ps - frac));
    return true;
}

// '.' digit*: the first nine digits are the nanoseconds, the rest is checked and dropped
RDF_TC_HD uint32_t tc_take_fraction(const uint8_t*& p, const uint8_t* e) {
    uint32_t nanos = 0, scale = 100000000u;
    while (p < e && tc_is_digit(*p)) {
        nanos += (uint32_t)(*p - '0') * scale;
        scale /= 10u;
        ++p;
    }
    return nanos;
}

RDF_TC_HD bool textconv_parse_timestamp_trimmed(const uint8_t* b, const uint8_t* e, int unit, int64_t* out) {
    int32_t y;
    uint32_t mo, d, hh = 0, mi = 0, ss = 0, nanos = 0;
    int stage;
    if (!tc_parse_date_part(b, e, &y, &mo, &d, &stage)) return false;
    int64_t zone = 0;   // seconds east
    if (b < e && (*b == ' ' || *b == 'T')) {
        if (stage != 3) return false;
        ++b;
        if (!tc_take_digits(b, e, 1, 2, &hh) || b == e || *b != ':') return false;
        ++b;
        if (!tc_take_digits(b, e, 1, 2, &mi)) return false;
        if (b < e && *b == ':') {
            ++b;
            if (!tc_take_digits(b, e, 1, 2, &ss)) return false;
            if (b < e && *b == '.') { ++b; nanos = tc_take_fraction(b, e); }
        }
        if (hh > 23u || mi > 59u || ss > 59u) return false;
    }
    if (b < e) {
        if (*b == 'Z') ++b;
        else if (e - b >= 3 && b[0] == 'U' && b[1] == 'T' && b[2] == 'C') b += 3;
        else if (*b == '+' || *b == '-') {
            const bool west = *b == '-';
            ++b;
            uint32_t zh, zm = 0;
            if (!tc_take_digits(b, e, 1, 2, &zh)) return false;
            if (b < e && *b == ':') {
                ++b;
                if (!tc_take_digits(b, e, 1, 2, &zm)) return false;
            }
            if (zm > 59u || zh * 60u + zm > 18u * 60u) return false;
            zone = (int64_t)(zh * 3600u + zm * 60u);
            if (west) zone = -zone;
        } else return false;
        if (b != e) return false;
    }
    const int64_t secs = days_from_civil(y, mo, d) * 86400ll + (int64_t)(hh * 3600u + mi * 60u + ss) - zone;
    return tc_compose(secs, nanos, unit, out);
}
RDF_TC_HD bool textconv_parse_timestamp(const uint8_t* b, const uint8_t* e, int unit, int64_t* out) {
    textconv_trim(b, e);
    return textconv_parse_timestamp_trimmed(b, e, unit, out);
}

// character i (0..2) of the name of month m (1..12) / weekday wd (Monday = 0)
RDF_TC_HD uint8_t tc_month_name(uint32_t m, int i) { return (uint8_t)"JanFebMarAprMayJunJulAugSepOctNovDec"[(m - 1u) * 3u + (uint32_t)i]; }
RDF_TC_HD uint8_t tc_weekday_name(uint32_t wd, int i) { return (uint8_t)"MonTueWedThuFriSatSun"[wd * 3u + (uint32_t)i]; }

enum : uint32_t { TCF_YEAR = 1, TCF_MONTH = 2, TCF_DAY = 4, TCF_DOY = 8, TCF_HOUR = 16, TCF_HOUR12 = 32, TCF_AMPM = 64, TCF_MINUTE = 128, TCF_SECOND = 256, TCF_FRAC = 512 };

// a field given twice has to say the same both times
RDF_TC_HD bool tc_set(uint32_t& set, uint32_t bit, uint32_t& field, uint32_t v) {
    if ((set & bit) && field != v) return false;
    set |= bit;
    field = v;
    return true;
}

// to_timestamp(s, fmt): the whole row has to be consumed, nothing is trimmed.  *day / *sod / *nanos: the resolved fields.
RDF_TC_HD bool tc_parse_pattern(const TcPattern& t, const uint8_t* p, const uint8_t* e, int64_t* day, uint32_t* sod, uint32_t* nanos_out) {
    uint32_t set = 0, year = 0, month = 1, dom = 1, doy = 1, hour = 0, hour12 = 0, pm = 0, minute = 0, second = 0, nanos = 0;
    int lit = 0;
    for (int k = 0; k < t.ntok; ++k) {
        const int arg = t.arg[k];
        uint32_t v = 0;
        switch (t.tok[k]) {
            case TCT_LIT:
                if (e - p < arg) return false;
                for (int i = 0; i < arg; ++i)
                    if (p[i] != t.lit[lit + i]) return false;
                p += arg;
                lit += arg;
                break;
            case TCT_YEAR4: {
                bool neg = false, sign = false;
                if (p < e && (*p == '+' || *p == '-')) { neg = *p == '-'; sign = true; ++p; }
                if (sign ? !tc_take_year(p, e, 7, &v) : !tc_take_digits(p, e, 4, 4, &v)) return false;
                if (!tc_set(set, TCF_YEAR, year, neg ? 0u - v : v)) return false;
                break;
            }
            case TCT_YEAR2:
                if (!tc_take_digits(p, e, 2, 2, &v) || !tc_set(set, TCF_YEAR, year, 2000u + v)) return false;
                break;
            case TCT_MONTH:
                if (!tc_take_digits(p, e, arg, 2, &v) || !tc_set(set, TCF_MONTH, month, v)) return false;
                break;
            case TCT_MONTH_NAME: {
                if (e - p < 3) return false;
                uint32_t m = 0;
                for (uint32_t c = 1; c <= 12u; ++c)
                    if (p[0] == tc_month_name(c, 0) && p[1] == tc_month_name(c, 1) && p[2] == tc_month_name(c, 2)) m = c;
                if (m == 0 || !tc_set(set, TCF_MONTH, month, m)) return false;
                p += 3;
                break;
            }
            case TCT_DAY:
                if (!tc_take_digits(p, e, arg, 2, &v) || !tc_set(set, TCF_DAY, dom, v)) return false;
                break;
            case TCT_DOY:
                if (!tc_take_digits(p, e, arg == 2 ? 3 : 1, 3, &v) || !tc_set(set, TCF_DOY, doy, v)) return false;
                break;
            case TCT_HOUR:
                if (!tc_take_digits(p, e, arg, 2, &v) || !tc_set(set, TCF_HOUR, hour, v)) return false;
                break;
            case TCT_HOUR12:
                if (!tc_take_digits(p, e, arg, 2, &v) || !tc_set(set, TCF_HOUR12, hour12, v)) return false;
                break;
            case TCT_AMPM:
                if (e - p < 2 || (p[0] != 'A' && p[0] != 'P') || p[1] != 'M') return false;
                if (!tc_set(set, TCF_AMPM, pm, p[0] == 'P' ? 1u : 0u)) return false;
                p += 2;
                break;
            case TCT_MINUTE:
                if (!tc_take_digits(p, e, arg, 2, &v) || !tc_set(set, TCF_MINUTE, minute, v)) return false;
                break;
            case TCT_SECOND:
                if (!tc_take_digits(p, e, arg, 2, &v) || !tc_set(set, TCF_SECOND, second, v)) return false;
                break;
            case TCT_FRAC: {
                if (!tc_take_digits(p, e, arg, arg, &v)) return false;
                for (int i = arg; i < 9; ++i) v *= 10u;
                if (!tc_set(set, TCF_FRAC, nanos, v)) return false;
                break;
            }
            default: return false;   // (TCT_WEEKDAY does not compile for parse)
        }
    }
    if (p != e) return false;
    const int32_t y = (set & TCF_YEAR) ? (int32_t)year : 1970;
    if (set & TCF_DOY) {
        if (doy < 1u || doy > (dt_is_leap(y) ? 366u : 365u)) return false;
        *day = days_from_civil(y, 1, 1) + (int64_t)doy - 1;
        if (set & (TCF_MONTH | TCF_DAY)) {
            int32_t dd;
            if (!tc_day_fits(*day, &dd)) return false;
            const DtCivil c = dt_civil_from_days(dd);
            if (((set & TCF_MONTH) && c.month != month) || ((set & TCF_DAY) && c.day != dom)) return false;
        }
    } else {
        if (month < 1u || month > 12u || dom < 1u || dom > dt_last_day_of_month(y, month)) return false;
        *day = days_from_civil(y, month, dom);
    }
    if (set & TCF_HOUR12) {
        if (hour12 < 1u || hour12 > 12u) return false;
        const uint32_t h = (hour12 == 12u ? 0u : hour12) + 12u * pm;
        if ((set & TCF_HOUR) && hour != h) return false;
        hour = h;
    } else if ((set & TCF_AMPM) && (set & TCF_HOUR) && (hour >= 12u) != (pm != 0u)) return false;
    if (hour > 23u || minute > 59u || second > 59u) return false;
    *sod = hour * 3600u + minute * 60u + second;
    *nanos_out = nanos;
    return true;
}
RDF_TC_HD bool textconv_parse_date_pattern(const TcPattern& t, const uint8_t* b, const uint8_t* e, int32_t* out) {
    int64_t day;
    uint32_t sod, nanos;
    return tc_parse_pattern(t, b, e, &day, &sod, &nanos) && tc_day_fits(day, out);
}
RDF_TC_HD bool textconv_parse_timestamp_pattern(const TcPattern& t, const uint8_t* b, const uint8_t* e, int unit, int64_t* out) {
    int64_t day;
    uint32_t sod, nanos;
    return tc_parse_pattern(t, b, e, &day, &sod, &nanos) && tc_compose(day * 86400ll + (int64_t)sod, nanos, unit, out);
}

// --------------------------------------------------------------------------------------------------------------- format
// One emitter per kind, run against a sink that counts (textconv_length_*) or stores (textconv_write_*).
struct TcCount { int n; RDF_TC_HD void put(uint8_t) { ++n; } };
struct TcStore { uint8_t* p; RDF_TC_HD void put(uint8_t c) { *p++ = c; } };

// v in decimal, at least min_digits wide: the digits come out high to low, by division
template <class S>
RDF_TC_HD void tc_put_u32(S& s, uint32_t v, int min_digits) {
    int n = 1;
    uint32_t p = 1;
    while (v / p >= 10u) { p *= 10u; ++n; }
    for (; min_digits > n; --min_digits) s.put('0');
    for (;;) {
        const uint32_t d = v / p;
        s.put((uint8_t)('0' + d));
        v -= d * p;
        if (p == 1u) break;
        p /= 10u;
    }
}
template <class S>
RDF_TC_HD void tc_put_u64(S& s, uint64_t v) {
    const uint64_t v1 = v / 1000000000ull;
    const uint32_t c = (uint32_t)(v - v1 * 1000000000ull);
    if (v1 == 0) { tc_put_u32(s, c, 1); return; }
    const uint64_t a = v1 / 1000000000ull;   // <= 18
    const uint32_t b = (uint32_t)(v1 - a * 1000000000ull);
    if (a) { tc_put_u32(s, (uint32_t)a, 1); tc_put_u32(s, b, 9); }
    else tc_put_u32(s, b, 1);
    tc_put_u32(s, c, 9);
}
// the year rule: 0..9999 four digits, above '+' and the digits, below 0 '-' and at least four digits
template <class S>
RDF_TC_HD void tc_put_year(S& s, int64_t y) {
    if (y < 0) s.put('-');
    else if (y > 9999) s.put('+');
    const uint64_t mag = y < 0 ? 0ull - (uint64_t)y : (uint64_t)y;
    if (mag < 0x100000000ull) tc_put_u32(s, (uint32_t)mag, 4);
    else tc_put_u64(s, mag);
}

// value -> its civil date, the units into the day and the TRUE year.  rdf_datetime_fields wraps the day number of a value to
// Int32; text must round-trip beyond that, so a day number outside Int32 is moved by whole eras of 400 years (146 097 days, a
// whole number of weeks) into the range of dt_civil_from_days and the years are added back: the same calendar, no second one.
struct TcWhen { DtCivil c; int64_t year; uint64_t rem; };
RDF_TC_HD TcWhen tc_when(int64_t v, int unit) {
    TcWhen w;
    int64_t q = v;
    w.rem = 0;
    switch (unit) {
        case DT_UNIT_S: dt_floor_divmod<DtUnit<DT_UNIT_S>::per_day>(v, q, w.rem); break;
        case DT_UNIT_MS: dt_floor_divmod<DtUnit<DT_UNIT_MS>::per_day>(v, q, w.rem); break;
        case DT_UNIT_US: dt_floor_divmod<DtUnit<DT_UNIT_US>::per_day>(v, q, w.rem); break;
        case DT_UNIT_NS: dt_floor_divmod<DtUnit<DT_UNIT_NS>::per_day>(v, q, w.rem); break;
        default: break;
    }
    int64_t eras = 0;
    if (q < -2147483648ll || q > 2147483647ll) {
        eras = dt_floor_div<(uint64_t)kDtEraDays>(q);
        q -= eras * (int64_t)kDtEraDays;
    }
    w.c = dt_civil_from_days((int32_t)q);
    w.year = (int64_t)w.c.year + 400 * eras;
    return w;
}

// bits: the value's storage, sign- or zero-extended to 64 bits by the caller
template <class S>
RDF_TC_HD void tc_emit_int(S& s, uint64_t bits, int dtype) {
    if (dtype < TC_DT_U8 && (int64_t)bits < 0) { s.put('-'); tc_put_u64(s, 0ull - bits); }
    else tc_put_u64(s, bits);
}
template <class S>
RDF_TC_HD void tc_emit_bool(S& s, bool v) {
    if (v) { s.put('t'); s.put('r'); s.put('u'); s.put('e'); }
    else { s.put('f'); s.put('a'); s.put('l'); s.put('s'); s.put('e'); }
}
template <class S>
RDF_TC_HD void tc_emit_date(S& s, const DtCivil& c, int64_t year) {
    tc_put_year(s, year);
    s.put('-');
    tc_put_u32(s, c.month, 2);
    s.put('-');
    tc_put_u32(s, c.day, 2);
}
RDF_TC_HD uint32_t tc_frac_of(uint64_t rem, uint32_t sod, int unit) { return unit == DT_UNIT_DAY || unit == DT_UNIT_S ? 0u : (uint32_t)(rem - (uint64_t)sod * tc_per_second(unit)); }
RDF_TC_HD int tc_frac_digits(int unit) { return unit == DT_UNIT_MS ? 3 : unit == DT_UNIT_US ? 6 : unit == DT_UNIT_NS ? 9 : 0; }

// CAST(x AS STRING) of a temporal value: kind DATE prints its date, kind TIMESTAMP date and time
template <class S>
RDF_TC_HD void tc_emit_temporal(S& s, int64_t v, int unit, int kind) {
    const TcWhen w = tc_when(v, unit);
    const uint64_t rem = w.rem;
    tc_emit_date(s, w.c, w.year);
    if (kind != TC_TIMESTAMP) return;
    const uint32_t sod = dt_second_of_day_rt(rem, unit);
    const uint32_t h = sod / 3600u, mi = (sod - h * 3600u) / 60u, sec = sod - h * 3600u - mi * 60u;
    s.put(' ');
    tc_put_u32(s, h, 2);
    s.put(':');
    tc_put_u32(s, mi, 2);
    s.put(':');
    tc_put_u32(s, sec, 2);
    uint32_t frac = tc_frac_of(rem, sod, unit);
    if (frac) {
        int w = tc_frac_digits(unit);
        while (frac % 10u == 0u) { frac /= 10u; --w; }
        s.put('.');
        tc_put_u32(s, frac, w);
    }
}
// date_format(x, fmt)
template <class S>
RDF_TC_HD void tc_emit_pattern(S& s, const TcPattern& t, int64_t v, int unit) {
    const TcWhen w = tc_when(v, unit);
    const DtCivil& c = w.c;
    const uint64_t rem = w.rem;
    const uint32_t sod = dt_second_of_day_rt(rem, unit);
    const uint32_t h = sod / 3600u, mi = (sod - h * 3600u) / 60u, sec = sod - h * 3600u - mi * 60u;
    int lit = 0;
    for (int k = 0; k < t.ntok; ++k) {
        const int arg = t.arg[k];
        switch (t.tok[k]) {
            case TCT_LIT:
                for (int i = 0; i < arg; ++i) s.put(t.lit[lit + i]);
                lit += arg;
                break;
            case TCT_YEAR4: tc_put_year(s, w.year); break;
            case TCT_YEAR2: tc_put_u32(s, c.yy - 100u * (c.yy / 100u), 2); break;   // the year modulo 100 (floor): yy is the year modulo 400
            case TCT_MONTH: tc_put_u32(s, c.month, arg); break;
            case TCT_MONTH_NAME: for (int i = 0; i < 3; ++i) s.put(tc_month_name(c.month, i)); break;
            case TCT_DAY: tc_put_u32(s, c.day, arg); break;
            case TCT_DOY: tc_put_u32(s, c.yday, arg == 2 ? 3 : 1); break;
            case TCT_HOUR: tc_put_u32(s, h, arg); break;
            case TCT_HOUR12: { const uint32_t h12 = h % 12u; tc_put_u32(s, h12 ? h12 : 12u, arg); break; }
            case TCT_AMPM: s.put(h >= 12u ? 'P' : 'A'); s.put('M'); break;
            case TCT_MINUTE: tc_put_u32(s, mi, arg); break;
            case TCT_SECOND: tc_put_u32(s, sec, arg); break;
            case TCT_FRAC: {
                uint32_t nanos = tc_frac_of(rem, sod, unit);
                for (int i = tc_frac_digits(unit); i < 9; ++i) nanos *= 10u;
                for (int i = arg; i < 9; ++i) nanos /= 10u;
                tc_put_u32(s, nanos, arg);
                break;
            }
            default: for (int i = 0; i < 3; ++i) s.put(tc_weekday_name(c.wd, i)); break;
        }
    }
}

// one value of any kind: pattern == nullptr is the cast.  bits: the storage value extended to 64 bits (Boolean: 0 / 1).
template <class S>
RDF_TC_HD void tc_emit(S& s, int kind, int dtype, int unit, const TcPattern* pattern, uint64_t bits) {
    if (kind == TC_BOOL) tc_emit_bool(s, bits != 0);
    else if (kind == TC_INT) tc_emit_int(s, bits, dtype);
    else if (pattern) tc_emit_pattern(s, *pattern, (int64_t)bits, unit);
    else tc_emit_temporal(s, (int64_t)bits, unit, kind);
}
RDF_TC_HD int textconv_length(int kind, int dtype, int unit, const TcPattern* pattern, uint64_t bits) {
    TcCount s = {0};
    tc_emit(s, kind, dtype, unit, pattern, bits);
    return s.n;
}
// writes exactly textconv_length(...) bytes at dst; returns the byte after the last
RDF_TC_HD uint8_t* textconv_write(int kind, int dtype, int unit, const TcPattern* pattern, uint64_t bits, uint8_t* dst) {
    TcStore s = {dst};
    tc_emit(s, kind, dtype, unit, pattern, bits);
    return s.p;
}
RDF_TC_HD int textconv_length_int(uint64_t bits, int dtype) { return textconv_length(TC_INT, dtype, 0, nullptr, bits); }
RDF_TC_HD int textconv_length_bool(bool v) { return v ? 4 : 5; }
RDF_TC_HD int textconv_length_temporal(int64_t v, int unit, int kind, const TcPattern* pattern) { return textconv_length(kind, TC_DT_I64, unit, pattern, (uint64_t)v); }
RDF_TC_HD uint8_t* textconv_write_int(uint64_t bits, int dtype, uint8_t* dst) { return textconv_write(TC_INT, dtype, 0, nullptr, bits, dst); }
RDF_TC_HD uint8_t* textconv_write_bool(bool v, uint8_t* dst) { return textconv_write(TC_BOOL, TC_DT_BOOL, 0, nullptr, v ? 1u : 0u, dst); }
RDF_TC_HD uint8_t* textconv_write_temporal(int64_t v, int unit, int kind, const TcPattern* pattern, uint8_t* dst) { return textconv_write(kind, TC_DT_I64, unit, pattern, (uint64_t)v, dst); }

// the most bytes a row of a call can have (the write kernel's LDS image is 256 rows of this)
RDF_TC_HD int textconv_max_row_bytes(int kind, int unit, const TcPattern* pattern) {
    if (kind == TC_BOOL) return 5;
    if (kind == TC_INT) return 20;
    if (pattern) return pattern->max_out;
    if (kind == TC_DATE) return 19;                                   // -292277022657-01-27: Int64 seconds reach years of twelve digits
    return 19 + 9 + (tc_frac_digits(unit) ? 1 + tc_frac_digits(unit) : 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// The kernels' argument blocks and launchers (hipcc only; everything above is plain C++).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "rdf_device.h"
#include "rdf_utf8.h"

constexpr int kTcTile = kUtf8PredThreads;   // rows of one chunk a block takes
constexpr int kTcLdsBytes = 8192;           // parse: a tile whose byte span is at most this is staged in LDS (+ 16 bytes of alignment slack)

struct TcParseOut { void* values; uint8_t* valid; };
struct TcParseArgs {
    const Utf8Chunk*   chunks;
    int64_t            nchunks;
    const int64_t*     tile_start;   // nchunks + 1 entries
    int64_t            ntiles;
    const TcParseOut*  outs;         // per chunk
    const TcPattern*   pattern;      // device copy, or nullptr: the cast grammar
    int32_t            kind, unit, dtype;   // dtype: of the output
    int32_t            stage;        // 0: never stage a tile in LDS (the fallback form alone, for measurements)
    unsigned long long* nulls;       // per chunk: NULL rows of the output
    unsigned long long* failed;      // per chunk: rows that were not NULL and did not parse
};
hipError_t launch_textconv_parse(const TcParseArgs& a, hipStream_t s);

struct TcFormatArgs {
    const rdfk::DevChunkCol* chunks;   // the value chunks
    const int64_t*     row_start;      // nchunks + 1 entries
    const int64_t*     tile_start;     // nchunks + 1 entries
    int64_t            nchunks, ntiles, n;
    const TcPattern*   pattern;
    int32_t            kind, unit, dtype;   // dtype: of the input storage
    int32_t            max_row;        // textconv_max_row_bytes of the call
    int64_t*           blen;           // per row: output bytes (scanned into bscan)
    const int64_t*     bscan;          // n + 1 entries
    unsigned long long* nulls;         // per chunk
    int64_t*           tot;            // per chunk: bytes
    const Utf8OutChunk* outs;          // per chunk (row_start, rows, byte_start, bytes set)
};
hipError_t launch_textconv_size(const TcFormatArgs& a, hipStream_t s);     // blen, nulls
hipError_t launch_textconv_totals(const TcFormatArgs& a, hipStream_t s);   // tot
hipError_t launch_textconv_write(const TcFormatArgs& a, hipStream_t s);    // offsets, validity, the bytes
#endif
