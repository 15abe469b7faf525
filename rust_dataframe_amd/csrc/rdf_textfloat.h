// rdf_textfloat.h — everything that is decided about ONE row of rdf_utf8_parse_float / rdf_utf8_format_float (kernels:
// rdf_textfloat.hip, host side: rdf_capi_textconv.inc).  ONE definition, __host__ __device__ inline: hipcc compiles it into the
// kernels, plain g++ into tests/cpp/test_textfloat_host.cpp.  The executable model of the same rules is tests/textfloat_ref.py.
//
// Parse    trim (textconv_trim), then [+-]? ( digit+ ( '.' digit* )? | '.' digit+ ) ( [eE] [+-]? digit+ )?  or, in either
//          case of the ASCII letters, nan (no sign), [+-]? inf, [+-]? infinity.  Everything else is NULL.  The value is the
//          exact decimal rounded ONCE, to nearest and ties to even, into the target type, however many digits the row has;
//          overflow gives an infinity, underflow a zero with the row's sign; NaN is the canonical quiet NaN.
//            tf_scan    sign, the first 19 significant digits m, the power of ten q of m's last digit (saturated), and whether
//                       a non-zero digit was dropped.  The value lies in [m, m + 1) * 10^q, and is m * 10^q when none was.
//            tf_fast    decided bits, or undecided.  With T the table's entry of q, (T - 1) 2^E < 10^q <= T 2^E, the exact
//                       value lies in the closed interval [m (T - 1), (m + 1) T] 2^E (the ends m T when T is exact and no
//                       digit was dropped).  Both ends are 192-bit integers; each is rounded to the type exactly.  Rounding to
//                       nearest is monotone, so when both ends give the same bits every value between them does: decided.
//                       Otherwise the row is undecided, whatever the reason (a tie, a near-tie, a binade boundary).
//            tf_exact   always right, alone: up to 770 significant digits as a big integer (no midpoint between two Float64
//                       has more than 767; further non-zero digits become one trailing 1), times 10^q for q >= 0, or divided
//                       by 5^-q bit by bit for 64 quotient bits and the remainder as sticky, then the same exact rounding.
//                       The ONLY code here with arrays indexed at run time (two big integers): the resolve kernel's scratch.
// Format   Java's Double.toString / Float.toString (JDK 19 and later): the shortest decimal that rounds back, the closest of
//          that length, ties to the even digit; never fewer than 2 digits chosen (4.9E-324, 1.4E-45); plain decimal for
//          10^-3 <= |x| < 10^7, else d.dddE[-]n; NaN, Infinity, -Infinity, 0.0, -0.0.
//            tf_shortest  Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020) over the same table: the value
//                         and its two rounding boundaries times 10^-k, each rounded to odd from 192-bit products; first the
//                         multiples of 10^(k+1) when they keep two digits, then the closer of the two multiples of 10^k.
//                         Digits come back as ONE integer and an exponent.
//            tf_emit      one emitter against a counting sink and a storing sink; digits are counted by compares against
//                         constants and taken by divisions by constants only.
// Rules kept throughout: no byte outside [b, e) is read, none outside the sized window written; no signed overflow; shifts
// stay below the width of their operand.
#pragma once
#include <stdint.h>

#include "rdf_textconv.h"

#define RDF_TF_HD RDF_TC_HD

constexpr int kTfPow10Min = -343, kTfPow10Max = 325, kTfPow10ExactMax = 55;   // (rdf_pow10_tables.h, static_asserted where both are seen)
constexpr int kTfPow10Words = 2 * (kTfPow10Max - kTfPow10Min + 1);
constexpr int kTfMaxRowF64 = 24, kTfMaxRowF32 = 15;
constexpr int kTfBigLimbs = 88;          // 2816 bits: 771 digits (2562 bits) against 5^1095 (2543 bits), aligned, plus one
constexpr int kTfExactDigits = 770;

typedef unsigned __int128 tf_u128;

RDF_TF_HD int tf_clz64(uint64_t x) {   // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}
RDF_TF_HD int tf_floor_log2_pow10(int e) { return (e * 1741647) >> 19; }   // |e| <= 1233 (checked by the table generator over the table's range)

template <bool F32> struct TfType;
template <> struct TfType<false> {
    static constexpr int MANT = 53, EMIN = -1022, EMAX = 1023, BIAS = 1023;
    static constexpr uint64_t INF = 0x7FF0000000000000ull, QNAN = 0x7FF8000000000000ull, SIGN = 0x8000000000000000ull;
};
template <> struct TfType<true> {
    static constexpr int MANT = 24, EMIN = -126, EMAX = 127, BIAS = 127;
    static constexpr uint64_t INF = 0x7F800000ull, QNAN = 0x7FC00000ull, SIGN = 0x80000000ull;
};

// (h + f) * 2^exp2 with h != 0 and 0 <= f < 1, f != 0 exactly when sticky -> the magnitude bits of the nearest value, ties to even
template <bool F32>
RDF_TF_HD uint64_t tf_round(uint64_t h, bool sticky, int exp2) {
    typedef TfType<F32> T;
    const int lz = tf_clz64(h);
    h <<= lz;
    const int e = exp2 - lz + 63;                 // 2^e <= the value < 2^(e + 1)
    if (e > T::EMAX) return T::INF;
    const int keep = e >= T::EMIN ? T::MANT : T::MANT - (T::EMIN - e);   // significand bits the value keeps (subnormals fewer)
    if (keep < 0) return 0;                       // below half the smallest subnormal
    uint64_t m, rest;                             // rest: the round bit on top, what is dropped after it below
    if (keep == 0) { m = 0; rest = h; }
    else { m = h >> (64 - keep); rest = h << keep; }
    const bool round_bit = (rest >> 63) != 0;
    const bool below = (rest << 1) != 0 || sticky;
    if (round_bit && (below || (m & 1))) ++m;
    if (e < T::EMIN) return m;                    // (a carry into 2^(MANT - 1) is the smallest normal's bits)
    const uint64_t bits = ((uint64_t)(e - T::EMIN + 1) << (T::MANT - 1)) + (m - (1ull << (T::MANT - 1)));   // (a carry moves to the next exponent)
    return bits < T::INF ? bits : T::INF;
}

// ------------------------------------------------------------------------------------------------------------------ parse
enum : int { TF_FAIL = 0, TF_NUM = 1, TF_INF = 2, TF_NAN = 3 };
struct TfScan {
    uint64_t m;        // the first 19 significant digits (fewer when the row has fewer)
    int32_t  q;        // the value is in [m, m + 1) * 10^q; saturated to +-100000
    int32_t  kind;
    bool     neg, sticky;
};

// the bytes of [p, e), at most 8, lower-cased letters, little endian; the length in *n
RDF_TF_HD uint64_t tf_word_ci(const uint8_t* p, const uint8_t* e, int* n) {
    uint64_t key = 0;
    int i = 0;
    for (; p + i < e && i < 8; ++i) {
        uint8_t c = p[i];
        if (c >= 'A' && c <= 'Z') c |= 0x20;
        key |= (uint64_t)c << (8 * i);
    }
    *n = (p + i < e) ? 9 : i;
    return key;
}

// the exponent part at p (after the digits): false = the row is NULL.  *ev: the signed exponent, saturated
RDF_TF_HD bool tf_take_exponent(const uint8_t*& p, const uint8_t* e, int64_t* ev) {
    *ev = 0;
    if (p < e && (*p == 'e' || *p == 'E')) {
        ++p;
        bool en = false;
        if (p < e && (*p == '+' || *p == '-')) { en = *p == '-'; ++p; }
        if (p == e || !tc_is_digit(*p)) return false;
        int64_t v = 0;
        for (; p < e; ++p) {
            const uint32_t d = (uint32_t)*p - (uint32_t)'0';
            if (d > 9u) break;
            if (v < 100000000000000000ll) v = v * 10 + (int64_t)d;
        }
        *ev = en ? -v : v;
    }
    return p == e;
}

RDF_TF_HD TfScan tf_scan(const uint8_t* b, const uint8_t* e) {
    TfScan s = {0, 0, TF_FAIL, false, false};
    textconv_trim(b, e);
    if (b == e) return s;
    const uint8_t* p = b;
    bool sign = false;
    if (*p == '+' || *p == '-') { s.neg = *p == '-'; sign = true; ++p; }
    if (p < e && !tc_is_digit(*p) && *p != '.') {
        int n;
        const uint64_t key = tf_word_ci(p, e, &n);
        if (n == 3 && key == 0x6e616eull && !sign) s.kind = TF_NAN;
        else if ((n == 3 && key == 0x666e69ull) || (n == 8 && key == 0x7974696e69666e69ull)) s.kind = TF_INF;
        return s;
    }
    uint64_t m = 0;
    int nd = 0;
    int64_t q = 0;
    bool any = false, sticky = false;
    for (; p < e; ++p) {
        const uint32_t d = (uint32_t)*p - (uint32_t)'0';
        if (d > 9u) break;
        any = true;
        if (nd < 19) {
            if (m | d) { m = m * 10ull + d; ++nd; }
        } else {
            ++q;
            sticky = sticky || d != 0;
        }
    }
    if (p < e && *p == '.') {
        ++p;
        for (; p < e; ++p) {
            const uint32_t d = (uint32_t)*p - (uint32_t)'0';
            if (d > 9u) break;
            any = true;
            if (nd < 19) {
                if (m | d) { m = m * 10ull + d; ++nd; }
                --q;
            } else {
                sticky = sticky || d != 0;
            }
        }
    }
    if (!any) return s;
    int64_t ev;
    if (!tf_take_exponent(p, e, &ev)) return s;
    q += ev;
    s.m = m;
    s.q = (int32_t)(q > 100000 ? 100000 : q < -100000 ? -100000 : q);
    s.sticky = sticky;
    s.kind = TF_NUM;
    return s;
}

// decided: true and the magnitude bits.  tab: kTfPow10 (any address space)
template <bool F32>
RDF_TF_HD bool tf_fast(const uint64_t* tab, uint64_t m, int q, bool sticky, uint64_t* bits) {
    typedef TfType<F32> T;
    if (m == 0) { *bits = 0; return true; }
    if (q > 308) { *bits = T::INF; return true; }            // m >= 1: at least 10^309
    if (q < kTfPow10Min) { *bits = 0; return true; }         // (m + 1) 10^q <= 10^19 10^-344 < 2^-1075, half the smallest subnormal
    const int lz = tf_clz64(m);
    const uint64_t w = m << lz;
    const uint64_t thi = tab[2 * (q - kTfPow10Min)], tlo = tab[2 * (q - kTfPow10Min) + 1];
    // x = w * T, 192 bits (x2, x1, x0); the value is x * 2^(E - lz) up to the table's and the dropped digits' errors
    const tf_u128 p0 = (tf_u128)w * tlo, p1 = (tf_u128)w * thi;
    const tf_u128 mid = p1 + (uint64_t)(p0 >> 64);
    const uint64_t x0 = (uint64_t)p0, x1 = (uint64_t)mid, x2 = (uint64_t)(mid >> 64);
    const int exp2 = tf_floor_log2_pow10(q) - 127 - lz + 128;   // of one unit of x2
    // the lower end: x - w when the table entry is rounded up
    uint64_t l0 = x0, l1 = x1, l2 = x2;
    if (q < 0 || q > kTfPow10ExactMax) {
        const uint64_t n0 = x0 - w;
        const uint64_t br = x0 < w ? 1u : 0u;
        const uint64_t n1 = x1 - br;
        l2 = x2 - ((x1 < br) ? 1u : 0u);
        l1 = n1;
        l0 = n0;
    }
    // the upper end: x + (T << lz) when a digit was dropped
    uint64_t h0 = x0, h1 = x1, h2 = x2;
    if (sticky) {
        const uint64_t t0 = tlo << lz;
        const uint64_t t1 = lz ? (thi << lz) | (tlo >> (64 - lz)) : thi;
        const uint64_t t2 = lz ? thi >> (64 - lz) : 0;
        const tf_u128 s0 = (tf_u128)x0 + t0;
        const tf_u128 s1 = (tf_u128)x1 + t1 + (uint64_t)(s0 >> 64);
        const tf_u128 s2 = (tf_u128)x2 + t2 + (uint64_t)(s1 >> 64);
        if ((uint64_t)(s2 >> 64)) return false;              // (the end leaves 192 bits: the exact path's)
        h0 = (uint64_t)s0; h1 = (uint64_t)s1; h2 = (uint64_t)s2;
    }
    const uint64_t lo = tf_round<F32>(l2, (l1 | l0) != 0, exp2);
    const uint64_t hi = tf_round<F32>(h2, (h1 | h0) != 0, exp2);
    if (lo != hi) return false;
    *bits = lo;
    return true;
}

// ---- the exact path: little-endian big integers of 32-bit limbs
struct TfBig {
    uint32_t v[kTfBigLimbs];
    int n;             // limbs in use: v[n - 1] != 0, or n == 0 for zero
};
RDF_TF_HD void tf_big_muladd(TfBig& a, uint32_t mul, uint32_t add) {
    uint64_t carry = add;
    for (int i = 0; i < a.n; ++i) {
        const uint64_t t = (uint64_t)a.v[i] * mul + carry;
        a.v[i] = (uint32_t)t;
        carry = t >> 32;
    }
    if (carry && a.n < kTfBigLimbs) a.v[a.n++] = (uint32_t)carry;
}
RDF_TF_HD int tf_big_bits(const TfBig& a) { return a.n == 0 ? 0 : 32 * a.n - (tf_clz64((uint64_t)a.v[a.n - 1]) - 32); }
RDF_TF_HD void tf_big_shl(TfBig& a, int s) {   // the result fits kTfBigLimbs by the caller's bounds
    if (a.n == 0 || s <= 0) return;
    const int ws = s >> 5, bs = s & 31;
    int n = a.n + ws + 1;
    if (n > kTfBigLimbs) n = kTfBigLimbs;
    for (int i = n - 1; i >= 0; --i) {
        const int j = i - ws;
        const uint32_t lo = (j >= 0 && j < a.n) ? a.v[j] : 0u;
        const uint32_t below = (j - 1 >= 0 && j - 1 < a.n) ? a.v[j - 1] : 0u;
        a.v[i] = bs ? (lo << bs) | (below >> (32 - bs)) : lo;
    }
    while (n > 0 && a.v[n - 1] == 0) --n;
    a.n = n;
}
RDF_TF_HD int tf_big_cmp(const TfBig& a, const TfBig& b) {
    if (a.n != b.n) return a.n < b.n ? -1 : 1;
    for (int i = a.n - 1; i >= 0; --i)
        if (a.v[i] != b.v[i]) return a.v[i] < b.v[i] ? -1 : 1;
    return 0;
}
RDF_TF_HD void tf_big_sub(TfBig& a, const TfBig& b) {   // a >= b
    uint64_t borrow = 0;
    for (int i = 0; i < a.n; ++i) {
        const uint64_t t = (uint64_t)a.v[i] - (i < b.n ? b.v[i] : 0u) - borrow;
        a.v[i] = (uint32_t)t;
        borrow = (t >> 32) & 1u;
    }
    while (a.n > 0 && a.v[a.n - 1] == 0) --a.n;
}
// the top 64 bits of a (a != 0) as h with 2^63 <= h when a has 64 bits or more; *exp2: the weight of one unit of h; *sticky
RDF_TF_HD uint64_t tf_big_top(const TfBig& a, int* exp2, bool* sticky) {
    const int bits = tf_big_bits(a);
    if (bits <= 64) {
        *exp2 = 0;
        *sticky = false;
        return (uint64_t)a.v[0] | (a.n > 1 ? (uint64_t)a.v[1] << 32 : 0ull);
    }
    const int sh = bits - 64;           // drop sh bits
    const int ws = sh >> 5, bs = sh & 31;
    uint64_t h = 0;
    for (int k = 2; k >= 0; --k) {      // limbs ws .. ws + 2 hold the 64 bits
        const uint64_t limb = ws + k < a.n ? a.v[ws + k] : 0u;
        if (k == 2) h = bs ? limb << (64 - bs) : 0ull;
        else if (k == 1) h |= bs ? limb << (32 - bs) : limb << 32;
        else h |= limb >> bs;
    }
    bool st = bs ? (a.v[ws] & ((1u << bs) - 1u)) != 0 : false;
    for (int i = 0; i < ws && !st; ++i) st = a.v[i] != 0;
    *exp2 = sh;
    *sticky = st;
    return h;
}

// a row tf_scan took as TF_NUM -> the magnitude bits, by exact arithmetic alone
template <bool F32>
RDF_TF_HD uint64_t tf_exact(const uint8_t* b, const uint8_t* e) {
    typedef TfType<F32> T;
    textconv_trim(b, e);
    const uint8_t* p = b;
    if (p < e && (*p == '+' || *p == '-')) ++p;
    TfBig A;
    A.n = 0;
    int nd = 0;
    int64_t q = 0;
    bool sticky = false;
    uint32_t acc = 0, mul = 1;
    for (int part = 0; part < 2; ++part) {       // the integer digits, then the fraction's
        for (; p < e; ++p) {
            const uint32_t d = (uint32_t)*p - (uint32_t)'0';
            if (d > 9u) break;
            if (nd == 0 && d == 0) { q -= part; continue; }
            if (nd < kTfExactDigits) {
                acc = acc * 10u + d;
                mul *= 10u;
                if (mul == 1000000000u) { tf_big_muladd(A, mul, acc); acc = 0; mul = 1; }
                ++nd;
                q -= part;
            } else {
                sticky = sticky || d != 0;
                q += 1 - part;
            }
        }
        if (part == 0) {
            if (p < e && *p == '.') ++p;
            else break;
        }
    }
    if (mul != 1u) tf_big_muladd(A, mul, acc);
    if (nd == 0) return 0;
    if (sticky) { tf_big_muladd(A, 10u, 1u); ++nd; --q; }
    int64_t ev;
    tf_take_exponent(p, e, &ev);
    q += ev;
    const int64_t e10 = q + nd - 1;              // 10^e10 <= the value < 10^(e10 + 1)
    if (e10 >= 309) return T::INF;
    if (e10 + 1 <= -324) return 0;               // below 10^-324 < 2^-1075
    int exp2;
    bool st;
    if (q >= 0) {                                // A * 10^q < 10^310
        int left = (int)q;
        for (; left >= 9; left -= 9) tf_big_muladd(A, 1000000000u, 0u);
        uint32_t m10 = 1;
        for (; left > 0; --left) m10 *= 10u;
        if (m10 != 1u) tf_big_muladd(A, m10, 0u);
        const uint64_t h = tf_big_top(A, &exp2, &st);
        return tf_round<F32>(h, st, exp2);
    }
    TfBig B;                                     // 5^-q, -q <= 324 + 771
    B.n = 1;
    B.v[0] = 1;
    int left = (int)-q;
    for (; left >= 13; left -= 13) tf_big_muladd(B, 1220703125u, 0u);
    uint32_t m5 = 1;
    for (; left > 0; --left) m5 *= 5u;
    if (m5 != 1u) tf_big_muladd(B, m5, 0u);
    const int d = tf_big_bits(A) - tf_big_bits(B);   // align the two: A' / B' in (1/2, 2), A / B = A' / B' * 2^d
    if (d > 0) tf_big_shl(B, d);
    else tf_big_shl(A, -d);
    uint64_t quo = 0;                            // floor(A' / B' * 2^63) >= 2^62
    for (int i = 0; i < 64; ++i) {
        quo <<= 1;
        if (tf_big_cmp(A, B) >= 0) { tf_big_sub(A, B); quo |= 1u; }
        tf_big_shl(A, 1);
    }
    return tf_round<F32>(quo, A.n != 0, (int)q + d - 63);
}

// one row, whole: what the host test and a caller without a resolve pass use.  *undecided (may be null): the fast path gave up.
template <bool F32>
RDF_TF_HD bool textfloat_parse(const uint64_t* tab, const uint8_t* b, const uint8_t* e, bool exact_only, uint64_t* bits, bool* undecided) {
    typedef TfType<F32> T;
    const TfScan s = tf_scan(b, e);
    if (undecided) *undecided = false;
    if (s.kind == TF_FAIL) return false;
    if (s.kind == TF_NAN) { *bits = T::QNAN; return true; }
    uint64_t mag = T::INF;
    if (s.kind == TF_NUM && (exact_only || !tf_fast<F32>(tab, s.m, s.q, s.sticky, &mag))) {
        if (undecided) *undecided = true;
        mag = tf_exact<F32>(b, e);
    }
    *bits = mag | (s.neg ? T::SIGN : 0ull);
    return true;
}

// ----------------------------------------------------------------------------------------------------------------- format
struct TfDec { uint64_t digits; int32_t exp10; };   // digits * 10^exp10

// floor(g * cp / 2^128) with the bits below folded into bit 0 (round to odd); g = (ghi, glo), cp * g < 2^192
RDF_TF_HD uint64_t tf_round_to_odd(uint64_t ghi, uint64_t glo, uint64_t cp) {
    const tf_u128 x = (tf_u128)glo * cp;
    const tf_u128 y = (tf_u128)ghi * cp + (uint64_t)(x >> 64);
    return (uint64_t)(y >> 64) | ((uint64_t)y > 1 ? 1u : 0u);
}

// finite, non-zero magnitude bits -> the decimal of the rules above (trailing zeros not yet removed)
template <bool F32>
RDF_TF_HD TfDec tf_shortest(const uint64_t* tab, uint64_t mag) {
    typedef TfType<F32> T;
    const uint64_t frac = mag & ((1ull << (T::MANT - 1)) - 1ull);
    const int ex = (int)(mag >> (T::MANT - 1));
    const uint64_t c = ex ? frac | (1ull << (T::MANT - 1)) : frac;
    const int q = (ex ? ex : 1) - T::BIAS - (T::MANT - 1);
    TfDec r;
    if (ex != 0 && q <= 0 && -q < T::MANT && (c & ((1ull << -q) - 1ull)) == 0) {   // an integer below 2^MANT: its own digits
        r.digits = c >> -q;
        r.exp10 = 0;
        return r;
    }
    const bool even = (c & 1) == 0;
    const bool lower_closer = frac == 0 && ex > 1;
    const uint64_t cbl = 4 * c - 2 + (lower_closer ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
    int k = lower_closer ? (q * 1262611 - 524031) >> 22 : (q * 1262611) >> 22;   // floor(log10(2^q)) or of 3/4 of it
    for (;;) {
        const int h = q + tf_floor_log2_pow10(-k) + 1;                             // 1 .. 4 (up to 8 on the second turn)
        const uint64_t ghi = tab[2 * (-k - kTfPow10Min)], glo = tab[2 * (-k - kTfPow10Min) + 1];
        const uint64_t vbl = tf_round_to_odd(ghi, glo, cbl << h), vb = tf_round_to_odd(ghi, glo, cb << h), vbr = tf_round_to_odd(ghi, glo, cbr << h);
        const uint64_t lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
        const uint64_t s = vb >> 2;
        if (s < 10) { --k; continue; }           // the smallest subnormals only: one more digit, so that two are chosen
        if (s >= 100) {                          // a multiple of 10^(k+1) that still has two digits
            const uint64_t sp = s / 10;
            const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
            if (up_in != wp_in) { r.digits = sp + (wp_in ? 1 : 0); r.exp10 = k + 1; return r; }
        }
        const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
        if (u_in != w_in) { r.digits = s + (w_in ? 1 : 0); r.exp10 = k; return r; }
        const uint64_t mid = 4 * s + 2;
        const bool up = vb > mid || (vb == mid && (s & 1));
        r.digits = s + (up ? 1 : 0);
        r.exp10 = k;
        return r;
    }
}

RDF_TF_HD uint64_t tf_pow10_u64(int n) {   // 0 <= n <= 16
    switch (n) {
        case 0: return 1ull; case 1: return 10ull; case 2: return 100ull; case 3: return 1000ull; case 4: return 10000ull;
        case 5: return 100000ull; case 6: return 1000000ull; case 7: return 10000000ull; case 8: return 100000000ull;
        case 9: return 1000000000ull; case 10: return 10000000000ull; case 11: return 100000000000ull; case 12: return 1000000000000ull;
        case 13: return 10000000000000ull; case 14: return 100000000000000ull; case 15: return 1000000000000000ull;
        default: return 10000000000000000ull;
    }
}
RDF_TF_HD int tf_count_digits(uint64_t v) {   // v < 10^17
    if (v < 100000000ull) {
        if (v < 10000ull) return v < 100ull ? (v < 10ull ? 1 : 2) : (v < 1000ull ? 3 : 4);
        return v < 1000000ull ? (v < 100000ull ? 5 : 6) : (v < 10000000ull ? 7 : 8);
    }
    if (v < 1000000000000ull) return v < 10000000000ull ? (v < 1000000000ull ? 9 : 10) : (v < 100000000000ull ? 11 : 12);
    if (v < 100000000000000ull) return v < 10000000000000ull ? 13 : 14;
    return v < 10000000000000000ull ? (v < 1000000000000000ull ? 15 : 16) : 17;
}

// digit i (0 = the first) of the 17-digit number hi * 10^9 + lo, hi < 10^8, lo < 10^9: I is a constant after unrolling
template <int I>
RDF_TF_HD uint8_t tf_digit(uint32_t hi, uint32_t lo) {
    constexpr uint32_t p = I < 8 ? (I == 0 ? 10000000u : I == 1 ? 1000000u : I == 2 ? 100000u : I == 3 ? 10000u : I == 4 ? 1000u : I == 5 ? 100u : I == 6 ? 10u : 1u)
                                 : (I == 8 ? 100000000u : I == 9 ? 10000000u : I == 10 ? 1000000u : I == 11 ? 100000u : I == 12 ? 10000u : I == 13 ? 1000u : I == 14 ? 100u : I == 15 ? 10u : 1u);
    const uint32_t v = (I < 8 ? hi : lo) / p;
    return (uint8_t)('0' + (v - 10u * (v / 10u)));
}
template <int I, class S>
struct TfDigits {
    RDF_TF_HD static void put(S& s, uint32_t hi, uint32_t lo, int len, int point_after) {
        if (I < len) {
            s.put(tf_digit<I>(hi, lo));
            if (I == point_after) s.put('.');
            TfDigits<I + 1, S>::put(s, hi, lo, len, point_after);
        }
    }
};
template <class S>
struct TfDigits<17, S> {
    RDF_TF_HD static void put(S&, uint32_t, uint32_t, int, int) {}
};

template <bool F32, class S>
RDF_TF_HD void tf_emit(S& s, const uint64_t* tab, uint64_t bits) {
    typedef TfType<F32> T;
    const uint64_t mag = bits & (T::SIGN - 1ull);
    if (mag > T::INF) { s.put('N'); s.put('a'); s.put('N'); return; }
    if (bits & T::SIGN) s.put('-');
    if (mag == T::INF) { s.put('I'); s.put('n'); s.put('f'); s.put('i'); s.put('n'); s.put('i'); s.put('t'); s.put('y'); return; }
    if (mag == 0) { s.put('0'); s.put('.'); s.put('0'); return; }
    TfDec d = tf_shortest<F32>(tab, mag);
    uint64_t D = d.digits;
    int k = d.exp10;
    if (D - 100000000ull * (D / 100000000ull) == 0) { D /= 100000000ull; k += 8; }   // trailing zeros, by constant divisors
    for (int i = 0; i < 8; ++i) {
        const uint64_t t = D / 10ull;
        if (D - 10ull * t != 0) break;
        D = t;
        ++k;
    }
    const int len = tf_count_digits(D);
    const int E = k + len - 1;                    // the scientific exponent
    const uint64_t D17 = D * tf_pow10_u64(17 - len);   // 17 digits, the value's first
    const uint64_t hi64 = D17 / 1000000000ull;
    const uint32_t hi = (uint32_t)hi64, lo = (uint32_t)(D17 - hi64 * 1000000000ull);
    if (E >= -3 && E < 7) {
        if (E < 0) {
            s.put('0');
            s.put('.');
            if (E < -1) s.put('0');
            if (E < -2) s.put('0');
            TfDigits<0, S>::put(s, hi, lo, len, -1);
        } else if (len > E + 1) {
            TfDigits<0, S>::put(s, hi, lo, len, E);
        } else {
            TfDigits<0, S>::put(s, hi, lo, len, -1);
            for (int i = len; i < E + 1; ++i) s.put('0');
            s.put('.');
            s.put('0');
        }
        return;
    }
    if (len > 1) TfDigits<0, S>::put(s, hi, lo, len, 0);
    else { TfDigits<0, S>::put(s, hi, lo, 1, 0); s.put('0'); }
    s.put('E');
    uint32_t a = (uint32_t)E;
    if (E < 0) { s.put('-'); a = (uint32_t)-E; }
    if (a >= 100u) { const uint32_t x = a / 100u; s.put((uint8_t)('0' + x)); a -= 100u * x; const uint32_t y = a / 10u; s.put((uint8_t)('0' + y)); s.put((uint8_t)('0' + (a - 10u * y))); }
    else if (a >= 10u) { const uint32_t y = a / 10u; s.put((uint8_t)('0' + y)); s.put((uint8_t)('0' + (a - 10u * y))); }
    else s.put((uint8_t)('0' + a));
}

// bits: the value's storage, zero-extended.  The length of its text / the text into a window of that length
template <bool F32>
RDF_TF_HD int textfloat_length(const uint64_t* tab, uint64_t bits) {
    TcCount s = {0};
    tf_emit<F32>(s, tab, bits);
    return s.n;
}
template <bool F32>
RDF_TF_HD uint8_t* textfloat_write(const uint64_t* tab, uint64_t bits, uint8_t* dst) {
    TcStore s = {dst};
    tf_emit<F32>(s, tab, bits);
    return s.p;
}

// ---------------------------------------------------------------------------------------------------------------------
// The kernels' argument blocks and launchers (hipcc only; everything above is plain C++).
#if defined(__HIPCC__)
struct TfParseArgs {
    const Utf8Chunk*   chunks;
    int64_t            nchunks;
    const int64_t*     tile_start;   // nchunks + 1 entries
    int64_t            ntiles;
    const TcParseOut*  outs;         // per chunk
    int32_t            f32;          // the output dtype is Float32
    int32_t            stage;        // 0: never stage a tile in LDS
    int32_t            exact;        // 1: every number goes to the resolve kernel
    int32_t            pad_;
    unsigned long long* nulls;       // per chunk: NULL rows of the output
    unsigned long long* failed;      // per chunk: rows that were not NULL and did not parse
    unsigned long long* undecided;   // per chunk: rows left to the resolve kernel
    uint64_t*          flags;        // per tile and wave (4 words a tile): the undecided rows of the wave
};
hipError_t launch_textfloat_parse(const TfParseArgs& a, hipStream_t s);
hipError_t launch_textfloat_resolve(const TfParseArgs& a, hipStream_t s);
// the format passes take rdf_utf8_format's argument block (kind and pattern unused, dtype RDF_F32 / RDF_F64, max_row 15 / 24)
hipError_t launch_textfloat_size(const TcFormatArgs& a, hipStream_t s);
hipError_t launch_textfloat_write(const TcFormatArgs& a, hipStream_t s);
#endif
