// rdf_percentile.h — what rdf_groupby_percentile decides about ONE group and ONE call (kernel: rdf_percentile.hip, host side:
// rdf_capi_percentile.inc, executable model: tests/percentile_ref.py).  ONE definition, __host__ __device__ inline: hipcc
// compiles it into the kernel, plain g++ compiles it into tests/cpp/test_percentile_host.cpp.  It includes nothing of HIP.
//
// Rules kept throughout:
//   m           the group's non-NULL values, taken in the sort's order (NaN after +inf, -0.0 and +0.0 peers)
//   CONT        Spark 3's percentile: pos = (m - 1) * p, the values at floor(pos) and ceil(pos), linear in between
//   DISC        SQL's percentile_disc: the value at sorted position max(0, ceil(p * m) - 1)
//   d(v)        a value as a double: Float32 widened, integers rounded to nearest even, -0.0 read as +0.0, one NaN
//   roundings   the interpolation is two multiplies and one add, each rounded on its own (the build has -ffp-contract=off and
//               the expression is kept out of any fused builtin), so the model reproduces it bit for bit
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RDF_PCT_HD __host__ __device__ inline
#else
#define RDF_PCT_HD inline
#endif

// rdf_percentile_kind and the numeric rdf_dtype codes of include/rdf_mi355x.h, restated so that this header stands alone
// (rdf_capi_percentile.inc static_asserts)
enum : int { PCT_CONT = 0, PCT_DISC = 1, PCT_NKINDS };
enum : int { PCT_I8 = 0, PCT_I16 = 1, PCT_I32 = 2, PCT_I64 = 3, PCT_U8 = 4, PCT_U16 = 5, PCT_U32 = 6, PCT_U64 = 7, PCT_F32 = 8, PCT_F64 = 9 };

constexpr uint64_t kPctNaN = 0x7FF8000000000000ull;     // the one NaN a result can be

// ---------------------------------------------------------------- the request
// p in [0, 1]; a NaN fails both comparisons.
RDF_PCT_HD bool pct_p_ok(double p) { return p >= 0.0 && p <= 1.0; }

// ---------------------------------------------------------------- the rank rule
// Where CONT reads among m >= 1 sorted values: positions lo <= hi <= m - 1 and their weights.  (m - 1 < 2^32 is exact as a
// double; the product rounds once; floor and ceil of a double below 2^52 are exact, and so are the two differences.)
struct PctRank { int64_t lo, hi; double wlo, whi; };
RDF_PCT_HD double pct_floor(double x) { return __builtin_floor(x); }
RDF_PCT_HD double pct_ceil(double x) { return __builtin_ceil(x); }
RDF_PCT_HD PctRank pct_rank(int64_t m, double p) {
    const double pos = (double)(m - 1) * p;
    const double lo = pct_floor(pos), hi = pct_ceil(pos);
    PctRank r;
    r.lo = (int64_t)lo;
    r.hi = (int64_t)hi;
    r.wlo = hi - pos;
    r.whi = pos - lo;
    if (r.hi > m - 1) r.hi = m - 1;      // (never taken for p <= 1: the product of m - 1 and p <= 1 rounds to at most m - 1)
    if (r.lo > r.hi) r.lo = r.hi;
    return r;
}

// The sorted position DISC reads among m >= 1 values.
RDF_PCT_HD int64_t pct_disc_index(int64_t m, double p) {
    const int64_t k = (int64_t)pct_ceil(p * (double)m) - 1;
    return k < 0 ? 0 : (k > m - 1 ? m - 1 : k);
}

// ---------------------------------------------------------------- d(v)
RDF_PCT_HD uint64_t pct_bits(double d) { return __builtin_bit_cast(uint64_t, d); }
RDF_PCT_HD double pct_canon(double d) {
    if (d != d) return __builtin_bit_cast(double, kPctNaN);
    return d == 0.0 ? 0.0 : d;           // -0.0 is read as +0.0
}
// raw: the value's own bits, zero-extended from its width.
RDF_PCT_HD double pct_d(int dtype, uint64_t raw) {
    switch (dtype) {
        case PCT_I8: return (double)(int8_t)(uint8_t)raw;
        case PCT_I16: return (double)(int16_t)(uint16_t)raw;
        case PCT_I32: return (double)(int32_t)(uint32_t)raw;
        case PCT_I64: return (double)(int64_t)raw;          // nearest even beyond 2^53
        case PCT_U8: case PCT_U16: case PCT_U32: case PCT_U64: return (double)raw;
        case PCT_F32: return pct_canon((double)__builtin_bit_cast(float, (uint32_t)raw));
        default: return pct_canon(__builtin_bit_cast(double, raw));
    }
}

// ---------------------------------------------------------------- the select route: keys and the planner step
// The ordered unsigned image of a value, at the dtype's own width (pct_key_bits): a < b under the sort exactly when
// key(a) < key(b), and peers (-0.0 / +0.0, the NaNs) have one key.  pct_unkey gives back the bits of the peers' canonical
// member, which d() reads like any other.
RDF_PCT_HD int pct_key_bits(int dtype) {
    switch (dtype) {
        case PCT_I8: case PCT_U8: return 8;
        case PCT_I16: case PCT_U16: return 16;
        case PCT_I32: case PCT_U32: case PCT_F32: return 32;
        default: return 64;
    }
}
RDF_PCT_HD uint64_t pct_key(int dtype, uint64_t raw) {
    switch (dtype) {
        case PCT_I8: return (raw ^ 0x80ull) & 0xFFull;
        case PCT_I16: return (raw ^ 0x8000ull) & 0xFFFFull;
        case PCT_I32: return (raw ^ 0x80000000ull) & 0xFFFFFFFFull;
        case PCT_I64: return raw ^ 0x8000000000000000ull;
        case PCT_U8: return raw & 0xFFull;
        case PCT_U16: return raw & 0xFFFFull;
        case PCT_U32: return raw & 0xFFFFFFFFull;
        case PCT_U64: return raw;
        case PCT_F32: {
            uint32_t b = (uint32_t)raw;
            if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0x7FC00000u;      // one NaN, above +inf
            else if (b == 0x80000000u) b = 0;                           // -0.0 is +0.0
            return (b & 0x80000000u) ? (uint32_t)~b : (b | 0x80000000u);
        }
        default: {
            uint64_t b = raw;
            if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) b = kPctNaN;
            else if (b == 0x8000000000000000ull) b = 0;
            return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
        }
    }
}
RDF_PCT_HD uint64_t pct_unkey(int dtype, uint64_t key) {
    switch (dtype) {
        case PCT_I8: return (key ^ 0x80ull) & 0xFFull;
        case PCT_I16: return (key ^ 0x8000ull) & 0xFFFFull;
        case PCT_I32: return (key ^ 0x80000000ull) & 0xFFFFFFFFull;
        case PCT_I64: return key ^ 0x8000000000000000ull;
        case PCT_U8: case PCT_U16: case PCT_U32: case PCT_U64: return key;
        case PCT_F32: { const uint32_t k = (uint32_t)key; return (k & 0x80000000u) ? (k ^ 0x80000000u) : (uint32_t)~k; }
        default: return (key & 0x8000000000000000ull) ? (key ^ 0x8000000000000000ull) : ~key;
    }
}

// The planner step: `hist` counts the candidates of one prefix by their next digit, `residual` is a target's 0-based rank
// among those candidates.  -> the digit the target has, and through *residual its rank among the candidates of that digit.
// A rank beyond the candidates (it does not happen: the ranks come from the same counts) ends in the last bucket at rank 0.
RDF_PCT_HD int pct_plan_bucket(const uint32_t* hist, int nbuckets, uint64_t* residual) {
    uint64_t r = *residual;
    for (int b = 0; b < nbuckets; ++b) {
        if (r < (uint64_t)hist[b]) { *residual = r; return b; }
        r -= (uint64_t)hist[b];
    }
    *residual = 0;
    return nbuckets - 1;
}

// ---------------------------------------------------------------- the interpolation
// dlo / dhi: d() of the values at r.lo / r.hi; peers: the two are peers under the sort (equal, or both NaN).  -> the bits of
// the result.  A -inf / +inf pair gives NaN, as IEEE has it; every NaN leaves as kPctNaN.
RDF_PCT_HD uint64_t pct_interpolate(const PctRank& r, double dlo, double dhi, bool peers) {
    double v;
    if (r.lo == r.hi || peers) v = dlo;
    else {
        const double a = r.wlo * dlo;
        const double b = r.whi * dhi;
        v = a + b;
    }
    return v != v ? kPctNaN : pct_bits(v);
}
