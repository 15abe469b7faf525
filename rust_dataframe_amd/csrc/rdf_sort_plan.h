// rdf_sort_plan.h — the top-bits decision of one numeric sort column (os_column_passes in rdf_capi.cpp; kernels: rdf_sort.hip).
// Pure host arithmetic, no HIP: tests/cpp/test_sort_plan.cpp compiles it with a plain C++ compiler.
//
// A column whose keys vary in 25 bits or more, of 65 536 rows or more, is sorted by stable passes over its TOP B bits (<= 8 bits
// per pass, least significant of them first) and then one block per bucket that sorts the remaining R bits in LDS.  B comes
// from the rows (integer keys and raw key bits: as many bits as leave ~kOsRowsPerBucketInt rows per bucket and the passes carry
// for free) or from the value-bucket map of a Float64 column (rdf_sort_map.h: `value_bits`, planned from a sample or linear over
// [min, max]); a value map leaves no R — the rows of a bucket share no key bits, the whole key is compared.  Everything else
// takes one pass per byte of (key - bias) that varies.
#pragma once
#include <stdint.h>

namespace rdfk {

constexpr int kOsPlanLocalMax = 4096;          // == kOsLocalMax (rdf_device.h): the rows one block sorts in LDS
constexpr int64_t kOsMsdMinRows = 65536;       // fewer rows: byte passes
constexpr int kOsRowsPerBucketInt = 1800;      // integer keys: average rows per bucket the pass count is chosen for (sorted as 2048)
constexpr int kOsRowsPerBucketF64 = 512;       // doubles: ~500 per bucket always (a bell curve's densest bucket holds 4-5 x the average)
constexpr int kOsMaxRbits = 52;                // the narrow LDS word is (R low bits << 12) | place: R + 12 <= 64

// key kinds, as os_column_passes names them
enum : int32_t { OS_KEYS_F32 = -1, OS_KEYS_INT = 0, OS_KEYS_F64 = 1, OS_KEYS_F64_DESC = 2 };

struct OsTopPlan {
    int32_t eligible;       // 0: byte passes at once
    int32_t B, npass;       // top bits and the passes that carry them: ceil(B / 8)
    int32_t shift[3], mask[3];   // pass p's digit = ((key - bias, or the value bucket) >> shift[p]) & mask[p]; pass 0 is the least significant and takes B's remainder
    int32_t R;              // bits left to the LDS finish: sig - B, 0 under a value map
    int32_t value;          // 1: the digits are taken from the value bucket (value_bits), not from the key bits
    int32_t check_top;      // 1: the top digit's counts are read back before any pass (not under a SAMPLED value map)
    int32_t wtop;           // bits of the top digit
    int64_t top_limit;      // a top-digit value held by more rows sends the column to the byte passes: kOsLocalMax << (B - wtop)
};

// bits of (max key - bias) that vary, at most those of the `need` bytes the column's dtype has
inline int os_sig_bits(uint64_t range, int need) {
    int sig = 0;
    for (uint64_t r = range; r; r >>= 1) ++sig;
    return sig < 8 * need ? sig : 8 * need;
}

// B as the rows alone give it (what a Float64 column's linear map over [min, max] is cut into, too)
inline int os_bits_by_rows(int64_t n, int key_kind) {
    int B = 12;
    while ((n >> B) > 512 && B < 24) ++B;
    if (key_kind <= 0) {
        // integer keys: 2 passes (16 bits) up to ~1.2e8 rows, a third pass beyond
        int np = 1;
        while (np < 3 && (n >> (8 * np)) > kOsRowsPerBucketInt) ++np;
        B = B < 8 * np ? B : 8 * np;
        if (B < 12) B = 12;
        if ((n >> B) > kOsRowsPerBucketInt) B = 24;      // (no pass count fits: os_top_plan refuses)
    }
    return B;
}

// value_bits: the bucket bits of the column's value map, 0 = none (integer keys, or a Float64 column whose plan was refused:
// raw key bits); sampled: that map was planned from a sample (rdf_sort_map.h), not linear over [min, max]
inline OsTopPlan os_top_plan(int64_t n, int sig, int need, int key_kind, int value_bits, bool sampled, bool sort_msd) {
    OsTopPlan p;
    p.eligible = 0; p.npass = 0; p.R = 0; p.wtop = 0; p.top_limit = 0;
    for (int i = 0; i < 3; ++i) { p.shift[i] = 0; p.mask[i] = 0; }
    if (sig > 8 * need) sig = 8 * need;
    const int per_bucket = key_kind > 0 ? kOsRowsPerBucketF64 : kOsRowsPerBucketInt;
    const bool planned = sampled && value_bits > 0;
    const int B = planned ? value_bits : os_bits_by_rows(n, key_kind);
    p.B = B;
    p.value = value_bits > 0 ? 1 : 0;
    p.check_top = planned ? 0 : 1;
    if (!sort_msd || key_kind < 0 || n < kOsMsdMinRows || n >= ((int64_t)1 << 32)) return p;
    if (!((n >> B) <= per_bucket || planned)) return p;
    if ((sig + 7) / 8 < (B + 7) / 8 + 2) return p;            // the top passes and the finish must save two byte passes
    if (!p.value && sig - B > kOsMaxRbits) return p;
    p.eligible = 1;
    p.R = p.value ? 0 : sig - B;
    p.npass = (B + 7) / 8;
    int sh = p.R;
    for (int i = 0; i < p.npass; ++i) {
        const int w = i == 0 ? B - 8 * (p.npass - 1) : 8;
        p.shift[i] = sh; p.mask[i] = (1 << w) - 1;
        sh += w;
    }
    p.wtop = p.npass == 1 ? B : 8;
    p.top_limit = (int64_t)kOsPlanLocalMax << (B - p.wtop);
    return p;
}

}  // namespace rdfk
