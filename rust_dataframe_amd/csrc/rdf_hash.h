// rdf_hash.h — the functions that DEFINE the 64-bit hashes rows are matched by before their keys are compared:
//   Utf8 rows   rdf_colstats.hip: cs_utf8_hash_kernel -> cs_utf8_verify_kernel / cs_dict_rep_kernel (rdf_utf8_uniques,
//               rdf_utf8_dictionary_encode and, through the encoder, GROUP BY and join on text keys)
//   key tuples  rdf_join.hip: join_combine_kernel -> join_verify (rdf_equijoin_indices_multi on 2..4 key columns)
// Shared by the kernels and a CPU program (tests/cpp/test_hash.cpp) that the Python models of tests/hash_models.py are held to:
// every mixer in here is a bijection of 64-bit words, so keys that really collide can be constructed, and the tests run the
// "hash equal, keys different" branches on them.  The kernels call these functions; the loops in here are the sequential
// statement of the sums the kernels spread over lanes.  No HIP types in here.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RDF_HASH_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define RDF_HASH_HD inline
#endif

namespace rdfk {

constexpr int kCsLongRow = 512;                        // Utf8 rows of this many bytes or more are hashed / compared by a whole wave
constexpr int kCsStreams = 64;                         // ... one stream of words per lane
constexpr uint64_t kCsEmpty = 0xFFF7A5A55A5A0001ull;   // free slot of the sets: a NaN payload no normalised Float64 key has

// MurmurHash3's finaliser
RDF_HASH_HD uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// bytes [8w, 8w + 8) of a row as a little-endian word, zero beyond the row's end (nothing past the row is read)
RDF_HASH_HD uint64_t cs_word(const uint8_t* p, int32_t len, int32_t w) {
    const int32_t o = w * 8;
    uint64_t x = 0;
    if (o + 8 <= len) { __builtin_memcpy(&x, p + o, 8); return x; }
    for (int b = 0; o + b < len; ++b) x |= (uint64_t)p[o + b] << (8 * b);
    return x;
}
// The hash of a row: word w goes into stream w mod 64, a stream chains its words, the streams are added, the length closes
// it.  A row below 512 bytes has at most one word per stream, so one lane can add its terms in a loop; a wave takes a
// longer row with lane j on stream j.  Same value either way.
RDF_HASH_HD uint64_t cs_term(uint64_t st, uint64_t word, int32_t w) {
    return mix64(st ^ (word + (uint64_t)(w + 1) * 0x9E3779B97F4A7C15ull));
}
// a hash equal to the table's free word becomes its neighbour: a collision of the code's own making, verified like any other
RDF_HASH_HD uint64_t cs_hash_close(uint64_t acc, int32_t len) {
    const uint64_t h = mix64(acc ^ ((uint64_t)(uint32_t)len * 0xD6E8FEB86659FD93ull));
    return h == kCsEmpty ? h ^ 1 : h;
}
// stream j of a row: its words j, j + 64, j + 128, ... chained (what lane j of the wave computes for a long row)
RDF_HASH_HD uint64_t cs_stream(const uint8_t* p, int32_t len, int32_t j) {
    const int32_t nw = (len + 7) >> 3;
    uint64_t st = 0;
    for (int32_t w = j; w < nw; w += kCsStreams) st = cs_term(st, cs_word(p, len, w), w);
    return st;
}
// the hash of a row of `len` bytes, sequentially
RDF_HASH_HD uint64_t cs_row_hash(const uint8_t* p, int32_t len) {
    uint64_t acc = 0;
    for (int32_t j = 0; j < kCsStreams; ++j) acc += cs_stream(p, len, j);   // (a stream without words is 0)
    return cs_hash_close(acc, len);
}

// multi-column join keys: one 64-bit hash per row over the columns' order-preserving key bits (SplitMix64's finaliser per
// column, chained)
constexpr uint64_t kJoinMul = 0x9E3779B97F4A7C15ull;     // slot = (key * kJoinMul) >> tshift; odd: key -> key * kJoinMul is a bijection
RDF_HASH_HD uint64_t join_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr uint64_t kJoinSeed = kJoinMul;
RDF_HASH_HD uint64_t join_tuple_step(uint64_t h, uint64_t bits, int k) { return join_mix(h ^ bits) + kJoinMul * (uint64_t)(k + 1); }
// bits[k] = the order-preserving key bits of column k (sort_keys_kernel's transform of the column's dtype)
RDF_HASH_HD uint64_t join_tuple_hash(const uint64_t* bits, int nkeys) {
    uint64_t h = kJoinSeed;
    for (int k = 0; k < nkeys; ++k) h = join_tuple_step(h, bits[k], k);
    return h;
}

}  // namespace rdfk
