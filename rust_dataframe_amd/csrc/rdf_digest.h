// rdf_digest.h — what rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32 compute about ONE row or ONE fixed-width value
// (kernels: rdf_digest.hip, host side: rdf_capi_digest.inc).  ONE definition, __host__ __device__ inline: hipcc compiles it
// into the kernels' lane-per-row path, plain g++ compiles it into tests/cpp/test_digest_host.cpp.  It includes nothing of HIP.
//
//   Murmur3_x86_32 as Spark hashes with it (hashInt, hashLong, hashUnsafeBytes: the byte tail is Spark's, every byte after
//   the 4-byte words alone, SIGNED, through a full mixK1 / mixH1 round), XXH64 (the standard one, the running hash as seed),
//   CRC-32 (zlib's, reflected 0xEDB88320), MD5, SHA-1, SHA-224/256, SHA-384/512 and the lowercase-hex text of a digest.
//
// Rules kept throughout:
//   bounds      a function handed [b, e) reads no byte outside it: a 4- or 8-byte load is issued only when all of its bytes
//               lie inside the row, heads and tails go byte by byte, any alignment.  The empty row [nullptr, nullptr) reads
//               nothing and forms no pointer other than nullptr + 0
//   registers   the padded final block(s) of MD5 / SHA are formed word by word (dg_padded_word): a word inside the row is
//               loaded, the word that takes the 0x80 is put together from at most 3 bytes, the words after it are 0 and the
//               length words are placed by comparison.  No array is indexed by a run-time value: the message schedule W[16]
//               and the state are indexed by the counters of fully unrolled loops only (rounds in groups of 16), so the
//               kernels keep them in registers and use no scratch
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RDF_DG_HD __host__ __device__ inline
#else
#define RDF_DG_HD inline
#endif
#if defined(__clang__)
#define RDF_DG_UNROLL _Pragma("unroll")
#define RDF_DG_NOUNROLL _Pragma("nounroll")
#else
#define RDF_DG_UNROLL
#define RDF_DG_NOUNROLL
#endif

// rdf_hash_kind / rdf_digest_kind / rdf_dtype of include/rdf_mi355x.h, restated so that this header stands alone
// (rdf_capi_digest.inc static_asserts that they agree)
enum : int { DGH_MURMUR3_32 = 0, DGH_XXHASH64 = 1, DGH_NKINDS };
enum : int { DG_MD5 = 0, DG_SHA1, DG_SHA224, DG_SHA256, DG_SHA384, DG_SHA512, DG_NKINDS };
enum : int { DGT_I8 = 0, DGT_I16, DGT_I32, DGT_I64, DGT_U8, DGT_U16, DGT_U32, DGT_U64, DGT_F32, DGT_F64, DGT_BOOL, DGT_NTYPES };
constexpr int kHashColsMax = 8;
constexpr int kDigestHexWords = 16;   // 8-byte words of the longest hex text (SHA-512: 128 characters)

// characters of the hex text = 2 x the digest's bytes
RDF_DG_HD constexpr int digest_hex_bytes(int kind) {
    return kind == DG_MD5 ? 32 : kind == DG_SHA1 ? 40 : kind == DG_SHA224 ? 56 : kind == DG_SHA256 ? 64 : kind == DG_SHA384 ? 96 : 128;
}

RDF_DG_HD uint32_t dg_load4(const uint8_t* p) { uint32_t w; __builtin_memcpy(&w, p, 4); return w; }
RDF_DG_HD uint64_t dg_load8(const uint8_t* p) { uint64_t w; __builtin_memcpy(&w, p, 8); return w; }
RDF_DG_HD uint32_t dg_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }   // r in 1 .. 31
RDF_DG_HD uint32_t dg_rotr32(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }
RDF_DG_HD uint64_t dg_rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }   // r in 1 .. 63
RDF_DG_HD uint64_t dg_rotr64(uint64_t x, int r) { return (x >> r) | (x << (64 - r)); }

// ---- Murmur3_x86_32, Spark's (org.apache.spark.unsafe.hash.Murmur3_x86_32)
RDF_DG_HD uint32_t mm3_mix_k1(uint32_t k1) { k1 *= 0xcc9e2d51u; k1 = dg_rotl32(k1, 15); return k1 * 0x1b873593u; }
RDF_DG_HD uint32_t mm3_mix_h1(uint32_t h1, uint32_t k1) { h1 ^= k1; h1 = dg_rotl32(h1, 13); return h1 * 5u + 0xe6546b64u; }
RDF_DG_HD uint32_t mm3_fmix(uint32_t h1, uint32_t len) {
    h1 ^= len; h1 ^= h1 >> 16; h1 *= 0x85ebca6bu; h1 ^= h1 >> 13; h1 *= 0xc2b2ae35u; return h1 ^ (h1 >> 16);
}
RDF_DG_HD uint32_t mm3_hash_int(uint32_t v, uint32_t seed) { return mm3_fmix(mm3_mix_h1(seed, mm3_mix_k1(v)), 4); }
RDF_DG_HD uint32_t mm3_hash_long(uint64_t v, uint32_t seed) {
    uint32_t h1 = mm3_mix_h1(seed, mm3_mix_k1((uint32_t)v));
    h1 = mm3_mix_h1(h1, mm3_mix_k1((uint32_t)(v >> 32)));
    return mm3_fmix(h1, 8);
}
RDF_DG_HD uint32_t mm3_hash_bytes(const uint8_t* b, const uint8_t* e, uint32_t seed) {
    const int64_t len = e - b;
    uint32_t h1 = seed;
    int64_t i = 0;
    for (; i + 4 <= len; i += 4) h1 = mm3_mix_h1(h1, mm3_mix_k1(dg_load4(b + i)));
    for (; i < len; ++i) h1 = mm3_mix_h1(h1, mm3_mix_k1((uint32_t)(int32_t)(int8_t)b[i]));   // Spark's tail: a signed byte a round
    return mm3_fmix(h1, (uint32_t)len);
}

// ---- XXH64
constexpr uint64_t kXxP1 = 0x9E3779B185EBCA87ull, kXxP2 = 0xC2B2AE3D27D4EB4Full, kXxP3 = 0x165667B19E3779F9ull,
                   kXxP4 = 0x85EBCA77C2B2AE63ull, kXxP5 = 0x27D4EB2F165667C5ull;
RDF_DG_HD uint64_t xx64_round(uint64_t acc, uint64_t v) { return dg_rotl64(acc + v * kXxP2, 31) * kXxP1; }
RDF_DG_HD uint64_t xx64_merge(uint64_t h, uint64_t v) { return (h ^ xx64_round(0, v)) * kXxP1 + kXxP4; }
RDF_DG_HD uint64_t xx64_fmix(uint64_t h) { h ^= h >> 33; h *= kXxP2; h ^= h >> 29; h *= kXxP3; return h ^ (h >> 32); }
RDF_DG_HD uint64_t xx64_hash_int(uint32_t v, uint64_t seed) {   // XXH64 of the 4 little-endian bytes
    uint64_t h = seed + kXxP5 + 4;
    h ^= (uint64_t)v * kXxP1;
    return xx64_fmix(dg_rotl64(h, 23) * kXxP2 + kXxP3);
}
RDF_DG_HD uint64_t xx64_hash_long(uint64_t v, uint64_t seed) {  // XXH64 of the 8 little-endian bytes
    uint64_t h = seed + kXxP5 + 8;
    h ^= xx64_round(0, v);
    return xx64_fmix(dg_rotl64(h, 27) * kXxP1 + kXxP4);
}
RDF_DG_HD uint64_t xx64_hash_bytes(const uint8_t* b, const uint8_t* e, uint64_t seed) {
    const int64_t len = e - b;
    int64_t i = 0;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = seed + kXxP1 + kXxP2, v2 = seed + kXxP2, v3 = seed, v4 = seed - kXxP1;
        for (; i + 32 <= len; i += 32) {
            v1 = xx64_round(v1, dg_load8(b + i));
            v2 = xx64_round(v2, dg_load8(b + i + 8));
            v3 = xx64_round(v3, dg_load8(b + i + 16));
            v4 = xx64_round(v4, dg_load8(b + i + 24));
        }
        h = dg_rotl64(v1, 1) + dg_rotl64(v2, 7) + dg_rotl64(v3, 12) + dg_rotl64(v4, 18);
        h = xx64_merge(h, v1); h = xx64_merge(h, v2); h = xx64_merge(h, v3); h = xx64_merge(h, v4);
    } else {
        h = seed + kXxP5;
    }
    h += (uint64_t)len;
    for (; i + 8 <= len; i += 8) { h ^= xx64_round(0, dg_load8(b + i)); h = dg_rotl64(h, 27) * kXxP1 + kXxP4; }
    if (i + 4 <= len) { h ^= (uint64_t)dg_load4(b + i) * kXxP1; h = dg_rotl64(h, 23) * kXxP2 + kXxP3; i += 4; }
    for (; i < len; ++i) { h ^= (uint64_t)b[i] * kXxP5; h = dg_rotl64(h, 11) * kXxP1; }
    return xx64_fmix(h);
}

// ---- one value of a fixed-width column folded into the running hash.  raw: the value's bytes, zero-extended (Boolean: the
// bit).  Signed integers are sign-extended, unsigned ones zero-extended; every NaN hashes as the canonical quiet NaN and
// -0.0 as +0.0 (the project's canonical-float rule)
RDF_DG_HD uint32_t dg_canon_f32(uint32_t bits) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0x7fc00000u;
    return bits == 0x80000000u ? 0u : bits;
}
RDF_DG_HD uint64_t dg_canon_f64(uint64_t bits) {
    if ((bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return 0x7ff8000000000000ull;
    return bits == 0x8000000000000000ull ? 0ull : bits;
}
RDF_DG_HD bool dg_is_long(int dtype) { return dtype == DGT_I64 || dtype == DGT_U64 || dtype == DGT_F64; }
RDF_DG_HD int dg_type_bytes(int dtype) {   // 0: bit-packed
    switch (dtype) {
        case DGT_I8: case DGT_U8: return 1;
        case DGT_I16: case DGT_U16: return 2;
        case DGT_I32: case DGT_U32: case DGT_F32: return 4;
        case DGT_BOOL: return 0;
        default: return 8;
    }
}
// the Int32 / Int64 a value is hashed as
RDF_DG_HD uint64_t dg_hashed_bits(int dtype, uint64_t raw) {
    switch (dtype) {
        case DGT_I8:   return (uint32_t)(int32_t)(int8_t)raw;
        case DGT_I16:  return (uint32_t)(int32_t)(int16_t)raw;
        case DGT_F32:  return dg_canon_f32((uint32_t)raw);
        case DGT_F64:  return dg_canon_f64(raw);
        case DGT_BOOL: return raw & 1;
        case DGT_I64: case DGT_U64: return raw;
        default:       return (uint32_t)raw;   // I32, U8, U16, U32
    }
}
template <int KIND>
RDF_DG_HD uint64_t dg_hash_fixed(int dtype, uint64_t raw, uint64_t h) {
    const uint64_t v = dg_hashed_bits(dtype, raw);
    if (KIND == DGH_MURMUR3_32) return dg_is_long(dtype) ? mm3_hash_long(v, (uint32_t)h) : mm3_hash_int((uint32_t)v, (uint32_t)h);
    return dg_is_long(dtype) ? xx64_hash_long(v, h) : xx64_hash_int((uint32_t)v, h);
}
template <int KIND>
RDF_DG_HD uint64_t dg_hash_bytes(const uint8_t* b, const uint8_t* e, uint64_t h) {
    if (KIND == DGH_MURMUR3_32) return mm3_hash_bytes(b, e, (uint32_t)h);
    return xx64_hash_bytes(b, e, h);
}

// ---- CRC-32.  The table is the caller's (the kernel fills it in LDS): entry i
RDF_DG_HD uint32_t crc32_table_entry(uint32_t i) {
    uint32_t c = i;
    RDF_DG_UNROLL
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}
RDF_DG_HD uint32_t crc32_row(const uint8_t* b, const uint8_t* e, const uint32_t* table) {
    const int64_t len = e - b;
    uint32_t c = 0xFFFFFFFFu;
    for (int64_t i = 0; i < len; ++i) c = table[(c ^ b[i]) & 0xFFu] ^ (c >> 8);
    return ~c;
}

// ---- the padded message of MD5 / SHA, word by word.  The little-endian 32-bit word at byte `pos` (a multiple of 4) of
// row bytes ++ 0x80 ++ zeros; the length words are the caller's
RDF_DG_HD uint32_t dg_padded_word(const uint8_t* b, int64_t len, int64_t pos) {
    if (pos + 4 <= len) return dg_load4(b + pos);
    if (pos > len) return 0;
    const int n = (int)(len - pos);   // 0 .. 3 bytes of the row, then the 0x80
    uint32_t w = 0x80u << (8 * n);
    if (n > 0) {
        const uint8_t* p = b + pos;
        w |= p[0];
        if (n > 1) w |= (uint32_t)p[1] << 8;
        if (n > 2) w |= (uint32_t)p[2] << 16;
    }
    return w;
}
// block `off` (a multiple of 64) of the padded message as 16 words, big- or little-endian; `last`: it carries the length
template <bool BE>
RDF_DG_HD void dg_block64(const uint8_t* b, int64_t len, int64_t off, bool last, uint32_t (&W)[16]) {
    if (off + 64 <= len) {
        RDF_DG_UNROLL
        for (int j = 0; j < 16; ++j) W[j] = dg_load4(b + off + 4 * j);
    } else {
        RDF_DG_UNROLL
        for (int j = 0; j < 16; ++j) W[j] = dg_padded_word(b, len, off + 4 * j);
    }
    if (BE) {
        RDF_DG_UNROLL
        for (int j = 0; j < 16; ++j) W[j] = __builtin_bswap32(W[j]);
    }
    const uint64_t bits = (uint64_t)len << 3;
    const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
    W[14] = last ? (BE ? hi : lo) : W[14];
    W[15] = last ? (BE ? lo : hi) : W[15];
}
RDF_DG_HD int64_t dg_padded_bytes64(int64_t len) { return ((len + 8) / 64 + 1) * 64; }     // + 0x80 + 8 length bytes, whole blocks
RDF_DG_HD int64_t dg_padded_bytes128(int64_t len) { return ((len + 16) / 128 + 1) * 128; } // + 0x80 + 16 length bytes

// ---- MD5
RDF_DG_HD void dg_md5_compress(uint32_t (&s)[4], const uint32_t (&W)[16]) {
    static constexpr uint32_t K[64] = {
        0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
        0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
        0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
        0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
        0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
        0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
        0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
        0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3];
    RDF_DG_UNROLL
    for (int i = 0; i < 64; ++i) {
        const int q = i & 3;
        uint32_t f;
        int g, r;
        if (i < 16)      { f = (b & c) | (~b & d); g = i;                r = q == 0 ? 7 : q == 1 ? 12 : q == 2 ? 17 : 22; }
        else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; r = q == 0 ? 5 : q == 1 ? 9 : q == 2 ? 14 : 20; }
        else if (i < 48) { f = b ^ c ^ d;          g = (3 * i + 5) & 15; r = q == 0 ? 4 : q == 1 ? 11 : q == 2 ? 16 : 23; }
        else             { f = c ^ (b | ~d);       g = (7 * i) & 15;     r = q == 0 ? 6 : q == 1 ? 10 : q == 2 ? 15 : 21; }
        f += a + K[i] + W[g];
        a = d; d = c; c = b;
        b += dg_rotl32(f, r);
    }
    s[0] += a; s[1] += b; s[2] += c; s[3] += d;
}

// ---- SHA-1
RDF_DG_HD void dg_sha1_compress(uint32_t (&s)[5], uint32_t (&W)[16]) {
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4];
    RDF_DG_UNROLL
    for (int t = 0; t < 80; ++t) {
        if (t >= 16) W[t & 15] = dg_rotl32(W[(t + 13) & 15] ^ W[(t + 8) & 15] ^ W[(t + 2) & 15] ^ W[t & 15], 1);
        uint32_t f, k;
        if (t < 20)      { f = (b & c) | (~b & d);          k = 0x5A827999u; }
        else if (t < 40) { f = b ^ c ^ d;                   k = 0x6ED9EBA1u; }
        else if (t < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8F1BBCDCu; }
        else             { f = b ^ c ^ d;                   k = 0xCA62C1D6u; }
        const uint32_t tmp = dg_rotl32(a, 5) + f + e + k + W[t & 15];
        e = d; d = c; c = dg_rotl32(b, 30); b = a; a = tmp;
    }
    s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e;
}

// ---- SHA-224 / SHA-256: 4 groups of 16 rounds, the schedule rolled over W[16] in place
RDF_DG_HD void dg_sha256_compress(uint32_t (&s)[8], uint32_t (&W)[16]) {
    static constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
        0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
        0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
        0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
    RDF_DG_NOUNROLL
    for (int r0 = 0; r0 < 64; r0 += 16) {
        RDF_DG_UNROLL
        for (int i = 0; i < 16; ++i) {
            if (r0) {
                const uint32_t w15 = W[(i + 1) & 15], w2 = W[(i + 14) & 15];
                W[i] += (dg_rotr32(w2, 17) ^ dg_rotr32(w2, 19) ^ (w2 >> 10)) + W[(i + 9) & 15] + (dg_rotr32(w15, 7) ^ dg_rotr32(w15, 18) ^ (w15 >> 3));
            }
            const uint32_t t1 = h + (dg_rotr32(e, 6) ^ dg_rotr32(e, 11) ^ dg_rotr32(e, 25)) + ((e & f) ^ (~e & g)) + K[r0 + i] + W[i];
            const uint32_t t2 = (dg_rotr32(a, 2) ^ dg_rotr32(a, 13) ^ dg_rotr32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
    }
    s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
}

// ---- SHA-384 / SHA-512: 5 groups of 16 rounds
RDF_DG_HD void dg_sha512_compress(uint64_t (&s)[8], uint64_t (&W)[16]) {
    static constexpr uint64_t K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
        0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
        0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
        0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
        0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
        0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
        0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
        0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
        0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
        0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
        0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
        0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
        0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
        0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
        0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
        0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
        0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
        0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
        0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    uint64_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
    RDF_DG_NOUNROLL
    for (int r0 = 0; r0 < 80; r0 += 16) {
        RDF_DG_UNROLL
        for (int i = 0; i < 16; ++i) {
            if (r0) {
                const uint64_t w15 = W[(i + 1) & 15], w2 = W[(i + 14) & 15];
                W[i] += (dg_rotr64(w2, 19) ^ dg_rotr64(w2, 61) ^ (w2 >> 6)) + W[(i + 9) & 15] + (dg_rotr64(w15, 1) ^ dg_rotr64(w15, 8) ^ (w15 >> 7));
            }
            const uint64_t t1 = h + (dg_rotr64(e, 14) ^ dg_rotr64(e, 18) ^ dg_rotr64(e, 41)) + ((e & f) ^ (~e & g)) + K[r0 + i] + W[i];
            const uint64_t t2 = (dg_rotr64(a, 28) ^ dg_rotr64(a, 34) ^ dg_rotr64(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
            h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
    }
    s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
}

// ---- lowercase hex.  v: 4 digest bytes as a big-endian value (the first byte on top); the result: their 8 characters as
// they lie in memory on a little-endian machine (the first character in the lowest byte)
RDF_DG_HD uint64_t digest_hex4(uint32_t v) {
    uint64_t x = __builtin_bswap32(v);                       // byte k = digest byte k
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;              // byte 2k = digest byte k
    const uint64_t n = ((x >> 4) & 0x000F000F000F000Full) | ((x & 0x000F000F000F000Full) << 8);   // a nibble a byte, the high one first
    const uint64_t af = ((n + 0x0606060606060606ull) >> 4) & 0x0101010101010101ull;               // 1 where the nibble is 10 .. 15
    return n + 0x3030303030303030ull + af * 39;              // '0' + n, 'a' - 10 + n
}

// ---- the digest of one row as hex text: hex[0 .. digest_hex_bytes(KIND) / 8) are its characters, 8 a word
template <int KIND>
RDF_DG_HD void digest_row_hex(const uint8_t* b, const uint8_t* e, uint64_t (&hex)[kDigestHexWords]) {
    const int64_t len = e - b;
    if (KIND == DG_MD5) {
        uint32_t s[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u}, W[16];
        const int64_t total = dg_padded_bytes64(len);
        for (int64_t off = 0; off < total; off += 64) {
            dg_block64<false>(b, len, off, off + 64 == total, W);
            dg_md5_compress(s, W);
        }
        RDF_DG_UNROLL
        for (int k = 0; k < 4; ++k) hex[k] = digest_hex4(__builtin_bswap32(s[k]));   // (MD5's words are little-endian)
    } else if (KIND == DG_SHA1) {
        uint32_t s[5] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u, 0xc3d2e1f0u}, W[16];
        const int64_t total = dg_padded_bytes64(len);
        for (int64_t off = 0; off < total; off += 64) {
            dg_block64<true>(b, len, off, off + 64 == total, W);
            dg_sha1_compress(s, W);
        }
        RDF_DG_UNROLL
        for (int k = 0; k < 5; ++k) hex[k] = digest_hex4(s[k]);
    } else if (KIND == DG_SHA224 || KIND == DG_SHA256) {
        uint32_t s[8] = {
        0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
        const uint32_t s224[8] = {
        0xc1059ed8u, 0x367cd507u, 0x3070dd17u, 0xf70e5939u, 0xffc00b31u, 0x68581511u, 0x64f98fa7u, 0xbefa4fa4u};
        if (KIND == DG_SHA224) {
            RDF_DG_UNROLL
            for (int k = 0; k < 8; ++k) s[k] = s224[k];
        }
        uint32_t W[16];
        const int64_t total = dg_padded_bytes64(len);
        for (int64_t off = 0; off < total; off += 64) {
            dg_block64<true>(b, len, off, off + 64 == total, W);
            dg_sha256_compress(s, W);
        }
        RDF_DG_UNROLL
        for (int k = 0; k < (KIND == DG_SHA224 ? 7 : 8); ++k) hex[k] = digest_hex4(s[k]);
    } else {
        uint64_t s[8] = {
        0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
        0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
        const uint64_t s384[8] = {
        0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull, 0x152fecd8f70e5939ull,
        0x67332667ffc00b31ull, 0x8eb44a8768581511ull, 0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull};
        if (KIND == DG_SHA384) {
            RDF_DG_UNROLL
            for (int k = 0; k < 8; ++k) s[k] = s384[k];
        }
        uint64_t W[16];
        const int64_t total = dg_padded_bytes128(len);
        for (int64_t off = 0; off < total; off += 128) {
            if (off + 128 <= len) {
                RDF_DG_UNROLL
                for (int j = 0; j < 16; ++j) W[j] = __builtin_bswap64(dg_load8(b + off + 8 * j));
            } else {
                RDF_DG_UNROLL
                for (int j = 0; j < 16; ++j)
                    W[j] = (uint64_t)__builtin_bswap32(dg_padded_word(b, len, off + 8 * j)) << 32 | __builtin_bswap32(dg_padded_word(b, len, off + 8 * j + 4));
            }
            W[15] = off + 128 == total ? (uint64_t)len << 3 : W[15];   // (W[14], the length's upper 64 bits, is 0 already)
            dg_sha512_compress(s, W);
        }
        RDF_DG_UNROLL
        for (int k = 0; k < (KIND == DG_SHA384 ? 6 : 8); ++k) {
            hex[2 * k] = digest_hex4((uint32_t)(s[k] >> 32));
            hex[2 * k + 1] = digest_hex4((uint32_t)s[k]);
        }
    }
}
