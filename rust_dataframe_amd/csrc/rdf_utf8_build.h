// rdf_utf8_build.h — what rdf_utf8_concat / _pad / _repeat / _reverse / _substring_index decide about ONE row (kernels:
// rdf_utf8_build.hip, host side: rdf_capi_utf8_build.inc).  ONE definition, __host__ __device__ inline: hipcc compiles it
// into the kernels, plain g++ compiles it into tests/cpp/test_utf8_build_host.cpp.  It includes nothing of HIP.
//
// Rules kept throughout (rdf_utf8_pattern.h's):
//   bytes       rows, pads and delimiters are byte strings; nothing is validated as UTF-8.  A code point begins at a byte that
//               is not a continuation byte (10xxxxxx), as rdf_utf8_measure(LENGTH) counts them
//   bounds      a function handed [b, e) or (p, n) reads no byte outside it; 8-byte loads are issued only by
//               utf8_count_code_points, and only where all 8 bytes lie inside
//
// A built row is a sequence of PIECES.  Piece i covers `len` output bytes that come from p[0 .. period), cycled: output
// byte t of the piece is p[t % period].  concat: the parts and the separators between them (period = len); lpad / rpad: the
// pad cycled over the padding bytes, and the kept bytes of the row; repeat: one piece, the row cycled; substring_index: one
// piece, a span of the row.  reverse is the one op that is not a list of pieces: utf8_reverse_at maps an output byte to its
// source byte by looking at most 3 bytes to either side of the mirror position.
#pragma once
#include <stdint.h>

#include "rdf_utf8_pattern.h"

enum : int { U8B_CONCAT = 0, U8B_CONCAT_WS, U8B_LPAD, U8B_RPAD, U8B_REPEAT, U8B_REVERSE, U8B_SUBSTRING_INDEX,
             U8B_COALESCE, U8B_CASE_WHEN,   // rdf_utf8_coalesce / rdf_utf8_case_when: a row is ONE piece, the chosen part's row or literal
             U8B_NOPS };

constexpr int kUtf8PartsMax = 8;                 // parts of one concat
constexpr int kUtf8SelectSlots = kUtf8PartsMax + 1;   // case_when: eight branches and `otherwise`; the chosen slot is 4 bits of a row's note
constexpr int64_t kUtf8BuildClamp = 1ll << 31;   // len / times are clamped to it, and so is one row's output length

RDF_U8P_HD int64_t utf8_build_clamp(int64_t v) { return v < 0 ? 0 : (v > kUtf8BuildClamp ? kUtf8BuildClamp : v); }

// ---- pad
// A row of n code points padded to len code points (len already clamped) with a pad of pad_bytes bytes / pad_cp code points.
// true: the row is kept whole and *full repetitions of the pad plus its first *part bytes (the first s % p code points)
// stand beside it.  false: nothing is added and the first min(n, len) code points of the row are kept (the row is truncated).
RDF_U8P_HD bool utf8_pad_fill(int64_t n, int64_t len, const uint8_t* pad, int64_t pad_bytes, int64_t pad_cp, int64_t* full, int64_t* part) {
    *full = 0;
    *part = 0;
    if (n >= len || pad_bytes <= 0 || pad_cp <= 0) return false;   // (a pad of continuation bytes only has no code point to repeat)
    const int64_t s = len - n;
    *full = s / pad_cp;
    const uint8_t* q = pad;
    utf8_skip_code_points(pad, pad + pad_bytes, s % pad_cp, &q);
    *part = q - pad;
    return true;
}
struct Utf8PadPlan { int64_t kept, full, part; };   // kept bytes of the row, full repetitions, bytes of the partial repetition
RDF_U8P_HD Utf8PadPlan utf8_pad_plan(const uint8_t* b, const uint8_t* e, int64_t len, const uint8_t* pad, int64_t pad_bytes, int64_t pad_cp) {
    Utf8PadPlan pl = {0, 0, 0};
    if (len <= 0) return pl;
    const int64_t n = utf8_count_code_points(b, e - b);
    if (utf8_pad_fill(n, len, pad, pad_bytes, pad_cp, &pl.full, &pl.part) || n <= len) { pl.kept = e - b; return pl; }
    const uint8_t* q = e;
    utf8_skip_code_points(b, e, len, &q);
    pl.kept = q - b;
    return pl;
}
RDF_U8P_HD int64_t utf8_pad_bytes_out(const Utf8PadPlan& pl, int64_t pad_bytes) {
    const int64_t v = pl.kept + pl.full * pad_bytes + pl.part;   // (kept < 2^31, full <= 2^31, pad_bytes <= 1024: no overflow)
    return v > kUtf8BuildClamp ? kUtf8BuildClamp : v;
}

// ---- pieces
struct Utf8Piece { const uint8_t* p; int64_t len; int64_t period; };

// Output byte j (0 <= j < the pieces' lengths added up) of a row of n pieces; piece(i) returns piece i.  *k = its piece,
// *run = how many output bytes from j on are consecutive source bytes of that piece; returns the source byte's address.
template <typename PieceFn>
RDF_U8P_HD const uint8_t* utf8_piece_at(PieceFn piece, int n, int64_t j, int* k, int64_t* run) {
    int i = 0;
    Utf8Piece pc = piece(0);
    while (i + 1 < n && j >= pc.len) {
        j -= pc.len;
        pc = piece(++i);
    }
    const int64_t t = pc.period >= pc.len ? j : (int64_t)((uint64_t)j % (uint64_t)pc.period);
    const int64_t left = pc.len - j, to_wrap = (pc.period >= pc.len ? pc.len : pc.period) - t;
    *k = i;
    *run = left < to_wrap ? left : to_wrap;
    return pc.p + t;
}

// the pieces of a concat row: 2 per part, [separator before part k][part k].  present: bit k = part k is there (a NULL part
// of concat_ws is not); the separator stands before every present part but the first present one
RDF_U8P_HD bool utf8_concat_sep_before(uint32_t present, int k) { return ((present >> k) & 1u) && (present & ((1u << k) - 1u)); }
RDF_U8P_HD int64_t utf8_concat_seps(uint32_t present) {
    const int c = __builtin_popcount(present);
    return c > 0 ? c - 1 : 0;
}
// the pieces of a padded row: side 0 (lpad) [padding][row], side 1 (rpad) [row][padding]
RDF_U8P_HD Utf8Piece utf8_pad_piece(int i, int side, const uint8_t* row, int64_t kept, const uint8_t* pad, int64_t pad_bytes, int64_t out_len) {
    if ((i == 0) == (side == 0)) return Utf8Piece{pad, out_len - kept, pad_bytes > 0 ? pad_bytes : 1};
    return Utf8Piece{row, kept, kept > 0 ? kept : 1};
}

// ---- reverse: the source byte of output byte j of a row [b, b + n), and *run = the output bytes from j on that are
// consecutive source bytes (the rest of j's code point).  The code point around the mirror byte m = n - 1 - j is
// [s, t): s at most 3 bytes left of m, t at most 3 bytes right of m + 1; it is written to [n - t, n - s).
RDF_U8P_HD const uint8_t* utf8_reverse_at(const uint8_t* b, int64_t n, int64_t j, int64_t* run) {
    const int64_t m = n - 1 - j;
    int64_t s = m, t = m + 1;
    while (s > 0 && m - s < 3 && utf8_is_cont(b[s])) --s;
    while (t < n && t - (m + 1) < 3 && utf8_is_cont(b[t])) ++t;
    *run = (n - s) - j;              // j lies in [n - t, n - s), so 1 <= run and the source run ends at t <= n
    return b + s + (t - 1 - m);
}

// ---- substring_index
RDF_U8P_HD bool utf8_bytes_at(const uint8_t* p, const uint8_t* d, int64_t m) {   // p[0 .. m) == d[0 .. m); the caller keeps p + m inside the row
    for (int64_t i = 0; i < m; ++i)
        if (p[i] != d[i]) return false;
    return true;
}
// the leftmost occurrence of d[0 .. m) (m > 0) that starts in [from, e - m]; nullptr: none
RDF_U8P_HD const uint8_t* utf8_find_forward(const uint8_t* from, const uint8_t* e, const uint8_t* d, int64_t m) {
    for (const uint8_t* p = from; e - p >= m; ++p)
        if (*p == d[0] && utf8_bytes_at(p, d, m)) return p;
    return nullptr;
}
// the rightmost occurrence that starts in [b, from] (from + m <= e is the caller's); nullptr: none
RDF_U8P_HD const uint8_t* utf8_find_backward(const uint8_t* b, const uint8_t* from, const uint8_t* d, int64_t m) {
    for (int64_t i = from - b; i >= 0; --i)
        if (b[i] == d[0] && utf8_bytes_at(b + i, d, m)) return b + i;
    return nullptr;
}
// Spark's substring_index: [*s0, *s1) inside [b, e).  count > 0: everything left of the count-th occurrence from the left,
// count < 0: everything right of the |count|-th from the right; each search resumes one byte after (before) the START of
// the previous hit, so occurrences may overlap; with fewer occurrences the whole row; an empty delimiter or count 0: empty.
RDF_U8P_HD void utf8_substring_index_span(const uint8_t* b, const uint8_t* e, const uint8_t* d, int64_t m, int64_t count,
                                          const uint8_t** s0, const uint8_t** s1) {
    *s0 = b;
    *s1 = b;
    if (m <= 0 || count == 0) return;
    *s1 = e;
    if (e - b < m) return;
    if (count > 0) {
        const uint8_t* p = b;
        for (;; ++p) {
            p = utf8_find_forward(p, e, d, m);
            if (!p) return;
            if (--count == 0) { *s1 = p; return; }
        }
    }
    const uint8_t* p = e - m;
    for (;; --p) {
        p = utf8_find_backward(b, p, d, m);
        if (!p) return;
        if (++count == 0) { *s0 = p + m; return; }
        if (p == b) return;
    }
}
