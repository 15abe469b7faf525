// rdf_utf8_pattern.h — what rdf_utf8_predicate / rdf_utf8_compare / rdf_utf8_measure decide about ONE row (kernels:
// rdf_utf8_pred.hip, host side: rdf_capi_utf8_pred.inc).  ONE definition, __host__ __device__ inline: hipcc compiles it into
// the kernels' lane-per-row path, plain g++ compiles it into tests/cpp/test_utf8_pattern_host.cpp.  It includes nothing of HIP.
//
// Rules kept throughout:
//   bytes       rows and patterns are byte strings; nothing is validated as UTF-8.  A code point begins at a byte that is
//               not a continuation byte (10xxxxxx), as rdf_utf8_substring counts them
//   bounds      a function handed [b, e) reads no byte outside it: 8-byte loads (utf8_load8) are issued only when all 8
//               bytes lie inside, the rest is read byte by byte.  Any alignment
//   order       unsigned byte order (memcmp), then the shorter string first: rdf_lexsort_to_indices' order
//
// LIKE.  utf8_pattern_compile removes the escapes and cuts the pattern at its unescaped '%' into segments; a segment is a run
// of ITEMS, each a literal byte or an any-one-code-point mark ('_').  Segment 0 is the head (what stands before the first
// '%'), the last segment the tail (after the last '%'); either may be empty; the segments between them are never empty
// (adjacent '%' collapse).  Every segment matches a fixed number of code points, so the greedy placement is exact:
// the head at the row's start, the tail ending at the row's end (its start found by walking back its code points), every
// inner segment at its leftmost place in what is left (leftmost start = leftmost end).  Patterns without '_' whose shape
// is a plain literal, lit%, %lit, %lit% or only '%' are reclassified as EQ, STARTS_WITH, ENDS_WITH, CONTAINS, NOT_NULL.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RDF_U8P_HD __host__ __device__ inline
#else
#define RDF_U8P_HD inline
#endif

// rdf_utf8_pred_op / rdf_utf8_measure_op of include/rdf_mi355x.h, restated so that this header stands alone
// (rdf_capi_utf8_pred.inc static_asserts that they agree); U8P_NOT_NULL exists only as a compiled kind
enum : int { U8P_EQ = 0, U8P_NE, U8P_LT, U8P_LE, U8P_GT, U8P_GE, U8P_STARTS_WITH, U8P_ENDS_WITH, U8P_CONTAINS, U8P_LIKE, U8P_NOPS, U8P_NOT_NULL = U8P_NOPS };
enum : int { U8M_LENGTH = 0, U8M_OCTET_LENGTH = 1, U8M_LOCATE = 2, U8M_NOPS };
enum : int { U8P_OK = 0, U8P_BAD_OP, U8P_BAD_LENGTH, U8P_BAD_ESCAPE, U8P_LONE_ESCAPE, U8P_TOO_MANY_SEGMENTS };

constexpr int kUtf8PatternMax = 1024;    // bytes of a literal / pattern
constexpr int kUtf8PatternSegs = 32;     // non-empty segments of a LIKE pattern

struct Utf8Pattern {
    int32_t  kind;             // U8P_*: what to run (LIKE patterns may be reclassified)
    int32_t  nitems;           // items = bytes of lit in use
    int32_t  nseg;             // stored segments: 1 without '%', else head + inner ones + tail
    int32_t  has_percent;
    int32_t  anchored_head;    // the head / tail segment is not empty
    int32_t  anchored_tail;
    uint16_t seg_begin[kUtf8PatternSegs + 3];   // segment s = items [seg_begin[s], seg_begin[s + 1])
    uint16_t seg_cp[kUtf8PatternSegs + 2];      // code points segment s matches
    uint32_t any[kUtf8PatternMax / 32];         // bit k: item k is an any-one-code-point mark
    uint8_t  lit[kUtf8PatternMax + 8];          // item k's byte (0 for a mark); 8 spare bytes: word reads of the literal stay inside
};
static_assert(sizeof(Utf8Pattern) % 4 == 0, "copied word by word");

RDF_U8P_HD bool utf8_is_cont(uint8_t c) { return (c & 0xC0) == 0x80; }
RDF_U8P_HD uint64_t utf8_load8(const uint8_t* p) {
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return w;
}
RDF_U8P_HD bool utf8_item_any(const Utf8Pattern& pt, int k) { return (pt.any[k >> 5] >> (k & 31)) & 1u; }

// memcmp order, then by length: < 0, 0, > 0
RDF_U8P_HD int utf8_compare_bytes(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb) {
    const int64_t n = na < nb ? na : nb;
    int64_t i = 0;
    for (; i + 8 <= n; i += 8) {
        const uint64_t wa = utf8_load8(a + i), wb = utf8_load8(b + i);
        if (wa != wb) return __builtin_bswap64(wa) < __builtin_bswap64(wb) ? -1 : 1;   // (little-endian loads: the first byte is the lowest)
    }
    for (; i < n; ++i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return na < nb ? -1 : (na > nb ? 1 : 0);
}
RDF_U8P_HD bool utf8_compare_result(int op, int c) {
    switch (op) {
        case U8P_EQ: return c == 0;
        case U8P_NE: return c != 0;
        case U8P_LT: return c < 0;
        case U8P_LE: return c <= 0;
        case U8P_GT: return c > 0;
        default:     return c >= 0;
    }
}

// code points of n bytes: the bytes that are not continuation bytes.  Word-wise: a continuation byte has bit 7 set and
// bit 6 clear
RDF_U8P_HD int utf8_word_starts(uint64_t w) {
    const uint64_t cont = w & ~(w << 1) & 0x8080808080808080ull;
    return 8 - __builtin_popcountll(cont);
}
RDF_U8P_HD int64_t utf8_count_code_points(const uint8_t* p, int64_t n) {
    int64_t c = 0, i = 0;
    for (; i + 8 <= n; i += 8) c += utf8_word_starts(utf8_load8(p + i));
    for (; i < n; ++i) c += !utf8_is_cont(p[i]);
    return c;
}
// *out = the start of code point number k (from 0) of [b, e); k == the row's code points gives e; false: the row has fewer
RDF_U8P_HD bool utf8_skip_code_points(const uint8_t* b, const uint8_t* e, int64_t k, const uint8_t** out) {
    const uint8_t* p = b;
    for (; k > 0; --k) {
        if (p >= e) return false;
        ++p;
        while (p < e && utf8_is_cont(*p)) ++p;
    }
    *out = p;
    return true;
}

// segment s matched at p, not beyond e: *end = where the match ends.  (A flag, not a null pointer: an empty row of a chunk
// without data bytes is [nullptr, nullptr).)
RDF_U8P_HD bool utf8_match_at(const Utf8Pattern& pt, int s, const uint8_t* p, const uint8_t* e, const uint8_t** end) {
    const int k1 = pt.seg_begin[s + 1];
    for (int k = pt.seg_begin[s]; k < k1; ++k) {
        if (p >= e) return false;
        if (utf8_item_any(pt, k)) {
            ++p;
            while (p < e && utf8_is_cont(*p)) ++p;
        } else {
            if (*p != pt.lit[k]) return false;
            ++p;
        }
    }
    *end = p;
    return true;
}
// can segment s start at p (p < e)?  the cheap test before utf8_match_at: its first byte, or a code point's start for a mark
RDF_U8P_HD bool utf8_may_start(const Utf8Pattern& pt, int k0, const uint8_t* p) {
    return utf8_item_any(pt, k0) ? !utf8_is_cont(*p) : *p == pt.lit[k0];
}
// the leftmost match of segment s inside [from, e)
RDF_U8P_HD bool utf8_find(const Utf8Pattern& pt, int s, const uint8_t* from, const uint8_t* e, const uint8_t** start, const uint8_t** end) {
    const int k0 = pt.seg_begin[s], n = pt.seg_begin[s + 1] - k0;
    if (n == 0) { *start = from; *end = from; return true; }
    for (const uint8_t* p = from; e - p >= n; ++p) {
        if (!utf8_may_start(pt, k0, p)) continue;
        if (utf8_match_at(pt, s, p, e, end)) { *start = p; return true; }
    }
    return false;
}
// LIKE, the two anchored ends: the head matched at b and the tail ending exactly at e leave [*p, *q) to the inner segments
RDF_U8P_HD bool utf8_like_ends(const Utf8Pattern& pt, const uint8_t* b, const uint8_t* e, const uint8_t** p_out, const uint8_t** q_out) {
    const uint8_t* p = b;
    if (!utf8_match_at(pt, 0, b, e, &p)) return false;
    const uint8_t* q = e;
    if (!pt.has_percent) {
        if (p != e) return false;
    } else {
        const int tail = pt.nseg - 1;
        for (int i = 0; i < (int)pt.seg_cp[tail]; ++i) {   // the tail's start: its code points back from e, not into the head
            if (q <= p) return false;
            --q;
            while (q > p && utf8_is_cont(*q)) --q;
        }
        const uint8_t* t = q;
        if (!utf8_match_at(pt, tail, q, e, &t) || t != e) return false;
    }
    *p_out = p;
    *q_out = q;
    return true;
}
RDF_U8P_HD bool utf8_like(const Utf8Pattern& pt, const uint8_t* b, const uint8_t* e) {
    const uint8_t *p = b, *q = e;
    if (!utf8_like_ends(pt, b, e, &p, &q)) return false;
    for (int s = 1; s + 1 < pt.nseg; ++s) {
        const uint8_t* st = p;
        if (!utf8_find(pt, s, p, q, &st, &p)) return false;
    }
    return true;
}

// one row of rdf_utf8_predicate under a compiled pattern
RDF_U8P_HD bool utf8_predicate_row(const Utf8Pattern& pt, const uint8_t* b, const uint8_t* e) {
    const int64_t n = e - b, m = pt.nitems;
    switch (pt.kind) {
        case U8P_EQ: return n == m && utf8_compare_bytes(b, n, pt.lit, m) == 0;   // (a row of another length reads no byte)
        case U8P_NE: return !(n == m && utf8_compare_bytes(b, n, pt.lit, m) == 0);
        case U8P_LT: case U8P_LE: case U8P_GT: case U8P_GE: return utf8_compare_result(pt.kind, utf8_compare_bytes(b, n, pt.lit, m));
        case U8P_STARTS_WITH: return n >= m && utf8_compare_bytes(b, m, pt.lit, m) == 0;
        case U8P_ENDS_WITH: return n >= m && utf8_compare_bytes(e - m, m, pt.lit, m) == 0;
        case U8P_CONTAINS: { const uint8_t *st = b, *en = b; return utf8_find(pt, 0, b, e, &st, &en); }
        case U8P_NOT_NULL: return true;
        default: return utf8_like(pt, b, e);
    }
}
// LOCATE: the 1-based code-point position of the first occurrence of the literal (segment 0) at or after code-point
// position pos; 0 if there is none or pos < 1.  Python's s.find(sub, pos - 1) + 1, the empty needle included
RDF_U8P_HD int32_t utf8_locate_row(const Utf8Pattern& pt, const uint8_t* b, const uint8_t* e, int32_t pos) {
    if (pos < 1) return 0;
    const uint8_t* s = b;
    if (!utf8_skip_code_points(b, e, (int64_t)pos - 1, &s)) return 0;
    if (pt.nitems == 0) return pos;
    const uint8_t *st = s, *en = s;
    if (!utf8_find(pt, 0, s, e, &st, &en)) return 0;
    return (int32_t)(pos + utf8_count_code_points(s, st - s));
}

// ---- the compiler (host only)
// op: U8P_EQ .. U8P_LIKE.  Every op but LIKE takes the n bytes as they are (one segment; LOCATE compiles its needle as
// U8P_CONTAINS).  escape: -1, or one ASCII byte 1..127 other than '%' and '_' (checked for every op, used by LIKE).
// classify = false keeps every LIKE pattern with the general matcher (the host test runs each pattern both ways).
inline int utf8_pattern_compile(int op, const uint8_t* pat, int64_t n, int escape, Utf8Pattern* out, bool classify = true) {
    __builtin_memset(out, 0, sizeof *out);
    if (op < U8P_EQ || op >= U8P_NOPS) return U8P_BAD_OP;
    if (n < 0 || n > kUtf8PatternMax) return U8P_BAD_LENGTH;
    if (escape != -1 && (escape < 1 || escape > 127 || escape == '%' || escape == '_')) return U8P_BAD_ESCAPE;
    out->kind = op;
    if (op != U8P_LIKE) {
        for (int64_t i = 0; i < n; ++i) out->lit[i] = pat[i];
        out->nitems = (int32_t)n;
        out->nseg = 1;
        out->seg_begin[1] = (uint16_t)n;
        out->seg_cp[0] = (uint16_t)utf8_count_code_points(out->lit, n);
        out->anchored_head = out->anchored_tail = 1;
        return U8P_OK;
    }
    // items, and the item index of every unescaped '%'
    uint16_t cut[kUtf8PatternMax + 1];
    int ncut = 0, k = 0, nany = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t c = pat[i];
        if (escape >= 0 && c == (uint8_t)escape) {
            if (i + 1 >= n) return U8P_LONE_ESCAPE;
            out->lit[k++] = pat[++i];
        } else if (c == '%') {
            cut[ncut++] = (uint16_t)k;
        } else if (c == '_') {
            out->any[k >> 5] |= 1u << (k & 31);
            ++k;
            ++nany;
        } else {
            out->lit[k++] = c;
        }
    }
    out->nitems = k;
    out->has_percent = ncut > 0;
    // pieces: [0, cut[0]) [cut[0], cut[1]) .. [cut[ncut - 1], k); the head and the tail are stored even when empty
    int nseg = 0, nonempty = 0, inner = 0;
    auto push = [&](int begin, int end) {
        out->seg_begin[nseg] = (uint16_t)begin;
        out->seg_begin[nseg + 1] = (uint16_t)end;
        int cps = 0;
        for (int j = begin; j < end; ++j) cps += utf8_item_any(*out, j) || !utf8_is_cont(out->lit[j]);
        out->seg_cp[nseg++] = (uint16_t)cps;
    };
    for (int i = 0; i <= ncut; ++i) {
        const int begin = i == 0 ? 0 : cut[i - 1], end = i == ncut ? k : cut[i];
        const bool is_end = i == 0 || i == ncut;
        if (end > begin) {
            if (++nonempty > kUtf8PatternSegs) return U8P_TOO_MANY_SEGMENTS;
            if (!is_end) ++inner;
        } else if (!is_end) {
            continue;
        }
        push(begin, end);
    }
    out->nseg = nseg;
    out->anchored_head = out->seg_begin[1] > 0;
    out->anchored_tail = out->has_percent ? out->seg_begin[nseg] > out->seg_begin[nseg - 1] : 1;
    if (nany == 0 && classify) {   // the shapes that need no LIKE
        const int kind = !out->has_percent ? U8P_EQ
                       : k == 0 ? U8P_NOT_NULL
                       : inner == 0 && out->anchored_head && !out->anchored_tail ? U8P_STARTS_WITH
                       : inner == 0 && !out->anchored_head && out->anchored_tail ? U8P_ENDS_WITH
                       : inner == 1 && !out->anchored_head && !out->anchored_tail ? U8P_CONTAINS
                       : U8P_LIKE;
        if (kind != U8P_LIKE) {   // one segment: the literal
            out->kind = kind;
            const int cps = (int)utf8_count_code_points(out->lit, k);
            __builtin_memset(out->seg_begin, 0, sizeof out->seg_begin);
            __builtin_memset(out->seg_cp, 0, sizeof out->seg_cp);
            out->nseg = 1;
            out->seg_begin[1] = (uint16_t)k;
            out->seg_cp[0] = (uint16_t)cps;
        }
    }
    return U8P_OK;
}
