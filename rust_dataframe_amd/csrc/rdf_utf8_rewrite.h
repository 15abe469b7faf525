// rdf_utf8_rewrite.h — what rdf_utf8_replace / _translate / _initcap / _split decide about ONE row (kernels:
// rdf_utf8_rewrite.hip, host side: rdf_capi_utf8_rewrite.inc; the executable model: tests/utf8_rewrite_ref.py).  ONE
// definition, __host__ __device__ inline: hipcc compiles it into the kernels, plain g++ compiles it into
// tests/cpp/test_utf8_rewrite_host.cpp.  It includes nothing of HIP.
//
// Rules kept throughout (rdf_utf8_pattern.h's): rows and literals are byte strings, nothing is validated as UTF-8, and a
// function handed (b, n) reads no byte outside [b, b + n).
//
//   hits     replace and split look for the NON-OVERLAPPING occurrences of a literal from the left: each search resumes at
//            the END of the previous hit (utf8_next_hit; substring_index resumes one byte after its START).
//   units    translate and initcap work on UNITS.  A unit begins at every byte that is not a continuation byte and runs
//            over the continuation bytes that follow it; continuation bytes at the start of a row stand alone.  A unit is
//            WELL-FORMED when its length is what its first byte announces (1: 0xxxxxxx, 2: 110xxxxx, 3: 1110xxxx,
//            4: 1111xxxx); nothing else is checked (overlong forms and surrogates are units).  A unit that is not
//            well-formed never matches, is never mapped and is copied byte for byte.  On valid UTF-8 the units are the code
//            points.  utf8_unit_at answers for ANY byte of a row by looking at most 3 bytes back and 4 ahead, so a lane of
//            a wave can decide about its byte alone.
//   emits    what one input byte contributes to the output is an Utf8Emit: up to three packed words of 0..4 bytes.  The
//            byte that begins a mapped unit emits the whole mapping and the unit's other bytes emit nothing; every byte
//            of a unit that is copied emits itself (or, in the row-at-a-time form, the first byte emits the unit).
#pragma once
#include <stdint.h>

#include "rdf_utf8_build.h"

enum : int { U8R_REPLACE = 0, U8R_TRANSLATE, U8R_INITCAP, U8R_SPLIT, U8R_NOPS };

constexpr int64_t kUtf8AllHits = INT64_MAX;

// ---- the occurrence scanner
// the start of the leftmost occurrence of d[0 .. m) that starts in [pos, n - m]; -1: none (or m <= 0).  A first-byte
// filter stands before the compare.
RDF_U8P_HD int64_t utf8_next_hit(const uint8_t* b, int64_t n, int64_t pos, const uint8_t* d, int64_t m) {
    if (m <= 0) return -1;
    const uint8_t d0 = d[0];
    for (int64_t p = pos; p + m <= n; ++p)
        if (b[p] == d0 && utf8_bytes_at(b + p, d, m)) return p;
    return -1;
}
// the non-overlapping hits of a row, at most maxhits of them
RDF_U8P_HD int64_t utf8_count_hits(const uint8_t* b, int64_t n, const uint8_t* d, int64_t m, int64_t maxhits) {
    int64_t k = 0, pos = 0;
    while (k < maxhits) {
        const int64_t h = utf8_next_hit(b, n, pos, d, m);
        if (h < 0) break;
        ++k;
        pos = h + m;
    }
    return k;
}
// split: the hits that split (limit > 0: the first limit - 1, so the last element holds the rest)
RDF_U8P_HD int64_t utf8_split_max_hits(int64_t limit) { return limit > 0 ? limit - 1 : kUtf8AllHits; }
// a row of n bytes with k hits of an m-byte literal, each replaced by r bytes (k <= n / m and r <= 1024: no overflow)
RDF_U8P_HD int64_t utf8_replace_bytes(int64_t n, int64_t k, int64_t m, int64_t r) { return utf8_build_clamp(n + k * (r - m)); }

// The row written hit by hit into out (utf8_replace_bytes of room); on_hit(j, o): hit j (from 1) has been replaced and
// element j of a split begins at output byte o.  Returns the bytes written.
template <typename HitFn>
RDF_U8P_HD int64_t utf8_replace_emit(const uint8_t* b, int64_t n, const uint8_t* d, int64_t m, const uint8_t* rep, int64_t r, int64_t maxhits,
                                     uint8_t* out, HitFn on_hit) {
    int64_t pos = 0, o = 0, k = 0;
    while (k < maxhits) {
        const int64_t h = utf8_next_hit(b, n, pos, d, m);
        if (h < 0) break;
        for (int64_t i = pos; i < h; ++i) out[o++] = b[i];
        for (int64_t i = 0; i < r; ++i) out[o++] = rep[i];
        pos = h + m;
        on_hit(++k, o);
    }
    for (int64_t i = pos; i < n; ++i) out[o++] = b[i];
    return o;
}

// ---- the same search, 64 candidate starts at a time (the wave's form: bit i of cand = an occurrence starts at base + i).
// The greedy choice from the left; *allowed (the earliest start the next hit may have = the end of the last one) and *k
// (hits so far) are carried from window to window, so literals longer than a window and self-overlapping ones work.
RDF_U8P_HD uint64_t utf8_select_hits(uint64_t cand, int64_t base, int64_t m, int64_t maxhits, int64_t* allowed, int64_t* k) {
    uint64_t sel = 0;
    while (cand && *k < maxhits) {
        const int i = __builtin_ctzll(cand);
        cand &= cand - 1;
        if (base + i < *allowed) continue;
        sel |= 1ull << i;
        *allowed = base + i + m;
        ++*k;
    }
    return sel;
}
// byte base + i of the row, given the window's chosen hits, the hits before the window (k0) and the end of the last of
// those (end0): *hits = the chosen hits that start at or before it, *covered = it lies inside one of them.  A byte that is
// not covered goes to output byte (base + i) + hits * (r - m); the hit that starts at it is hit number *hits.
RDF_U8P_HD void utf8_window_byte(uint64_t sel, int i, int64_t base, int64_t m, int64_t k0, int64_t end0, int64_t* hits, bool* covered) {
    const uint64_t below = sel & (~0ull >> (63 - i));
    *hits = k0 + __builtin_popcountll(below);
    if (below) *covered = base + i < base + (63 - __builtin_clzll(below)) + m;
    else *covered = base + i < end0;
}

// ---- units
RDF_U8P_HD int utf8_lead_len(uint32_t b0) { return b0 < 0x80 ? 1 : b0 < 0xC0 ? 0 : b0 < 0xE0 ? 2 : b0 < 0xF0 ? 3 : 4; }
// the unit that holds byte q of the row: false = it is not well-formed; else [*s, *s + *len)
RDF_U8P_HD bool utf8_unit_at(const uint8_t* b, int64_t n, int64_t q, int64_t* s, int* len) {
    int64_t t = q;
    while (t > 0 && q - t < 3 && utf8_is_cont(b[t])) --t;
    const int L = utf8_lead_len(b[t]);   // 0: no start within reach
    if (L == 0 || t + L > n || q - t >= L) return false;
    for (int i = 1; i < L; ++i)
        if (!utf8_is_cont(b[t + i])) return false;
    if (t + L < n && utf8_is_cont(b[t + L])) return false;   // the unit goes on past its announced length
    *s = t;
    *len = L;
    return true;
}
// the end of the unit that begins at pos (how literals are cut: every unit, well-formed or not)
RDF_U8P_HD int64_t utf8_unit_end(const uint8_t* b, int64_t n, int64_t pos) {
    int64_t e = pos + 1;   // (continuation bytes at the very start of a literal stand alone: the same walk)
    while (e < n && utf8_is_cont(b[e])) ++e;
    return e;
}
RDF_U8P_HD uint32_t utf8_pack(const uint8_t* p, int len) {   // len <= 4 bytes, the first one lowest
    uint32_t w = 0;
    for (int i = 0; i < len; ++i) w |= (uint32_t)p[i] << (8 * i);
    return w;
}
RDF_U8P_HD uint32_t utf8_decode_packed(uint32_t w, int len) {
    const uint32_t b0 = w & 0xFF;
    if (len == 1) return b0;
    uint32_t cp = b0 & (len == 4 ? 0x07u : len == 3 ? 0x0Fu : 0x1Fu);
    for (int i = 1; i < len; ++i) cp = (cp << 6) | ((w >> (8 * i)) & 0x3Fu);
    return cp;
}
RDF_U8P_HD uint32_t utf8_encode_packed(uint32_t cp, int* len) {
    if (cp < 0x80) { *len = 1; return cp; }
    if (cp < 0x800) { *len = 2; return (0xC0 | (cp >> 6)) | ((0x80 | (cp & 0x3F)) << 8); }
    if (cp < 0x10000) { *len = 3; return (0xE0 | (cp >> 12)) | ((0x80 | ((cp >> 6) & 0x3F)) << 8) | ((0x80 | (cp & 0x3F)) << 16); }
    *len = 4;
    return (0xF0 | ((cp >> 18) & 0x07)) | ((0x80 | ((cp >> 12) & 0x3F)) << 8) | ((0x80 | ((cp >> 6) & 0x3F)) << 16) | ((0x80 | (cp & 0x3F)) << 24);
}

// ---- emits
struct Utf8Emit { uint32_t w0, w1, w2, lens; };   // word j holds (lens >> 4 j) & 15 bytes, the first one lowest
RDF_U8P_HD int utf8_emit_len(const Utf8Emit& e) { return (int)((e.lens & 15) + ((e.lens >> 4) & 15) + ((e.lens >> 8) & 15)); }
RDF_U8P_HD uint8_t* utf8_put(uint8_t* d, uint32_t w, int len) {
    for (int i = 0; i < len; ++i) d[i] = (uint8_t)(w >> (8 * i));
    return d + len;
}
RDF_U8P_HD uint8_t* utf8_emit_put(const Utf8Emit& e, uint8_t* d) {
    d = utf8_put(d, e.w0, (int)(e.lens & 15));
    d = utf8_put(d, e.w1, (int)((e.lens >> 4) & 15));
    return utf8_put(d, e.w2, (int)((e.lens >> 8) & 15));
}

// ---- translate: the compiled table.  ASCII keys sit in a direct table, the others sorted by their packed bytes; an entry
// holds the replacement's 0..4 bytes.  Compiled once on the host, copied into LDS by the kernels.
//   matching and replace are cut into units; unit i of matching maps to unit i of replace, to nothing when replace has no
//   unit i.  The FIRST position of a unit in matching decides.  A unit of matching that is not well-formed never matches (it
//   still counts as a position); one whose replacement is longer than 4 bytes (only a unit that is not well-formed can be)
//   maps to itself.
constexpr int kUtf8TranslateWide = kUtf8PatternMax / 2;
constexpr uint8_t kUtf8NoKey = 0xFF;
struct Utf8TranslateTable {
    uint32_t ascii_val[128];
    uint32_t wide_key[kUtf8TranslateWide];
    uint32_t wide_val[kUtf8TranslateWide];
    uint8_t  ascii_len[128];                 // kUtf8NoKey: no key
    uint8_t  wide_len[kUtf8TranslateWide];
    int32_t  nwide;
};
static_assert(sizeof(Utf8TranslateTable) % 4 == 0, "copied word by word");

// the replacement of a well-formed unit (its packed bytes, its length): its length 0..4 and *val, or -1: no key
RDF_U8P_HD int utf8_translate_lookup(const Utf8TranslateTable& t, uint32_t key, int len, uint32_t* val) {
    if (len == 1) {
        const uint8_t l = t.ascii_len[key & 127];
        if (l == kUtf8NoKey) return -1;
        *val = t.ascii_val[key & 127];
        return l;
    }
    int lo = 0, hi = t.nwide;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t.wide_key[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo >= t.nwide || t.wide_key[lo] != key) return -1;
    *val = t.wide_val[lo];
    return t.wide_len[lo];
}
inline void utf8_translate_compile(const uint8_t* mt, int64_t mn, const uint8_t* rp, int64_t rn, Utf8TranslateTable* t) {
    for (int i = 0; i < 128; ++i) { t->ascii_val[i] = 0; t->ascii_len[i] = kUtf8NoKey; }
    for (int i = 0; i < kUtf8TranslateWide; ++i) { t->wide_key[i] = 0; t->wide_val[i] = 0; t->wide_len[i] = 0; }
    t->nwide = 0;
    int64_t mp = 0, rpos = 0;
    while (mp < mn) {
        const int64_t me = utf8_unit_end(mt, mn, mp);
        int64_t re = rpos;
        if (rpos < rn) re = utf8_unit_end(rp, rn, rpos);
        int64_t s = 0;
        int L = 0;
        if (utf8_unit_at(mt, mn, mp, &s, &L) && s == mp) {
            const uint32_t key = utf8_pack(mt + mp, L);
            uint32_t val = key, seen;
            int vl = L;
            if (re - rpos <= 4) { vl = (int)(re - rpos); val = utf8_pack(rp + rpos, vl); }
            if (utf8_translate_lookup(*t, key, L, &seen) < 0) {
                if (L == 1) { t->ascii_val[key] = val; t->ascii_len[key] = (uint8_t)vl; }
                else if (t->nwide < kUtf8TranslateWide) {
                    int at = t->nwide++;
                    for (; at > 0 && t->wide_key[at - 1] > key; --at) {
                        t->wide_key[at] = t->wide_key[at - 1];
                        t->wide_val[at] = t->wide_val[at - 1];
                        t->wide_len[at] = t->wide_len[at - 1];
                    }
                    t->wide_key[at] = key;
                    t->wide_val[at] = val;
                    t->wide_len[at] = (uint8_t)vl;
                }
            }
        }
        mp = me;
        rpos = re;
    }
}

// What byte q of the row emits.  whole: the row-at-a-time form, called at the first byte of every unit only: a copied unit
// is emitted whole.  *adv = the bytes to step over in that form.
RDF_U8P_HD Utf8Emit utf8_translate_emit(const uint8_t* b, int64_t n, int64_t q, const Utf8TranslateTable& t, bool whole, int* adv) {
    const uint32_t c0 = b[q];
    Utf8Emit e = {c0, 0, 0, 1};
    *adv = 1;
    if (c0 < 0x80 && (q + 1 >= n || !utf8_is_cont(b[q + 1]))) {   // ASCII, the common case: a unit of its own, looked up directly
        const uint8_t l = t.ascii_len[c0];
        if (l != kUtf8NoKey) { e.w0 = t.ascii_val[c0]; e.lens = l; }
        return e;
    }
    int64_t s = 0;
    int L = 0;
    if (!utf8_unit_at(b, n, q, &s, &L)) return e;
    const uint32_t key = utf8_pack(b + s, L);
    uint32_t val = 0;
    const int vl = utf8_translate_lookup(t, key, L, &val);
    if (q != s) {
        if (vl >= 0) e.lens = 0;
        return e;
    }
    *adv = L;
    if (vl >= 0) { e.w0 = val; e.lens = (uint32_t)vl; }
    else if (whole) { e.w0 = key; e.lens = (uint32_t)L; }
    return e;
}
// the row mapped unit by unit: the bytes of the result, written to out unless it is nullptr (the size pass)
RDF_U8P_HD int64_t utf8_translate_row(const uint8_t* b, int64_t n, const Utf8TranslateTable& t, uint8_t* out) {
    int64_t o = 0;
    for (int64_t q = 0; q < n;) {
        int adv = 1;
        const Utf8Emit e = utf8_translate_emit(b, n, q, t, true, &adv);
        if (out) utf8_emit_put(e, out + o);
        o += utf8_emit_len(e);
        q += adv;
    }
    return o;
}

#ifndef RDF_UTF8_REWRITE_NO_CASE
// ---- initcap = title_words(lower(row)).  The tables are generated for the device; plain g++ reads them as host arrays.
#if !defined(__HIPCC__) && !defined(__CUDACC__) && !defined(__device__)
#define __device__
#define RDF_U8R_DEVICE_DEFINED_HERE
#endif
#include "rdf_unicode_case.h"
#include "rdf_unicode_title.h"
#ifdef RDF_U8R_DEVICE_DEFINED_HERE
#undef __device__
#undef RDF_U8R_DEVICE_DEFINED_HERE
#endif

RDF_U8P_HD int utf8_last_le(const uint32_t* starts, int n, uint32_t c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= c) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}
// rdf_utf8_lower's mapping of one code point (context-free part): the code points written, 1..3
RDF_U8P_HD int utf8_lower_map(uint32_t c, uint32_t* m0, uint32_t* m1, uint32_t* m2) {
    *m0 = c; *m1 = 0; *m2 = 0;
    if (c < 0x80) { if (c >= 'A' && c <= 'Z') *m0 = c + 32; return 1; }
    const int i = utf8_last_le(k_lower_start, RDF_CASE_LOWER_RUNS, c);
    if (i < 0) return 1;
    const uint32_t inf = k_lower_info[i], d = c - k_lower_start[i];
    const uint32_t stride = (inf & RDF_CASE_FLAG_STRIDE2) ? 2u : 1u;
    if (d % stride != 0 || d / stride >= (inf & RDF_CASE_COUNT_MASK)) return 1;
    if (inf & RDF_CASE_FLAG_MULTI) {
        const uint32_t* e = k_lower_multi + 4 * k_lower_delta[i];
        *m0 = e[1]; *m1 = e[2]; *m2 = e[3];
        return (int)e[0];
    }
    *m0 = (uint32_t)((int32_t)c + k_lower_delta[i]);
    return 1;
}
// the upper mapping where it is one code point, else c
RDF_U8P_HD uint32_t utf8_upper_single(uint32_t c) {
    if (c < 0x80) return (c >= 'a' && c <= 'z') ? c - 32 : c;
    const int i = utf8_last_le(k_upper_start, RDF_CASE_UPPER_RUNS, c);
    if (i < 0) return c;
    const uint32_t inf = k_upper_info[i], d = c - k_upper_start[i];
    const uint32_t stride = (inf & RDF_CASE_FLAG_STRIDE2) ? 2u : 1u;
    if (d % stride != 0 || d / stride >= (inf & RDF_CASE_COUNT_MASK) || (inf & RDF_CASE_FLAG_MULTI)) return c;
    return (uint32_t)((int32_t)c + k_upper_delta[i]);
}
// the simple title mapping: t = c.title(); t if it is one code point, else c.  Stored as the exceptions to utf8_upper_single
RDF_U8P_HD uint32_t utf8_title_simple(uint32_t c) {
    if (c < 0x80) return (c >= 'a' && c <= 'z') ? c - 32 : c;
    const int i = utf8_last_le(k_title_exc_cp, RDF_TITLE_EXCEPTIONS, c);
    if (i >= 0 && k_title_exc_cp[i] == c) return k_title_exc_to[i];
    return utf8_upper_single(c);
}
RDF_U8P_HD bool utf8_in_ranges(const uint32_t* lo, const uint32_t* hi, int n, uint32_t c) {
    const int i = utf8_last_le(lo, n, c);
    return i >= 0 && c <= hi[i];
}
// A word begins at the first byte of the row and after every byte 0x20 (UTF8String.toTitleCase); no other white space does
RDF_U8P_HD bool utf8_word_start(const uint8_t* b, int64_t s) { return s == 0 || b[s - 1] == 0x20; }
// Final_Sigma for the sigma whose unit is [s, s + slen): a cased letter before it and none after it, case-ignorable ones
// skipped; a byte outside a well-formed unit is neither
RDF_U8P_HD bool utf8_final_sigma(const uint8_t* b, int64_t n, int64_t s, int slen) {
    bool before = false;
    int64_t q = s, us = 0;
    int L = 0;
    while (q > 0) {
        if (!utf8_unit_at(b, n, q - 1, &us, &L)) break;
        const uint32_t c = utf8_decode_packed(utf8_pack(b + us, L), L);
        q = us;
        if (utf8_in_ranges(k_case_ignorable_lo, k_case_ignorable_hi, RDF_CASE_IGNORABLE_RANGES, c)) continue;
        before = utf8_in_ranges(k_cased_lo, k_cased_hi, RDF_CASED_RANGES, c);
        break;
    }
    if (!before) return false;
    for (int64_t p = s + slen; p < n; p += L) {
        if (!utf8_unit_at(b, n, p, &us, &L)) return true;
        const uint32_t c = utf8_decode_packed(utf8_pack(b + us, L), L);
        if (utf8_in_ranges(k_case_ignorable_lo, k_case_ignorable_hi, RDF_CASE_IGNORABLE_RANGES, c)) continue;
        return !utf8_in_ranges(k_cased_lo, k_cased_hi, RDF_CASED_RANGES, c);
    }
    return true;
}
// What byte q of the row emits (whole / *adv as for translate).  A unit whose mapping is itself is copied.
RDF_U8P_HD Utf8Emit utf8_initcap_emit(const uint8_t* b, int64_t n, int64_t q, bool whole, int* adv) {
    const uint32_t c0 = b[q];
    Utf8Emit e = {c0, 0, 0, 1};
    *adv = 1;
    if (c0 < 0x80 && (q + 1 >= n || !utf8_is_cont(b[q + 1]))) {   // ASCII, the common case
        const uint32_t l = (c0 >= 'A' && c0 <= 'Z') ? c0 + 32 : c0;
        e.w0 = (utf8_word_start(b, q) && l >= 'a' && l <= 'z') ? l - 32 : l;
        return e;
    }
    int64_t s = 0;
    int L = 0;
    if (!utf8_unit_at(b, n, q, &s, &L)) return e;
    const uint32_t key = utf8_pack(b + s, L), cp = utf8_decode_packed(key, L);
    uint32_t m0 = cp, m1 = 0, m2 = 0;
    int k = 1;
    const bool ws = utf8_word_start(b, s);
    if (cp == 0x3A3) {   // both lower forms of the sigma have it as their title: it stays at a word's start, and changes anywhere else
        if (!ws && q != s) { e.lens = 0; return e; }   // (no context needed to know that)
        if (!ws) m0 = utf8_final_sigma(b, n, s, L) ? 0x3C2u : 0x3C3u;
    } else {
        k = utf8_lower_map(cp, &m0, &m1, &m2);
        if (ws) m0 = utf8_title_simple(m0);
    }
    const bool changed = !(k == 1 && m0 == cp);
    if (q != s) {
        if (changed) e.lens = 0;
        return e;
    }
    *adv = L;
    if (changed) {
        int l0 = 0, l1 = 0, l2 = 0;
        e.w0 = utf8_encode_packed(m0, &l0);
        if (k > 1) e.w1 = utf8_encode_packed(m1, &l1);
        if (k > 2) e.w2 = utf8_encode_packed(m2, &l2);
        e.lens = (uint32_t)(l0 | (l1 << 4) | (l2 << 8));
    } else if (whole) { e.w0 = key; e.lens = (uint32_t)L; }
    return e;
}
RDF_U8P_HD int64_t utf8_initcap_row(const uint8_t* b, int64_t n, uint8_t* out) {
    int64_t o = 0;
    for (int64_t q = 0; q < n;) {
        int adv = 1;
        const Utf8Emit e = utf8_initcap_emit(b, n, q, true, &adv);
        if (out) utf8_emit_put(e, out + o);
        o += utf8_emit_len(e);
        q += adv;
    }
    return o;
}
#endif   // RDF_UTF8_REWRITE_NO_CASE
