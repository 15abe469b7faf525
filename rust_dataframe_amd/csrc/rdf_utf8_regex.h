// rdf_utf8_regex.h — regular expressions over ONE Utf8 row: rdf_utf8_regexp_match / _count / _extract / _replace / _split
// (kernels: rdf_utf8_regex.hip, host side: rdf_capi_utf8_regex.inc; the executable model: tests/utf8_regex_ref.py).  ONE
// definition: hipcc compiles the stepping half into the kernels, plain g++ compiles both halves into
// tests/cpp/test_utf8_regex_host.cpp.  It includes nothing of HIP.
//
// The rules are Spark 3's, that is java.util.regex: leftmost-FIRST matching.  tests/utf8_regex_ref.py states what is accepted
// and what is refused; the parser here follows the model's rule for rule and reports the same construct at the same byte.
// ONE KNOWN DIFFERENCE FROM SPARK: `$` is Java's \z.  Java's `$` also matches before a final line terminator.
// Three constructs are refused beyond the documented list because their Java meaning is not certain: a quantifier on a
// quantifier, a quantifier on an anchor, and a quantifier that may repeat more than once over an operand that can match empty.
//
//   compile (host only)
//     parser     -> a syntax tree of sets of code points, concatenations, alternations, repetitions and the two anchors.
//                   (?i) folds ASCII letters into the sets; (?s) decides what `.` is.
//     program    -> a Thompson program: BYTE lo..hi, SPLIT x y (x has priority), BOL, EOL, MATCH.  A set expands to the UTF-8
//                   byte-range sequences of its code points (RFC 3629: no overlong forms, no surrogates), so a consuming
//                   element matches whole well-formed sequences and nothing else.  It is built twice, forward and REVERSED.
//     two DFAs   -> ordered subset construction.  A DFA state is the ordered list of program counters BEFORE their closure;
//                   the closure is taken when the next input class is known, so an anchor is decided by the class that
//                   follows it and "matching" is known one symbol late: a state is FLAGGED when a MATCH was reached before
//                   the symbol that led to it.  Two input classes beyond the byte classes stand for the row's start and end.
//       forward    an implicit lowest-priority prefix thread starts the pattern at every byte that is not a continuation
//                  byte and at the row's end (earlier starts win), and the threads behind a MATCH are dropped (leftmost-
//                  first).  The last flagged position is where the leftmost-first match ENDS.  Two start states: at byte 0,
//                  where ^ holds, and anywhere else.
//       reverse    over the reversed program, anchored at that end, no prefix, nothing dropped: the last flagged position is
//                  the LONGEST reverse match, the smallest s with [s, e) in the language.  The leftmost-first match starts
//                  at the smallest s for which any match exists, and [s, e) is one: the two are the same s.  The walk stops
//                  at the search's resume point.  Two start states: at the row's end, where $ holds, and anywhere else; the
//                  row-start class makes ^ hold, the row-end class only flushes the late flag.
//     tables     -> a 256-byte class map and 16-bit entries [state][class]; state 0 is dead; the flagged states have the
//                   highest numbers, so "matching" is one compare.
//   caps         kUtf8RegexMaxAtoms / MaxProgram / MaxStates / MaxTableBytes.  A pattern past a cap is refused with the
//                count in the message.  Tables of up to kUtf8RegexLdsBytes are walked out of LDS, larger ones in HBM.
//   stepping (__host__ __device__)
//     utf8_regex_any / utf8_regex_find and the row functions of the five operations.  A walk is linear in the bytes it
//     reads: two dependent look-ups a byte, its class in the map and then the entry [state][class].  Row bytes are read 8 at a time where the address allows.  Nothing reads outside
//     [b, b + n).  After a match the forward walk restarts at its end, so a pattern whose higher-priority threads run far
//     beyond each match (a(?:.*z)?) reads those bytes once per match; that is RE2's arrangement and its cost.
#pragma once
#include <stdint.h>

#include "rdf_utf8_rewrite.h"

enum : int { U8X_MATCH = 0, U8X_COUNT, U8X_EXTRACT, U8X_REPLACE, U8X_SPLIT, U8X_NOPS };

constexpr int kUtf8RegexMaxAtoms = 1000;          // leaves of the tree once counted repetitions are expanded
constexpr int kUtf8RegexMaxCount = 1000;          // the largest n or m of {n,m}
constexpr int kUtf8RegexMaxProgram = 4096;        // instructions of one program
constexpr int kUtf8RegexMaxStates = 2048;         // states of one DFA
constexpr int kUtf8RegexLdsBytes = 32 * 1024;     // class map + both tables: walked out of LDS up to here
constexpr int kUtf8RegexMaxTableBytes = 256 * 1024;   // ... and out of HBM up to here
constexpr int kUtf8RegexHeaderBytes = 64;

// the compiled pattern as the kernels get it: this header, the class map (256 bytes), the forward table, the reverse table
struct Utf8RegexHeader {
    int32_t classes;                       // byte classes + 2: class classes - 2 is the row's start, classes - 1 its end
    int32_t fwd_states, rev_states;
    int32_t fwd_flagged, rev_flagged;      // states >= this are flagged
    int32_t fwd_start0, fwd_start;         // the search begins at byte 0 / elsewhere
    int32_t rev_start_end, rev_start;      // the match ends at the row's end / elsewhere
    int32_t can_match_empty, anchored_start;
    int32_t program_len;
    int32_t table_bytes;                   // of the whole image, this header included
    int32_t pad[3];
};
static_assert(sizeof(Utf8RegexHeader) == kUtf8RegexHeaderBytes, "the image's layout");

struct Utf8RegexView {   // pointers into an image, in LDS or HBM
    const uint8_t* cls;
    const uint16_t* fwd;
    const uint16_t* rev;
    int32_t nc, fwd_flagged, rev_flagged, fwd_start0, fwd_start, rev_start_end, rev_start;
};
RDF_U8P_HD Utf8RegexView utf8_regex_view(const Utf8RegexHeader& h, const uint8_t* image) {
    Utf8RegexView v;
    v.cls = image + kUtf8RegexHeaderBytes;
    v.fwd = (const uint16_t*)(image + kUtf8RegexHeaderBytes + 256);
    v.rev = v.fwd + (int64_t)h.fwd_states * h.classes;
    v.nc = h.classes;
    v.fwd_flagged = h.fwd_flagged; v.rev_flagged = h.rev_flagged;
    v.fwd_start0 = h.fwd_start0; v.fwd_start = h.fwd_start;
    v.rev_start_end = h.rev_start_end; v.rev_start = h.rev_start;
    return v;
}

// ---- stepping
RDF_U8P_HD bool utf8_regex_aligned8(const uint8_t* p) { return ((uintptr_t)p & 7) == 0; }
RDF_U8P_HD uint64_t utf8_regex_load8(const uint8_t* p) {   // p is 8-byte aligned and p + 8 lies inside the row
    uint64_t w;
    __builtin_memcpy(&w, __builtin_assume_aligned(p, 8), 8);
    return w;
}

// The forward walk from byte `from`.  FIRST: stop at the first flagged state (rlike).  Returns the end of the leftmost-first
// match that begins at or after `from` (FIRST: the position where some match was seen to end), or -1.
template <bool FIRST>
RDF_U8P_HD int64_t utf8_regex_forward(const Utf8RegexView& v, const uint8_t* b, int64_t n, int64_t from) {
    uint32_t st = from == 0 ? (uint32_t)v.fwd_start0 : (uint32_t)v.fwd_start;
    const uint32_t nc = (uint32_t)v.nc, flagged = (uint32_t)v.fwd_flagged;
    int64_t end = -1, q = from;
    while (q < n && st != 0) {
        if (q + 8 <= n && utf8_regex_aligned8(b + q)) {
            uint64_t w = utf8_regex_load8(b + q);
            for (int k = 0; k < 8 && st != 0; ++k, ++q, w >>= 8) {
                st = v.fwd[st * nc + v.cls[w & 0xFF]];
                if (st >= flagged) { end = q; if (FIRST) return end; }
            }
        } else {
            st = v.fwd[st * nc + v.cls[b[q]]];
            if (st >= flagged) { end = q; if (FIRST) return end; }
            ++q;
        }
    }
    if (st != 0 && v.fwd[st * nc + nc - 1] >= flagged) end = n;   // (st != 0: the walk reached the row's end)
    return end;
}
// The reverse walk from the match's end e down to `from`: where the match starts.
RDF_U8P_HD int64_t utf8_regex_backward(const Utf8RegexView& v, const uint8_t* b, int64_t n, int64_t from, int64_t e) {
    uint32_t st = e == n ? (uint32_t)v.rev_start_end : (uint32_t)v.rev_start;
    const uint32_t nc = (uint32_t)v.nc, flagged = (uint32_t)v.rev_flagged;
    int64_t start = e, q = e;
    while (q > from && st != 0) {
        if (q - 8 >= from && utf8_regex_aligned8(b + q)) {
            const uint64_t w = utf8_regex_load8(b + q - 8);
            for (int k = 7; k >= 0 && st != 0; --k) {
                st = v.rev[st * nc + v.cls[(w >> (8 * k)) & 0xFF]];
                if (st >= flagged) start = q;
                --q;
            }
        } else {
            --q;
            st = v.rev[st * nc + v.cls[b[q]]];
            if (st >= flagged) start = q + 1;
        }
    }
    if (st != 0 && v.rev[st * nc + (q == 0 ? nc - 2 : nc - 1)] >= flagged) start = q;   // (st != 0: q == from)
    return start;
}
// rlike: a match exists anywhere in the row
RDF_U8P_HD bool utf8_regex_any(const Utf8RegexView& v, const uint8_t* b, int64_t n) { return utf8_regex_forward<true>(v, b, n, 0) >= 0; }
// Matcher.find from byte `from` (<= n): the leftmost-first match [*s, *e) that begins at or after it
RDF_U8P_HD bool utf8_regex_find(const Utf8RegexView& v, const uint8_t* b, int64_t n, int64_t from, int64_t* s, int64_t* e) {
    const int64_t end = utf8_regex_forward<false>(v, b, n, from);
    if (end < 0) return false;
    *e = end;
    *s = utf8_regex_backward(v, b, n, from, end);
    return true;
}
// where the search after the match [s, e) resumes (the prefix thread skips the starts that are not allowed); > n: stop
RDF_U8P_HD int64_t utf8_regex_resume(int64_t s, int64_t e) { return e > s ? e : e + 1; }
RDF_U8P_HD int64_t utf8_regex_split_max_hits(int64_t limit) { return limit > 0 ? limit - 1 : kUtf8AllHits; }

RDF_U8P_HD int64_t utf8_regex_count(const Utf8RegexView& v, const uint8_t* b, int64_t n) {
    int64_t k = 0, from = 0, s = 0, e = 0;
    while (from <= n && utf8_regex_find(v, b, n, from, &s, &e)) {
        ++k;
        from = utf8_regex_resume(s, e);
    }
    return k;
}
// One row of extract / replace / split: the bytes of the result (replace: n - sum |hit| + k r; extract: |first hit|; split:
// n - sum |splitting hits|), clamped by the caller; written to out unless it is nullptr (the size pass).  *elems: split's
// elements; on_hit(j, o): element j (from 1) of a split begins at output byte o.  split: a zero-width match at byte 0 never
// splits and only the first maxhits hits do.
template <typename HitFn>
RDF_U8P_HD int64_t utf8_regex_row(const Utf8RegexView& v, int op, const uint8_t* b, int64_t n, const uint8_t* rep, int64_t r, int64_t maxhits,
                                  uint8_t* out, int64_t* elems, HitFn on_hit) {
    int64_t s = 0, e = 0, o = 0, pos = 0, from = 0, k = 0;
    *elems = 1;
    if (op == U8X_EXTRACT) {
        if (!utf8_regex_find(v, b, n, 0, &s, &e)) return 0;
        if (out)
            for (int64_t i = s; i < e; ++i) out[i - s] = b[i];
        return e - s;
    }
    while (from <= n && k < maxhits && utf8_regex_find(v, b, n, from, &s, &e)) {
        from = utf8_regex_resume(s, e);
        if (op == U8X_SPLIT && e == 0) continue;
        if (out) {
            for (int64_t i = pos; i < s; ++i) out[o + i - pos] = b[i];
            for (int64_t i = 0; i < r; ++i) out[o + (s - pos) + i] = rep[i];
        }
        o += (s - pos) + r;
        pos = e;
        on_hit(++k, o);
    }
    if (out)
        for (int64_t i = pos; i < n; ++i) out[o + i - pos] = b[i];
    *elems = k + 1;
    return o + (n - pos);
}

// the bytes a replacement stands for: \x is x.  Returns -1, or the position of a trailing backslash / an unescaped $
// (*dollar says which).  out has room for rn bytes.
inline int64_t utf8_regex_replacement(const uint8_t* rp, int64_t rn, uint8_t* out, int64_t* out_bytes, bool* dollar) {
    int64_t o = 0;
    *dollar = false;
    for (int64_t i = 0; i < rn; ++i) {
        if (rp[i] == '\\') {
            if (i + 1 >= rn) return i;
            out[o++] = rp[++i];
        } else if (rp[i] == '$') {
            *dollar = true;
            return i;
        } else out[o++] = rp[i];
    }
    *out_bytes = o;
    return -1;
}

#ifndef RDF_UTF8_REGEX_NO_COMPILER
// ================================================================ the compiler (host only)
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

enum : int { U8X_OK = 0, U8X_SYNTAX = 1, U8X_CAP = 2 };

struct Utf8RegexCompiled {
    int status = U8X_OK;
    std::string what;            // the construct refused, or the cap passed (with the count)
    int64_t pos = 0;             // its byte in the pattern
    std::vector<uint8_t> image;  // header, class map, tables
    Utf8RegexHeader h;
};

namespace utf8_regex_detail {

struct Range { uint32_t lo, hi; };
typedef std::vector<Range> Set;
constexpr uint32_t kCpMax = 0x10FFFF;

inline Set norm(Set s) {
    std::sort(s.begin(), s.end(), [](const Range& a, const Range& b) { return a.lo < b.lo || (a.lo == b.lo && a.hi < b.hi); });
    Set out;
    for (const Range& r : s) {
        if (!out.empty() && r.lo <= out.back().hi + 1) out.back().hi = std::max(out.back().hi, r.hi);
        else out.push_back(r);
    }
    return out;
}
inline Set negate(const Set& in) {
    Set out;
    uint32_t at = 0;
    for (const Range& r : norm(in)) {
        if (r.lo > at) out.push_back({at, r.lo - 1});
        at = r.hi + 1;
    }
    if (at <= kCpMax) out.push_back({at, kCpMax});
    return out;
}
inline Set fold(const Set& in) {
    Set out = in;
    for (const Range& r : in) {
        const uint32_t ab[2][2] = {{0x41, 0x5A}, {0x61, 0x7A}};
        for (int k = 0; k < 2; ++k) {
            const uint32_t l = std::max(r.lo, ab[k][0]), h = std::min(r.hi, ab[k][1]);
            if (l <= h) out.push_back(k == 0 ? Range{l + 32, h + 32} : Range{l - 32, h - 32});
        }
    }
    return norm(out);
}
inline Set set_of(const char* which) {
    switch (*which) {
        case 'd': return {{0x30, 0x39}};
        case 'w': return {{0x30, 0x39}, {0x41, 0x5A}, {0x5F, 0x5F}, {0x61, 0x7A}};
        case 's': return {{0x09, 0x0D}, {0x20, 0x20}};
        default: return {{0x0A, 0x0A}, {0x0D, 0x0D}, {0x85, 0x85}, {0x2028, 0x2029}};   // what `.` leaves out
    }
}

enum : int { N_SET, N_CAT, N_ALT, N_REP, N_BOL, N_EOL };
struct Node {
    int kind = N_SET;
    Set set;
    std::vector<int> kids;
    int lo = 0, hi = 0;   // N_REP: hi < 0 = unbounded
    bool greedy = true;
    bool nullable = false, anchored = false;
    int64_t atoms = 1;
};

struct Refusal { const char* what; int64_t pos; };

// a well-formed sequence at p[i]: its code point and length, or length 0
inline int decode_at(const uint8_t* p, int64_t n, int64_t i, uint32_t* cp) {
    const uint32_t c = p[i];
    if (c < 0x80) { *cp = c; return 1; }
    if (c < 0xC2 || c > 0xF4) return 0;
    const int L = c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4;
    if (i + L > n) return 0;
    for (int k = 1; k < L; ++k)
        if ((p[i + k] & 0xC0) != 0x80) return 0;
    if (L == 2) { *cp = ((c & 0x1F) << 6) | (p[i + 1] & 0x3Fu); return 2; }
    if (L == 3) {
        *cp = ((c & 0x0F) << 12) | ((p[i + 1] & 0x3Fu) << 6) | (p[i + 2] & 0x3Fu);
        return (*cp >= 0x800 && !(*cp >= 0xD800 && *cp <= 0xDFFF)) ? 3 : 0;
    }
    *cp = ((c & 0x07) << 18) | ((p[i + 1] & 0x3Fu) << 12) | ((p[i + 2] & 0x3Fu) << 6) | (p[i + 3] & 0x3Fu);
    return (*cp >= 0x10000 && *cp <= kCpMax) ? 4 : 0;
}

struct Parser {
    std::vector<int32_t> cp;
    std::vector<int64_t> at;
    size_t i = 0;
    bool icase = false, dotall = false;
    int depth = 0;
    std::vector<Node> nodes;

    int peek(size_t k = 0) const { return i + k < cp.size() ? cp[i + k] : -1; }
    int64_t pos(size_t k = 0) const { return at[std::min(i + k, cp.size())]; }
    static bool is_flag(int c) { return (c >= 0x41 && c <= 0x5A) || (c >= 0x61 && c <= 0x7A); }
    static bool is_punct(int c) { return (c >= 0x21 && c <= 0x2F) || (c >= 0x3A && c <= 0x40) || (c >= 0x5B && c <= 0x60) || (c >= 0x7B && c <= 0x7E); }

    int add(Node n) {
        switch (n.kind) {
            case N_SET: n.nullable = false; n.anchored = false; n.atoms = 1; break;
            case N_BOL: n.nullable = true; n.anchored = true; n.atoms = 1; break;
            case N_EOL: n.nullable = true; n.anchored = false; n.atoms = 1; break;
            case N_CAT:
                n.nullable = true; n.atoms = 0;
                for (int k : n.kids) { n.nullable = n.nullable && nodes[k].nullable; n.atoms += nodes[k].atoms; }
                n.anchored = !n.kids.empty() && nodes[n.kids[0]].anchored;
                break;
            case N_ALT:
                n.nullable = false; n.anchored = true; n.atoms = 0;
                for (int k : n.kids) { n.nullable = n.nullable || nodes[k].nullable; n.anchored = n.anchored && nodes[k].anchored; n.atoms += nodes[k].atoms; }
                break;
            default:
                n.nullable = n.lo == 0 || nodes[n.kids[0]].nullable;
                n.anchored = n.lo >= 1 && nodes[n.kids[0]].anchored;
                n.atoms = nodes[n.kids[0]].atoms * (n.hi >= 0 ? n.hi : std::max(n.lo, 1));
        }
        n.atoms = std::min<int64_t>(n.atoms, (int64_t)1 << 31);
        nodes.push_back(std::move(n));
        return (int)nodes.size() - 1;
    }
    int add_set(Set s) {
        Node n;
        n.kind = N_SET;
        n.set = icase ? fold(norm(std::move(s))) : norm(std::move(s));
        return add(std::move(n));
    }

    int parse(const uint8_t* p, int64_t n) {
        for (int64_t k = 0; k < n;) {
            uint32_t c = 0;
            const int L = decode_at(p, n, k, &c);
            if (L == 0) throw Refusal{"a byte that is not UTF-8", k};
            cp.push_back((int32_t)c);
            at.push_back(k);
            k += L;
        }
        at.push_back(n);
        if (peek() == '(' && peek(1) == '?' && (is_flag(peek(2)) || peek(2) == '-')) {
            size_t j = 2;
            for (; is_flag(peek(j)) || peek(j) == '-'; ++j) {
                const int c = peek(j);
                if (c == 'i' && !icase) icase = true;
                else if (c == 's' && !dotall) dotall = true;
                else throw Refusal{"an unsupported flag", pos(j)};
            }
            if (peek(j) != ')') throw Refusal{"a flag group that is not (?i) (?s) (?is) (?si)", pos()};
            i += j + 1;
        }
        const int t = alt();
        if (peek() == ')') throw Refusal{"an unmatched )", pos()};
        if (nodes[t].atoms > kUtf8RegexMaxAtoms) throw Refusal{"a pattern past the size cap", 0};
        return t;
    }
    int alt() {
        std::vector<int> br;
        br.push_back(cat());
        while (peek() == '|') {
            ++i;
            br.push_back(cat());
        }
        if (br.size() == 1) return br[0];
        Node n;
        n.kind = N_ALT;
        n.kids = br;
        return add(std::move(n));
    }
    int cat() {
        std::vector<int> items;
        while (peek() != -1 && peek() != '|' && peek() != ')') {
            const int t = atom();
            items.push_back(quant(t));
        }
        if (items.size() == 1) return items[0];
        Node n;
        n.kind = N_CAT;
        n.kids = items;
        return add(std::move(n));
    }
    int anchor(int kind) {
        Node n;
        n.kind = kind;
        return add(std::move(n));
    }
    int atom() {
        const int c = peek();
        const int64_t a = pos();
        if (c == '*' || c == '+' || c == '?') throw Refusal{"a quantifier without an operand", a};
        if (c == '{') throw Refusal{"a dangling {", a};
        ++i;
        if (c == '(') return group(a);
        if (c == '[') return klass(a);
        if (c == '.') {
            Node n;
            n.kind = N_SET;
            n.set = negate(dotall ? Set() : set_of("."));
            return add(std::move(n));
        }
        if (c == '^') return anchor(N_BOL);
        if (c == '$') return anchor(N_EOL);
        if (c == '\\') {
            Set s;
            uint32_t v = 0;
            const int kind = escape(a, false, &v, &s);
            if (kind == 0) return add_set({{v, v}});
            if (kind == 1) return add_set(s);
            return anchor(kind == 2 ? N_BOL : N_EOL);
        }
        return add_set({{(uint32_t)c, (uint32_t)c}});
    }
    int group(int64_t a) {
        if (peek() == '?') {
            const int c = peek(1);
            if (c == ':') i += 2;
            else if (c == '=' || c == '!') throw Refusal{"a look-ahead", a};
            else if (c == '<' && (peek(2) == '=' || peek(2) == '!')) throw Refusal{"a look-behind", a};
            else if (c == '<' || c == 'P') throw Refusal{"a named group", a};
            else if (c == '>') throw Refusal{"an atomic group", a};
            else if (is_flag(c) || c == '-') throw Refusal{"flags anywhere but at the front", a};
            else throw Refusal{"an unknown group", a};
        }
        if (++depth > 64) throw Refusal{"groups nested deeper than 64", a};
        const int t = alt();
        --depth;
        if (peek() != ')') throw Refusal{"an unclosed group", a};
        ++i;
        return t;
    }
    uint32_t hex(int n, int64_t a, const char* what) {
        uint32_t v = 0;
        for (int k = 0; k < n; ++k) {
            const int c = peek();
            int d;
            if (c >= '0' && c <= '9') d = c - '0';
            else if ((c >= 'A' && c <= 'F') || (c >= 'a' && c <= 'f')) d = (c | 0x20) - 'a' + 10;
            else throw Refusal{what, a};
            v = v * 16 + (uint32_t)d;
            ++i;
        }
        return v;
    }
    // after the backslash.  0: a code point (*v); 1: a set (*s); 2: row start; 3: row end
    int escape(int64_t a, bool in_class, uint32_t* v, Set* s) {
        const int c = peek();
        if (c == -1) throw Refusal{"a trailing backslash", a};
        ++i;
        switch (c) {
            case 'd': *s = set_of("d"); return 1;
            case 'w': *s = set_of("w"); return 1;
            case 's': *s = set_of("s"); return 1;
            case 'D': case 'W': case 'S':
                if (in_class) throw Refusal{"a negated class escape inside a class", a};
                *s = negate(set_of(c == 'D' ? "d" : c == 'W' ? "w" : "s"));
                return 1;
            case 't': *v = 9; return 0;
            case 'n': *v = 10; return 0;
            case 'r': *v = 13; return 0;
            case 'f': *v = 12; return 0;
            case 'x': *v = hex(2, a, "a malformed \\x escape"); return 0;
            case 'u':
                *v = hex(4, a, "a malformed \\u escape");
                if (*v >= 0xD800 && *v <= 0xDFFF) throw Refusal{"a surrogate \\u escape", a};
                return 0;
            case 'A': if (!in_class) return 2; break;
            case 'z': if (!in_class) return 3; break;
            case '0': throw Refusal{"an octal escape", a};
            case '1': case '2': case '3': case '4': case '5': case '6': case '7': case '8': case '9': case 'k': throw Refusal{"a backreference", a};
            case 'b': case 'B': throw Refusal{"a word boundary", a};
            case 'p': case 'P': throw Refusal{"a Unicode property class", a};
            case 'Q': case 'E': throw Refusal{"a \\Q..\\E quotation", a};
            default: break;
        }
        if (is_punct(c)) { *v = (uint32_t)c; return 0; }
        throw Refusal{"an unsupported escape", a};
    }
    int klass(int64_t a) {
        bool neg = false;
        if (peek() == '^') { neg = true; ++i; }
        if (peek() == ']') throw Refusal{"a ] that opens a class", a};
        Set ranges;
        for (;;) {
            const int c = peek();
            const int64_t ca = pos();
            if (c == -1) throw Refusal{"an unterminated class", a};
            if (c == ']') { ++i; break; }
            if (c == '[') throw Refusal{"a nested class", ca};
            if (c == '&' && peek(1) == '&') throw Refusal{"a class intersection", ca};
            ++i;
            int kind = 0;
            uint32_t v = (uint32_t)c;
            Set s;
            if (c == '\\') kind = escape(ca, true, &v, &s);
            if (peek() == '-' && peek(1) != ']' && peek(1) != -1) {
                if (kind != 0) throw Refusal{"a range from a class escape", ca};
                ++i;
                const int h = peek();
                const int64_t ha = pos();
                if (h == '[') throw Refusal{"a nested class", ha};
                ++i;
                int hk = 0;
                uint32_t hv = (uint32_t)h;
                Set hs;
                if (h == '\\') hk = escape(ha, true, &hv, &hs);
                if (hk != 0) throw Refusal{"a class escape as a range end", ha};
                if (hv < v) throw Refusal{"a reversed range", ca};
                ranges.push_back({v, hv});
            } else if (kind == 0) ranges.push_back({v, v});
            else ranges.insert(ranges.end(), s.begin(), s.end());
        }
        ranges = norm(ranges);
        if (icase) ranges = fold(ranges);
        Node n;
        n.kind = N_SET;
        n.set = neg ? negate(ranges) : ranges;
        return add(std::move(n));
    }
    int number() {
        int v = 0, digits = 0;
        while (peek() >= '0' && peek() <= '9') {
            v = std::min(v * 10 + (peek() - '0'), kUtf8RegexMaxCount + 1);
            ++i;
            ++digits;
        }
        return digits ? v : -1;
    }
    int quant(int t) {
        const int c = peek();
        const int64_t a = pos();
        int lo, hi;
        if (c == '*') { lo = 0; hi = -1; ++i; }
        else if (c == '+') { lo = 1; hi = -1; ++i; }
        else if (c == '?') { lo = 0; hi = 1; ++i; }
        else if (c == '{') {
            ++i;
            lo = number();
            hi = lo;
            if (lo >= 0 && peek() == ',') {
                ++i;
                hi = peek() != '}' ? number() : -1;
                if (hi == -1 && peek() != '}') lo = -1;
            }
            if (lo < 0 || peek() != '}') throw Refusal{"a dangling {", a};
            ++i;
            if (lo > kUtf8RegexMaxCount || hi > kUtf8RegexMaxCount) throw Refusal{"a repetition count above 1000", a};
            if (hi >= 0 && lo > hi) throw Refusal{"{n,m} with n > m", a};
        } else return t;
        bool greedy = true;
        if (peek() == '?') { greedy = false; ++i; }
        else if (peek() == '+') throw Refusal{"a possessive quantifier", pos()};
        if (peek() == '*' || peek() == '+' || peek() == '?' || peek() == '{') throw Refusal{"a quantifier on a quantifier", pos()};
        if (nodes[t].kind == N_BOL || nodes[t].kind == N_EOL) throw Refusal{"a quantifier on an anchor", a};
        if ((hi < 0 || hi > 1) && nodes[t].nullable) throw Refusal{"a repeated operand that can match empty", a};
        Node n;
        n.kind = N_REP;
        n.kids = {t};
        n.lo = lo;
        n.hi = hi;
        n.greedy = greedy;
        const int r = add(std::move(n));
        if (nodes[r].atoms > kUtf8RegexMaxAtoms) throw Refusal{"counted repetition past the size cap", a};
        return r;
    }
};

// ---- the Thompson program
enum : uint8_t { I_BYTE, I_SPLIT, I_BOL, I_EOL, I_MATCH };
struct Inst { uint8_t op, lo, hi; int32_t x, y; };   // BYTE / BOL / EOL: x = next; SPLIT: x before y

struct Builder {
    const std::vector<Node>& nodes;
    bool reverse;
    std::vector<Inst> prog;
    bool overflow = false;

    int emit_inst(Inst in) {
        if ((int)prog.size() >= kUtf8RegexMaxProgram) { overflow = true; return 0; }
        prog.push_back(in);
        return (int)prog.size() - 1;
    }
    static int encode(uint32_t cp, uint8_t* out) {
        if (cp < 0x80) { out[0] = (uint8_t)cp; return 1; }
        if (cp < 0x800) { out[0] = (uint8_t)(0xC0 | (cp >> 6)); out[1] = (uint8_t)(0x80 | (cp & 0x3F)); return 2; }
        if (cp < 0x10000) { out[0] = (uint8_t)(0xE0 | (cp >> 12)); out[1] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F)); out[2] = (uint8_t)(0x80 | (cp & 0x3F)); return 3; }
        out[0] = (uint8_t)(0xF0 | (cp >> 18)); out[1] = (uint8_t)(0x80 | ((cp >> 12) & 0x3F)); out[2] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F));
        out[3] = (uint8_t)(0x80 | (cp & 0x3F));
        return 4;
    }
    // the byte-range sequences of the code points lo..hi, which encode to the same length and avoid the surrogates
    void seqs(uint32_t lo, uint32_t hi, std::vector<std::vector<Range>>* out) {
        uint8_t a[4], b[4];
        const int n = encode(lo, a);
        for (int k = 1; k < n; ++k) {
            const uint32_t m = (1u << (6 * k)) - 1;
            if ((lo & ~m) != (hi & ~m)) {
                if ((lo & m) != 0) { seqs(lo, lo | m, out); seqs((lo | m) + 1, hi, out); return; }
                if ((hi & m) != m) { seqs(lo, (hi & ~m) - 1, out); seqs(hi & ~m, hi, out); return; }
            }
        }
        encode(hi, b);
        std::vector<Range> s;
        for (int k = 0; k < n; ++k) s.push_back({a[k], b[k]});
        out->push_back(s);
    }
    int emit_set(const Set& set, int next) {
        std::vector<std::vector<Range>> all;
        static const uint32_t cuts[5][2] = {{0, 0x7F}, {0x80, 0x7FF}, {0x800, 0xD7FF}, {0xE000, 0xFFFF}, {0x10000, kCpMax}};
        for (const Range& r : set)
            for (int k = 0; k < 5; ++k) {
                const uint32_t l = std::max(r.lo, cuts[k][0]), h = std::min(r.hi, cuts[k][1]);
                if (l <= h) seqs(l, h, &all);
            }
        int entry = -1;
        for (size_t q = all.size(); q-- > 0;) {   // a chain of SPLITs over the (disjoint) alternatives
            const std::vector<Range>& s = all[q];
            int at = next;
            if (!reverse) for (size_t k = s.size(); k-- > 0;) at = emit_inst({I_BYTE, (uint8_t)s[k].lo, (uint8_t)s[k].hi, at, 0});
            else for (size_t k = 0; k < s.size(); ++k) at = emit_inst({I_BYTE, (uint8_t)s[k].lo, (uint8_t)s[k].hi, at, 0});
            entry = entry < 0 ? at : emit_inst({I_SPLIT, 0, 0, at, entry});
            if (overflow) return next;
        }
        if (entry < 0) {   // the empty set matches nothing: a byte range no byte is in
            entry = emit_inst({I_BYTE, 1, 0, next, 0});
        }
        return entry;
    }
    int emit(int t, int next) {
        if (overflow) return next;
        const Node& n = nodes[t];
        switch (n.kind) {
            case N_SET: return emit_set(n.set, next);
            case N_BOL: return emit_inst({I_BOL, 0, 0, next, 0});
            case N_EOL: return emit_inst({I_EOL, 0, 0, next, 0});
            case N_CAT:
                if (!reverse) for (size_t k = n.kids.size(); k-- > 0;) next = emit(n.kids[k], next);
                else for (size_t k = 0; k < n.kids.size(); ++k) next = emit(n.kids[k], next);
                return next;
            case N_ALT: {
                int entry = -1;
                for (size_t k = n.kids.size(); k-- > 0;) {
                    const int e = emit(n.kids[k], next);
                    entry = entry < 0 ? e : emit_inst({I_SPLIT, 0, 0, e, entry});
                }
                return entry;
            }
            default: break;
        }
        const int body = n.kids[0];
        if (n.hi >= 0) {
            for (int k = 0; k < n.hi - n.lo && !overflow; ++k) {   // x{0,k} = (x(x(..)?)?)?
                const int b = emit(body, next);
                next = n.greedy ? emit_inst({I_SPLIT, 0, 0, b, next}) : emit_inst({I_SPLIT, 0, 0, next, b});
            }
        } else {
            const int loop = emit_inst({I_SPLIT, 0, 0, 0, 0});
            const int b = emit(body, loop);
            if (!overflow) {
                prog[loop].x = n.greedy ? b : next;
                prog[loop].y = n.greedy ? next : b;
            }
            next = loop;
        }
        for (int k = 0; k < n.lo && !overflow; ++k) next = emit(body, next);
        return next;
    }
};

// ---- the subset construction
struct Dfa {
    std::vector<uint16_t> table;   // [state][class], renumbered: 0 dead, flagged states last
    int states = 0, flagged = 0, start_a = 0, start_b = 0;
    bool overflow = false;
    int seen = 0;
};

struct Subset {
    const std::vector<Inst>& prog;
    int entry;
    bool reverse, prefix, oneshot;   // oneshot: an anchored pattern starts at byte 0 only
    int nc;                        // byte classes + 2
    const std::vector<uint8_t>& rep;   // a byte of every byte class
    int P_FORK, P_LEAF;
    std::vector<int> stamp;
    int tick = 0;
    std::map<std::vector<int32_t>, int> ids;   // key: [edge << 1 | flagged, pcs...]
    std::vector<std::vector<int32_t>> keys;

    Subset(const std::vector<Inst>& p, int e, bool rev, bool pre, bool one, int classes, const std::vector<uint8_t>& r)
        : prog(p), entry(e), reverse(rev), prefix(pre), oneshot(one), nc(classes), rep(r), P_FORK((int)p.size()), P_LEAF((int)p.size() + 1), stamp(p.size() + 2, 0) {}

    int id_of(const std::vector<int32_t>& key) {
        auto it = ids.find(key);
        if (it != ids.end()) return it->second;
        const int id = (int)keys.size();
        ids.emplace(key, id);
        keys.push_back(key);
        return id;
    }
    // the state reached from `key` by class c
    std::vector<int32_t> step(const std::vector<int32_t>& key, int c) {
        const bool edge = (key[0] >> 1) & 1;             // forward: at byte 0; reverse: at the row's end
        const bool is_begin = c == nc - 2, is_end = c == nc - 1;
        const int byte = c < nc - 2 ? rep[(size_t)c] : -1;
        const bool bol = reverse ? is_begin : edge, eol = reverse ? edge : is_end;
        const bool may_start = is_end || (byte >= 0 && (byte & 0xC0) != 0x80);
        ++tick;
        std::vector<int32_t> out(1, 0), stack;
        bool flagged = false;
        for (size_t k = 1; k < key.size() && !(flagged && !reverse); ++k) {
            stack.push_back(key[k]);
            while (!stack.empty()) {
                const int pc = stack.back();
                stack.pop_back();
                if (stamp[(size_t)pc] == tick) continue;
                stamp[(size_t)pc] = tick;
                if (pc == P_FORK) {
                    stack.push_back(P_LEAF);
                    if (may_start) stack.push_back(entry);
                    continue;
                }
                if (pc == P_LEAF) {
                    if (!is_end && !oneshot) out.push_back(P_FORK);
                    continue;
                }
                const Inst& in = prog[(size_t)pc];
                if (in.op == I_SPLIT) { stack.push_back(in.y); stack.push_back(in.x); }
                else if (in.op == I_BOL) { if (bol) stack.push_back(in.x); }
                else if (in.op == I_EOL) { if (eol) stack.push_back(in.x); }
                else if (in.op == I_MATCH) {
                    flagged = true;
                    if (!reverse) { stack.clear(); break; }   // leftmost-first: the threads behind a match are dropped
                } else if (byte >= 0 && in.lo <= byte && byte <= in.hi) out.push_back(in.x);
            }
        }
        // a kernel keeps the first occurrence of a pc (the highest priority)
        ++tick;
        size_t w = 1;
        for (size_t k = 1; k < out.size(); ++k)
            if (stamp[(size_t)out[k]] != tick) { stamp[(size_t)out[k]] = tick; out[w++] = out[k]; }
        out.resize(w);
        out[0] = flagged ? 1 : 0;
        return out;
    }
    Dfa build() {
        Dfa d;
        const std::vector<int32_t> dead(1, 0);
        id_of(dead);
        std::vector<int32_t> a(2), b(2);
        a[0] = 2; b[0] = 0;
        a[1] = b[1] = prefix ? P_FORK : entry;
        const int ia = id_of(a);
        // an anchored pattern cannot begin anywhere but at byte 0
        const int ib = oneshot ? 0 : id_of(b);
        std::vector<uint16_t> raw;
        for (size_t s = 0; s < keys.size(); ++s) {
            if ((int)keys.size() > kUtf8RegexMaxStates) { d.overflow = true; d.seen = (int)keys.size(); return d; }
            const std::vector<int32_t> key = keys[s];
            for (int c = 0; c < nc; ++c) {
                int to = 0;
                if (key.size() > 1) to = id_of(step(key, c));
                raw.push_back((uint16_t)std::min(to, 65535));
            }
        }
        const int n = (int)keys.size();
        if (n > kUtf8RegexMaxStates) { d.overflow = true; d.seen = n; return d; }
        std::vector<int> renum((size_t)n);
        int at = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int s = 0; s < n; ++s)
                if ((keys[(size_t)s][0] & 1) == pass) renum[(size_t)s] = at++;   // (the dead state is the first unflagged one: 0)
        d.states = n;
        d.flagged = n;
        for (int s = 0; s < n; ++s)
            if (keys[(size_t)s][0] & 1) d.flagged = std::min(d.flagged, renum[(size_t)s]);
        d.table.assign((size_t)n * nc, 0);
        for (int s = 0; s < n; ++s)
            for (int c = 0; c < nc; ++c) d.table[(size_t)renum[(size_t)s] * nc + c] = (uint16_t)renum[raw[(size_t)s * nc + c]];
        d.start_a = renum[(size_t)ia];
        d.start_b = renum[(size_t)ib];
        return d;
    }
};

}  // namespace utf8_regex_detail

inline Utf8RegexCompiled utf8_regex_compile(const uint8_t* pattern, int64_t n) {
    using namespace utf8_regex_detail;
    Utf8RegexCompiled out;
    memset(&out.h, 0, sizeof out.h);
    Parser ps;
    int root;
    try {
        root = ps.parse(pattern, n);
    } catch (const Refusal& r) {
        out.status = U8X_SYNTAX;
        out.what = r.what;
        out.pos = r.pos;
        return out;
    }
    const Node& top = ps.nodes[(size_t)root];
    Builder fb{ps.nodes, false, {}, false}, rb{ps.nodes, true, {}, false};
    const int fmatch = fb.emit_inst({I_MATCH, 0, 0, 0, 0}), rmatch = rb.emit_inst({I_MATCH, 0, 0, 0, 0});
    const int fentry = fb.emit(root, fmatch), rentry = rb.emit(root, rmatch);
    if (fb.overflow || rb.overflow) {
        out.status = U8X_CAP;
        out.what = "a program of more than " + std::to_string(kUtf8RegexMaxProgram) + " instructions";
        return out;
    }
    // byte classes: the coarsest partition that no BYTE range and neither 0x80 nor 0xC0 cuts
    bool cut[257] = {false};
    cut[0] = cut[0x80] = cut[0xC0] = cut[256] = true;
    for (const Inst& in : fb.prog)
        if (in.op == I_BYTE && in.lo <= in.hi) { cut[in.lo] = true; cut[in.hi + 1] = true; }
    uint8_t cls[256];
    std::vector<uint8_t> rep;
    for (int b = 0; b < 256; ++b) {
        if (cut[b]) rep.push_back((uint8_t)b);
        cls[b] = (uint8_t)(rep.size() - 1);
    }
    const int nc = (int)rep.size() + 2;
    Subset fs(fb.prog, fentry, false, true, top.anchored, nc, rep), rs(rb.prog, rentry, true, false, false, nc, rep);
    const Dfa fd = fs.build();
    const Dfa rd = fd.overflow ? Dfa() : rs.build();
    if (fd.overflow || rd.overflow) {
        out.status = U8X_CAP;
        out.what = std::string(fd.overflow ? "a forward" : "a reverse") + " DFA of more than " + std::to_string(kUtf8RegexMaxStates) + " states (" +
                   std::to_string(fd.overflow ? fd.seen : rd.seen) + " seen)";
        return out;
    }
    const int64_t bytes = kUtf8RegexHeaderBytes + 256 + 2 * ((int64_t)fd.states + rd.states) * nc;
    const int64_t padded = (bytes + 15) & ~(int64_t)15;
    Utf8RegexHeader& h = out.h;
    h.classes = nc;
    h.fwd_states = fd.states; h.rev_states = rd.states;
    h.fwd_flagged = fd.flagged; h.rev_flagged = rd.flagged;
    h.fwd_start0 = fd.start_a; h.fwd_start = fd.start_b;
    h.rev_start_end = rd.start_a; h.rev_start = rd.start_b;
    h.can_match_empty = top.nullable;
    h.anchored_start = top.anchored;
    h.program_len = (int32_t)fb.prog.size();
    h.table_bytes = (int32_t)padded;
    if (padded > kUtf8RegexMaxTableBytes) {
        out.status = U8X_CAP;
        out.what = "tables of " + std::to_string(padded) + " bytes (" + std::to_string(fd.states) + " + " + std::to_string(rd.states) + " states), at most " +
                   std::to_string(kUtf8RegexMaxTableBytes);
        return out;
    }
    out.image.assign((size_t)padded, 0);
    memcpy(out.image.data(), &h, sizeof h);
    memcpy(out.image.data() + kUtf8RegexHeaderBytes, cls, 256);
    if (!fd.table.empty()) memcpy(out.image.data() + kUtf8RegexHeaderBytes + 256, fd.table.data(), fd.table.size() * 2);
    if (!rd.table.empty()) memcpy(out.image.data() + kUtf8RegexHeaderBytes + 256 + fd.table.size() * 2, rd.table.data(), rd.table.size() * 2);
    return out;
}
#endif   // RDF_UTF8_REGEX_NO_COMPILER
