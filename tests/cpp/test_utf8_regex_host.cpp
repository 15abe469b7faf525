// rust_dataframe_amd/csrc/rdf_utf8_regex.h under plain g++ -fsanitize=address,undefined: no HIP, no GPU, no Python in the
// process.  Reads the table tests/utf8_regex_ref.py writes (byte strings as hex, '-' = empty):
//     X <pattern> <position>                 the pattern is refused at that byte
//     P <pattern> <replacement> <limit>      the pattern compiles; the R lines that follow belong to it
//     C <pattern> <replacement> <limit>      ... or it is refused by a cap, and by nothing else
//     R <row> <s,e,s,e,..> <replaced> <n>:<split bytes>:<offset,..>
// Every span and every output byte of the five operations is produced through the header's stepping functions, sizes first
// and then the bytes into a block of exactly that size.  Every row sits in a heap block of exactly its length.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rust_dataframe_amd/csrc/rdf_utf8_regex.h"

static long g_checks = 0, g_failed = 0, g_line = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { if (++g_failed <= 20) { printf("FAIL line %ld: ", g_line); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Bytes {   // exactly n bytes on the heap
    uint8_t* p;
    int64_t n;
    explicit Bytes(const char* hex) {
        n = strcmp(hex, "-") == 0 ? 0 : (int64_t)strlen(hex) / 2;
        p = new uint8_t[(size_t)n];
        for (int64_t i = 0; i < n; ++i) {
            unsigned v = 0;
            sscanf(hex + 2 * i, "%2x", &v);
            p[i] = (uint8_t)v;
        }
    }
    explicit Bytes(int64_t len) : n(len) { p = new uint8_t[(size_t)n]; memset(p, 0xEE, (size_t)n); }
    ~Bytes() { delete[] p; }
    Bytes(const Bytes&) = delete;
};
static bool same(const Bytes& a, const Bytes& b) { return a.n == b.n && (a.n == 0 || memcmp(a.p, b.p, (size_t)a.n) == 0); }
static std::vector<int64_t> numbers(const char* s) {
    std::vector<int64_t> v;
    if (strcmp(s, "-") == 0) return v;
    for (const char* p = s; *p;) {
        v.push_back(strtoll(p, (char**)&p, 10));
        if (*p == ',') ++p;
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    static char line[1 << 20];
    long patterns = 0, pairs = 0, refused = 0, capped = 0;
    Utf8RegexCompiled rx;
    Bytes* rep = nullptr;
    int64_t limit = -1;
    bool live = false;
    while (fgets(line, sizeof line, f)) {
        ++g_line;
        std::vector<char*> tok;
        for (char* t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        if (tok.empty()) continue;
        if (tok[0][0] == 'X') {
            const Bytes pat(tok[1]);
            const Utf8RegexCompiled c = utf8_regex_compile(pat.p, pat.n);
            CHECK(c.status == U8X_SYNTAX && c.pos == atoll(tok[2]), "refusal: status %d (%s) at %lld, expected at %s", c.status, c.what.c_str(), (long long)c.pos, tok[2]);
            ++refused;
        } else if (tok[0][0] == 'P' || tok[0][0] == 'C') {
            const Bytes pat(tok[1]);
            rx = utf8_regex_compile(pat.p, pat.n);
            delete rep;
            const Bytes raw(tok[2]);
            rep = new Bytes(raw.n);
            bool dollar = false;
            int64_t rn = 0;
            CHECK(utf8_regex_replacement(raw.p, raw.n, rep->p, &rn, &dollar) < 0, "the replacement is refused");
            rep->n = rn;
            limit = atoll(tok[3]);
            live = rx.status == U8X_OK;
            if (!live && tok[0][0] == 'C' && rx.status == U8X_CAP) { ++capped; printf("capped: %s\n", rx.what.c_str()); }
            else CHECK(live, "the pattern is refused: %s at %lld", rx.what.c_str(), (long long)rx.pos);
            if (live) {
                ++patterns;
                CHECK(rx.h.fwd_states <= kUtf8RegexMaxStates && rx.h.rev_states <= kUtf8RegexMaxStates && rx.h.table_bytes == (int64_t)rx.image.size() &&
                          rx.h.table_bytes <= kUtf8RegexMaxTableBytes && rx.h.program_len <= kUtf8RegexMaxProgram, "a cap is passed");
            }
        } else if (tok[0][0] == 'R' && live && tok.size() == 5) {
            ++pairs;
            const Bytes image((int64_t)rx.image.size());   // the tables too sit in a block of exactly their size
            memcpy(image.p, rx.image.data(), rx.image.size());
            const Utf8RegexView v = utf8_regex_view(rx.h, image.p);
            const Bytes row(tok[1]);
            const std::vector<int64_t> want = numbers(tok[2]);
            std::vector<int64_t> got;
            int64_t from = 0, s = 0, e = 0;
            while (from <= row.n && utf8_regex_find(v, row.p, row.n, from, &s, &e)) {
                got.push_back(s);
                got.push_back(e);
                CHECK(s >= from && e >= s && e <= row.n, "a span outside the search");
                from = utf8_regex_resume(s, e);
                if (got.size() > 4 * (size_t)row.n + 8) break;
            }
            CHECK(got == want, "spans differ (%zu, expected %zu numbers)", got.size(), want.size());
            CHECK(utf8_regex_any(v, row.p, row.n) == !want.empty(), "rlike");
            CHECK(utf8_regex_count(v, row.p, row.n) == (int64_t)want.size() / 2, "count");
            const auto none = [](int64_t, int64_t) {};
            int64_t elems = 0;
            {   // extract
                const int64_t n0 = utf8_regex_row(v, U8X_EXTRACT, row.p, row.n, nullptr, 0, kUtf8AllHits, nullptr, &elems, none);
                Bytes out(n0);
                utf8_regex_row(v, U8X_EXTRACT, row.p, row.n, nullptr, 0, kUtf8AllHits, out.p, &elems, none);
                const int64_t ws = want.empty() ? 0 : want[0], we = want.empty() ? 0 : want[1];
                CHECK(n0 == we - ws && (n0 == 0 || memcmp(out.p, row.p + ws, (size_t)n0) == 0), "extract");
            }
            {   // replace
                const Bytes exp(tok[3]);
                const int64_t n0 = utf8_regex_row(v, U8X_REPLACE, row.p, row.n, rep->p, rep->n, kUtf8AllHits, nullptr, &elems, none);
                Bytes out(n0);
                const int64_t n1 = utf8_regex_row(v, U8X_REPLACE, row.p, row.n, rep->p, rep->n, kUtf8AllHits, out.p, &elems, none);
                CHECK(n0 == n1 && same(out, exp), "replace: %lld bytes, expected %lld", (long long)n0, (long long)exp.n);
            }
            {   // split
                char* a = strtok(tok[4], ":");
                char* b = strtok(nullptr, ":");
                char* c = strtok(nullptr, ":");
                const int64_t nel = atoll(a);
                const Bytes exp(b);
                const std::vector<int64_t> woffs = numbers(c);
                const int64_t mh = utf8_regex_split_max_hits(limit);
                const int64_t n0 = utf8_regex_row(v, U8X_SPLIT, row.p, row.n, nullptr, 0, mh, nullptr, &elems, none);
                CHECK(elems == nel, "split: %lld elements, expected %lld", (long long)elems, (long long)nel);
                Bytes out(n0);
                std::vector<int64_t> offs(1, 0);
                utf8_regex_row(v, U8X_SPLIT, row.p, row.n, nullptr, 0, mh, out.p, &elems, [&](int64_t j, int64_t o) { CHECK(j == (int64_t)offs.size(), "hit order"); offs.push_back(o); });
                CHECK(same(out, exp) && offs == woffs, "split: bytes or offsets differ");
            }
        }
    }
    delete rep;
    fclose(f);
    printf("%ld patterns, %ld pairs, %ld refusals, %ld capped, %ld checks, %ld failed\n", patterns, pairs, refused, capped, g_checks, g_failed);
    return g_failed ? 1 : 0;
}
