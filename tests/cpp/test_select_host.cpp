// rust_dataframe_amd/csrc/rdf_select.h under a plain host compiler (g++ -std=c++17, no HIP): the functions the kernels run
// for one row — the chosen part of coalesce / case_when, Spark's ordering, extremum's fold, nanvl — over the table that
// tests/select_ref.py writes (argv[1]; the formats of its lines are described there).  Every number of the table is hex; a
// part and a result are `valid bits`.
// Usage: test_select_host <select_cases.txt>.  Exit status 0 = everything agreed.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../../rust_dataframe_amd/csrc/rdf_select.h"

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            if (++g_failed <= 20) { printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                  \
    } while (0)

struct Cell { bool valid; uint64_t bits; };

struct Line {
    char* at;
    bool word(char* out, size_t cap) {
        while (*at == ' ') ++at;
        size_t n = 0;
        while (*at && *at != ' ' && *at != '\n' && n + 1 < cap) out[n++] = *at++;
        out[n] = 0;
        return n > 0;
    }
    bool hex(uint64_t& v) {
        char buf[32];
        if (!word(buf, sizeof buf)) return false;
        char* end = nullptr;
        v = strtoull(buf, &end, 16);
        return *end == 0;
    }
    bool cell(Cell& c) {
        uint64_t v, b;
        if (!hex(v) || !hex(b)) return false;
        c.valid = v != 0; c.bits = b;
        return true;
    }
};

template <int CLS, int ES>
static void row_x(const Cell* parts, int nparts, const Cell& co, const Cell& gr, const Cell& le, long line) {
    using U = typename SelBits<ES>::U;
    uint32_t valid = 0;
    for (int k = 0; k < nparts; ++k) valid |= (uint32_t)parts[k].valid << k;
    const int k = sel_coalesce(valid, nparts);
    CHECK((k >= 0) == co.valid, "line %ld: coalesce chose %d", line, k);
    {   // the kernels' chain on words, this row in bit `line % 64`, its neighbours undecided and never taken
        const uint64_t me = 1ull << (line & 63);
        uint64_t undecided = ~0ull;
        int chosen = -1;
        for (int i = 0; i < nparts; ++i)
            if (sel_take(undecided, parts[i].valid ? me : 0ull) & me) chosen = chosen < 0 ? i : -2;
        CHECK(chosen == k && undecided == (k >= 0 ? ~me : ~0ull), "line %ld: the word chain chose %d, the row rule %d", line, chosen, k);
    }
    CHECK((k >= 0 ? parts[k].bits : 0) == co.bits, "line %ld: coalesce chose %d", line, k);
    for (int g = 0; g < 2; ++g) {
        U acc = 0;
        bool have = false;
        for (int i = 0; i < nparts; ++i) { sel_fold<CLS, ES>(g != 0, (U)parts[i].bits, parts[i].valid, acc, have); }
        const Cell& want = g ? gr : le;
        CHECK(have == want.valid && (uint64_t)acc == want.bits, "line %ld: %s gave %d %" PRIx64 ", expected %d %" PRIx64, line, g ? "greatest" : "least",
              (int)have, (uint64_t)acc, (int)want.valid, want.bits);
    }
    if (nparts >= 2) {   // the ordering itself: irreflexive, asymmetric, lt the mirror of gt
        const U a = (U)parts[0].bits, b = (U)parts[1].bits;
        const bool gaa = sel_gt<CLS, ES>(a, a), laa = sel_lt<CLS, ES>(a, a), gab = sel_gt<CLS, ES>(a, b), gba = sel_gt<CLS, ES>(b, a), lab = sel_lt<CLS, ES>(a, b);
        CHECK(!gaa && !laa, "line %ld", line);
        CHECK(!(gab && gba), "line %ld", line);
        CHECK(lab == gba, "line %ld", line);
    }
}

static void row_w(const Cell* parts, int nbranches, uint32_t holds, const Cell& want, long line) {
    const int k = sel_case_when(holds, nbranches);
    CHECK(k >= 0 && k <= nbranches, "line %ld: slot %d", line, k);
    {   // the kernels' chain on words: the branches take by their conditions, `otherwise` what is left
        const uint64_t me = 1ull << (line & 63);
        uint64_t undecided = ~0ull;
        int chosen = -1;
        for (int i = 0; i <= nbranches; ++i)
            if (sel_take(undecided, i == nbranches ? ~0ull : ((holds >> i) & 1u) ? me : 0ull) & me) chosen = chosen < 0 ? i : -2;
        CHECK(chosen == k && undecided == 0, "line %ld: the word chain chose %d, the row rule %d", line, chosen, k);
    }
    CHECK(parts[k].valid == want.valid && (parts[k].valid ? parts[k].bits : 0) == want.bits, "line %ld: case_when chose slot %d", line, k);
}

template <int ES>
static void row_n(const Cell& a, const Cell& b, const Cell& want, long line) {
    using U = typename SelBits<ES>::U;
    U out;
    bool valid;
    sel_nanvl<ES>((U)a.bits, a.valid, (U)b.bits, b.valid, out, valid);
    CHECK(valid == want.valid && (uint64_t)out == want.bits, "line %ld: nanvl gave %d %" PRIx64 ", expected %d %" PRIx64, line, (int)valid, (uint64_t)out, (int)want.valid, want.bits);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <select_cases.txt>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    // the first-bit chain on its own: every mask of eight parts
    for (uint32_t m = 0; m < 256; ++m)
        for (int n = 1; n <= 8; ++n) {
            int want = -1;
            for (int k = n - 1; k >= 0; --k) if ((m >> k) & 1u) want = k;
            CHECK(sel_coalesce(m, n) == want, "mask %x of %d", m, n);
            CHECK(sel_case_when(m, n) == (want < 0 ? n : want), "mask %x of %d", m, n);
        }
    const std::map<std::string, int> dtypes = {{"i8", 0}, {"i16", 1}, {"i32", 2}, {"i64", 3}, {"u8", 4}, {"u16", 5}, {"u32", 6}, {"u64", 7}, {"f32", 8}, {"f64", 9}};
    std::map<std::string, long> rows;
    char* buf = (char*)malloc(4096);
    long line = 0, bad = 0;
    while (fgets(buf, 4096, f)) {
        ++line;
        Line in = {buf};
        char kind[8], name[8];
        if (!in.word(kind, sizeof kind) || !in.word(name, sizeof name) || !dtypes.count(name)) { ++bad; continue; }
        const int dt = dtypes.at(name);
        Cell parts[kSelSlots], r[3];
        uint64_t n = 0, holds = 0;
        bool ok = true;
        if (kind[0] == 'X') {
            ok = in.hex(n) && n >= 1 && n <= (uint64_t)kSelMaxParts;
            for (uint64_t k = 0; ok && k < n; ++k) ok = in.cell(parts[k]);
            ok = ok && in.cell(r[0]) && in.cell(r[1]) && in.cell(r[2]);
            if (!ok) { ++bad; continue; }
            switch (dt) {
                case 0: row_x<SEL_SIGNED, 1>(parts, (int)n, r[0], r[1], r[2], line); break;
                case 1: row_x<SEL_SIGNED, 2>(parts, (int)n, r[0], r[1], r[2], line); break;
                case 2: row_x<SEL_SIGNED, 4>(parts, (int)n, r[0], r[1], r[2], line); break;
                case 3: row_x<SEL_SIGNED, 8>(parts, (int)n, r[0], r[1], r[2], line); break;
                case 4: row_x<SEL_UNSIGNED, 1>(parts, (int)n, r[0], r[1], r[2], line); break;
                case 5: row_x<SEL_UNSIGNED, 2>(parts, (int)n, r[0], r[1], r[2], line); break;
                case 6: row_x<SEL_UNSIGNED, 4>(parts, (int)n, r[0], r[1], r[2], line); break;
                case 7: row_x<SEL_UNSIGNED, 8>(parts, (int)n, r[0], r[1], r[2], line); break;
                case 8: row_x<SEL_FLOAT, 4>(parts, (int)n, r[0], r[1], r[2], line); break;
                default: row_x<SEL_FLOAT, 8>(parts, (int)n, r[0], r[1], r[2], line); break;
            }
        } else if (kind[0] == 'W') {
            ok = in.hex(n) && n >= 1 && n <= (uint64_t)kSelMaxParts && in.hex(holds);
            for (uint64_t k = 0; ok && k <= n; ++k) ok = in.cell(parts[k]);
            ok = ok && in.cell(r[0]);
            if (!ok) { ++bad; continue; }
            row_w(parts, (int)n, (uint32_t)holds, r[0], line);
        } else if (kind[0] == 'N' && dt >= 8) {
            ok = in.cell(parts[0]) && in.cell(parts[1]) && in.cell(r[0]);
            if (!ok) { ++bad; continue; }
            if (dt == 8) row_n<4>(parts[0], parts[1], r[0], line);
            else row_n<8>(parts[0], parts[1], r[0], line);
        } else { ++bad; continue; }
        ++rows[std::string(kind) + "_" + name];
    }
    free(buf);
    fclose(f);
    CHECK(bad == 0, "%ld lines could not be read", bad);
    printf("rows:");
    for (const auto& kv : rows) printf(" %s %ld", kv.first.c_str(), kv.second);
    printf("\n%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
