// rust_dataframe_amd/csrc/rdf_utf8_rewrite.h under plain g++ -fsanitize=address,undefined: no HIP, no GPU, no Python in the
// process.  Reads the table tests/utf8_rewrite_ref.py writes, one case a line (byte strings as hex, '-' = empty):
//     replace <search> <replacement> <row> <expected>      translate <matching> <replace> <row> <expected>
//     initcap <row> <expected>                             split <limit> <delim> <row> <expected bytes> <offset,offset,...>
// Every row is produced TWICE through the header, the way the kernels produce it: by the row-at-a-time functions a lane runs
// (utf8_replace_emit, utf8_translate_row, utf8_initcap_row), and by the wave's form — 64 bytes of the row at a time, the
// candidate mask, utf8_select_hits and utf8_window_byte for replace / split, the per-byte emits and a prefix sum for
// translate / initcap.  The sizes come from the size pass's functions first.  Every row, literal and output sits in a heap
// block of exactly its length, so a byte touched outside is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../rust_dataframe_amd/csrc/rdf_utf8_rewrite.h"

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

static void expect(const Bytes& out, const Bytes& exp, const char* what) {
    CHECK(out.n == exp.n, "%s: %lld bytes, expected %lld", what, (long long)out.n, (long long)exp.n);
    if (out.n == exp.n) CHECK(out.n == 0 || memcmp(out.p, exp.p, (size_t)out.n) == 0, "%s: bytes differ", what);
}

// the wave's form of replace / split: returns the hits; out has utf8_replace_bytes of room; offs[j] = where element j begins
static int64_t wave_replace(const Bytes& row, const Bytes& d, const Bytes& rep, int64_t maxhits, Bytes& out, std::vector<int64_t>& offs) {
    const int64_t n = row.n, m = d.n, r = rep.n;
    int64_t allowed = 0, k = 0;
    for (int64_t base = 0; base < n; base += 64) {
        uint64_t cand = 0;
        for (int i = 0; i < 64; ++i) {
            const int64_t q = base + i;
            if (m > 0 && q + m <= n && row.p[q] == d.p[0] && utf8_bytes_at(row.p + q, d.p, m)) cand |= 1ull << i;
        }
        const int64_t k0 = k, end0 = allowed;
        const uint64_t sel = utf8_select_hits(cand, base, m, maxhits, &allowed, &k);
        for (int i = 0; i < 64 && base + i < n; ++i) {
            int64_t h = 0;
            bool covered = false;
            utf8_window_byte(sel, i, base, m, k0, end0, &h, &covered);
            const int64_t q = base + i;
            if ((sel >> i) & 1) {
                const int64_t at = q + (h - 1) * (r - m);
                CHECK(at >= 0 && at + r <= out.n, "a replacement outside the row's output");
                if (at >= 0 && at + r <= out.n) memcpy(out.p + at, rep.p, (size_t)r);
                offs.push_back(at + r);
            } else if (!covered) {
                const int64_t at = q + h * (r - m);
                CHECK(at >= 0 && at < out.n, "a byte outside the row's output");
                if (at >= 0 && at < out.n) out.p[at] = row.p[q];
            }
        }
    }
    return k;
}

template <typename EmitFn>
static void wave_map(const Bytes& row, Bytes& out, EmitFn emit) {
    int64_t o = 0;
    for (int64_t q = 0; q < row.n; ++q) {
        int adv = 0;
        const Utf8Emit e = emit(q, &adv);
        const int len = utf8_emit_len(e);
        CHECK(o + len <= out.n, "an emit outside the row's output");
        if (o + len > out.n) return;
        utf8_emit_put(e, out.p + o);
        o += len;
    }
    CHECK(o == out.n, "the per-byte emits add up to %lld bytes, the row pass to %lld", (long long)o, (long long)out.n);
}

static int table(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { printf("cannot open %s\n", path); return 1; }
    std::vector<char> line(1 << 18);
    long rows[4] = {0, 0, 0, 0};
    Utf8TranslateTable* tt = new Utf8TranslateTable;
    std::string tt_key;
    while (fgets(line.data(), (int)line.size(), f)) {
        ++g_line;
        if (line[0] == '#' || line[0] == '\n') continue;
        std::vector<char*> tok;
        for (char* t = strtok(line.data(), " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        const std::string kind = tok[0];
        if (kind == "replace" && tok.size() == 5) {
            ++rows[0];
            const Bytes d(tok[1]), rep(tok[2]), row(tok[3]), exp(tok[4]);
            const int64_t k = utf8_count_hits(row.p, row.n, d.p, d.n, kUtf8AllHits);
            const int64_t L = utf8_replace_bytes(row.n, k, d.n, rep.n);
            Bytes out(L), out2(L);
            const int64_t w = utf8_replace_emit(row.p, row.n, d.p, d.n, rep.p, rep.n, kUtf8AllHits, out.p, [](int64_t, int64_t) {});
            CHECK(w == L, "replace wrote %lld bytes, sized %lld", (long long)w, (long long)L);
            expect(out, exp, "replace");
            std::vector<int64_t> offs;
            CHECK(wave_replace(row, d, rep, kUtf8AllHits, out2, offs) == k, "the wave's form counts other hits");
            expect(out2, exp, "replace (wave)");
        } else if (kind == "split" && tok.size() == 6) {
            ++rows[3];
            const int64_t limit = atoll(tok[1]);
            const Bytes d(tok[2]), row(tok[3]), exp(tok[4]), none("-");
            std::vector<int64_t> want;
            for (char* t = strtok(tok[5], ","); t; t = strtok(nullptr, ",")) want.push_back(atoll(t));
            const int64_t maxhits = utf8_split_max_hits(limit);
            const int64_t k = utf8_count_hits(row.p, row.n, d.p, d.n, maxhits);
            const int64_t L = utf8_replace_bytes(row.n, k, d.n, 0);
            CHECK(k + 2 == (int64_t)want.size(), "%lld elements, expected %zu", (long long)(k + 1), want.size() - 1);
            Bytes out(L), out2(L);
            std::vector<int64_t> offs(1, 0), offs2(1, 0);
            utf8_replace_emit(row.p, row.n, d.p, d.n, none.p, 0, maxhits, out.p, [&](int64_t j, int64_t o) {
                CHECK(j == (int64_t)offs.size(), "hits out of order");
                offs.push_back(o);
            });
            offs.push_back(L);
            expect(out, exp, "split");
            CHECK(offs == want, "split: the elements' offsets differ");
            CHECK(wave_replace(row, d, none, maxhits, out2, offs2) == k, "the wave's form counts other hits");
            offs2.push_back(L);
            expect(out2, exp, "split (wave)");
            CHECK(offs2 == want, "split (wave): the elements' offsets differ");
        } else if (kind == "translate" && tok.size() == 5) {
            ++rows[1];
            const Bytes m(tok[1]), r(tok[2]), row(tok[3]), exp(tok[4]);
            const std::string key = std::string(tok[1]) + " " + tok[2];
            if (key != tt_key) { utf8_translate_compile(m.p, m.n, r.p, r.n, tt); tt_key = key; }
            const int64_t L = utf8_translate_row(row.p, row.n, *tt, nullptr);
            Bytes out(L), out2(L);
            CHECK(utf8_translate_row(row.p, row.n, *tt, out.p) == L, "the two passes disagree");
            expect(out, exp, "translate");
            wave_map(row, out2, [&](int64_t q, int* adv) { return utf8_translate_emit(row.p, row.n, q, *tt, false, adv); });
            expect(out2, exp, "translate (wave)");
        } else if (kind == "initcap" && tok.size() == 3) {
            ++rows[2];
            const Bytes row(tok[1]), exp(tok[2]);
            const int64_t L = utf8_initcap_row(row.p, row.n, nullptr);
            Bytes out(L), out2(L);
            CHECK(utf8_initcap_row(row.p, row.n, out.p) == L, "the two passes disagree");
            expect(out, exp, "initcap");
            wave_map(row, out2, [&](int64_t q, int* adv) { return utf8_initcap_emit(row.p, row.n, q, false, adv); });
            expect(out2, exp, "initcap (wave)");
        } else {
            CHECK(false, "a line that is no case: %s with %zu fields", tok[0], tok.size());
            break;
        }
    }
    fclose(f);
    delete tt;
    printf("replace %ld, translate %ld, initcap %ld, split %ld rows\n", rows[0], rows[1], rows[2], rows[3]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: %s <table>\n", argv[0]); return 2; }
    if (table(argv[1]) != 0) return 1;
    printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
