// test_textfloat_host.cpp — rust_dataframe_amd/csrc/rdf_textfloat.h under plain g++ with -fsanitize=address,undefined: no HIP,
// no GPU, no Python in the process.  It reads the case table tests/textfloat_ref.py writes (write_case_table) and holds
//   parse    the default routing (fast path, exact path for what it leaves undecided) and the exact path alone to the model's
//            bits; a row flagged "must be undecided" to being undecided by the fast path
//   format   textfloat_length and textfloat_write to the model's bytes
// Every text is parsed out of an exactly sized heap block, every row written into one.
//
//   P f32 family must_be_undecided xTEXT ok bits(hex)
//   F f32 bits(hex) xTEXT
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#define RDF_TF_TABLE_QUAL static
#include "../../rust_dataframe_amd/csrc/rdf_pow10_tables.h"
#include "../../rust_dataframe_amd/csrc/rdf_textfloat.h"

static_assert(kTfPow10TableMin == kTfPow10Min && kTfPow10TableMax == kTfPow10Max && kTfPow10TableExactMax == kTfPow10ExactMax, "rdf_textfloat.h restates the table's range");
static_assert(sizeof(kTfPow10) == sizeof(uint64_t) * kTfPow10Words, "the table's size");

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out;
    auto nib = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (size_t i = 1; i + 1 < s.size(); i += 2) out.push_back((uint8_t)(nib(s[i]) * 16 + nib(s[i + 1])));
    return out;
}

// an exactly sized heap copy of a span (never a null pointer: an empty span still has an address)
struct Exact {
    uint8_t* p;
    size_t n;
    explicit Exact(const std::vector<uint8_t>& v) : p((uint8_t*)malloc(v.size() ? v.size() : 1)), n(v.size()) {
        if (n) memcpy(p, v.data(), n);
    }
    ~Exact() { free(p); }
};

static const char* kFamilies[6] = {"branch", "hard", "longrow", "bits", "human", "long"};

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <case table>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    long nparse[2] = {0, 0}, nformat[2] = {0, 0}, failed = 0;
    long fam_rows[2][6] = {{0}}, fam_undecided[2][6] = {{0}};
    std::string line;
    auto complain = [&](const std::string& what) {
        if (++failed <= 20) std::cout << "FAIL " << what << ": " << line.substr(0, 200) << "\n";
    };
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        if (tag == "P") {
            int f32, fam, must;
            std::string text;
            int ok;
            uint64_t want;
            ss >> f32 >> fam >> must >> text >> ok >> std::hex >> want >> std::dec;
            const Exact t(unhex(text));
            for (int exact_only = 0; exact_only < 2; ++exact_only) {
                uint64_t bits = 0;
                bool und = false;
                const bool got = f32 ? textfloat_parse<true>(kTfPow10, t.p, t.p + t.n, exact_only != 0, &bits, &und)
                                     : textfloat_parse<false>(kTfPow10, t.p, t.p + t.n, exact_only != 0, &bits, &und);
                if (got != (ok != 0)) complain(exact_only ? "exact: ok" : "ok");
                else if (got && bits != want) complain(exact_only ? "exact: bits" : "bits");
                if (!exact_only) {
                    if (must && !und) complain("decided by the fast path");
                    ++fam_rows[f32][fam];
                    fam_undecided[f32][fam] += und;
                }
            }
            ++nparse[f32];
        } else if (tag == "F") {
            int f32;
            uint64_t bits;
            std::string text;
            ss >> f32 >> std::hex >> bits >> std::dec >> text;
            const std::vector<uint8_t> want = unhex(text);
            const int n = f32 ? textfloat_length<true>(kTfPow10, bits) : textfloat_length<false>(kTfPow10, bits);
            if (n != (int)want.size() || n > (f32 ? kTfMaxRowF32 : kTfMaxRowF64)) complain("length");
            else {
                const Exact out(std::vector<uint8_t>((size_t)n, 0xEE));
                const uint8_t* end = f32 ? textfloat_write<true>(kTfPow10, bits, out.p) : textfloat_write<false>(kTfPow10, bits, out.p);
                if (end != out.p + n || memcmp(out.p, want.data(), (size_t)n) != 0) complain("bytes");
            }
            ++nformat[f32];
        } else if (!tag.empty()) {
            complain("unknown line");
        }
    }
    for (int f32 = 0; f32 < 2; ++f32)
        for (int k = 0; k < 6; ++k)
            if (fam_rows[f32][k])
                printf("undecided %s %s: %ld of %ld rows (%.4f %%)\n", f32 ? "f32" : "f64", kFamilies[k], fam_undecided[f32][k], fam_rows[f32][k],
                       100.0 * (double)fam_undecided[f32][k] / (double)fam_rows[f32][k]);
    printf("parse: f64 %ld, f32 %ld rows; format: f64 %ld, f32 %ld rows; %ld failed\n", nparse[0], nparse[1], nformat[0], nformat[1], failed);
    return failed ? 1 : 0;
}
