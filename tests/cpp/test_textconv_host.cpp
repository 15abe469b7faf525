// test_textconv_host.cpp — rust_dataframe_amd/csrc/rdf_textconv.h under plain g++ with -fsanitize=address,undefined: no HIP,
// no GPU, no Python in the process.  It reads the case table tests/textconv_ref.py writes (write_case_table) and holds every
// textconv_parse_* / textconv_length / textconv_write result to the model's.  Every span is copied into an exactly sized
// heap block, so a read before or past it is caught; every row is written into an exactly sized block, so is a stray write.
//
//   P kind unit dtype xPATTERN xTEXT ok value
//   F kind unit dtype xPATTERN value xTEXT
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../rust_dataframe_amd/csrc/rdf_textconv.h"

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

static bool parse_one(int kind, int unit, int dtype, const TcPattern* pt, const uint8_t* b, const uint8_t* e, int64_t* value) {
    if (kind == TC_BOOL) {
        bool v = false;
        const bool ok = textconv_parse_bool(b, e, &v);
        *value = v;
        return ok;
    }
    if (kind == TC_INT) {
        uint64_t bits = 0;
        const bool ok = textconv_parse_int(b, e, dtype, &bits);
        *value = (int64_t)bits;   // (UInt64 values beyond Int64 come back as their two's complement: the table writes them so)
        return ok;
    }
    if (kind == TC_DATE) {
        int32_t d = 0;
        const bool ok = pt ? textconv_parse_date_pattern(*pt, b, e, &d) : textconv_parse_date(b, e, &d);
        *value = d;
        return ok;
    }
    return pt ? textconv_parse_timestamp_pattern(*pt, b, e, unit, value) : textconv_parse_timestamp(b, e, unit, value);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <case table>\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    long counts[2][TC_NKINDS] = {{0}}, failed = 0;
    std::map<std::string, TcPattern> compiled[2];
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string dir, pat_hex, a, b;
        int kind, unit, dtype;
        ls >> dir >> kind >> unit >> dtype >> pat_hex;
        const bool parse = dir == "P";
        const TcPattern* pt = nullptr;
        if (pat_hex.size() > 1) {
            auto& cache = compiled[parse ? 1 : 0];
            auto it = cache.find(pat_hex);
            if (it == cache.end()) {
                const std::vector<uint8_t> raw = unhex(pat_hex);
                Exact px(raw);
                TcPattern t;
                int64_t pos = 0;
                const int err = textconv_compile(px.p, (int64_t)px.n, parse, &t, &pos);
                if (err != TC_OK) {
                    printf("FAIL the pattern of line `%s` does not compile: %s at %lld\n", line.c_str(), textconv_compile_message(err), (long long)pos);
                    return 1;
                }
                it = cache.emplace(pat_hex, t).first;
            }
            pt = &it->second;
        }
        ++counts[parse ? 0 : 1][kind];
        if (parse) {
            std::string text_hex;
            int ok_exp;
            long long val_exp;
            ls >> text_hex >> ok_exp >> val_exp;
            Exact tx(unhex(text_hex));
            int64_t got = 0;
            const bool ok = parse_one(kind, unit, dtype, pt, tx.p, tx.p + tx.n, &got);
            uint64_t exp_bits = (uint64_t)val_exp;
            if (kind == TC_INT && dtype == TC_DT_U64) exp_bits = strtoull(line.substr(line.rfind(' ') + 1).c_str(), nullptr, 10);
            if (ok != (ok_exp != 0) || (ok && (uint64_t)got != exp_bits)) {
                if (++failed <= 20) printf("FAIL %s -> ok %d value %lld\n", line.c_str(), (int)ok, (long long)got);
            }
        } else {
            std::string val_s, text_hex;
            ls >> val_s >> text_hex;
            const uint64_t bits = val_s[0] == '-' ? (uint64_t)strtoll(val_s.c_str(), nullptr, 10) : strtoull(val_s.c_str(), nullptr, 10);
            const std::vector<uint8_t> exp = unhex(text_hex);
            const int len = textconv_length(kind, dtype, unit, pt, bits);
            std::vector<uint8_t> none((size_t)(len > 0 ? len : 0));
            Exact out(none);
            uint8_t* end = len >= 0 ? textconv_write(kind, dtype, unit, pt, bits, out.p) : out.p;
            if (len != (int)exp.size() || end != out.p + len || memcmp(out.p, exp.data(), exp.size()) != 0 ||
                len > textconv_max_row_bytes(kind, unit, pt)) {
                if (++failed <= 20) printf("FAIL %s -> %d bytes `%.*s`\n", line.c_str(), len, len, (const char*)out.p);
            }
        }
    }
    printf("parse: bool %ld, int %ld, date %ld, timestamp %ld rows; format: bool %ld, int %ld, date %ld, timestamp %ld rows; %ld failed\n",
           counts[0][0], counts[0][1], counts[0][2], counts[0][3], counts[1][0], counts[1][1], counts[1][2], counts[1][3], failed);
    return failed ? 1 : 0;
}
