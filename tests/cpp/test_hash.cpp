// The hashes of rust_dataframe_amd/csrc/rdf_hash.h (the functions the kernels call) on the CPU, as a filter: one request per
// line of standard input, one answer per line of standard output, every number in hexadecimal.
//   U <hex bytes>        the hash of a Utf8 row ("-" = the empty row)
//   T <bits> <bits> ...  the hash of a key tuple, given as the columns' order-preserving key bits
//   M <x>  /  J <x>      mix64(x)  /  join_mix(x)
//   K                    kCsEmpty kCsLongRow kCsStreams
// tests/test_hash_models.py holds the Python models of tests/hash_models.py, and every collision they construct, to it.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../rust_dataframe_amd/csrc/rdf_hash.h"

using namespace rdfk;

namespace {
int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line.substr(1));
        std::string tok;
        if (line[0] == 'U') {
            in >> tok;
            std::vector<uint8_t> row;
            if (tok != "-") {
                if (tok.size() % 2) return 2;
                for (size_t i = 0; i < tok.size(); i += 2) {
                    const int hi = nibble(tok[i]), lo = nibble(tok[i + 1]);
                    if (hi < 0 || lo < 0) return 2;
                    row.push_back((uint8_t)(hi * 16 + lo));
                }
            }
            // an exact-size copy: a read past the row's end is a read past the allocation
            uint8_t* p = (uint8_t*)std::malloc(row.size() ? row.size() : 1);
            for (size_t i = 0; i < row.size(); ++i) p[i] = row[i];
            std::printf("%" PRIx64 "\n", cs_row_hash(p, (int32_t)row.size()));
            std::free(p);
        } else if (line[0] == 'T') {
            std::vector<uint64_t> bits;
            while (in >> tok) bits.push_back(std::strtoull(tok.c_str(), nullptr, 16));
            if (bits.empty() || bits.size() > 4) return 2;
            std::printf("%" PRIx64 "\n", join_tuple_hash(bits.data(), (int)bits.size()));
        } else if (line[0] == 'M' || line[0] == 'J') {
            in >> tok;
            const uint64_t x = std::strtoull(tok.c_str(), nullptr, 16);
            std::printf("%" PRIx64 "\n", line[0] == 'M' ? mix64(x) : join_mix(x));
        } else if (line[0] == 'K') {
            std::printf("%" PRIx64 " %x %x\n", kCsEmpty, (unsigned)kCsLongRow, (unsigned)kCsStreams);
        } else return 2;
    }
    return 0;
}
