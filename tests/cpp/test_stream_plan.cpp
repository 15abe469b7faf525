// The host logic of the streamed batch loop (rust_dataframe_amd/csrc/rdf_stream_plan.h) on the CPU, no library linked:
//   * stream_plan_build over seeded random layouts — 1-6 columns of every element width and BOOL, validity present or absent,
//     a different offset on every batch, batch lengths around every byte / tile / piece boundary and one batch many pieces long,
//     slabs from 4 KiB to 2 MiB, page-locked or pageable per buffer.  The upload is emulated (every item's bytes to its dev_off in
//     a fake slab) and every view is read back through values_item / values_off / dev_off / offset: every row of every batch exactly
//     once, in batch order, with its value and validity bit; items disjoint, staged ones in [0, pin_bytes), direct ones behind on
//     256-byte boundaries; a merged run only over bytes that are contiguous in the caller's memory; a slab over budget only when it
//     is one piece; plan.max_* bound (and are reached by) the slabs.
//   * DownLayout: destinations disjoint, offsets inside `dev`, merged direct runs contiguous in the caller's memory, a staged
//     validity item between two direct value items.
//   * bits_append against a per-bit loop for every source phase, destination phase and length up to 300 bits.
// Source buffers are allocated at their exact size: built with -fsanitize=address,undefined a read past a column's end is an error.
#include <array>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>

#include "mini_test.hpp"
#include "../../rust_dataframe_amd/csrc/rdf_stream_plan.h"

namespace {

using Rng = std::mt19937_64;

struct Layout {
    int ncols = 0;
    int64_t nchunks = 0;
    size_t S = 0, extra = 0;
    std::vector<rdf_array> cols;                          // [k * nchunks + c]
    std::vector<std::unique_ptr<uint8_t[]>> bufs;         // exact-size storage
    std::map<const void*, bool> pinned;
    bool asked_unknown = false;
    uint8_t* alloc(Rng& g, size_t n, bool pin) {
        bufs.emplace_back(new uint8_t[n]);
        uint8_t* p = bufs.back().get();
        uint64_t x = g() | 1;                                  // xorshift: the bytes only have to differ from place to place
        for (size_t i = 0; i < n; i += 8) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; memcpy(p + i, &x, std::min<size_t>(8, n - i)); }
        pinned[p] = pin;
        return p;
    }
};

const int kDtypes[] = {RDF_I8, RDF_I16, RDF_I32, RDF_I64, RDF_U8, RDF_U16, RDF_U32, RDF_U64, RDF_F32, RDF_F64, RDF_BOOL};
const size_t kSlabs[] = {4 << 10, 8 << 10, 16 << 10, 64 << 10, 200 << 10, 256 << 10, 1 << 20, (5 << 20) / 4, 2 << 20};
const int64_t kLens[] = {0, 1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049};

size_t es_of(int dt) { return dt == RDF_I8 || dt == RDF_U8 ? 1 : dt == RDF_I16 || dt == RDF_U16 ? 2 : dt == RDF_I32 || dt == RDF_U32 || dt == RDF_F32 ? 4 : dt == RDF_BOOL ? 0 : 8; }
size_t value_bytes(int dt, int64_t rows) { return dt == RDF_BOOL ? (size_t)(rows + 7) / 8 : (size_t)rows * es_of(dt); }
bool bit(const uint8_t* p, int64_t i) { return (p[i >> 3] >> (i & 7)) & 1; }
// bits [doff, doff + n) of d against bits [soff, soff + n) of s, bit by bit (whole bytes at once where both sides are on one); *zeros: zero bits of d
bool same_bits(const uint8_t* d, int64_t doff, const uint8_t* s, int64_t soff, int64_t n, int64_t* zeros) {
    for (int64_t i = 0; i < n;) {
        if (((doff + i) & 7) == 0 && ((soff + i) & 7) == 0 && n - i >= 8) {
            const uint8_t x = d[(doff + i) >> 3];
            if (x != s[(soff + i) >> 3]) return false;
            *zeros += 8 - __builtin_popcount(x);
            i += 8;
        } else {
            if (bit(d, doff + i) != bit(s, soff + i)) return false;
            *zeros += !bit(d, doff + i);
            ++i;
        }
    }
    return true;
}
int64_t zero_bits(const uint8_t* p, int64_t from, int64_t n) { int64_t z = 0; for (int64_t i = 0; i < n; ++i) z += !bit(p, from + i); return z; }

// every batch in buffers of its own, at an offset of its own
Layout private_buffers(Rng& g) {
    Layout L;
    L.ncols = 1 + (int)(g() % 6);
    L.nchunks = 1 + (int64_t)(g() % 12);
    L.S = kSlabs[g() % (sizeof kSlabs / sizeof *kSlabs)];
    L.extra = (g() % 3 == 0) ? 1 + g() % 9 : 0;
    std::vector<int> dt((size_t)L.ncols);
    std::vector<int> nullable((size_t)L.ncols);          // 0 never, 1 always, 2 per batch
    size_t row_bytes = L.extra;
    for (int k = 0; k < L.ncols; ++k) { dt[(size_t)k] = kDtypes[g() % 11]; nullable[(size_t)k] = (int)(g() % 3); row_bytes += std::max<size_t>(1, es_of(dt[(size_t)k])); }
    std::vector<int64_t> len((size_t)L.nchunks);
    for (auto& n : len) n = g() % 4 == 0 ? (int64_t)(g() % 3000) : kLens[g() % (sizeof kLens / sizeof *kLens)];
    // one batch many pieces long (a piece is about a quarter slab of rows, never below 1024)
    const double u = (double)(g() % 1000) / 1000.0;
    int64_t longest = (int64_t)((double)(L.S / (row_bytes + 1)) * (0.3 + 1.5 * u));
    longest = std::min<int64_t>(300000, std::max<int64_t>(3000 + (int64_t)(g() % 9000), longest));
    len[g() % (size_t)L.nchunks] = longest + (int64_t)(g() % 3) - 1;
    L.cols.resize((size_t)L.ncols * (size_t)L.nchunks);
    for (int k = 0; k < L.ncols; ++k)
        for (int64_t c = 0; c < L.nchunks; ++c) {
            rdf_array a{};
            a.offset = (int64_t)(g() % 16);
            a.length = len[(size_t)c];
            a.dtype = dt[(size_t)k];
            a.mem = RDF_MEM_HOST;
            a.values = L.alloc(g, value_bytes(a.dtype, a.offset + a.length), g() % 2);
            const bool has = nullable[(size_t)k] == 1 || (nullable[(size_t)k] == 2 && g() % 2);
            uint8_t* v = has ? L.alloc(g, (size_t)(a.offset + a.length + 7) / 8, g() % 2) : nullptr;
            a.validity = v;
            a.null_count = !has ? 0 : g() % 2 ? -1 : zero_bits(v, a.offset, a.length);
            L.cols[(size_t)k * (size_t)L.nchunks + (size_t)c] = a;
        }
    return L;
}

// every column ONE buffer, its batches slices of it (the same base pointer, a growing offset): consecutive, or with a gap
Layout sliced_columns(Rng& g) {
    Layout L;
    L.ncols = g() % 2 ? 1 : 1 + (int)(g() % 3);
    L.nchunks = 2 + (int64_t)(g() % 6);
    const size_t big[] = {(5 << 20) / 4, (3 << 20) / 2, 2 << 20};
    L.S = big[g() % 3];
    L.extra = g() % 4 == 0 ? 9 : 0;
    const int64_t shapes[] = {32768, 35840, 40008, 65536, 71680, 1000, 229376, 0, 143360, 100000}, odd[] = {40001, 35843, 7};
    std::vector<int64_t> len((size_t)L.nchunks), gap((size_t)L.nchunks);
    for (auto& n : len) n = g() % 8 ? shapes[g() % 10] : odd[g() % 3];       // (after an odd length no later batch starts on a byte of its bitmap)
    for (auto& x : gap) x = g() % 5 == 0 ? 1 + (int64_t)(g() % 100) : 0;
    gap[0] = g() % 2 ? 0 : (int64_t)(g() % 6);
    L.cols.resize((size_t)L.ncols * (size_t)L.nchunks);
    for (int k = 0; k < L.ncols; ++k) {
        const int dt = g() % 3 ? (g() % 2 ? RDF_F64 : RDF_I64) : kDtypes[g() % 11];
        int64_t total = 0;
        for (int64_t c = 0; c < L.nchunks; ++c) total += gap[(size_t)c] + len[(size_t)c];
        const uint8_t* vals = L.alloc(g, value_bytes(dt, total), g() % 4 != 0);
        const uint8_t* valid = g() % 2 ? L.alloc(g, (size_t)(total + 7) / 8, g() % 2) : nullptr;
        int64_t at = 0;
        for (int64_t c = 0; c < L.nchunks; ++c) {
            at += gap[(size_t)c];
            rdf_array a{};
            a.values = vals; a.validity = valid; a.offset = at; a.length = len[(size_t)c]; a.dtype = dt; a.mem = RDF_MEM_HOST;
            a.null_count = !valid ? 0 : g() % 2 ? -1 : zero_bits(valid, at, a.length);
            at += a.length;
            L.cols[(size_t)k * (size_t)L.nchunks + (size_t)c] = a;
        }
    }
    return L;
}

struct Tally { int64_t slabs = 0, pieces = 0, direct_items = 0, merged_views = 0, staged_items = 0, over_budget = 0; };

void check_layout(Layout& L, Tally& t) {
    StreamPlan plan;
    int bad = -1;
    const StreamPlanError e = stream_plan_build(L.cols.data(), L.ncols, L.nchunks, L.extra, L.S,
                                                [&](const void* p) { auto it = L.pinned.find(p); if (it == L.pinned.end()) { L.asked_unknown = true; return false; } return it->second; },
                                                plan, &bad);
    CHECK_EQ(e, kStreamPlanOk);
    CHECK(!L.asked_unknown);                   // the question is asked of the buffers the caller named, nothing else
    CHECK_EQ(plan.slabs.size(), plan.origin.size());
    const size_t nc = (size_t)L.ncols;
    int64_t next_chunk = 0, next_row = 0;      // the next row a piece must start at
    size_t seen_pin = 0, seen_dev = 0;
    int64_t seen_rows = 0, seen_pieces = 0;
    for (size_t si = 0; si < plan.slabs.size(); ++si) {
        const StreamSlab& s = plan.slabs[si];
        const std::vector<PieceOrigin>& org = plan.origin[si];
        ++t.slabs;
        CHECK(s.npieces >= 1);
        CHECK_EQ((size_t)s.npieces, org.size());
        CHECK_EQ(s.views.size(), nc * (size_t)s.npieces);
        CHECK_EQ(s.values_item.size(), s.views.size()); CHECK_EQ(s.validity_item.size(), s.views.size());
        CHECK_EQ(s.values_off.size(), s.views.size()); CHECK_EQ(s.validity_off.size(), s.views.size());
        CHECK(s.pin_bytes <= s.dev_bytes);
        // the upload, emulated: every item's bytes to its place, no byte of the slab written twice
        std::vector<uint8_t> dev(s.dev_bytes + 64, 0xEE);
        std::vector<std::pair<size_t, size_t>> spans;
        for (const StreamItem& it : s.items) {
            CHECK(it.dev_off + it.bytes <= s.dev_bytes);
            if (it.direct) { CHECK(it.dev_off >= s.pin_bytes); CHECK_EQ(it.dev_off & 255, (size_t)0); CHECK(it.bytes >= kSmallCopy); ++t.direct_items; }
            else { CHECK_EQ(it.dev_off, it.pin_off); CHECK(it.pin_off + it.bytes <= s.pin_bytes); CHECK_EQ(it.pin_off & 63, (size_t)0); ++t.staged_items; }
            if (it.bytes) { memcpy(dev.data() + it.dev_off, it.src, it.bytes); spans.emplace_back(it.dev_off, it.dev_off + it.bytes); }
        }
        std::sort(spans.begin(), spans.end());
        for (size_t i = 1; i < spans.size(); ++i) CHECK(spans[i - 1].second <= spans[i].first);      // no byte of the slab belongs to two items
        for (size_t b = s.dev_bytes; b < dev.size(); ++b) CHECK_EQ(dev[b], 0xEE);
        int64_t rows = 0;
        size_t budget = 0;
        for (int64_t p = 0; p < s.npieces; ++p) {
            const PieceOrigin& o = org[(size_t)p];
            ++t.pieces;
            // exactly once, in batch order: this piece starts where the one before it ended (empty batches have no piece)
            while (next_chunk < L.nchunks && next_row == L.cols[(size_t)next_chunk].length) { ++next_chunk; next_row = 0; }
            CHECK_EQ(o.chunk, next_chunk);
            CHECK_EQ(o.row0, next_row);
            CHECK(o.rows >= 1 && o.row0 + o.rows <= L.cols[(size_t)o.chunk].length);
            CHECK_EQ(o.row0 % 1024, 0);        // a long batch is cut on 1024-row boundaries
            next_row += o.rows;
            rows += o.rows;
            budget += (size_t)o.rows * L.extra;
            for (size_t k = 0; k < nc; ++k) {
                const rdf_array& a = L.cols[k * (size_t)L.nchunks + (size_t)o.chunk];
                const size_t vix = (size_t)p * nc + k;
                const rdf_array& v = s.views[vix];
                CHECK_EQ(v.length, o.rows); CHECK_EQ(v.dtype, a.dtype); CHECK_EQ(v.mem, (int32_t)RDF_MEM_DEVICE);
                CHECK(v.offset >= 0 && v.offset < 8);
                CHECK_EQ(v.offset, (a.offset + o.row0) & 7);
                const int64_t first = a.offset + o.row0;           // the piece's first row inside the caller's buffer
                const size_t es = es_of(a.dtype);
                // values
                CHECK(s.values_item[vix] < s.items.size());
                const StreamItem& vit = s.items[s.values_item[vix]];
                const size_t voff = s.values_off[vix];
                const size_t vbytes = a.dtype == RDF_BOOL ? (size_t)((v.offset + o.rows + 7) >> 3) : (size_t)(v.offset + o.rows) * es;
                const char* vsrc = (const char*)a.values + (a.dtype == RDF_BOOL ? (size_t)((first - v.offset) >> 3) : (size_t)(first - v.offset) * es);
                CHECK(voff + vbytes <= vit.bytes);
                CHECK(vit.src + voff == vsrc);                     // a (merged) item covers this piece only where the caller's memory is contiguous
                CHECK_EQ((vit.dev_off + voff) & 63, (size_t)0);
                if (voff) { CHECK(vit.direct); CHECK_EQ(voff & 255, (size_t)0); ++t.merged_views; }
                budget += vbytes + 256;
                const uint8_t* dv = dev.data() + vit.dev_off + voff;
                if (a.dtype == RDF_BOOL) { int64_t z = 0; CHECK(same_bits(dv, v.offset, (const uint8_t*)a.values, first, o.rows, &z)); }
                else CHECK(memcmp(dv + (size_t)v.offset * es, (const char*)a.values + (size_t)first * es, (size_t)o.rows * es) == 0);
                // validity
                if (!a.validity) { CHECK_EQ(s.validity_item[vix], kNoItem); CHECK_EQ(v.null_count, 0); }
                else {
                    CHECK(s.validity_item[vix] < s.items.size());
                    const StreamItem& bit_it = s.items[s.validity_item[vix]];
                    const size_t boff = s.validity_off[vix];
                    const size_t bbytes = (size_t)((v.offset + o.rows + 7) >> 3);
                    CHECK(boff + bbytes <= bit_it.bytes);
                    CHECK(bit_it.src + boff == (const char*)a.validity + ((first - v.offset) >> 3));
                    CHECK_EQ((bit_it.dev_off + boff) & 63, (size_t)0);
                    if (boff) { CHECK(bit_it.direct); CHECK_EQ(boff & 255, (size_t)0); ++t.merged_views; }
                    budget += bbytes + 256;
                    const uint8_t* db = dev.data() + bit_it.dev_off + boff;
                    int64_t zeros = 0;
                    CHECK(same_bits(db, v.offset, a.validity, first, o.rows, &zeros));
                    if (v.null_count >= 0 && a.null_count >= 0) CHECK_EQ(v.null_count, zeros);     // a known count is the true one
                    if (a.null_count < 0) CHECK_EQ(v.null_count, -1);
                }
            }
        }
        if (budget > L.S) { CHECK_EQ(s.npieces, 1); ++t.over_budget; }          // over budget only as a single piece
        CHECK(s.pin_bytes <= plan.max_pin); CHECK(s.dev_bytes <= plan.max_dev); CHECK(rows <= plan.max_rows); CHECK(s.npieces <= plan.max_pieces);
        seen_pin = std::max(seen_pin, s.pin_bytes); seen_dev = std::max(seen_dev, s.dev_bytes);
        seen_rows = std::max(seen_rows, rows); seen_pieces = std::max(seen_pieces, s.npieces);
    }
    while (next_chunk < L.nchunks && next_row == L.cols[(size_t)next_chunk].length) { ++next_chunk; next_row = 0; }
    CHECK_EQ(next_chunk, L.nchunks);           // every row of every batch
    CHECK_EQ(seen_pin, plan.max_pin); CHECK_EQ(seen_dev, plan.max_dev); CHECK_EQ(seen_rows, plan.max_rows); CHECK_EQ(seen_pieces, plan.max_pieces);
}

}  // namespace

TEST(plans_over_batches_in_buffers_of_their_own) {
    Rng g(20240611);
    Tally t;
    for (int rep = 0; rep < 2000; ++rep) { Layout L = private_buffers(g); check_layout(L, t); }
    std::printf("     %lld slabs, %lld pieces, %lld staged and %lld direct items, %lld single pieces over budget\n", (long long)t.slabs, (long long)t.pieces, (long long)t.staged_items, (long long)t.direct_items, (long long)t.over_budget);
    CHECK(t.slabs > 10000 && t.direct_items > 50 && t.over_budget > 0);        // the generator reaches every kind of slab
}

TEST(plans_over_slices_of_one_buffer_per_column) {
    Rng g(77);
    Tally t;
    for (int rep = 0; rep < 500; ++rep) { Layout L = sliced_columns(g); check_layout(L, t); }
    std::printf("     %lld slabs, %lld pieces, %lld staged and %lld direct items, %lld views inside a merged run\n", (long long)t.slabs, (long long)t.pieces, (long long)t.staged_items, (long long)t.direct_items, (long long)t.merged_views);
    CHECK(t.direct_items > 300 && t.merged_views > 100 && t.staged_items > 300);
}

TEST(a_run_merges_only_what_is_contiguous_and_256_byte_sized) {
    // one page-locked f64 column, slab 1.25 MiB: pieces of 35 840 rows = 280 KiB travel on their own
    Rng g(5);
    auto direct_items = [&](const std::vector<int64_t>& len, const std::vector<int64_t>& start, bool pin, size_t* slabs, size_t S = (5 << 20) / 4) {
        Layout L;
        L.ncols = 1; L.nchunks = (int64_t)len.size(); L.S = S; L.extra = 0;
        int64_t total = 0;
        for (size_t c = 0; c < len.size(); ++c) total = std::max(total, start[c] + len[c]);
        const uint8_t* vals = L.alloc(g, (size_t)total * 8, pin);
        for (size_t c = 0; c < len.size(); ++c) { rdf_array a{}; a.values = vals; a.offset = start[c]; a.length = len[c]; a.dtype = RDF_F64; a.mem = RDF_MEM_HOST; L.cols.push_back(a); }
        Tally t;
        check_layout(L, t);
        StreamPlan plan;
        CHECK_EQ(stream_plan_build(L.cols.data(), 1, L.nchunks, 0, L.S, [&](const void* p) { return L.pinned[p]; }, plan, nullptr), kStreamPlanOk);
        *slabs = plan.slabs.size();
        size_t n = 0;
        for (const StreamSlab& s : plan.slabs) for (const StreamItem& it : s.items) n += it.direct;
        return n;
    };
    size_t slabs = 0;
    // four consecutive 35 840-row slices: a slab holds up to four such pieces (4 x (280 KiB + 256) <= 1.25 MiB), one copy per slab
    CHECK_EQ(direct_items({35840, 35840, 35840, 35840}, {0, 35840, 71680, 107520}, true, &slabs), slabs);
    CHECK_EQ(slabs, (size_t)1);
    // 40 001 rows: 35 840 + 4161 rows each; the tails are staged, and a staged item ends the run
    CHECK_EQ(direct_items({40001, 40001, 40001}, {0, 40001, 80002}, true, &slabs), (size_t)3);
    // 40 008 rows at 2 MiB (pieces of 57 344 rows): every batch one piece that starts at its predecessor's end, but 320 064 bytes
    // are no multiple of 256 — merged, the second would start off a 256-byte boundary in HBM
    CHECK_EQ(direct_items({40008, 40008, 40008}, {0, 40008, 80016}, true, &slabs, 2 << 20), (size_t)3);
    CHECK_EQ(slabs, (size_t)1);
    CHECK_EQ(direct_items({40960, 40960, 40960}, {0, 40960, 81920}, true, &slabs, 2 << 20), (size_t)1);
    // offsets 3 and 5: a piece's byte-rounded start (row 0 of its byte) lies before the previous batch's end
    CHECK_EQ(direct_items({35840, 35840, 35840}, {3, 35843, 71683}, true, &slabs), (size_t)3);
    // a gap between the slices
    CHECK_EQ(direct_items({35840, 35840, 35840}, {0, 35848, 71696}, true, &slabs), (size_t)3);
    // pageable memory: nothing travels on its own
    CHECK_EQ(direct_items({35840, 35840, 35840}, {0, 35840, 71680}, false, &slabs), (size_t)0);
}

TEST(mismatched_batches_are_refused) {
    Rng g(9);
    Layout L = private_buffers(g);
    while (L.ncols < 2) L = private_buffers(g);
    StreamPlan plan;
    int bad = -1;
    auto no = [](const void*) { return false; };
    L.cols[(size_t)L.nchunks].length += 1;                 // column 1, batch 0
    CHECK_EQ(stream_plan_build(L.cols.data(), L.ncols, L.nchunks, 0, L.S, no, plan, &bad), kStreamPlanLengths);
    L.cols[(size_t)L.nchunks].length -= 1;
    if (L.nchunks > 1) {
        rdf_array& a = L.cols[(size_t)L.nchunks + 1];
        a.dtype = a.dtype == RDF_I8 ? RDF_U8 : RDF_I8;
        StreamPlan p2;
        CHECK_EQ(stream_plan_build(L.cols.data(), L.ncols, L.nchunks, 0, L.S, no, p2, &bad), kStreamPlanDtypes);
        CHECK_EQ(bad, 1);
    }
}

// ---- the way back
namespace {

struct Dest { std::vector<uint8_t> mem; bool pinned; };

// adds as pipeline_stream_store makes them; then the kernel's writes, the copies and the unpacking, emulated
void check_down(std::vector<Dest>& dests, const std::vector<std::array<size_t, 3>>& adds /* dest, offset, bytes */, size_t* ncopies, size_t* ndirect) {
    DownLayout lay([&](const void* p) { for (const Dest& d : dests) if (d.mem.data() == p) return d.pinned; throw Failure{"asked about a pointer that is no destination's base"}; });
    lay.reset();
    std::vector<size_t> idx;
    for (const auto& a : adds) idx.push_back(lay.add((char*)dests[a[0]].mem.data() + a[1], a[2], dests[a[0]].mem.data()));
    lay.close();
    CHECK(lay.pin <= lay.dev);
    // every item has a place of its own inside [0, dev); staged ones inside [0, pin)
    std::vector<uint8_t> dev(lay.dev + 64, 0xEE), used(lay.dev + 64, 0);
    for (size_t i = 0; i < adds.size(); ++i) {
        const DownItem& it = lay.items[idx[i]];
        CHECK_EQ(it.bytes, adds[i][2]);
        CHECK(it.off + it.bytes <= lay.dev);
        CHECK_EQ(it.off & 255, (size_t)0);                 // what a kernel writes starts on a 256-byte boundary
        if (!it.direct) CHECK(it.off + it.bytes <= lay.pin); else CHECK(it.off >= lay.pin);
        for (size_t b = 0; b < it.bytes; ++b) { CHECK(!used[it.off + b]); used[it.off + b] = 1; dev[it.off + b] = (uint8_t)(i * 31 + b * 7 + 1); }
    }
    // the staged region in one copy, then unpacked item by item; the direct copies out of the slab's buffer
    std::vector<uint8_t> stage(dev.begin(), dev.begin() + (std::ptrdiff_t)lay.pin);
    std::vector<std::vector<uint8_t>> expect;
    for (const Dest& d : dests) expect.push_back(d.mem);
    for (size_t i = 0; i < adds.size(); ++i) for (size_t b = 0; b < adds[i][2]; ++b) expect[adds[i][0]][adds[i][1] + b] = (uint8_t)(i * 31 + b * 7 + 1);
    *ncopies = lay.copies.size(); *ndirect = 0;
    size_t copied = 0;
    for (const DownItem& c : lay.copies) {
        bool inside = false;
        for (const Dest& d : dests) inside = inside || ((uint8_t*)c.dst >= d.mem.data() && (uint8_t*)c.dst + c.bytes <= d.mem.data() + d.mem.size());
        CHECK(inside);
        if (c.direct) { CHECK(c.off + c.bytes <= lay.dev); CHECK_EQ(c.off & 255, (size_t)0); if (c.bytes) memcpy(c.dst, dev.data() + c.off, c.bytes); ++*ndirect; }
        else { CHECK(c.off + c.bytes <= lay.pin); if (c.bytes) memcpy(c.dst, stage.data() + c.off, c.bytes); }
        copied += c.bytes;
    }
    size_t asked = 0;
    for (const auto& a : adds) asked += a[2];
    CHECK_EQ(copied, asked);                               // disjoint destinations: every byte travels once
    for (size_t d = 0; d < dests.size(); ++d) CHECK(dests[d].mem == expect[d]);     // every byte in place, nothing else touched
}

}  // namespace

TEST(down_layout_staged_validity_between_direct_values) {
    // four 35 840-row f64 pieces of one page-locked output column (280 KiB each) with their bitmaps (4480 bytes: staged)
    std::vector<Dest> d(2);
    d[0].mem.assign(4 * 286720 + 64, 0xAB); d[0].pinned = true;
    d[1].mem.assign(4 * 4480 + 64, 0xCD); d[1].pinned = true;
    std::vector<std::array<size_t, 3>> adds;
    for (size_t p = 0; p < 4; ++p) { adds.push_back({0, p * 286720, 286720}); adds.push_back({1, p * 4480, 4480}); }
    size_t copies = 0, direct = 0;
    check_down(d, adds, &copies, &direct);
    CHECK_EQ(direct, (size_t)1);                           // the values leave as ONE run although a staged item lies between its parts
    CHECK_EQ(copies, (size_t)5);
    // 40 001 rows: 320 008 bytes are no multiple of 256 — every piece a copy of its own
    d[0].mem.assign(3 * 320008 + 64, 0xAB);
    adds.clear();
    for (size_t p = 0; p < 3; ++p) adds.push_back({0, p * 320008, 320008});
    check_down(d, adds, &copies, &direct);
    CHECK_EQ(direct, (size_t)3);
    // a gap in the caller's memory ends the run; pageable memory is staged whatever its size
    d[0].mem.assign(4 * 286720 + 64, 0xAB);
    adds = {{0, 0, 286720}, {0, 286720, 286720}, {0, 2 * 286720 + 8, 286720}};
    check_down(d, adds, &copies, &direct);
    CHECK_EQ(direct, (size_t)2);
    d[0].pinned = false;
    check_down(d, adds, &copies, &direct);
    CHECK_EQ(direct, (size_t)0);
    CHECK_EQ(copies, (size_t)3);
}

TEST(down_layouts_at_random) {
    Rng g(31);
    size_t merged = 0, all_direct = 0;
    for (int rep = 0; rep < 400; ++rep) {
        const size_t nd = 1 + g() % 4;
        std::vector<Dest> d(nd);
        std::vector<size_t> at(nd, 0);
        std::vector<std::array<size_t, 3>> adds;
        const size_t n = 1 + g() % 14;
        const size_t sizes[] = {0, 1, 128, 1024, 4480, 8192, 262143, 262144, 262400, 286720, 320008, 524288};
        for (size_t i = 0; i < n; ++i) {
            const size_t k = g() % nd, bytes = sizes[g() % 12];
            if (g() % 5 == 0) at[k] += 1 + g() % 300;      // a gap
            adds.push_back({k, at[k], bytes});
            at[k] += bytes;
        }
        for (size_t k = 0; k < nd; ++k) { d[k].mem.assign(at[k] + 32, (uint8_t)(0xA0 + k)); d[k].pinned = g() % 3 != 0; }
        size_t copies = 0, direct = 0, direct_adds = 0;
        check_down(d, adds, &copies, &direct);
        for (const auto& a : adds) direct_adds += a[2] >= kSmallCopy && d[a[0]].pinned;
        CHECK(direct <= direct_adds);
        merged += direct_adds - direct; all_direct += direct_adds;
    }
    CHECK(merged > 20 && all_direct > 300);
}

// ---- bits_append
TEST(bits_append_matches_a_per_bit_loop) {
    Rng g(123);
    int64_t cases = 0;
    for (int sp = 0; sp < 8; ++sp)
        for (int dp = 0; dp < 8; ++dp)
            for (int64_t n = 0; n <= 300; ++n) {
                const int64_t src_bit = sp + 8 * (int64_t)(g() % 3), dst_bit = dp + 8 * (int64_t)(g() % 3);
                std::unique_ptr<uint8_t[]> src(new uint8_t[(size_t)((src_bit + n + 7) / 8)]);      // exact: a read past the last bit's byte is out of bounds
                for (int64_t i = 0; i < (src_bit + n + 7) / 8; ++i) src[(size_t)i] = (uint8_t)(g() >> 7);
                if (n % 7 == 3) for (int64_t i = 0; i < (src_bit + n + 7) / 8; ++i) src[(size_t)i] = n % 2 ? 0xFF : 0x00;
                const size_t dbytes = (size_t)((dst_bit + n + 7) / 8);
                std::unique_ptr<uint8_t[]> dst(new uint8_t[dbytes]), exp(new uint8_t[dbytes]);
                for (size_t i = 0; i < dbytes; ++i) dst[i] = exp[i] = (uint8_t)(g() >> 9);
                int64_t zeros = 0;
                for (int64_t i = 0; i < n; ++i) {
                    const bool b = bit(src.get(), src_bit + i);
                    uint8_t& e = exp[(size_t)((dst_bit + i) >> 3)];
                    e = (uint8_t)((e & ~(1u << ((dst_bit + i) & 7))) | ((unsigned)b << ((dst_bit + i) & 7)));
                    zeros += !b;
                }
                CHECK_EQ(bits_append(dst.get(), dst_bit, src.get(), src_bit, n), zeros);
                CHECK(memcmp(dst.get(), exp.get(), dbytes) == 0);      // the bits in place, every bit in front of and behind them as it was
                ++cases;
            }
    CHECK_EQ(cases, 8 * 8 * 301);
}

int main() { return run_all(); }
