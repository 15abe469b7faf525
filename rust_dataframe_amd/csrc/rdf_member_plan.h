// rdf_member_plan.h — table size and route of rdf_member_mask / rdf_first_occurrence (kernels: rdf_member.hip).  Pure host /
// device arithmetic, no HIP: tests/cpp/test_member_plan.cpp compiles it with a plain C++ compiler.
//
// The table is open addressing with linear probing over 2^tbits slots, slot = (word * kJoinMul) >> (64 - tbits).  It is sized
// from the BUILD ROWS (the distinct keys are not known before the build): the smallest power of two that holds them at load
// <= 0.5, at least 2^kMemberMinBits slots, at most 2^budget ("member_table_bits").  A budget below the need leaves a table
// that may fill up: every probe loop is bounded by the slots, and a build that finds no free slot reports it (the call
// returns RDF_MEMORY_ERROR), so a shrunk table costs a refusal, never a wrong answer or a walk without end.
//
// LDS form (rdf_member_mask on ONE key column): while the table fits the block's LDS budget — the 80 KB of
// rdf_groupby_multi_plan.h, two blocks per CU of 160 KB — every probe block copies the 8-byte slots into LDS once and probes
// there.  The budget holds 2^13 slots (64 KB); the capacity, the most build rows the form is chosen for, is half of that.
#pragma once
#include <stdint.h>

namespace rdfk {

constexpr int kMemberLdsBudget = 80 * 1024;
constexpr int kMemberMinBits = 4;
constexpr int kMemberMaxBits = 32;
constexpr int kMemberDefaultBits = 30;     // 8 GB of 8-byte slots: 5e8 build rows at load <= 0.5
enum : int32_t { MEMBER_ROUTE_AUTO = 0, MEMBER_ROUTE_LDS = 1, MEMBER_ROUTE_HBM = 2 };

struct MemberPlan {
    int32_t  tbits;         // log2 of the slots: kMemberMinBits .. kMemberMaxBits
    int32_t  tshift;        // 64 - tbits: 32 .. 60, never the word width
    uint64_t slots;         // 1 << tbits
    int32_t  route;         // MEMBER_ROUTE_LDS / MEMBER_ROUTE_HBM
    int32_t  lds_slots;     // slots the LDS form may use (a power of two)
    int64_t  lds_capacity;  // lds_slots / 2: most build rows of the LDS form
    int32_t  lds_bytes;     // dynamic LDS of the probe in the LDS form: 8 * slots (0 on the HBM route)
    int32_t  ok;            // 0: the forced route cannot serve the call
};

inline int32_t member_clamp_bits(int64_t bits) {
    return bits < kMemberMinBits ? kMemberMinBits : bits > kMemberMaxBits ? kMemberMaxBits : (int32_t)bits;
}

// log2 of the slots for this many build rows: the smallest table with slots >= 2 * rows, within [kMemberMinBits, budget]
inline int32_t member_table_bits(int64_t build_rows, int64_t budget_bits) {
    const int32_t budget = member_clamp_bits(budget_bits);
    const uint64_t want = build_rows <= 0 ? 0 : 2 * (uint64_t)build_rows;
    int32_t bits = kMemberMinBits;
    while (bits < budget && ((uint64_t)1 << bits) < want) ++bits;
    return bits;
}

// slots of the LDS form: the largest power of two whose 8-byte slots the budget holds; "member_slots" shrinks it (rounded
// down to a power of two, at least 2^kMemberMinBits; 0 or anything not smaller: planned)
inline int32_t member_lds_slots(int64_t slots_override) {
    int32_t planned = 1 << kMemberMinBits;
    while (2 * planned * 8 <= kMemberLdsBudget) planned *= 2;
    if (slots_override >= (1 << kMemberMinBits) && slots_override < planned) {
        int32_t s = 1 << kMemberMinBits;
        while (2 * s <= slots_override) s *= 2;
        return s;
    }
    return planned;
}

// single_word: one key column (the table stores the key word itself); route_override: "member_route"
inline MemberPlan member_plan(int64_t build_rows, bool single_word, int64_t budget_bits, int64_t slots_override, int32_t route_override) {
    MemberPlan p;
    p.tbits = member_table_bits(build_rows, budget_bits);
    p.tshift = 64 - p.tbits;
    p.slots = (uint64_t)1 << p.tbits;
    p.lds_slots = member_lds_slots(slots_override);
    p.lds_capacity = p.lds_slots / 2;
    const bool fits = single_word && build_rows <= p.lds_capacity && p.slots <= (uint64_t)p.lds_slots;
    p.route = fits ? MEMBER_ROUTE_LDS : MEMBER_ROUTE_HBM;
    p.ok = 1;
    if (route_override == MEMBER_ROUTE_HBM) p.route = MEMBER_ROUTE_HBM;
    else if (route_override == MEMBER_ROUTE_LDS && !fits) p.ok = 0;
    p.lds_bytes = p.route == MEMBER_ROUTE_LDS ? (int32_t)(8 * p.slots) : 0;
    return p;
}

}  // namespace rdfk
