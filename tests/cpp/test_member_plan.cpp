// Table size and route of rdf_member_mask / rdf_first_occurrence (csrc/rdf_member_plan.h) on the CPU: the table bits for 0, 1
// and 2^k +- 1 build rows, the budget clamp, the capacity boundary of the LDS form, forced routes, and no shift by the word
// width.  Stand-alone: no library, no device.
#include <cstdio>
#include <initializer_list>

#include "../../rust_dataframe_amd/csrc/rdf_member_plan.h"

using namespace rdfk;

static int g_run = 0, g_failed = 0;
#define CHECK(c) do { ++g_run; if (!(c)) { ++g_failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static void check_plan(const MemberPlan& p) {
    CHECK(p.tbits >= kMemberMinBits && p.tbits <= kMemberMaxBits);
    CHECK(p.tshift == 64 - p.tbits && p.tshift >= 32 && p.tshift <= 60);   // never the word width, never negative
    CHECK(p.slots == (uint64_t)1 << p.tbits);
    CHECK((p.lds_slots & (p.lds_slots - 1)) == 0 && p.lds_slots >= (1 << kMemberMinBits));
    CHECK(8 * (int64_t)p.lds_slots <= kMemberLdsBudget && p.lds_capacity == p.lds_slots / 2);
    if (p.route == MEMBER_ROUTE_LDS) CHECK(p.lds_bytes == (int32_t)(8 * p.slots) && p.lds_bytes <= kMemberLdsBudget && p.slots <= (uint64_t)p.lds_slots);
    else CHECK(p.route == MEMBER_ROUTE_HBM && p.lds_bytes == 0);
}

int main() {
    // table bits: the smallest table with slots >= 2 * rows, never below the minimum
    CHECK(member_table_bits(0, kMemberDefaultBits) == kMemberMinBits);
    CHECK(member_table_bits(-3, kMemberDefaultBits) == kMemberMinBits);
    CHECK(member_table_bits(1, kMemberDefaultBits) == kMemberMinBits);
    CHECK(member_table_bits(8, kMemberDefaultBits) == 4 && member_table_bits(9, kMemberDefaultBits) == 5);
    for (int k = 4; k <= 28; ++k) {
        const int64_t r = (int64_t)1 << k;
        CHECK(member_table_bits(r - 1, kMemberDefaultBits) == k + 1);
        CHECK(member_table_bits(r, kMemberDefaultBits) == k + 1);
        CHECK(member_table_bits(r + 1, kMemberDefaultBits) == k + 2);
        for (int64_t rows : {r - 1, r, r + 1}) {
            const int b = member_table_bits(rows, kMemberMaxBits);
            CHECK(((uint64_t)1 << b) >= 2 * (uint64_t)rows);               // load <= 0.5
            CHECK(b == kMemberMinBits || ((uint64_t)1 << (b - 1)) < 2 * (uint64_t)rows);   // and no larger than that needs
        }
    }
    // the budget clamp: bits never exceed the budget, the budget itself is held to [min, max]
    CHECK(member_table_bits((int64_t)1 << 20, 10) == 10);
    CHECK(member_table_bits((int64_t)1 << 20, 2) == kMemberMinBits);
    CHECK(member_table_bits(((int64_t)1 << 32) - 1, 64) == kMemberMaxBits);
    CHECK(member_table_bits(((int64_t)1 << 32) - 1, kMemberDefaultBits) == kMemberDefaultBits);
    CHECK(member_clamp_bits(-1) == kMemberMinBits && member_clamp_bits(0) == kMemberMinBits && member_clamp_bits(33) == kMemberMaxBits && member_clamp_bits(17) == 17);
    for (int64_t rows : {(int64_t)0, (int64_t)1, (int64_t)1000, (int64_t)1 << 31, ((int64_t)1 << 32) - 1})
        for (int64_t budget : {(int64_t)-7, (int64_t)0, (int64_t)4, (int64_t)5, (int64_t)24, (int64_t)32, (int64_t)99}) {
            check_plan(member_plan(rows, true, budget, 0, 0));
            check_plan(member_plan(rows, false, budget, 64, 2));
        }

    // the LDS form: what the budget holds, and the capacity boundary
    const int planned = member_lds_slots(0);
    CHECK(planned == 8192 && 8 * planned <= kMemberLdsBudget && 16 * planned > kMemberLdsBudget);
    {
        const int64_t cap = planned / 2;
        CHECK(member_plan(0, true, kMemberDefaultBits, 0, 0).route == MEMBER_ROUTE_LDS);
        CHECK(member_plan(cap - 1, true, kMemberDefaultBits, 0, 0).route == MEMBER_ROUTE_LDS);
        CHECK(member_plan(cap, true, kMemberDefaultBits, 0, 0).route == MEMBER_ROUTE_LDS);
        CHECK(member_plan(cap + 1, true, kMemberDefaultBits, 0, 0).route == MEMBER_ROUTE_HBM);
        CHECK(member_plan(cap, false, kMemberDefaultBits, 0, 0).route == MEMBER_ROUTE_HBM);    // tuples never take it
        CHECK(member_plan(cap, true, kMemberDefaultBits, 0, 0).lds_bytes == 8 * planned);
    }
    // "member_slots": rounded down to a power of two, at least the minimum; 0, negative or not smaller: planned
    CHECK(member_lds_slots(64) == 64 && member_lds_slots(65) == 64 && member_lds_slots(127) == 64 && member_lds_slots(128) == 128);
    CHECK(member_lds_slots(16) == 16 && member_lds_slots(15) == planned && member_lds_slots(1) == planned);
    CHECK(member_lds_slots(-4) == planned && member_lds_slots(planned) == planned && member_lds_slots((int64_t)1 << 40) == planned);
    {
        CHECK(member_plan(31, true, kMemberDefaultBits, 64, 0).route == MEMBER_ROUTE_LDS);
        const MemberPlan p = member_plan(32, true, kMemberDefaultBits, 64, 0);
        CHECK(p.route == MEMBER_ROUTE_LDS && p.lds_capacity == 32 && p.slots == 64 && p.lds_bytes == 512);
        CHECK(member_plan(33, true, kMemberDefaultBits, 64, 0).route == MEMBER_ROUTE_HBM);
    }

    // forced routes: HBM always; LDS only where it can serve the call; an unknown override is no override
    CHECK(member_plan(1, true, kMemberDefaultBits, 0, MEMBER_ROUTE_HBM).route == MEMBER_ROUTE_HBM);
    CHECK(member_plan(1, true, kMemberDefaultBits, 0, MEMBER_ROUTE_HBM).ok == 1);
    CHECK(member_plan(32, true, kMemberDefaultBits, 64, MEMBER_ROUTE_LDS).ok == 1);
    CHECK(member_plan(32, true, kMemberDefaultBits, 64, MEMBER_ROUTE_LDS).route == MEMBER_ROUTE_LDS);
    CHECK(member_plan(33, true, kMemberDefaultBits, 64, MEMBER_ROUTE_LDS).ok == 0);
    CHECK(member_plan(8, false, kMemberDefaultBits, 0, MEMBER_ROUTE_LDS).ok == 0);
    CHECK(member_plan(33, true, kMemberDefaultBits, 64, 7).ok == 1 && member_plan(33, true, kMemberDefaultBits, 64, 7).route == MEMBER_ROUTE_HBM);

    std::printf("%d checks, %d failed\n", g_run, g_failed);
    return g_failed ? 1 : 0;
}
