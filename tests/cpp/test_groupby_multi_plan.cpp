// The route and LDS layout of rdf_groupby_multi (csrc/rdf_groupby_multi_plan.h) on the CPU: capacity monotone in the number of
// calls, every layout inside the budget with its arrays disjoint and 8-byte aligned, the route flipping exactly between
// capacity and capacity + 1, the slots and route overrides honoured.  Stand-alone: no library, no device.
#include <cstdio>
#include <vector>

#include "../../rust_dataframe_amd/csrc/rdf_groupby_multi_plan.h"

using namespace rdfk;

static int g_run = 0, g_failed = 0;
#define CHECK(c) do { ++g_run; if (!(c)) { ++g_failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static void check_layout(const GbmPlan& p, int k) {
    CHECK(p.ncalls == k && p.entries == p.slots + 2 && p.capacity == p.slots / 2 && p.slots % 2 == 0 && p.slots >= 2);
    CHECK(p.lds_bytes <= kGbmLdsBudget);
    // the arrays in order, none overlapping the next, the 64-bit ones (and the tail) on 8-byte boundaries
    CHECK(p.off_keys == 0);
    CHECK(p.off_acc >= p.off_keys + 8 * p.entries && p.off_acc % 8 == 0);
    CHECK(p.off_rows >= p.off_acc + 8 * k * p.entries && p.off_rows % 8 == 0);
    CHECK(p.off_cnt >= p.off_rows + 4 * p.entries && p.off_cnt % 4 == 0);
    CHECK(p.off_tail >= p.off_cnt + 4 * k * p.entries && p.off_tail % 8 == 0);
    CHECK(p.lds_bytes == p.off_tail + kGbmTail);
    CHECK(2 * p.capacity <= p.slots);   // load <= 0.5 at capacity
}

int main() {
    // capacity: positive, monotone (more calls never hold more groups), 0 outside 1..8, and the most the budget holds
    for (int k = 1; k <= kGbmMaxCalls; ++k) {
        CHECK(gbm_capacity(k) > 0);
        if (k > 1) CHECK(gbm_capacity(k) <= gbm_capacity(k - 1));
        const GbmPlan p = gbm_plan(k, 1, 0, 0);
        check_layout(p, k);
        CHECK(p.capacity == gbm_capacity(k));
        // two more slots would not fit
        CHECK((p.slots + 2 + 2) * gbm_entry_bytes(k) + kGbmTail > kGbmLdsBudget);
    }
    CHECK(gbm_capacity(1) > gbm_capacity(8));
    CHECK(gbm_capacity(0) == 0 && gbm_capacity(9) == 0 && gbm_capacity(-1) == 0);

    // the route flips exactly between capacity and capacity + 1
    for (int k = 1; k <= kGbmMaxCalls; ++k) {
        const int64_t cap = gbm_capacity(k);
        CHECK(gbm_plan(k, 1, 0, 0).route == GBM_ROUTE_STREAM);
        CHECK(gbm_plan(k, cap - 1, 0, 0).route == GBM_ROUTE_STREAM);
        CHECK(gbm_plan(k, cap, 0, 0).route == GBM_ROUTE_STREAM);
        CHECK(gbm_plan(k, cap + 1, 0, 0).route == GBM_ROUTE_TABLE);
        CHECK(gbm_plan(k, (int64_t)1 << 40, 0, 0).route == GBM_ROUTE_TABLE);
        // forced routes, either side of the boundary
        CHECK(gbm_plan(k, cap + 1, 0, GBM_ROUTE_STREAM).route == GBM_ROUTE_STREAM);
        CHECK(gbm_plan(k, 1, 0, GBM_ROUTE_TABLE).route == GBM_ROUTE_TABLE);
        CHECK(gbm_plan(k, cap + 1, 0, 7).route == GBM_ROUTE_TABLE);   // an unknown override is no override
    }

    // the slots override: honoured when smaller than planned (made even), ignored when 0, 1 or beyond the budget
    for (int k = 1; k <= kGbmMaxCalls; ++k) {
        const int planned = gbm_planned_slots(k);
        for (int64_t n : {(int64_t)2, (int64_t)3, (int64_t)64, (int64_t)65, (int64_t)planned - 1}) {
            const GbmPlan p = gbm_plan(k, 1, n, 0);
            check_layout(p, k);
            CHECK(p.slots == (n & ~(int64_t)1));
            CHECK(gbm_plan(k, p.capacity, n, 0).route == GBM_ROUTE_STREAM);
            CHECK(gbm_plan(k, p.capacity + 1, n, 0).route == GBM_ROUTE_TABLE);
        }
        for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)-5, (int64_t)planned, (int64_t)planned + 1, (int64_t)1 << 40}) {
            const GbmPlan p = gbm_plan(k, 1, n, 0);
            check_layout(p, k);
            CHECK(p.slots == planned);
        }
    }
    {
        const GbmPlan p = gbm_plan(5, 32, 64, 0);
        CHECK(p.slots == 64 && p.capacity == 32 && p.route == GBM_ROUTE_STREAM);
        CHECK(gbm_plan(5, 33, 64, 0).route == GBM_ROUTE_TABLE);
    }

    // rows a thread holds per batch: fewer for wide value lists, a divisor of what the loaders are instantiated for
    CHECK(gbm_rows_per_thread(0) == 4 && gbm_rows_per_thread(2) == 4 && gbm_rows_per_thread(3) == 2 && gbm_rows_per_thread(4) == 2);
    CHECK(gbm_rows_per_thread(5) == 1 && gbm_rows_per_thread(8) == 1);

    std::printf("%d checks, %d failed\n", g_run, g_failed);
    return g_failed ? 1 : 0;
}
