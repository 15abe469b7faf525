// rdf_groupby_multi_plan.h — route and LDS layout of rdf_groupby_multi (kernels: rdf_groupby_multi.hip).  Pure host / device
// arithmetic, no HIP: tests/cpp/test_groupby_multi_plan.cpp compiles it with a plain C++ compiler.
//
// The block table of gbm_stream_kernel holds `slots` hashed keys, open addressing with linear probing, and behind them the two
// groups that never enter it (index slots: the key whose hash is the free marker; slots + 1: the NULL key).  Per entry:
//   8 bytes  hashed key                      keys[entries]
//   8 bytes  accumulator of every call       acc[ncalls][entries]
//   4 bytes  rows of the group               rows[entries]
//   4 bytes  non-NULL values of every call   cnt[ncalls][entries]
// entries = slots + 2; the 64-bit arrays come first, so every array starts 8-byte aligned whatever `slots` is.  A 16-byte
// tail pads the table.  The budget is the 80 KB the single-aggregate stream kernel lives in (512 threads,
// two blocks per CU of 160 KB); the capacity — the most groups the route is chosen for — is half the slots (load <= 0.5).
#pragma once
#include <stdint.h>

namespace rdfk {

constexpr int kGbmMaxCalls = 8;
constexpr int kGbmMaxValues = 8;
constexpr int kGbmLdsBudget = 80 * 1024;
constexpr int kGbmTail = 16;
enum : int32_t { GBM_ROUTE_AUTO = 0, GBM_ROUTE_STREAM = 1, GBM_ROUTE_TABLE = 2 };

struct GbmPlan {
    int32_t ncalls;
    int32_t slots;        // hashed-key slots of the block table
    int32_t entries;      // slots + 2
    int32_t route;        // GBM_ROUTE_STREAM / GBM_ROUTE_TABLE
    int64_t capacity;     // most groups the stream route is planned for: slots / 2
    // byte offsets inside the block's dynamic LDS
    int32_t off_keys, off_acc, off_rows, off_cnt, off_tail, lds_bytes;
};

inline int32_t gbm_entry_bytes(int32_t ncalls) { return 12 + 12 * ncalls; }

// slots the budget holds for this many calls (even, so that capacity = slots / 2 exactly)
inline int32_t gbm_planned_slots(int32_t ncalls) {
    const int32_t entries = (kGbmLdsBudget - kGbmTail) / gbm_entry_bytes(ncalls);
    return (entries - 2) & ~1;
}

inline int64_t gbm_capacity(int32_t ncalls) {
    if (ncalls < 1 || ncalls > kGbmMaxCalls) return 0;
    return gbm_planned_slots(ncalls) / 2;
}

// slots_override: rdf_set_option("groupby_multi_slots", n) — a smaller table (tests reach the capacity boundary with a few
// groups); 0 or anything the budget cannot hold: planned.  route_override: rdf_set_option("groupby_multi_route", ...).
inline GbmPlan gbm_plan(int32_t ncalls, int64_t max_groups, int64_t slots_override, int32_t route_override) {
    GbmPlan p;
    p.ncalls = ncalls;
    int32_t slots = gbm_planned_slots(ncalls);
    if (slots_override >= 2 && slots_override < slots) slots = (int32_t)slots_override & ~1;
    p.slots = slots;
    p.entries = slots + 2;
    p.capacity = slots / 2;
    p.off_keys = 0;
    p.off_acc = p.off_keys + 8 * p.entries;
    p.off_rows = p.off_acc + 8 * ncalls * p.entries;
    p.off_cnt = p.off_rows + 4 * p.entries;
    p.off_tail = (p.off_cnt + 4 * ncalls * p.entries + 7) & ~7;
    p.lds_bytes = p.off_tail + kGbmTail;
    p.route = max_groups <= p.capacity ? GBM_ROUTE_STREAM : GBM_ROUTE_TABLE;
    if (route_override == GBM_ROUTE_STREAM || route_override == GBM_ROUTE_TABLE) p.route = route_override;
    return p;
}

// rows a thread holds per batch in gbm_stream_kernel: two batches of (key, nvalues values, their validity bytes) must stay in
// registers next to the fold's state at 128 VGPRs a thread (two 512-thread blocks per CU) — wide value lists take fewer rows
inline int32_t gbm_rows_per_thread(int32_t nvalues) { return nvalues <= 2 ? 4 : nvalues <= 4 ? 2 : 1; }

}  // namespace rdfk
