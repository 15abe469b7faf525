// rdf_window.h — argument blocks and launchers of the window functions (kernels: rdf_window.hip, host side:
// rdf_capi_window.inc).  The sort that orders the rows is sort_core's; what is here turns its permutation into partition
// and peer-group structure and into per-row answers in the original row order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdf_device.h"
#include "rdf_utf8.h"

constexpr int kWinThreads = 256;
constexpr int kWinMaxKeys = 2 * RDF_WINDOW_MAX_KEYS;   // partition keys first, then order keys
constexpr int kWinLongRow = 512;                       // Utf8 rows of this many bytes or more are compared by a whole wave

// One key column: numeric chunks (DevChunkCol per chunk) or Utf8 chunks.
struct WinKey {
    const rdfk::DevChunkCol* chunks;    // numeric, else nullptr
    const Utf8Chunk*         utf8;      // Utf8, else nullptr
    int32_t                  dtype;     // numeric: rdf_dtype
    int32_t                  order;     // 0 = partition key, 1 = order key
};

// flags[j] of sorted position j: bit 32 = the row starts a partition (P), bit 0 = it starts a peer group (P or a change of
// an order key).  Their running sums, one 64-bit scan, number the partitions (high word) and the peer groups (low word):
// n < 2^32 rows keep the low count from carrying.
constexpr uint64_t kWinFlagP = 1ull << 32;
constexpr uint64_t kWinFlagG = 1ull;

struct WinFlagArgs {
    WinKey          keys[kWinMaxKeys];
    int32_t         nkeys;
    const int64_t*  row_start;          // [nchunks + 1]
    int64_t         nchunks, n;
    const uint32_t* perm;               // sorted position -> row (nullptr = identity)
    int64_t*        flags;              // [n] out
};

struct WinStartArgs {
    const int64_t* scan;                // [n + 1] exclusive scan of flags
    int64_t        n;
    uint32_t*      pstart;              // [partitions + 1] first sorted position of every partition, then n
    uint32_t*      gstart;              // [peer groups + 1] first sorted position of every peer group, then n
};

struct WinCallOut { int32_t fn, pad; uint64_t param; void* values; uint8_t* vbytes; };
struct WinEmitArgs {
    const int64_t*  scan;
    const uint32_t* pstart;
    const uint32_t* gstart;
    const uint32_t* perm;               // nullptr = identity
    int64_t         n;
    int32_t         ncalls, pad;
    WinCallOut      calls[RDF_WINDOW_MAX_CALLS];   // values: [n] by ORIGINAL row; vbytes (LAG / LEAD): [n] 1 = valid, or nullptr
    unsigned long long* nulls;          // [RDF_WINDOW_MAX_CALLS], zeroed
};

hipError_t launch_win_flags(const WinFlagArgs& a, hipStream_t s);
hipError_t launch_win_starts(const WinStartArgs& a, hipStream_t s);
hipError_t launch_win_emit(const WinEmitArgs& a, hipStream_t s);
hipError_t launch_win_pack(const uint8_t* vbytes, int64_t n, uint64_t* words, hipStream_t s);   // ceil(n / 64) words, LSB first
