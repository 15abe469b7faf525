// rdf_window_agg.h — argument blocks and launchers of the window frame aggregates (kernels: rdf_window_agg.hip, host
// side: rdf_capi_window_agg.inc).  The order, the partition / peer-group scan words and the start tables are rdf_window's
// (rdf_window.h); what is here gathers a value column through the permutation, builds prefix structures over it that
// restart at partition, peer-group or block bounds, and resolves every row's frame [a, b] against them.
#pragma once
#include "rdf_window.h"

constexpr int kWaggThreads = 1024;
constexpr int kWaggPer = 4;
constexpr int kWaggSeg = kWaggThreads * kWaggPer;   // a scan segment: 4096 positions, as launch_scan's

// What a scan carries per position (64-bit words, one array per word):
//   SUMF  w0, w1 = the running sum of the finite values as a double-double (hi, lo); w2 = valid rows << 32 | NaNs;
//         w3 = +inf << 32 | -inf.  Int64 columns enter `as f64` (AVG).
//   SUMI  w0 = the wrapping Int64 sum; w1 = valid rows << 32.
//   EXT   w0 = min or max over the order-preserving image of the value (absent rows: the fold's identity).
enum { kWaggSumF = 0, kWaggSumI = 1, kWaggExt = 2 };
constexpr int wagg_words(int kind) { return kind == kWaggSumF ? 4 : kind == kWaggSumI ? 2 : 1; }
// Where a scan restarts: at partition starts, at peer-group starts, or at partition starts and every w-th position of the
// partition (blocks aligned to the PARTITION's start).  A backward scan restarts at the ends instead.
enum { kWaggRestartPartition = 0, kWaggRestartPeer = 1, kWaggRestartBlock = 2 };

struct WaggScanArgs {
    const int64_t*  scan;               // [n + 1] rdf_window's exclusive scan of the flags
    const uint32_t* pstart;             // rdf_window's partition start table
    const uint32_t* perm;               // sorted position -> row (nullptr = identity)
    const rdfk::DevChunkCol* chunks;    // the value column, one descriptor per chunk
    const int64_t*  row_start;          // [nchunks + 1]
    int64_t         nchunks, n;
    int32_t         f64;                // the column is Float64 (else Int64)
    int32_t         restart, backward, ismax;
    uint32_t        w;                  // kWaggRestartBlock: the block width, >= 1
    uint32_t        pad;
    uint64_t*       out[4];             // [n] per word of the payload, by sorted position
    uint64_t*       seg[4];             // [segments] per word: the segments' aggregates, then their running fold
    uint32_t*       seg_first;          // [segments] first restart inside the segment (kWaggSeg = none)
};

// How MIN / MAX read their scans.
enum { kWaggExtForward = 0,             // the answer is F[b]
       kWaggExtBackward = 1,            // the answer is B[a]
       kWaggExtBlock = 2 };             // F[b] and B[a] of blocks of width w: one block or two adjacent ones

struct WaggCallOut {
    int32_t  fn, f64;                   // rdf_window_agg_fn; the value column is Float64
    int32_t  unit, start_kind, end_kind, ext_mode;
    int64_t  start, end;                // offsets, clamped to 2^32
    uint32_t w, pad;
    const uint64_t* sum[4];             // SUMF: hi, lo, counts, infinities; SUMI: sum, -, counts, -
    const uint64_t* fwd;                // EXT scans
    const uint64_t* bwd;
    void*    values;                    // [n] by ORIGINAL row
    uint8_t* vbytes;                    // [n] 1 = valid, or nullptr (COUNT)
};
struct WaggEmitArgs {
    const int64_t*  scan;
    const uint32_t* pstart;
    const uint32_t* gstart;
    const uint32_t* perm;
    int64_t         n;
    int32_t         ncalls, pad;
    WaggCallOut     calls[RDF_WINDOW_MAX_CALLS];
    unsigned long long* nulls;          // [RDF_WINDOW_MAX_CALLS], zeroed
};

hipError_t launch_wagg_scan(int kind, const WaggScanArgs& a, hipStream_t s);   // three launches; no block waits on another
hipError_t launch_wagg_emit(const WaggEmitArgs& a, hipStream_t s);

// rdf_window_range_agg: per call, the frame's resolved ends by sorted position, relative to the partition's start
// (rdf_window_range.hip writes them).  nullptr = that end is UNBOUNDED or CURRENT ROW and comes from n, f, l as before.
struct WaggRangeBounds {
    const uint32_t* start[RDF_WINDOW_MAX_CALLS];    // [n] the frame's first position
    const uint32_t* endx[RDF_WINDOW_MAX_CALLS];     // [n] one past its last position (0: empty at the partition's start)
};
hipError_t launch_wagg_emit_range(const WaggEmitArgs& a, const WaggRangeBounds& rb, hipStream_t s);
