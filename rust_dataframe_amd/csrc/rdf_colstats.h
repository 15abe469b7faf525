// rdf_colstats.h — argument blocks and launchers of Column::hist / Column::uniques (kernels: rdf_colstats.hip, host side:
// rdf_capi_colstats.inc), and the ONE definition of a histogram's bucket edges, shared by host and device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdf_device.h"
#include "rdf_hash.h"
#include "rdf_utf8.h"

// edges[i] of numpy.histogram(bins = nbins, range = (lo, hi)): lo + i * step with two roundings (the library is compiled
// -ffp-contract=off, host and device alike), the last edge hi exactly.
__host__ __device__ inline double cs_edge(double lo, double hi, double step, int64_t nbins, int64_t i) {
    if (i >= nbins) return hi;
    const double p = (double)i * step;
    return lo + p;
}

constexpr int kCsThreads = 256;
constexpr int kCsRowsPerLane = 8;
constexpr int kCsTile = kCsThreads * kCsRowsPerLane;   // rows of one tile of a numeric column: 8 coalesced 8-byte loads per lane
constexpr int kCsHistLdsBins = 4096;                   // up to here the counters of a block live in LDS (16 KiB of 32-bit words)
constexpr int kCsHistWaveBins = 1024;                  // up to here every wave of the block has its own copy of them
constexpr int kCsLdsSetSlots = 2048;                   // the block's LDS set of the numeric distinct pass (16 KiB), filled to half
using rdfk::kCsLongRow;                                // (rdf_hash.h: they are part of what a Utf8 row's hash is)
using rdfk::kCsEmpty;

// A chunked 8-byte column cut into tiles that never cross a chunk: tile t belongs to the chunk c with
// tile_start[c] <= t < tile_start[c + 1].
struct CsCol {
    const rdfk::DevChunkCol* chunks;       // [nchunks]
    const int64_t*           row_start;    // [nchunks + 1]
    const int64_t*           tile_start;   // [nchunks + 1]
    int64_t                  nchunks, ntiles, n;
};

struct CsHistArgs {
    CsCol    col;
    int32_t  is_int;       // Int64 values, converted `as f64`
    int32_t  peels;        // rounds of "count the lanes that share the first lane's bucket" before single adds
    double   lo, hi, step, scale;
    int64_t  nbins;
    unsigned long long* counts;    // [nbins], zeroed
    unsigned long long* counted;   // [1], zeroed
};

// counters of the distinct passes (one zeroed block of 8 words)
enum : int { CS_G_COUNT = 0, CS_G_OVERFLOW = 1, CS_G_SPECIAL = 2, CS_G_EMITTED = 3, CS_G_MISMATCH = 4 };

struct CsSetArgs {
    CsCol     col;
    int32_t   is_f64;
    uint64_t* table;       // [slots], kCsEmpty
    uint32_t* rep;         // [slots] Utf8: the smallest row with the slot's hash (0xFFFFFFFF), else nullptr
    uint64_t  mask;        // slots - 1
    uint64_t  max_fill;    // keys the table may take before the pass gives up
    unsigned long long* g;
    uint64_t* out64;       // emit: the keys (numeric)
    uint32_t* out32;       // emit: the representative rows (Utf8)
};

// the sort route: rows in sorted order, first of every run of equal values kept
struct CsRunArgs {
    CsCol           col;
    int32_t         is_f64;
    const uint32_t* perm;      // [n]
    uint64_t*       out64;     // nullptr = count only
    unsigned long long* g;
};

struct CsUtf8Args {
    const Utf8Chunk* chunks;
    int64_t          nchunks, n;
    uint64_t*        hash;     // [n]
    CsSetArgs        set;
    const uint32_t*  perm;     // exact route: rows in sorted order
    uint32_t*        out32;    // exact route: first row of every run (nullptr = count only)
};

// ---- dictionary encoding of a Utf8 column (rdf_utf8_dictionary_encode).  Both routes end in rep[row] = the smallest row
// that holds the row's value (kCsNoRow for a NULL row) and flags[row] = 1 where a row is its own representative; the
// exclusive scan of the flags is the rank of a value's first occurrence, which is the code.
constexpr uint32_t kCsNoRow = 0xFFFFFFFFu;

// one output chunk of codes; tiles of kCsThreads rows never cross a chunk, so no validity byte has two writers
struct CsDictOut {
    uint32_t* codes;       // [rows]
    uint8_t*  valid;       // [(rows + 7) / 8] or nullptr
    int64_t   row_start;   // first row of the chunk in the concatenation
    int64_t   tile_start;  // first tile of the chunk
    int64_t   rows;
};

struct CsDictArgs {
    CsUtf8Args       u;        // chunks, n; hash route: hash, set; exact route: perm
    uint32_t*        rep;      // [n]
    int64_t*         flags;    // [n] exact route, first by sorted position: 1 = the position starts a run of equal values
    const int64_t*   scan;     // [n + 1] exclusive scan of flags (of the run starts / of the first occurrences)
    uint32_t*        heads;    // exact route: [runs] the first (smallest) row of every run
    uint32_t*        firsts;   // [count] the representatives in first-occurrence order
    const CsDictOut* outs;     // [nouts]
    int64_t          nouts, ntiles;
    unsigned long long* nulls; // [nouts] zeroed: NULL rows per chunk
};

int        cs_grid(int64_t items);
hipError_t launch_cs_hist(const CsHistArgs& a, hipStream_t s);
hipError_t launch_cs_fill64(uint64_t* p, int64_t n, uint64_t v, hipStream_t s);
hipError_t launch_cs_distinct(const CsSetArgs& a, hipStream_t s);        // numeric keys -> LDS set -> table
hipError_t launch_cs_emit(const CsSetArgs& a, hipStream_t s);            // table -> out64 / out32
hipError_t launch_cs_runs(const CsRunArgs& a, hipStream_t s);
hipError_t launch_cs_utf8_hash(const CsUtf8Args& a, hipStream_t s);      // hash[], table, rep
hipError_t launch_cs_utf8_verify(const CsUtf8Args& a, hipStream_t s);    // every row against its hash's representative
hipError_t launch_cs_utf8_runs(const CsUtf8Args& a, hipStream_t s);
hipError_t launch_cs_dict_rep(const CsDictArgs& a, hipStream_t s);       // hash route: verify + rep[], flags[]
hipError_t launch_cs_dict_heads(const CsDictArgs& a, hipStream_t s);     // exact route: run starts by sorted position, NULL rows marked in rep[]
hipError_t launch_cs_dict_spread(const CsDictArgs& a, hipStream_t s);    // exact route, two launches: heads[] <- run starts, then rep[], flags[] by row
hipError_t launch_cs_dict_firsts(const CsDictArgs& a, hipStream_t s);    // firsts[rank] <- the rows that are their own representative
hipError_t launch_cs_dict_codes(const CsDictArgs& a, hipStream_t s);     // codes, validity bytes and NULL counts of every output chunk
