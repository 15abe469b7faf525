// rdf_digest_kernels.h — device-side argument blocks of rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32 (kernels:
// rdf_digest.hip, host side: rdf_capi_digest.inc, what is computed about one row: rdf_digest.h).  The tiling is the
// predicates': a block of kUtf8PredThreads lanes takes tiles of as many rows that never straddle a chunk (tile_start: the
// prefix of the chunks' tile counts), a wave 64 consecutive rows, a lane one row at every length (the SHA-2 digests hand a
// tile's rows above kUtf8ShortRow to the block's first lanes: rdf_digest.hip).
#pragma once
#include "rdf_device.h"
#include "rdf_utf8.h"

struct HashCol {                     // one column of rdf_hash_columns: exactly one of num / utf8
    const rdfk::DevChunkCol* num;          // nchunks fixed-width (or Boolean) chunks
    const Utf8Chunk*   utf8;         // nchunks Utf8 chunks
    int32_t            dtype;        // rdf_dtype of a fixed-width column
};
struct HashColsArgs {
    const HashCol*     cols;         // device copy: ncols
    int32_t            ncols, kind;  // kind: DGH_*
    int64_t            seed;
    const int64_t*     row_start;    // nchunks + 1 entries: chunk c has row_start[c + 1] - row_start[c] rows
    int64_t            nchunks;
    const int64_t*     tile_start;   // nchunks + 1 entries
    int64_t            ntiles;
    const Utf8PredOut* outs;         // per chunk: Int32 / Int64 values; the validity, if given, is written all ones
};
hipError_t launch_hash_columns(const HashColsArgs& a, hipStream_t s);

struct Utf8DigestArgs {
    const Utf8Chunk*    chunks;
    int64_t             nchunks;
    const int64_t*      tile_start;  // nchunks + 1 entries
    int64_t             ntiles;
    int32_t             kind;        // DG_*
    int64_t*            tile_count;  // [ntiles] rows of the tile that are not NULL (scanned into tile_scan)
    const int64_t*      tile_scan;   // [ntiles + 1]
    int64_t*            tot;         // per chunk: rows that are not NULL
    const Utf8OutChunk* outs;        // write pass: offs, valid, data (rows as the input chunk's)
};
hipError_t launch_utf8_digest_count(const Utf8DigestArgs& a, hipStream_t s);    // tile_count
hipError_t launch_utf8_digest_totals(const Utf8DigestArgs& a, hipStream_t s);   // tot
hipError_t launch_utf8_digest_write(const Utf8DigestArgs& a, hipStream_t s);    // offsets, validity, the hex text

struct Utf8Crc32Args {
    const Utf8Chunk*    chunks;
    int64_t             nchunks;
    const int64_t*      tile_start;
    int64_t             ntiles;
    const Utf8PredOut*  outs;        // per chunk: Int64 values, validity
    unsigned long long* nulls;       // per chunk: NULL rows added up (nullptr: the host knows them)
};
hipError_t launch_utf8_crc32(const Utf8Crc32Args& a, hipStream_t s);
