// rdf_utf8.h — device-side argument blocks of the Utf8 kernels (rdf_utf8.hip) and their launchers.  Host side:
// rdf_capi_utf8.inc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum : int32_t {
    UTF8_FILTER = 0, UTF8_TAKE = 1, UTF8_TRIM = 2, UTF8_LTRIM = 3, UTF8_RTRIM = 4, UTF8_SUBSTRING = 5,
    UTF8_LOWER = 6, UTF8_UPPER = 7
};
// per-row flags of the span pass
enum : uint8_t { UTF8_ROW_VALID = 1, UTF8_ROW_WIDE = 2 };   // WIDE: lower / upper of a row with a byte >= 0x80

constexpr int kUtf8CopyThreads = 256;
constexpr int kUtf8CopyTile = kUtf8CopyThreads * 16;   // output bytes per copy block: 16 per lane
constexpr int kUtf8WindowRows = 1024;                  // rows of a copy tile held in LDS; more (empty rows) -> searched in HBM

// One input chunk as the kernels see it.  data[o] is the byte at value offset o; [lo, hi] are the first and last value
// offsets of the chunk and every row's span is clamped into them, so no kernel reads outside the bytes the host checked.
struct Utf8Chunk {
    const uint8_t* data;
    const int32_t* offs;        // value_offsets of row 0 (the row offset applied): rows + 1 entries
    const uint8_t* valid;       // row validity, nullptr = all valid
    int64_t        valid_off;   // bit of row 0
    const uint8_t* mask;        // filter: mask values / validity (same bit offset), else nullptr
    const uint8_t* mask_valid;
    int64_t        mask_off;
    int64_t        row_start;   // global number of row 0 over the virtual concatenation of the chunks
    int64_t        rows;
    int32_t        lo, hi;
};

// One output chunk (device pointers: the caller's buffers, or staging space for host outputs).
struct Utf8OutChunk {
    int32_t* offs;        // rows + 1 entries
    uint8_t* valid;       // nullptr = not requested
    uint8_t* data;
    int64_t  row_start;   // global output row of row 0
    int64_t  rows;
    int64_t  byte_start;  // global output byte of byte 0 (in the scan of the row lengths)
    int64_t  bytes;
    int64_t  tile_start;  // first copy tile
};

struct Utf8Args {
    const Utf8Chunk* chunks;
    int64_t          nchunks;
    int32_t          op;
    int64_t          n;            // candidate rows: the input rows, or the indices for take
    // take
    const void*      idx;
    const uint8_t*   idx_valid;
    int64_t          idx_off;
    int32_t          idx64;
    int64_t          total_rows;
    // substring
    int32_t          pos, len;
    // per candidate row
    int64_t*         keep;         // filter: 1 = kept (scanned into rscan)
    int64_t*         blen;         // output bytes (scanned into bscan)
    uint64_t*        src;          // address of the first source byte
    uint8_t*         flags;        // UTF8_ROW_*
    const int64_t*   rscan;        // n + 1 entries (filter)
    const int64_t*   bscan;        // n + 1 entries
    uint32_t*        err;          // [0]: an index out of range
    int64_t*         tot;          // per output chunk: bytes, rows
    // outputs
    const Utf8OutChunk* outs;
    int64_t          nout;
    int64_t          ntiles;
    uint64_t*        osrc;         // per global output row: source address
    int64_t*         tile_row;     // per copy tile: the output row (of its chunk) that holds the tile's first byte
    uint8_t*         oflags;
    unsigned long long* null_counts;   // per output chunk
    int32_t*         bounds;       // per input chunk: first, last value offset (device-resident inputs)
};

hipError_t launch_utf8_bounds(const Utf8Args& a, hipStream_t s);   // bounds[2c], bounds[2c+1] = offs[0], offs[rows]
hipError_t launch_utf8_span(const Utf8Args& a, hipStream_t s);     // keep / blen / src / flags, err
hipError_t launch_utf8_totals(const Utf8Args& a, hipStream_t s);   // tot
hipError_t launch_utf8_write(const Utf8Args& a, hipStream_t s);    // offsets, validity, null counts, the bytes

// ---- sort by a Utf8 criterion (rdf_utf8_sort.hip; host side: rdf_capi_sort_utf8.inc)
// One criterion refines the incoming row order `perm` in rounds.  A round takes m rows ("round rows", in permutation
// order), each in a segment of rows that were equal so far; segment s compares its rows from byte sdepth[s] on.  Every row
// gets a 64-bit word: its next 7 bytes big-endian, then an end code min(bytes left, 8) (a proper prefix sorts first;
// 8 = the row goes on past the word), complemented when descending.  The rows are sorted stably by (segment, word),
// written back into the slots they came from, and the rows that are still tied with a neighbour and not ended go on.
constexpr int kUtf8SortWordBytes = 7;
constexpr int32_t kUtf8SortNoLcp = 0x7fffffff;
struct Utf8SortArgs {
    const Utf8Chunk* chunks;
    int64_t          nchunks;
    int64_t          n, m;          // rows of the criterion, rows of this round
    int32_t          round0, descending;
    uint32_t*        perm;          // [n] position -> row: the criterion's order, refined in place
    const uint32_t*  order_in;      // init: the incoming order (nullptr = identity)
    const uint32_t*  upos;          // [m] position of round row j (round 0: j itself)
    const uint32_t*  useg;          // [m] segment of round row j (round 0: all 0)
    int32_t*         sdepth;        // [S] compare depth of each segment
    int32_t*         slcp;          // [S] common prefix of the segment's rows beyond sdepth (min over rows, starts kUtf8SortNoLcp)
    const uint32_t*  sfirst;        // [S] the segment's first round row
    int64_t          nseg;
    uint64_t*        word;          // [m] the rows' words (round order)
    uint64_t*        keys;          // [m] sort keys out
    uint8_t*         nullflags;     // [m] round 0: 1 = NULL (by round row)
    uint64_t*        bit_stats;     // [2] min / max over the non-NULL words
    const uint32_t*  order;         // [m] round rows in sorted order (nullptr = identity)
    uint32_t*        trow;          // [m] in sorted order: the row,
    uint64_t*        tword;         //      its word,
    uint32_t*        tseg;          //      its segment,
    uint8_t*         tnull;         //      NULL
    int64_t*         fu;            // [m] 1 = the row is unresolved (goes on to the next round)
    int64_t*         fh;            // [m] 1 = ... and heads a new segment
    const int64_t*   su;            // exclusive scans of fu, fh
    const int64_t*   sh;
    uint32_t*        nupos;         // next round: upos, useg, sdepth, sfirst
    uint32_t*        nuseg;
    int32_t*         nsdepth;
    uint32_t*        nsfirst;
};
hipError_t launch_utf8_sort_init(const Utf8SortArgs& a, hipStream_t s);   // perm = order_in
hipError_t launch_utf8_sort_lcp(const Utf8SortArgs& a, hipStream_t s);    // slcp, then sdepth += slcp
hipError_t launch_utf8_sort_keys(const Utf8SortArgs& a, hipStream_t s);   // word, keys, nullflags, bit_stats
hipError_t launch_utf8_sort_seg_keys(const Utf8SortArgs& a, hipStream_t s);   // keys[t] = useg[order[t]]
hipError_t launch_utf8_sort_mark(const Utf8SortArgs& a, hipStream_t s);   // trow .. tnull, perm written back, fu, fh
hipError_t launch_utf8_sort_next(const Utf8SortArgs& a, hipStream_t s);   // nupos .. nsfirst, slcp reset

// ---- predicates and measures over Utf8 (rdf_utf8_pred.hip; host side: rdf_capi_utf8_pred.inc; what is decided about one
// row: rdf_utf8_pattern.h).  One streaming kernel per call: a block of kUtf8PredThreads lanes takes tiles of as many rows
// that never straddle a chunk (tile_start: the prefix of the chunks' tile counts), a wave 64 consecutive rows.
struct Utf8Pattern;
constexpr int kUtf8PredThreads = 256;
constexpr int kUtf8ShortRow = 256;     // bytes: a scanning op finishes a row up to this length on its lane, a longer one on the wave
enum : int32_t { UTF8_FAM_LITERAL = 0, UTF8_FAM_SCAN = 1, UTF8_FAM_COMPARE = 2 };
struct Utf8PredOut {
    void*    values;       // the Boolean bitmap, or Int32 values
    uint8_t* valid;        // nullptr = not requested
};
struct Utf8PredArgs {
    const Utf8Chunk*    a;            // nchunks chunks
    const Utf8Chunk*    b;            // UTF8_FAM_COMPARE: the other column, chunked alike
    int64_t             nchunks;
    const int64_t*      tile_start;   // nchunks + 1 entries
    int64_t             ntiles;
    const Utf8PredOut*  outs;         // per chunk
    const Utf8Pattern*  pattern;      // device copy, nullptr for the ops that take none
    int32_t             family, measure;
    int32_t             op;           // compare: U8P_EQ .. U8P_GE; measure: U8M_*; predicate: the pattern's kind decides
    int32_t             pos;          // locate
    unsigned long long* nulls;        // per chunk: NULL rows added up (nullptr: the host knows them)
    const uint8_t*      regex;        // rdf_utf8_regex.hip: the compiled pattern's image (device copy, 16-byte aligned)
};
hipError_t launch_utf8_pred(const Utf8PredArgs& a, hipStream_t s);

// ---- builders of Utf8 columns (rdf_utf8_build.hip; host side: rdf_capi_utf8_build.inc; what is decided about one row:
// rdf_utf8_build.h).  The three steps of the byte-gather above with a row made of several pieces: a size pass in the tiles
// of the predicates (256 rows of one chunk a block, long rows on the wave), the scans, and a write pass driven by the
// destination.  Output chunk c has the rows of input chunk c.
struct Utf8BuildPart {
    const Utf8Chunk* col;      // nchunks chunks of a column part, or nullptr
    const uint8_t*   lit;      // a literal part's bytes
    int32_t          lit_bytes; // (coalesce / case_when: -1 = the NULL literal)
};
struct Utf8BuildCond {         // one RDF_BOOL chunk of a case_when condition
    const uint8_t* values;
    const uint8_t* validity;   // nullptr = all valid
    int64_t        offset;     // bit of row 0, of both
};
struct Utf8BuildArgs {
    const Utf8BuildPart* parts;      // device copy: nparts (1 for every op but concat)
    int32_t          nparts, op;     // op: U8B_*
    const Utf8Chunk* shape;          // the first column part's chunks: rows and row_start of every chunk
    int64_t          nchunks;
    const int64_t*   tile_start;     // size pass: nchunks + 1 entries, tiles of kUtf8PredThreads rows
    int64_t          nsize_tiles;
    const uint8_t*   lit;            // separator / pad / delimiter (device copy)
    int32_t          lit_bytes, lit_cp;
    int64_t          param;          // pad: len; repeat: times (both clamped to [0, 2^31]); substring_index: count
    int64_t          n;              // rows
    int64_t*         blen;           // per row: output bytes (scanned into bscan)
    uint32_t*        aux;            // per row: bit 31 = valid; concat: the present parts' bits; pad: kept bytes; substring_index: the span's start; coalesce / case_when: the chosen part
    const int64_t*   bscan;          // n + 1 entries
    int64_t*         tot;            // per chunk: bytes, rows
    unsigned long long* null_counts; // per chunk
    const Utf8OutChunk* outs;
    int64_t          ntiles;         // copy tiles
    int64_t*         tile_row;       // per copy tile: the row (of its chunk) that holds the tile's first byte
    const Utf8BuildCond* conds;      // case_when: [nconds * nchunks], condition k of chunk c at k * nchunks + c; parts[nconds] is `otherwise`
    int32_t          nconds;
};
hipError_t launch_utf8_build_size(const Utf8BuildArgs& a, hipStream_t s);     // blen, aux, null_counts
hipError_t launch_utf8_build_totals(const Utf8BuildArgs& a, hipStream_t s);   // tot
hipError_t launch_utf8_build_write(const Utf8BuildArgs& a, hipStream_t s);    // offsets, validity, the bytes

// ---- rewrites of Utf8 columns by their content: replace, translate, initcap, split (rdf_utf8_rewrite.hip; host side:
// rdf_capi_utf8_rewrite.inc; what is decided about one row: rdf_utf8_rewrite.h).  Size pass in the tiles of the predicates,
// the scans, and a SOURCE-driven write pass: a block assembles the output of a run of rows in an LDS image of
// kUtf8RewriteImage bytes and streams it out in aligned 16-byte stores.  Output chunk c has the rows of input chunk c; for
// split it is the child Utf8 chunk (one row per element) and list_offs are the list's offsets.
struct Utf8TranslateTable;
constexpr int kUtf8RewriteImage = 16384;
struct Utf8RewriteOut {
    int32_t* offs;        // rows + 1 entries (split: elems + 1)
    uint8_t* valid;       // validity of the rows, nullptr = not requested
    uint8_t* data;
    int32_t* list_offs;   // split: rows + 1 entries
    int64_t  row_start, rows;
    int64_t  byte_start, bytes;   // in the scan of the row lengths
    int64_t  elem_start, elems;   // in the scan of the rows' element counts (split)
};
struct Utf8RewriteArgs {
    const Utf8Chunk* chunks;
    int64_t          nchunks;
    const int64_t*   tile_start;   // nchunks + 1 entries, tiles of kUtf8PredThreads rows
    int64_t          ntiles;
    int32_t          op;           // U8R_*
    const uint8_t*   lit;          // search / delimiter (device copy)
    const uint8_t*   rep;          // replacement
    int32_t          lit_bytes, rep_bytes;
    const Utf8TranslateTable* table;   // translate (device copy)
    int64_t          maxhits;      // split: the hits that split; replace: all
    int64_t          n;            // rows
    int64_t*         blen;         // per row: output bytes (scanned into bscan)
    int64_t*         elen;         // split: per row: elements (scanned into escan)
    const int64_t*   bscan;        // n + 1 entries
    const int64_t*   escan;
    int64_t*         tot;          // per chunk: bytes, rows, elements
    unsigned long long* null_counts;   // per chunk
    const Utf8RewriteOut* outs;
    const uint8_t*   regex;        // rdf_utf8_regex.hip: the compiled pattern's image (device copy, 16-byte aligned)
    int32_t          regex_op;     // U8X_EXTRACT / _REPLACE / _SPLIT
};
hipError_t launch_utf8_rewrite_size(const Utf8RewriteArgs& a, hipStream_t s);     // blen, elen, null_counts
hipError_t launch_utf8_rewrite_totals(const Utf8RewriteArgs& a, hipStream_t s);   // tot
hipError_t launch_utf8_rewrite_write(const Utf8RewriteArgs& a, hipStream_t s);    // offsets, validity, the bytes

// ---- regular expressions over Utf8 (rdf_utf8_regex.hip; host side: rdf_capi_utf8_regex.inc; the compiler and what is decided
// about one row: rdf_utf8_regex.h).  rlike and regexp_count are ONE kernel in the tiles and with the outputs of the
// predicates (measure != 0: the count); extract, replace and split are the three steps of the rewrites with the rewrites'
// scans, totals kernel and outputs.  Every block copies the pattern's tables into LDS when they fit kUtf8RegexLdsBytes; a
// row stays on one lane, and a tile's rows beyond kUtf8ShortRow are dealt over the block's four waves.
hipError_t launch_utf8_regex_measure(const Utf8PredArgs& a, int64_t image_bytes, hipStream_t s);
hipError_t launch_utf8_regex_size(const Utf8RewriteArgs& a, int64_t image_bytes, hipStream_t s);    // blen, elen, null_counts
hipError_t launch_utf8_regex_write(const Utf8RewriteArgs& a, int64_t image_bytes, hipStream_t s);   // offsets, validity, the bytes
