// rdf_member.h — argument blocks and launchers of rdf_member_mask / rdf_first_occurrence (kernels: rdf_member.hip, host
// side: rdf_capi_member.inc, sizes and routes: rdf_member_plan.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdf_colstats.h"
#include "rdf_datetime.h"
#include "rdf_member_plan.h"

constexpr uint64_t kMemberEmpty = rdfk::kCsEmpty;     // free slot of a table of key words (a key equal to it is set aside in a flag)
constexpr uint32_t kMemberNoRow = 0xFFFFFFFFu;        // free slot of a table of representative rows
enum : int { MEMBER_F_MARKER = 0, MEMBER_F_NULL = 1, MEMBER_F_OVERFLOW = 2, MEMBER_F_WORDS = 4 };

// One side's rows: tiles of kCsTile rows that never cross a chunk.  One key column is read where it lies; 2..4 columns
// go through member_prep_kernel first.
struct MemberSide {
    CsCol     col;             // col.chunks[k * nchunks + c] = chunk c of key column k
    int32_t   nkeys;
    int32_t   dtype[4];
    uint64_t* hash;            // [n] 2..4 keys: the tuple's 64-bit hash
    uint64_t* bits[4];         // [n] ... every column's key word (0 where the column is NULL)
    uint8_t*  nullbits;        // [n] ... bit k = column k is NULL
};

struct MemberTable {
    uint64_t* keys;            // one key: [slots] key words, kMemberEmpty = free
    uint32_t* lo;              // tuples: [slots] a row of the slot's tuple (kMemberNoRow = free), claimed by compare-and-swap;
                               // first occurrence: the smallest row of the slot's key ([slots + 2]: then the free-marker key, the NULL key)
    uint32_t* hi;              // first occurrence: the largest row ([slots + 2])
    uint64_t  mask;            // slots - 1
    int32_t   tshift;          // slot = (word * kJoinMul) >> tshift
    int32_t   pad;
    unsigned int* flags;       // [MEMBER_F_WORDS] zeroed: the build side holds the free-marker key / a NULL row; a build found no free slot
};

struct MemberArgs {
    MemberSide   probe, build;     // rdf_first_occurrence: probe alone
    MemberTable  t;
    int32_t      kind;             // rdf_member_kind / rdf_keep
    int32_t      descending;       // fold pass: 0 = tiles in ascending row order, the smallest row folded; 1 = descending, the largest
    const DtOut* outs;             // [nchunks] mask words (and validity words) of every chunk, or nullptr: count only
    unsigned long long* partial;   // [grid] TRUE rows per block
    unsigned long long* chunk_nulls;   // [nchunks] zeroed (IS_IN): NULL results per chunk
    unsigned long long* skipped;   // fold pass: rows whose atomic the load-and-compare saved ([1] zeroed), or nullptr
};

int        member_grid(int64_t ntiles, bool lds);
hipError_t launch_member_prep(const MemberSide& s, int with_nulls, hipStream_t st);
hipError_t launch_member_build(const MemberArgs& a, hipStream_t s);
hipError_t launch_member_probe(const MemberArgs& a, int grid, size_t lds_bytes, hipStream_t s);   // lds_bytes != 0: the LDS form
hipError_t launch_member_fold(const MemberArgs& a, hipStream_t s);
hipError_t launch_member_first(const MemberArgs& a, int grid, hipStream_t s);
hipError_t launch_member_total(const unsigned long long* partial, int n, unsigned long long* total, hipStream_t s);
