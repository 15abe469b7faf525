// rdf_select.h — what rdf_null_test / rdf_coalesce / rdf_case_when / rdf_extremum / rdf_nanvl decide about ONE row (kernels:
// rdf_select.hip, host side: rdf_capi_select.inc).  ONE definition, __host__ __device__ inline: hipcc compiles it into the
// kernels, plain g++ compiles it into tests/cpp/test_select_host.cpp.  It includes nothing of HIP.
//
// Rules kept throughout:
//   bits        a value is carried as the unsigned integer of its width; it becomes its type only inside a comparison, so a
//               NaN's payload and the sign of -0.0 come out as they went in
//   ordering    Spark's: integers in their own signedness; floats with -0.0 == 0.0, NaN == NaN and NaN above every number
//   ties        extremum folds left to right with a STRICT comparison: of equal parts the leftmost one's bits are returned
//   choice      coalesce / case_when choose a part from one bit per part (bit k: part k can decide the row); the lowest set
//               bit wins.  The kernels run the same chain on 64 rows at a time: taken = undecided & can, undecided &= ~can.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RDF_SEL_HD __host__ __device__ inline
#else
#define RDF_SEL_HD inline
#endif

// rdf_null_test_op of include/rdf_mi355x.h, restated so that this header stands alone (rdf_capi_select.inc static_asserts)
enum : int { SEL_IS_NULL = 0, SEL_IS_NOT_NULL = 1, SEL_IS_NAN = 2, SEL_NTESTS };
// how a dtype compares
enum : int { SEL_SIGNED = 0, SEL_UNSIGNED = 1, SEL_FLOAT = 2 };

constexpr int kSelMaxParts = 8;                // RDF_SELECT_PARTS_MAX
constexpr int kSelSlots = kSelMaxParts + 1;    // case_when: eight branches and `otherwise`

template <int ES> struct SelBits;
template <> struct SelBits<1> { using U = uint8_t; };
template <> struct SelBits<2> { using U = uint16_t; };
template <> struct SelBits<4> { using U = uint32_t; };
template <> struct SelBits<8> { using U = uint64_t; };

template <int CLS, int ES> struct SelType;
template <> struct SelType<SEL_SIGNED, 1> { using T = int8_t; };
template <> struct SelType<SEL_SIGNED, 2> { using T = int16_t; };
template <> struct SelType<SEL_SIGNED, 4> { using T = int32_t; };
template <> struct SelType<SEL_SIGNED, 8> { using T = int64_t; };
template <> struct SelType<SEL_UNSIGNED, 1> { using T = uint8_t; };
template <> struct SelType<SEL_UNSIGNED, 2> { using T = uint16_t; };
template <> struct SelType<SEL_UNSIGNED, 4> { using T = uint32_t; };
template <> struct SelType<SEL_UNSIGNED, 8> { using T = uint64_t; };
template <> struct SelType<SEL_FLOAT, 4> { using T = float; };
template <> struct SelType<SEL_FLOAT, 8> { using T = double; };

// ---------------------------------------------------------------- the chosen part
// The lowest set bit of `can`, or -1.
RDF_SEL_HD int sel_first(uint32_t can) {
    for (int k = 0; k < 32; ++k)
        if ((can >> k) & 1u) return k;
    return -1;
}
// coalesce: bit k of `valid` = part k is not NULL in the row.  The part whose bits the row takes, or -1: the row is NULL.
RDF_SEL_HD int sel_coalesce(uint32_t valid, int nparts) { return sel_first(valid & ((1u << nparts) - 1u)); }
// case_when: bit k of `holds` = condition k is valid AND true.  The value slot the row takes: the first such branch, else
// nbranches (`otherwise`; an absent one is the NULL literal).  The row is NULL when the chosen value is.
RDF_SEL_HD int sel_case_when(uint32_t holds, int nbranches) {
    const int k = sel_first(holds & ((1u << nbranches) - 1u));
    return k < 0 ? nbranches : k;
}

// One step of that chain on 64 rows at a time, as the kernels run it: `undecided` holds the rows no earlier part took, `can`
// the rows part k can decide.  -> the rows part k takes; they leave `undecided`.  (sel_first / sel_coalesce / sel_case_when
// above are the same rule for one row, the specification tests/cpp/test_select_host.cpp holds this function to.)
RDF_SEL_HD uint64_t sel_take(uint64_t& undecided, uint64_t can) {
    const uint64_t taken = undecided & can;
    undecided &= ~taken;
    return taken;
}

// ---------------------------------------------------------------- Spark's ordering, on bits
template <int CLS, int ES>
RDF_SEL_HD typename SelType<CLS, ES>::T sel_value(typename SelBits<ES>::U bits) {
    using T = typename SelType<CLS, ES>::T;
    static_assert(sizeof(T) == ES, "a value and its bits have one size");
    return __builtin_bit_cast(T, bits);
}
template <int CLS, int ES>
RDF_SEL_HD bool sel_is_nan(typename SelBits<ES>::U bits) {
    if (CLS != SEL_FLOAT) return false;
    const auto x = sel_value<CLS, ES>(bits);
    return x != x;
}
// a > b: NaN is greater than every number and equal to NaN
template <int CLS, int ES>
RDF_SEL_HD bool sel_gt(typename SelBits<ES>::U a, typename SelBits<ES>::U b) {
    if (CLS == SEL_FLOAT) {
        if (sel_is_nan<CLS, ES>(a)) return !sel_is_nan<CLS, ES>(b);
        if (sel_is_nan<CLS, ES>(b)) return false;
    }
    return sel_value<CLS, ES>(a) > sel_value<CLS, ES>(b);
}
template <int CLS, int ES>
RDF_SEL_HD bool sel_lt(typename SelBits<ES>::U a, typename SelBits<ES>::U b) { return sel_gt<CLS, ES>(b, a); }

// ---------------------------------------------------------------- extremum: one step of the left-to-right fold
// (acc, have) is the result over the parts so far; a NULL part (valid == false) is skipped.
template <int CLS, int ES>
RDF_SEL_HD void sel_fold(bool greatest, typename SelBits<ES>::U x, bool valid, typename SelBits<ES>::U& acc, bool& have) {
    const bool better = greatest ? sel_gt<CLS, ES>(x, acc) : sel_lt<CLS, ES>(x, acc);
    const bool take = valid && (!have || better);
    acc = take ? x : acc;
    have = have || valid;
}

// ---------------------------------------------------------------- nanvl(a, b): a unless it is NaN; NULL with a, or with b where a is NaN
template <int ES>
RDF_SEL_HD void sel_nanvl(typename SelBits<ES>::U a, bool a_valid, typename SelBits<ES>::U b, bool b_valid, typename SelBits<ES>::U& out, bool& valid) {
    const bool nan = sel_is_nan<SEL_FLOAT, ES>(a);
    valid = a_valid && (!nan || b_valid);
    out = valid ? (nan ? b : a) : (typename SelBits<ES>::U)0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The kernels' argument block and launchers (hipcc only; everything above is plain C++).
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "rdf_datetime.h"

enum SelKind : int { SEL_K_NULL_TEST = 0, SEL_K_COALESCE, SEL_K_CASE_WHEN, SEL_K_EXTREMUM, SEL_K_NANVL };

// One value slot of a call, read by the kernels through the constant address space: the slot index is a run-time loop
// counter, and a table entry is one scalar load of 32 bytes per wave tile and part
struct SelSlotDesc {
    const rdfk::DevChunkCol* col;     // [nchunks]; nullptr: the slot is the literal `lit`
    const rdfk::DevChunkCol* cond;    // case_when: [nchunks] RDF_BOOL chunks of the branch; nullptr for `otherwise`
    uint64_t lit;                     // a literal's bits in the low bytes
    uint64_t lit_null;                // != 0: the literal is NULL
};

struct SelArgs {
    CsCol    col;                     // row_start / tile_start of the call's chunking (chunks: null_test's column)
    const SelSlotDesc* slots;         // [nparts] (case_when: branches + 1, the last is `otherwise`)
    int32_t  nparts;
    int32_t  nconds;                  // case_when: branches
    const DtOut* outs;                // [nchunks]
    uint32_t* wave_nulls;             // as DtArgs
    int64_t*  chunk_nulls;
    int64_t   null_split;
    int32_t  kind;                    // SelKind
    int32_t  es, cls;                 // bytes and SEL_SIGNED / SEL_UNSIGNED / SEL_FLOAT of the value dtype
    int32_t  op;                      // null_test: SEL_IS_*; extremum: greatest != 0
};

hipError_t launch_select(const SelArgs& a, hipStream_t s);
#endif
