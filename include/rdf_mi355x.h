/*
 * rdf_mi355x.h — C ABI of librdf_mi355x.so, the MI355X (gfx950) engine for rust-dataframe's
 * Arrow compute hot path.
 *
 * The reference (nevi-me/rust-dataframe, Rust) has no FFI of its own; the seams this ABI replaces are
 * the Rust signatures named next to each entry point (paths relative to the reference root).  A Rust
 * shim binds these with `extern "C"` and passes raw Arrow buffer pointers
 * (`array.data().buffers()[0].raw_data()`, `null_buffer()`, `offset()`, `len()`, `null_count()`);
 * see INTEGRATION.md.
 *
 * Conventions (mirroring the reference):
 *   - inputs are borrowed and never written; outputs are caller-allocated and owned by the caller;
 *   - a column is a list of `nchunks` arrays (ChunkedArray, src/table.rs:13-18); chunk i of every
 *     column of a frame is RecordBatch i (src/dataframe.rs:128-163);
 *   - errors are values (rdf_status mirrors DataFrameError, src/error.rs:6-15); nothing aborts;
 *   - every entry point is re-entrant; state (stream, arena, last error) is per calling thread;
 *   - `mem` says where the buffers live: RDF_MEM_HOST (Arrow buffers in host RAM: staged to HBM,
 *     computed there, results copied back) or RDF_MEM_DEVICE (already resident in HBM: kernels run
 *     in place, nothing crosses PCIe).  All arrays of one call must share one `mem`.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute entry point returns
 *     RDF_DEVICE_ERROR.
 *
 * Buffer rules (Arrow columnar format): values little-endian natives, element `offset` is the first
 * logical element; validity is LSB-first, 1 = valid, NULL = all valid, and shares `offset`.
 * RDF_BOOL arrays are bit-packed in `values` like a validity bitmap.  Bitmap buffers must be
 * readable up to the next 8-byte boundary (Arrow allocates in 64-byte multiples).  Output buffers
 * with mem == RDF_MEM_DEVICE must have room for `capacity` elements rounded up to a multiple of 64
 * (values and bitmap alike).
 */
#ifndef RDF_MI355X_H
#define RDF_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* DataFrameError (src/error.rs:6-15) / ArrowError as raised on the path. */
typedef enum {
    RDF_OK = 0,
    RDF_COMPUTE_ERROR = 1,    /* ArrowError::ComputeError / DataFrameError::ComputeError */
    RDF_DIVIDE_BY_ZERO = 2,   /* ArrowError::DivideByZero / DataFrameError::DivideByZero */
    RDF_INVALID_ARGUMENT = 3, /* ArrowError::InvalidArgumentError, the reference's panic!("Unsupported operation") arms */
    RDF_MEMORY_ERROR = 4,     /* DataFrameError::MemoryError */
    RDF_DEVICE_ERROR = 5      /* no counterpart: HIP runtime failure / no gfx950 device */
} rdf_status;

/* arrow::datatypes::DataType subset that reaches the path (src/evaluation.rs:107-293). */
typedef enum {
    RDF_I8 = 0, RDF_I16 = 1, RDF_I32 = 2, RDF_I64 = 3,
    RDF_U8 = 4, RDF_U16 = 5, RDF_U32 = 6, RDF_U64 = 7,
    RDF_F32 = 8, RDF_F64 = 9, RDF_BOOL = 10,
    RDF_NULLTYPE = 11 /* only as the dtype of a Scalar::Null literal (src/expression.rs:719) */
} rdf_dtype;

typedef enum { RDF_MEM_HOST = 0, RDF_MEM_DEVICE = 1 } rdf_mem;

/* One Arrow array (chunk), borrowed and read-only: PrimitiveArray<T> / BooleanArray. */
typedef struct {
    const void*    values;
    const uint8_t* validity;   /* NULL = no nulls */
    int64_t        offset;     /* in elements (and bits) */
    int64_t        length;
    int64_t        null_count; /* -1 = unknown */
    int32_t        dtype;      /* rdf_dtype */
    int32_t        mem;        /* rdf_mem */
} rdf_array;

/* One output chunk.  Caller allocates `values` (capacity elements) and, when nulls can result,
 * `validity`; callee fills them and sets length / null_count.  Output offset is always 0. */
typedef struct {
    void*    values;
    uint8_t* validity;   /* may be NULL when no input carries a validity bitmap */
    int64_t  capacity;   /* in elements */
    int64_t  length;     /* set by callee */
    int64_t  null_count; /* set by callee */
    int32_t  dtype;
    int32_t  mem;
} rdf_out;

typedef enum {
    /* arrow::compute::{add,subtract,multiply,divide} via ScalarFunctions (src/functions/scalar.rs:16-103) */
    RDF_OP_ADD = 1, RDF_OP_SUB = 2, RDF_OP_MUL = 3, RDF_OP_DIV = 4,
    /* math_op users (src/functions/scalar.rs:148,274,291): atan2(a,b), hypot(a,b), log of a in base b */
    RDF_OP_ATAN2 = 5, RDF_OP_HYPOT = 6, RDF_OP_LOG = 7,
    /* scalar_op users (src/functions/scalar.rs:106-452) */
    RDF_OP_ABS = 8, RDF_OP_ACOS = 9, RDF_OP_ASIN = 10, RDF_OP_ATAN = 11, RDF_OP_CBRT = 12,
    RDF_OP_CEIL = 13, RDF_OP_COS = 14, RDF_OP_COSH = 15, RDF_OP_DEGREES = 16, RDF_OP_EXP = 17,
    RDF_OP_EXPM1 = 18, RDF_OP_FLOOR = 19, RDF_OP_LOG10 = 20, RDF_OP_LOG2 = 21, RDF_OP_RADIANS = 22,
    RDF_OP_ROUND = 23, RDF_OP_SIN = 24, RDF_OP_SINH = 25, RDF_OP_SQRT = 26, RDF_OP_TAN = 27,
    RDF_OP_TANH = 28,
    /* arrow::compute::cast (src/evaluation.rs:296-315) */
    RDF_OP_CAST = 29,
    /* BooleanFilter (src/expression.rs:752-763): comparisons are evaluated in f64 (:844-845) */
    RDF_OP_GT = 30, RDF_OP_GE = 31, RDF_OP_EQ = 32, RDF_OP_NE = 33, RDF_OP_LT = 34, RDF_OP_LE = 35,
    RDF_OP_NOT = 36, RDF_OP_AND = 37, RDF_OP_OR = 38,
    /* arrow::compute::hour via ScalarFunctions::hour (src/functions/scalar.rs:267-273), one opcode per time unit of
     * the temporal input (Time32 s/ms, Time64 us/ns, Date64 ms, Timestamp s/ms/us/ns; Date32 counts days: hour 0).
     * Operand Int32 or Int64 (the temporal types' storage), result of the operand's type, 0..23. */
    RDF_OP_HOUR_S = 39, RDF_OP_HOUR_MS = 40, RDF_OP_HOUR_US = 41, RDF_OP_HOUR_NS = 42, RDF_OP_HOUR_DAY = 43,
    /* ScalarFunction::{Cotangent, Secant, Cosecant} (src/expression.rs:670-672): plannable names the reference never
     * evaluates (its plan builder panics, :487-489).  Unary math like the others: 1 / tan(x), 1 / cos(x), 1 / sin(x) in
     * the operand's float type (IEEE division: cot(0) = +inf). */
    RDF_OP_COT = 44, RDF_OP_SEC = 45, RDF_OP_CSC = 46
} rdf_op;

/* time units of the temporal arrays handed to rdf_hour */
typedef enum { RDF_TIME_SECOND = 0, RDF_TIME_MILLISECOND = 1, RDF_TIME_MICROSECOND = 2, RDF_TIME_NANOSECOND = 3, RDF_TIME_DAY = 4 } rdf_time_unit;

/* ------------------------------------------------------------------ library / device plumbing */

const char* rdf_version(void);
/* Thread-local message of the last failing call -> DataFrameError::ComputeError(String). */
const char* rdf_last_error(void);
rdf_status  rdf_device_count(int32_t* count);
rdf_status  rdf_set_device(int32_t device);
/* Use the caller's hipStream_t for this thread (NULL = the library's own stream). */
rdf_status  rdf_set_stream(void* hip_stream);
rdf_status  rdf_synchronize(void);
rdf_status  rdf_dev_alloc(void** ptr, int64_t bytes);
rdf_status  rdf_dev_free(void* ptr);
rdf_status  rdf_copy_h2d(void* dst_dev, const void* src_host, int64_t bytes);
rdf_status  rdf_copy_d2h(void* dst_host, const void* src_dev, int64_t bytes);
/* Ingestion (DataFrame::from_csv / from_arrow, src/dataframe.rs:349-407): page-locked host buffers and uploads that do not
 * block the reader.  rdf_host_alloc gives a pinned buffer (a CSV parser writes its typed column into it, an IPC file is read
 * into it); rdf_host_register pins memory the caller already holds (a file image) — RDF_MEMORY_ERROR when the platform
 * refuses, the caller then uses rdf_copy_h2d.  rdf_copy_h2d_async queues the upload on the thread's copy stream and returns:
 * the source must be pinned and stay untouched until rdf_copy_fence, which waits for every queued upload of the thread.
 * Kernels launched after the fence see the data. */
rdf_status  rdf_host_alloc(void** ptr, int64_t bytes);
rdf_status  rdf_host_free(void* ptr);
rdf_status  rdf_host_register(void* ptr, int64_t bytes);
rdf_status  rdf_host_unregister(void* ptr);
rdf_status  rdf_copy_h2d_async(void* dst_dev, const void* src_host_pinned, int64_t bytes);
rdf_status  rdf_copy_fence(void);

/* ------------------------------------------------------------------ scalar kernels */

/* ScalarFunctions::{add,subtract,multiply,divide,par_multiply} (src/functions/scalar.rs:16-103) and
 * ::{atan2,hypot,log} (:148,:274,:291).  a[i] op b[i] per chunk pair; validity = AND; chunk length
 * mismatch -> RDF_COMPUTE_ERROR; DIV with a zero divisor at a valid slot -> RDF_DIVIDE_BY_ZERO;
 * integers wrap.  a, b, out: nchunks entries each, one dtype. */
rdf_status rdf_binary(int32_t op, const rdf_array* a, const rdf_array* b, int64_t nchunks, rdf_out* out);

/* ScalarFunctions::{abs,acos,...,tanh} through scalar_op (src/functions/scalar.rs:525-540):
 * out[i] = f(a[i]) where valid, null elsewhere. */
rdf_status rdf_unary(int32_t op, const rdf_array* a, int64_t nchunks, rdf_out* out);

/* Function::Cast arm (src/evaluation.rs:296-315): arrow::compute::cast per chunk to out[i].dtype.  The arrow crate of
 * the reference's era casts numeric arrays element by element through num::cast::cast and appends NULL where that
 * returns None: an integer that the target type cannot represent (-1 -> UInt8, 300 -> UInt8), NaN / an out-of-range
 * float on the way to an integer (floats truncate toward zero when the truncated value fits); int -> float, float -> float
 * and numeric <-> Boolean always succeed; input NULLs stay NULL.  Since a narrowing / sign-changing / float -> integer cast
 * can produce NULLs, its outputs need a validity buffer even when the input has none.  The same rule holds for
 * RDF_OP_CAST inside fused programs (the NULLs it produces are skipped by aggregates, dropped by filters). */
rdf_status rdf_cast(const rdf_array* a, int64_t nchunks, rdf_out* out);

/* ScalarFunctions::hour (src/functions/scalar.rs:267-273) = arrow::compute::hour per chunk: the hour of day of a
 * Time32 / Time64 / Date32 / Date64 / Timestamp array, passed as its Int32 / Int64 storage plus its `unit`
 * (rdf_time_unit; timestamps carry no time zone here, like the reference's).  out: RDF_I32 per chunk, NULL where
 * the input is NULL.  hour = floor_mod(floor_div(value, units per second), 86400) / 3600 — chrono's
 * NaiveDateTime::from_timestamp / NaiveTime::from_num_seconds_from_midnight for every value they accept; values
 * the reference panics on (a time of day outside [0, 86400 s), a negative sub-second remainder) follow the same
 * formula instead. */
rdf_status rdf_hour(const rdf_array* a, int64_t nchunks, int32_t unit, rdf_out* out);

/* ------------------------------------------------------------------ date and time functions
 *
 * ScalarFunctions::{year, quarter, month, day_of_month, day_of_week, day_of_year, week_of_year, minute, second, to_date,
 * date_trunc, trunc, date_add, date_sub, add_months, last_day, next_day, date_diff} (src/functions/scalar.rs declares them
 * with empty bodies): Spark 3's semantics over a temporal column passed as rdf_hour takes it — its Int32 / Int64 storage plus
 * its rdf_time_unit; no time zones.  Every unit but RDF_TIME_DAY accepts either storage type, RDF_TIME_DAY (Date32) is Int32.
 *
 * Calendar: proleptic Gregorian, astronomical year numbering (year 0 = 1 BC), day 0 = 1970-01-01, a Thursday.
 * Domain ("integers wrap", as rdf_binary): the day number of a value is floor_div(value, units per day) computed in Int64 and
 * truncated to Int32 by wrapping — only Int64 seconds / milliseconds beyond year +-5.8 million reach the wrap; the calendar
 * conversion is exact for every Int32 day number (-5877641-06-23 .. 5881580-07-11); hour, minute and second are exact for every
 * Int64.  No call fails or yields NULL because of a value's magnitude: an output needs a validity buffer only when an input
 * of its chunk has one (and for per-row next_day weekdays, see below).  NULL rows hold 0; an output's bitmap is the input's
 * re-based to bit 0 (two inputs: their AND), bits past `length` in its last byte are 0, as rdf_unary writes them.
 *
 * Fields, each RDF_I32: YEAR; QUARTER 1..4; MONTH 1..12; DAY_OF_MONTH 1..31; DAY_OF_WEEK 1 = Sunday .. 7 = Saturday;
 * DAY_OF_YEAR 1..366; WEEK_OF_YEAR the ISO-8601 week 1..53 (weeks start on Monday, week 1 holds the year's first Thursday);
 * HOUR 0..23 — the bytes rdf_hour returns; MINUTE 0..59; SECOND the whole second 0..59, the fraction dropped by floor;
 * DATE (to_date) the Int32 day number.  RDF_TIME_DAY values have hour = minute = second = 0.
 *
 * Refused with RDF_INVALID_ARGUMENT before any device work and with nothing written: an unknown unit, field, level or
 * operation; nfields outside 1..8 or a repeated field; a NULL list with nchunks > 0, negative nchunks; chunk lengths that
 * differ between paired columns; two memory kinds in one call; an input with validity but an output without; an output of
 * the wrong dtype; Int64 storage with RDF_TIME_DAY; chunks of two storage types.  An output capacity below its chunk's rows
 * is RDF_MEMORY_ERROR; a storage dtype other than Int32 / Int64 is RDF_COMPUTE_ERROR ("... does not support type").
 * nchunks == 0 is RDF_OK.  Without a device a valid call returns RDF_DEVICE_ERROR (no CPU fallback). */
typedef enum { RDF_DT_YEAR = 0, RDF_DT_QUARTER, RDF_DT_MONTH, RDF_DT_DAY_OF_MONTH, RDF_DT_DAY_OF_WEEK, RDF_DT_DAY_OF_YEAR,
               RDF_DT_WEEK_OF_YEAR, RDF_DT_HOUR, RDF_DT_MINUTE, RDF_DT_SECOND, RDF_DT_DATE } rdf_datetime_field;
typedef enum { RDF_TRUNC_YEAR = 0, RDF_TRUNC_QUARTER, RDF_TRUNC_MONTH, RDF_TRUNC_WEEK, RDF_TRUNC_DAY, RDF_TRUNC_HOUR,
               RDF_TRUNC_MINUTE, RDF_TRUNC_SECOND } rdf_trunc_level;
typedef enum { RDF_SHIFT_DAYS = 0, RDF_SHIFT_MONTHS, RDF_SHIFT_LAST_DAY, RDF_SHIFT_NEXT_DAY } rdf_date_shift_op;   /* (rdf_date_shift is the function) */

/* year / quarter / month / ... of one column in ONE read of it.  outs[f * nchunks + c]: field f of chunk c, RDF_I32.
 * 1 <= nfields <= 8, a field may not repeat. */
rdf_status rdf_datetime_fields(const rdf_array* a, int64_t nchunks, int32_t unit, const int32_t* fields, int32_t nfields, rdf_out* outs);
/* date_trunc(level, ts); trunc(date, fmt) is this call on RDF_TIME_DAY.  out: the input's storage type, same unit.
 * YEAR / QUARTER / MONTH: the first day of the period at midnight; WEEK: its Monday; DAY and finer: v - floor_mod(v, step).
 * Results wrap modulo 2^64 (2^32 for Int32 storage), reached only within the first or last partial period of a unit's range.
 * A level whose step is shorter than one unit (HOUR / MINUTE / SECOND on RDF_TIME_DAY) is RDF_INVALID_ARGUMENT; SECOND on
 * seconds is the identity. */
rdf_status rdf_datetime_trunc(const rdf_array* a, int64_t nchunks, int32_t unit, int32_t level, rdf_out* out);
/* date_add / date_sub / add_months / last_day / next_day.  out: always the RDF_I32 day number (Spark casts timestamps to
 * dates first); results wrap.  amounts == NULL: `amount` for every row; else an Int32 column chunked like a (validity
 * ANDed) and `amount` ignored.
 *   DAYS      date_add; a negative amount is date_sub
 *   MONTHS    add_months: the day of the month is kept and clamped to the last day of the target month
 *             (2016-08-31 + 1 -> 2016-09-30, 2019-02-28 + 1 -> 2019-03-28)
 *   LAST_DAY  the last day of the value's month; the amount is ignored, passing `amounts` is RDF_INVALID_ARGUMENT
 *   NEXT_DAY  the amount is the target weekday, 1 = Sunday .. 7 = Saturday: the first date STRICTLY later than the input on
 *             that weekday.  A scalar outside 1..7 is RDF_INVALID_ARGUMENT; a per-row amount outside 1..7 gives a NULL row,
 *             so that call needs an output bitmap (RDF_INVALID_ARGUMENT without one). */
rdf_status rdf_date_shift(const rdf_array* a, int64_t nchunks, int32_t unit, int32_t op, const rdf_array* amounts, int32_t amount, rdf_out* out);
/* date_diff(end, start) = day(end) - day(start) as RDF_I32, wrapping; each column has its own storage type and unit. */
rdf_status rdf_date_diff(const rdf_array* end, int32_t end_unit, const rdf_array* start, int32_t start_unit, int64_t nchunks, rdf_out* out);

/* ------------------------------------------------------------------ conditional and NULL functions */

/* ScalarFunctions::coalesce / greatest / least / nanv1 / when and Column::is_null (src/functions/scalar.rs declares them
 * with empty bodies): the row-wise choice between columns and literals, with Spark 3's semantics.  Stand-alone streaming
 * calls with the conventions of rdf_datetime_*: inputs are chunk lists of rdf_array (element offset, bit offset and chunking
 * are free; host or device memory, all of one kind), outputs are one rdf_out per chunk at offset 0, NULL rows hold 0, bits
 * past `length` in a bitmap's last byte are 0, null_count is set.  One kernel per call, plus the NULL-count reduce.
 *
 * A value part is a column (nchunks chunks) or a literal; all value parts and the output share ONE dtype, one of the ten
 * fixed-width numeric types RDF_I8 .. RDF_F64 (Boolean-valued and List-valued results: RDF_COMPUTE_ERROR, "does not support
 * type").  At least one part must be a column; its chunking gives the row counts.
 *
 *   null_test  IS_NULL / IS_NOT_NULL take any dtype, RDF_BOOL included; `values` is never read and may be NULL.  IS_NAN takes
 *              RDF_F32 / RDF_F64; isnan(NULL) is false.  The output is RDF_BOOL and never NULL: a bitmap, if given, is
 *              written all ones and null_count is 0.
 *   coalesce   1..8 parts: the first part that is not NULL in the row, its bits unchanged (NaN payloads and -0.0 kept); NULL
 *              when there is none.
 *   case_when  1..8 branches: conds[k] is nchunks RDF_BOOL chunks.  The row takes values[k] of the first k whose condition
 *              is valid AND true (a NULL condition is false), else `otherwise` (NULL pointer: NULL).  The result is NULL
 *              when the chosen value is.  One branch plus `otherwise` is if_else.
 *   extremum   2..8 parts: greatest != 0 gives greatest, else least.  NULL parts are skipped; the result is NULL only when
 *              every part is NULL.  Integers compare in their own signedness; floats under Spark's ordering: -0.0 == 0.0,
 *              NaN equals NaN and is greater than every number.  The fold is strict, so on a tie the LEFTMOST part's bits
 *              are returned: greatest(NaN, 1) = NaN, least(NaN, 1) = 1, greatest(-0.0, 0.0) is -0.0.
 *   nanvl      RDF_F32 / RDF_F64: a where a is not NaN, else b.  NULL when a is NULL, and when a is NaN and b is NULL.
 *
 * out[c].validity is required when the result of chunk c can be NULL, judged from the arguments alone — coalesce / extremum:
 * no part is never-NULL in chunk c (never-NULL: a non-NULL literal, or a column whose chunk c has no validity buffer);
 * case_when: `otherwise` is absent, or any value or `otherwise` can be NULL; nanvl: a or b can be NULL.  A bitmap given
 * without need is written (all ones).
 *
 * Refused before any device work and with nothing written, in this order, RDF_INVALID_ARGUMENT unless said otherwise: an
 * unknown test; nparts / nbranches outside their range; a NULL list with nchunks > 0, or negative nchunks; no column part; a
 * column part together with literal_is_null != 0; a condition that is not RDF_BOOL; value dtypes that differ from each other
 * or from the output; mixed memory kinds; a missing required bitmap; an unsupported dtype (RDF_COMPUTE_ERROR); chunk row
 * counts that differ between parts or conditions (RDF_COMPUTE_ERROR); a capacity below the rows (RDF_MEMORY_ERROR; every
 * chunk's `length` is set to the rows it needs, nothing else is written).  nchunks == 0 is RDF_OK.  Without a device a valid
 * call returns RDF_DEVICE_ERROR (no CPU fallback). */
#define RDF_SELECT_PARTS_MAX 8
typedef struct {
    const rdf_array* column;     /* nchunks chunks of this part, or NULL: the part is a literal      */
    uint64_t literal_bits;       /* the literal in the call's dtype, little endian in the low bytes  */
    int32_t  literal_is_null;    /* the literal is NULL (literal_bits ignored)                       */
} rdf_value_part;
typedef enum { RDF_IS_NULL = 0, RDF_IS_NOT_NULL = 1, RDF_IS_NAN = 2 } rdf_null_test_op;

rdf_status rdf_null_test(int32_t op, const rdf_array* a, int64_t nchunks, rdf_out* mask);
rdf_status rdf_coalesce(const rdf_value_part* parts, int32_t nparts, int64_t nchunks, rdf_out* out);
rdf_status rdf_case_when(const rdf_array* const* conds, const rdf_value_part* values, int32_t nbranches,
                         const rdf_value_part* otherwise, int64_t nchunks, rdf_out* out);
rdf_status rdf_extremum(int32_t greatest, const rdf_value_part* parts, int32_t nparts, int64_t nchunks, rdf_out* out);
rdf_status rdf_nanvl(const rdf_value_part* a, const rdf_value_part* b, int64_t nchunks, rdf_out* out);

/* ------------------------------------------------------------------ aggregate kernels */

/* AggregateFunctions::sum (src/functions/aggregate.rs:82-93): nulls skipped, empty/all-null -> 0,
 * always Some.  out_scalar has the array's native type (integers wrap). */
rdf_status rdf_sum(const rdf_array* a, int64_t nchunks, void* out_scalar, int32_t* out_is_some);
/* AggregateFunctions::min / max (:12-31) with the evident intent (min is min; floats accepted;
 * None when every slot is null or there are no chunks).  See DESIGN.md "divergences". */
rdf_status rdf_min(const rdf_array* a, int64_t nchunks, void* out_scalar, int32_t* out_is_some);
rdf_status rdf_max(const rdf_array* a, int64_t nchunks, void* out_scalar, int32_t* out_is_some);
/* AggregateFunctions::count (:70-80): sum(len - null_count) as i64; counts validity bits when
 * null_count is unknown (-1). */
rdf_status rdf_count(const rdf_array* a, int64_t nchunks, int64_t* out_count, int32_t* out_is_some);
/* AggregateFunctions::avg (:32-65): mean of the valid values as f64, None when there are none. */
rdf_status rdf_avg(const rdf_array* a, int64_t nchunks, double* out_mean, int32_t* out_is_some);

/* ------------------------------------------------------------------ moments: variance, stddev, skewness, kurtosis, corr
 *
 * AggregateFunctions::variance / stddev / skewness / kurtosis (declared with empty bodies and a TODO for "population and
 * sample" forms, src/functions/aggregate.rs:94-102) and ScalarFunctions::corr (src/functions/scalar.rs:184), with Spark's
 * semantics.  One pass over the column produces a STATE; the statistics are read off the state on the host, and states
 * of shards, ranks or slabs combine with rdf_moments_merge (Chan / Pebay's pairwise update).
 *
 *   count            rows that count
 *   mean + mean_lo   their mean as an unevaluated sum of two doubles
 *   m2, m3, m4       sum (x - mean)^k over them
 *   m2x, m2y, cxy    the same sums per column, and sum (x - mean_x)(y - mean_y)
 * Zero rows give a state of all zeros.
 *
 * a / x / y: any of the ten numeric dtypes (x and y may differ), every value converted `as f64` like rdf_avg; chunks may
 * carry any offset and validity.  mask: NULL, or nchunks RDF_BOOL chunks of the same lengths.  A row counts when its value
 * is valid (rdf_comoments: both values), the mask slot is valid and the mask bit is set — Column::filter's rule, so
 * filter -> variance is one pass with no compacted copy.
 *
 * The kernel never forms sum x^2: every tile of rows is centred on its own mean first and tile states are merged, so a
 * column such as 1e9 + noise keeps every digit (DESIGN.md 13 has the bound).  The same input gives the same bytes on
 * every call, from host and from device memory.  A non-finite valid value makes every statistic except the count NaN
 * (rdf_avg stays the way to an infinite mean).  Deviations whose fourth power overflows a double (|x - mean| >~ 1e77) give
 * inf or NaN in m4 (m3 from ~1e102, m2 from ~1e154).
 *
 * Refused with RDF_INVALID_ARGUMENT before any device work: a non-numeric dtype or chunks of different dtypes, chunk
 * lengths that differ between x, y and mask, a mask that is not RDF_BOOL, a NULL `out`, an unknown stat.  nchunks == 0
 * (and zero rows) is the zero state and RDF_OK.  The merge and stat functions run on the host and need no device.
 *
 * Statistics (out_is_some = 0: count == 0; a _SAMP statistic with count < 2; SKEWNESS / KURTOSIS with m2 == 0; CORR with
 * m2x or m2y == 0):
 *   VAR_POP m2 / n, VAR_SAMP m2 / (n - 1), STDDEV_* their square roots, SKEWNESS sqrt(n) m3 / m2^1.5,
 *   KURTOSIS n m4 / m2^2 - 3 (excess), COVAR_POP cxy / n, COVAR_SAMP cxy / (n - 1), CORR cxy / sqrt(m2x m2y). */
typedef struct { int64_t count; double mean, mean_lo, m2, m3, m4; } rdf_moments_state;
typedef struct { int64_t count; double mean_x, mean_x_lo, mean_y, mean_y_lo, m2x, m2y, cxy; } rdf_comoments_state;
typedef enum { RDF_STAT_MEAN = 0, RDF_STAT_VAR_POP, RDF_STAT_VAR_SAMP, RDF_STAT_STDDEV_POP, RDF_STAT_STDDEV_SAMP,
               RDF_STAT_SKEWNESS, RDF_STAT_KURTOSIS } rdf_stat;
typedef enum { RDF_COSTAT_COVAR_POP = 0, RDF_COSTAT_COVAR_SAMP, RDF_COSTAT_CORR } rdf_costat;

rdf_status rdf_moments(const rdf_array* a, const rdf_array* mask, int64_t nchunks, rdf_moments_state* out);
rdf_status rdf_comoments(const rdf_array* x, const rdf_array* y, const rdf_array* mask, int64_t nchunks, rdf_comoments_state* out);
/* into <- the state of the rows of `into` and of `other` together.  Merging with the zero state is the identity. */
rdf_status rdf_moments_merge(rdf_moments_state* into, const rdf_moments_state* other);
rdf_status rdf_comoments_merge(rdf_comoments_state* into, const rdf_comoments_state* other);
rdf_status rdf_moments_stat(const rdf_moments_state* s, int32_t stat, double* out, int32_t* out_is_some);
rdf_status rdf_comoments_stat(const rdf_comoments_state* s, int32_t stat, double* out, int32_t* out_is_some);

/* ------------------------------------------------------------------ expressions */

typedef enum { RDF_NODE_COLUMN = 0, RDF_NODE_SCALAR = 1, RDF_NODE_OP = 2 } rdf_node_kind;

/* One node of an expression tree stored as an array, children before parents.  It restates
 * BooleanFilter / BooleanInput / Scalar (src/expression.rs:718-763) and, for value expressions,
 * a run of Calculation steps (src/expression.rs:410-500) folded into one tree. */
typedef struct {
    int32_t kind;    /* rdf_node_kind */
    int32_t op;      /* rdf_op when kind == RDF_NODE_OP */
    int32_t dtype;   /* SCALAR: literal type (RDF_NULLTYPE for Scalar::Null); OP CAST: target type */
    int32_t lhs;     /* child node index or -1 */
    int32_t rhs;     /* child node index or -1 */
    int32_t column;  /* COLUMN: index into the cols argument */
    double  f64;     /* SCALAR of RDF_F32 / RDF_F64 */
    int64_t i64;     /* SCALAR of integer / RDF_BOOL type */
} rdf_expr_node;

/* BooleanFilter::eval_to_array for every RecordBatch (src/expression.rs:766-861 as driven by
 * DataFrame::evaluate_boolean_filter, src/dataframe.rs:612-624).  cols is laid out
 * cols[c * nchunks + i] = chunk i of column c.  mask: nchunks RDF_BOOL outputs (values + validity
 * bitmaps); the value bit of a null slot is 0.  The root must be boolean-typed. */
rdf_status rdf_predicate(const rdf_expr_node* nodes, int32_t nnodes, int32_t root,
                         const rdf_array* cols, int32_t ncols, int64_t nchunks, rdf_out* mask);

/* ------------------------------------------------------------------ filter / take */

/* Rows Column::filter would keep per chunk (two-phase filter: size the outputs with this). */
rdf_status rdf_filter_count(const rdf_array* mask, int64_t nchunks, int64_t* counts);
/* Column::filter -> ChunkedArray::filter -> arrow::compute::filter per chunk pair
 * (src/table.rs:97-107,213-215): keeps rows whose mask bit is set (and valid), order and chunk
 * boundaries preserved, validity carried.  mask[i].length must equal col[i].length. */
rdf_status rdf_filter(const rdf_array* col, const rdf_array* mask, int64_t nchunks, rdf_out* out);
/* DataFrame::filter's per-column loop (src/dataframe.rs:183-187) as ONE pass: ranks are computed
 * once per tile and every column is compacted with them.  cols/outs laid out [c * nchunks + i];
 * 1..256 columns per call. */
rdf_status rdf_filter_columns(const rdf_array* cols, int32_t ncols, const rdf_array* mask,
                              int64_t nchunks, rdf_out* outs);
/* Column::take (src/table.rs:218-241): gather over the virtual concatenation of the chunks
 * (Column::to_array, :180-182, without the concat copy).  indices: ONE RDF_U32 (drop-in) or RDF_U64
 * array; null index -> null; out of range -> RDF_COMPUTE_ERROR.  out: ONE chunk (B4 in SURVEY.md). */
rdf_status rdf_take(const rdf_array* chunks, int64_t nchunks, const rdf_array* indices, rdf_out* out);

/* ------------------------------------------------------------------ sort */

/* SortCriteria (src/expression.rs:305-318) as arrow's SortOptions: the reference always passes
 * nulls_first = false (src/dataframe.rs:208), so nulls sort last whatever this field says. */
typedef struct { int32_t descending; int32_t nulls_first; } rdf_sort_options;

/* DataFrame::sort -> arrow::compute::lexsort_to_indices (src/dataframe.rs:194-214): the row order given
 * by the sort columns, column 0 most significant; ties keep ascending row order (stable); floats in
 * IEEE total order (NaN after +inf).  cols[c * nchunks + i]; indices refer to the concatenation of the
 * chunks (what Column::take consumes).  out_indices: ONE RDF_U32 array of all rows. */
rdf_status rdf_sort_to_indices(const rdf_array* cols, int32_t ncols, int64_t nchunks, const rdf_sort_options* opts,
                               rdf_out* out_indices);

/* ------------------------------------------------------------------ join */

typedef enum { RDF_JOIN_LEFT = 0, RDF_JOIN_RIGHT = 1, RDF_JOIN_INNER = 2, RDF_JOIN_FULL = 3 } rdf_join_type;  /* JoinType, src/expression.rs:339-345 */

/* calc_equijoin_indices (src/functions/join.rs:19-137) for ONE numeric key column per side (same dtype: the
 * caller casts first, as join.rs:17-18 says): the (left row, right row) pairs of the equi-join, as two
 * UInt32 index arrays with NULL where a side has no partner — exactly what DataFrame::join feeds to
 * Column::take (src/dataframe.rs:705-711).  NULL keys never match; LEFT/RIGHT/FULL keep them with a
 * NULL partner.  FULL is a true full outer join (the reference's FullJoin arm drops unmatched non-NULL
 * rows: not copied).  Pair order: probe rows ascending, partners ascending, then (FULL) the unmatched
 * build rows in unspecified order — the reference's order is HashMap iteration order.  (RIGHT probes with
 * the right rows: right rows ascending, their left partners ascending.)
 * Keys are equal when their BITS are equal, as in the reference's HashMap over key bytes: a Float32 /
 * Float64 key -0.0 does not join +0.0, and a NaN joins exactly the NaNs of its own sign and payload.
 * *out_rows = rows of the result; with out_left == out_right == NULL only the count is computed;
 * capacity too small -> RDF_MEMORY_ERROR with *out_rows set. */
rdf_status rdf_equijoin_indices(const rdf_array* left_keys, int64_t left_nchunks, const rdf_array* right_keys,
                                int64_t right_nchunks, int32_t join_type, rdf_out* out_left, rdf_out* out_right,
                                int64_t* out_rows);
/* The same for 1..4 key columns per side (JoinCriteria.criteria holds a Vec of column pairs, src/expression.rs:332-337;
 * build_hash_inputs hashes the tuple, src/functions/join.rs:139-235): left_keys[k * left_nchunks + i] pairs with
 * right_keys[k * right_nchunks + i]; pair k shares one dtype; a row with a NULL in any key column never matches.
 * Rows are matched through a 64-bit hash of the tuple and every candidate pair is verified column by column. */
rdf_status rdf_equijoin_indices_multi(const rdf_array* left_keys, int64_t left_nchunks, const rdf_array* right_keys,
                                      int64_t right_nchunks, int32_t nkeys, int32_t join_type, rdf_out* out_left,
                                      rdf_out* out_right, int64_t* out_rows);

/* ------------------------------------------------------------------ group-by */

/* Transformation::GroupAggregate(groups, [Sum, Count]) for ONE integer key column — planned by
 * Dataset::try_aggregate (src/expression.rs:114-221) but not executed by the reference
 * (src/evaluation.rs:73 panics), so the semantics are SQL's: NULL keys form one group, NULL values
 * are skipped, a group's count is its number of non-null values (of rows when values == NULL).
 * Outputs are ONE chunk each, in unspecified group order: keys (key dtype), sums (Float64 for float
 * values, wrapping Int64 otherwise), counts (Int64); capacity >= max_groups + 2.  More than
 * max_groups distinct keys -> RDF_MEMORY_ERROR.  f64 sums are accumulated with hardware atomics:
 * the rounding order is not deterministic (within 1e-6 relative of any sequential order). */
rdf_status rdf_groupby_sum(const rdf_array* keys, const rdf_array* values, int64_t nchunks, int64_t max_groups,
                           rdf_out* out_keys, rdf_out* out_sums, rdf_out* out_counts);   /* = rdf_groupby_agg(keys, 1, values, ..., RDF_AGG_SUM, ...) */

/* AggregateFunction (src/expression.rs:696-711).  Avg is Sum / Count on the caller's side (AggregateFunctions::avg,
 * src/functions/aggregate.rs:32-65). */
typedef enum { RDF_AGG_SUM = 0, RDF_AGG_MIN = 1, RDF_AGG_MAX = 2, RDF_AGG_COUNT = 3 } rdf_agg_fn;

#define RDF_MAX_GROUP_KEYS 4

/* Transformation::GroupAggregate(groups, [aggregation]) for 1..RDF_MAX_GROUP_KEYS integer grouping columns and ONE
 * aggregation of one value column (Dataset::try_aggregate, src/expression.rs:114-221, plans a list of them: one call
 * each; the reference never executes the step, src/evaluation.rs:73 panics — SQL semantics, parity unpinned by the
 * reference).  keys[k * nchunks + i] = chunk i of grouping column k; a NULL in a grouping column is a group value of
 * its own; NULL values are skipped; counts[g] = non-NULL values of group g (rows, for RDF_AGG_COUNT / values == NULL).
 * out_keys: nkeys one-chunk outputs (key dtypes; validity required for a nullable grouping column);
 * out_values: Float64 for float values, UInt64 for MIN / MAX of UInt64 values, Int64 otherwise (sums wrap);
 *   MIN / MAX of a group without a non-NULL value is NULL (validity required when the value column is nullable);
 *   NaN never wins a MIN / MAX unless every value of the group is NaN (the column aggregates' rule, rdf_min / rdf_max);
 * out_counts: Int64.  Capacities >= min(max_groups, rows) + 2; group order unspecified.  More than max_groups distinct key
 * tuples (the NULL tuple is one of them) -> RDF_MEMORY_ERROR; exactly max_groups succeed.  Several grouping columns are
 * packed into one 64-bit key after range compression (bits(max - min) per column, + 1 code for NULL); when the ranges together pass 64 bits (several sparse columns) the
 * widest columns are dictionary-coded instead (rank among the column's distinct values, found by a count-only GROUP BY
 * of that column).  Tuples needing more than 64 bits either way -> RDF_INVALID_ARGUMENT.
 * f64 sums are accumulated with hardware atomics: the rounding order is not deterministic (<= 1e-6 relative). */
rdf_status rdf_groupby_agg(const rdf_array* keys, int32_t nkeys, const rdf_array* values, int64_t nchunks, int32_t agg,
                           int64_t max_groups, rdf_out* out_keys, rdf_out* out_values, rdf_out* out_counts);

/* Merge of partial groups: (key, partial aggregate, count) triples -> one row per key, partials combined by `agg`
 * (sums added, minima / maxima compared, counts added).  What a rank does with the partial groups it receives in the
 * multi-GPU GROUP BY (replaces the panic! at src/evaluation.rs:73 for RecordBatches sharded over GPUs).
 * One chunk each: keys Int64 / UInt64, partial Float64 / Int64 / UInt64 (may be NULL for counts only), counts Int64;
 * a partial with count 0 (or a NULL one) contributes nothing but its key.  Outputs as rdf_groupby_agg. */
rdf_status rdf_groupby_merge(const rdf_array* keys, const rdf_array* partial, const rdf_array* counts, int32_t agg,
                             int64_t max_groups, rdf_out* out_keys, rdf_out* out_values, rdf_out* out_counts);

/* The exchange itself, device-resident: rows (key, partial, count) of this rank's local groups are bucketed by owning
 * rank, owner = ((key * 0x9E3779B97F4A7C15) >> 33) % world, into `packed_dev` — n rows of 3 x 64-bit words, the rows of
 * owner 0 first — and owner_counts[r] (host) receives the number of rows for rank r: exactly the send buffer and split
 * sizes of an all_to_all(v) (RCCL over xGMI on the GPU box).  _unpack splits a received buffer back into three columns
 * for rdf_groupby_merge.  RDF_MEM_DEVICE only; 8-byte key and partial dtypes; no NULL keys. */
rdf_status rdf_group_exchange_pack(const rdf_array* keys, const rdf_array* partial, const rdf_array* counts, int32_t world,
                                   void* packed_dev, int64_t* owner_counts);
rdf_status rdf_group_exchange_unpack(const void* packed_dev, int64_t n, rdf_out* keys, rdf_out* partial, rdf_out* counts);
/* The row-shuffle fallback of the same exchange: when a rank's rows hold about as many groups as rows, pre-aggregating
 * them gains nothing — the rows themselves are bucketed by owner (16 bytes each: key, value; no NULLs), exchanged the
 * same way, and every rank runs rdf_groupby_agg over the rows it received.  packed_dev: 16 * rows bytes. */
rdf_status rdf_row_exchange_pack(const rdf_array* keys, const rdf_array* values, int32_t world, void* packed_dev, int64_t* owner_counts);
rdf_status rdf_row_exchange_unpack(const void* packed_dev, int64_t n, rdf_out* keys, rdf_out* values);

/* ------------------------------------------------------------------ ArrayFunctions over List<primitive> columns */

/* A ListArray with primitive numeric children as the reference's ArrayFunctions see it (src/functions/array.rs):
 * row i is the slice values[value_offset(i) .. value_offset(i + 1)) of the child array.  `offsets` is the Int32
 * value_offsets buffer described as an RDF_I32 array of rows + 1 elements whose validity / offset / null_count
 * fields describe the LIST rows (bit i = list i is not NULL); `values` is the child array.  Child validity is
 * ignored, exactly as the reference's value_slice() ignores it. */
typedef struct {
    rdf_array offsets;
    rdf_array values;
} rdf_list_array;

/* ArrayFunctions::array_contains (array.rs:15-37): NULL list -> NULL, else whether the slice holds `value`
 * (a native scalar of the child dtype; float equality is IEEE: NaN equals nothing).  out: RDF_BOOL, rows elements. */
rdf_status rdf_list_contains(const rdf_list_array* list, const void* value, rdf_out* out);
/* ArrayFunctions::array_position (array.rs:233-260): 1-based position of the first occurrence, 0 when absent or
 * when the list is NULL (never NULL).  out: RDF_I32. */
rdf_status rdf_list_position(const rdf_list_array* list, const void* value, rdf_out* out);
/* ArrayFunctions::array_max / array_min (array.rs:182-231): per-row extremum, NULL for a NULL list.  An EMPTY
 * list gives NULL (the reference unwraps None and panics); floats are accepted, NaN loses against any number
 * (the column aggregates' rule; a row of nothing but NaNs gives a NaN of unspecified sign and payload), and -0.0
 * orders below +0.0 as in array_sort: max{-0.0, +0.0} is +0.0 wherever the zeros stand.  A NULL result holds 0.
 * out: child dtype.
 * The bitmaps rdf_list_contains / _position / _max / _min write to device memory (RDF_MEM_DEVICE: the RDF_BOOL values
 * of array_contains and every output validity) are stored in whole 64-bit words: such a buffer holds
 * ceil(rows / 64) * 8 bytes and is 8-byte aligned. */
rdf_status rdf_list_max(const rdf_list_array* list, rdf_out* out);
rdf_status rdf_list_min(const rdf_list_array* list, rdf_out* out);
/* ArrayFunctions::array_remove (array.rs:262-292): every element equal to `value` dropped, order kept; a NULL
 * list becomes an empty (valid) list like the reference's ListBuilder::append(true).  out_offsets: RDF_I32 with
 * rows + 1 elements (starting at 0), out_values: child dtype, capacity >= the slice total. */
rdf_status rdf_list_remove(const rdf_list_array* list, const void* value, rdf_out* out_offsets, rdf_out* out_values);
/* ArrayFunctions::array_sort (array.rs:320-354): every row's slice sorted ascending (floats in IEEE total order);
 * the value_offsets do not change.  out_values: the child values of rows 0 .. rows-1 re-ordered, i.e.
 * values[value_offset(0) .. value_offset(rows)). */
rdf_status rdf_list_sort(const rdf_list_array* list, rdf_out* out_values);
/* The set-valued ArrayFunctions, each row rebuilt with the array_tool crate's Vec algebra (Cargo.toml:19) under the
 * element type's `==` (NaN equals nothing).  Outputs as for rdf_list_remove; a NULL row of `list` / `a` becomes an
 * empty valid list, `b`'s validity is not looked at (array.rs:82,126,372).
 *   array_distinct  (array.rs:39-65):   `unique()`      first occurrences, in order.  The reference never closes the
 *                                        row of a non-NULL list (no `b.append(true)`, a private, untested function);
 *                                        this entry point returns the evident per-row result.
 *   array_except    (array.rs:66-109):  `a.uniq(b)`     unique(a) without the members of b
 *   array_intersect (array.rs:110-153): `a.intersect(b)` unique(a) restricted to the members of b
 *   array_union     (array.rs:356-399): `a.union(b)`    unique(a ++ b)
 *   array_repeat    (array.rs:294-326): `times(count)`  the row's slice `count` times over (count >= 0)
 * a and b must have the same number of rows (RDF_COMPUTE_ERROR "Expected array a and b to have the same length")
 * and the same child dtype; a result with more than 2^31-1 elements is RDF_COMPUTE_ERROR (Int32 value_offsets).
 * out_values capacity: distinct / except / intersect <= elements of a, union <= a + b, repeat = a * count. */
rdf_status rdf_list_distinct(const rdf_list_array* list, rdf_out* out_offsets, rdf_out* out_values);
rdf_status rdf_list_except(const rdf_list_array* a, const rdf_list_array* b, rdf_out* out_offsets, rdf_out* out_values);
rdf_status rdf_list_intersect(const rdf_list_array* a, const rdf_list_array* b, rdf_out* out_offsets, rdf_out* out_values);
rdf_status rdf_list_union(const rdf_list_array* a, const rdf_list_array* b, rdf_out* out_offsets, rdf_out* out_values);
rdf_status rdf_list_repeat(const rdf_list_array* list, int32_t count, rdf_out* out_offsets, rdf_out* out_values);

/* ------------------------------------------------------------------ Utf8 (StringArray) columns */

/* A StringArray (Utf8, Int32 offsets): row i is the bytes data[offsets[i] .. offsets[i+1]).  `offsets` is an RDF_I32
 * array of rows + 1 elements whose validity / offset / null_count describe the ROWS; `data` is an RDF_U8 array of the
 * value bytes (its validity is ignored).  Bytes are valid UTF-8 (Arrow's guarantee; not re-checked). */
typedef struct { rdf_array offsets; rdf_array data; } rdf_utf8_array;

/* Column::filter / Column::take and the string ScalarFunctions over chunked StringArrays.  `chunks[i]` is chunk i; the
 * outputs are out_offsets[i] (RDF_I32, rows + 1 entries starting at 0, row validity in its `validity` and `null_count`)
 * and out_data[i] (RDF_U8).  A NULL input row gives a NULL output row of zero bytes (StringBuilder::append(false)).
 * Sizing, one rule for all of them: on return out_data[i].length holds the bytes of chunk i (out_offsets[i].length its
 * rows + 1).  If any out_data[i].capacity (or, for filter, out_offsets[i].capacity) is too small the call returns
 * RDF_MEMORY_ERROR with those lengths set for every chunk and nothing written: values == NULL, capacity == 0 is the
 * sizing call.  Input bytes bound the output of filter, trim and substring, 3 x input bytes that of lower / upper.
 * An output chunk beyond 2^31-1 bytes is RDF_COMPUTE_ERROR (Int32 offsets).  Input offsets are used as given (offset
 * by the row `offset`, the first not necessarily 0); the first and last must lie within data.length.  An output whose
 * rows can be NULL needs out_offsets[i].validity.
 *   filter:    Column::filter (src/table.rs:97-107): per chunk the rows whose mask bit is set AND valid, order and chunk
 *              boundaries kept; mask[i].length == rows of chunk i.
 *   take:      Column::take (src/table.rs:213-241): gather over the virtual concatenation of the chunks; `indices` is one
 *              RDF_U32 / RDF_U64 array; a NULL index gives NULL, out of range RDF_COMPUTE_ERROR.  ONE output chunk.
 *   trim / ltrim / rtrim: str::trim / trim_start / trim_end: Unicode White_Space (Rust's char::is_whitespace) stripped.
 *   substring: chars().skip(pos).take(len) (scalar.rs:428-441), counted in code points; pos, len >= 0.
 *   lower / upper: str::to_lowercase / to_uppercase: full Unicode case mapping (one-to-many mappings, Final_Sigma), from
 *              the Unicode version recorded in rdf_unicode_case.h. */
rdf_status rdf_utf8_filter(const rdf_utf8_array* chunks, const rdf_array* mask, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_take(const rdf_utf8_array* chunks, int64_t nchunks, const rdf_array* indices, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_trim(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_ltrim(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_rtrim(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_substring(const rdf_utf8_array* chunks, int64_t nchunks, int64_t pos, int64_t len, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_lower(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_upper(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);

/* ------------------------------------------------------------------ Utf8 predicates and measures */

/* Masks and integers from text: WHERE city = 'London', name LIKE 'A%', length(s) > 10.  The reference declares length,
 * locate, ... as empty stubs (src/functions/scalar.rs:287-290) and compares strings as Float64 (src/expression.rs:844-845),
 * so these follow SQL / Spark; the executable model is tests/utf8_pred_ref.py.
 * Inputs follow the rdf_utf8_array conventions exactly as rdf_utf8_trim takes them (row `offset`, value offsets that need
 * not start at 0, validity at any bit offset, host or device memory, all one kind).  mask[i] is an RDF_BOOL output per
 * chunk, out[i] an RDF_I32 one; both have length == rows and offset 0.  A NULL row gives a NULL result (validity bit 0,
 * value bit / value 0); null_count is set.  An output needs a `validity` buffer whenever its chunk (for rdf_utf8_compare:
 * either of its chunks) has one.  Bits beyond the last row in the last byte are 0; nothing is written past (rows + 7) / 8
 * bytes of a caller's bitmap.  The results feed rdf_utf8_filter, rdf_filter, rdf_filter_columns, rdf_moments' mask, and
 * rdf_predicate as Boolean input columns.  Neither the rows nor the pattern are validated as UTF-8: literals compare as
 * bytes, and a code point begins at a byte that is not a continuation byte, as rdf_utf8_substring counts them.
 *   EQ .. GE:  unsigned byte order, the same as rdf_lexsort_to_indices: a proper prefix sorts first, 0x00 is an ordinary
 *              byte, "é" > "z".  rdf_utf8_predicate compares every row with the `pattern_bytes` bytes of `pattern`;
 *              rdf_utf8_compare is the column-against-column form and takes these six ops only: a and b have the same
 *              chunking, a row is NULL if either side is.
 *   STARTS_WITH / ENDS_WITH / CONTAINS: the bytes of `pattern` as a literal; an empty pattern is true for every non-NULL
 *              row; a match never extends past its own row.
 *   LIKE:      '%' matches any run of code points, the empty run included, '_' exactly one code point; the whole row must
 *              match.  `escape` is -1 (none) or one ASCII byte 1..127 other than '%' and '_'; the escape followed by any
 *              character means that character literally; a pattern ending in a lone escape is RDF_INVALID_ARGUMENT, and so
 *              is one with more than 32 non-empty segments between its '%'.  `escape` is checked for every op and used by
 *              LIKE only.
 *   LENGTH / OCTET_LENGTH: code points / bytes of the row; `pattern` and `pos` are ignored.
 *   LOCATE:    the 1-based code-point position of the first occurrence of `pattern` at or after code-point position `pos`,
 *              0 if there is none or pos < 1: s.find(sub, pos - 1) + 1 if pos >= 1 else 0 on a Python str, the empty
 *              needle included (locate("", "abc", 4) == 4, pos 5 gives 0).  instr is pos = 1.
 * Errors, all before any device work, in this order: an unknown op or a non-comparison op given to rdf_utf8_compare;
 * pattern_bytes < 0 or > RDF_UTF8_PATTERN_MAX; pattern == NULL with pattern_bytes > 0; a bad escape; wrong dtypes; mixed
 * memory kinds; a missing validity buffer: RDF_INVALID_ARGUMENT.  Chunk row counts that differ between a and b:
 * RDF_COMPUTE_ERROR.  A capacity below the rows: RDF_MEMORY_ERROR with `length` set.  No device: RDF_DEVICE_ERROR.
 * nchunks == 0 is RDF_OK. */
typedef enum { RDF_UTF8_EQ = 0, RDF_UTF8_NE, RDF_UTF8_LT, RDF_UTF8_LE, RDF_UTF8_GT, RDF_UTF8_GE,
               RDF_UTF8_STARTS_WITH, RDF_UTF8_ENDS_WITH, RDF_UTF8_CONTAINS, RDF_UTF8_LIKE } rdf_utf8_pred_op;
typedef enum { RDF_UTF8_LENGTH = 0, RDF_UTF8_OCTET_LENGTH = 1, RDF_UTF8_LOCATE = 2 } rdf_utf8_measure_op;
#define RDF_UTF8_PATTERN_MAX 1024   /* bytes of a literal / pattern */

rdf_status rdf_utf8_predicate(int32_t op, const rdf_utf8_array* chunks, int64_t nchunks,
                              const uint8_t* pattern, int64_t pattern_bytes, int32_t escape, rdf_out* mask);
rdf_status rdf_utf8_compare(int32_t op, const rdf_utf8_array* a, const rdf_utf8_array* b, int64_t nchunks, rdf_out* mask);
rdf_status rdf_utf8_measure(int32_t what, const rdf_utf8_array* chunks, int64_t nchunks,
                            const uint8_t* pattern, int64_t pattern_bytes, int64_t pos, rdf_out* out);

/* ------------------------------------------------------------------ Utf8 builders */

/* Text columns made of more than one source: city || ', ' || country as a GROUP BY key, a zero-padded id, the host part of
 * a URL.  The reference declares concat, concat_ws, lpad, rpad, repeat, reverse and substring_index with empty bodies
 * (src/functions/scalar.rs), so these follow Spark 3; the executable model is tests/utf8_build_ref.py.
 * Inputs follow the rdf_utf8_array conventions exactly as rdf_utf8_trim takes them (row `offset`, value offsets that need
 * not start at 0, validity at any bit offset, host or device memory, all one kind).  Outputs are chunked like the inputs:
 * out_offsets[i] / out_data[i] hold the rows of input chunk i, under the one sizing rule of rdf_utf8_filter .. _upper
 * (values == NULL, capacity == 0 is the sizing call; a capacity that is too small gives RDF_MEMORY_ERROR with every length
 * set and nothing written; an output chunk beyond 2^31-1 bytes is RDF_COMPUTE_ERROR).  An output whose rows can be NULL
 * needs out_offsets[i].validity; null_count is set.  A code point begins at every byte that is not a continuation byte,
 * as rdf_utf8_measure(LENGTH) counts them; bytes are not validated.
 *   concat     (with_separator == 0; sep_bytes must be 0) the parts joined in order; a part is a column (nchunks chunks) or
 *              a literal; a row is NULL if any column part is NULL in that row.
 *   concat_ws  (with_separator == 1) NULL parts are skipped and `sep` stands between the remaining ones; empty strings are
 *              not skipped; the result is never NULL (a row without a non-NULL part is the empty string): a validity buffer,
 *              if given, is written all ones and null_count is 0.
 *              Both: all column parts share one chunking; at least one part is a column (the row count is its).
 *   pad        side 0 = lpad, 1 = rpad.  With n the row's and p the pad's code points: len <= 0 gives the empty string;
 *              n >= len or an empty pad gives the first min(n, len) code points of the row (the row is TRUNCATED);
 *              otherwise the pad repeated (len - n) / p times followed by its first (len - n) % p code points stands left
 *              (right) of the row.
 *   repeat     the row `times` times; times <= 0 gives the empty string.
 *   reverse    the row's code points in reverse order, each one's bytes kept in order (not grapheme clusters).  On bytes
 *              that are not valid UTF-8 the output row has the input row's length and nothing outside the row is touched.
 *   substring_index  byte-wise: for count > 0 everything left of the count-th occurrence of `delim` from the left, for
 *              count < 0 everything right of the |count|-th from the right; each search resumes one byte after (before) the
 *              START of the previous hit, so occurrences may overlap ('aaaa', 'aa', 2 -> 'a'); with fewer occurrences the
 *              whole row; an empty delim or count == 0 gives the empty string.
 *   A NULL row gives NULL for pad, repeat, reverse and substring_index.  len and times are clamped to 2^31, and so is a
 *   single row's computed length: a size never wraps, the call returns RDF_COMPUTE_ERROR.
 * Errors, all before any device work, in this order, RDF_INVALID_ARGUMENT unless said otherwise: nparts outside
 * 1..RDF_UTF8_PARTS_MAX or a bad side; a part that sets both pointers or neither, or no column part; a literal, sep, pad or
 * delim whose length is negative or above RDF_UTF8_PATTERN_MAX, or a NULL pointer with a positive length; sep_bytes != 0
 * with with_separator == 0; wrong dtypes, mixed memory kinds, a missing validity buffer; chunk row counts that differ
 * between parts: RDF_COMPUTE_ERROR; no device: RDF_DEVICE_ERROR.  nchunks == 0 is RDF_OK. */
#define RDF_UTF8_PARTS_MAX 8
typedef struct {                 /* exactly one of utf8 / literal is set */
    const rdf_utf8_array* utf8;  /* nchunks chunks of this part, or NULL */
    const uint8_t* literal;      /* literal_bytes bytes (may be 0 bytes with a non-NULL pointer), or NULL */
    int64_t literal_bytes;       /* 0 .. RDF_UTF8_PATTERN_MAX */
} rdf_utf8_part;

/* coalesce / case_when over text (the numeric forms and their semantics: rdf_coalesce, rdf_case_when).  They reuse rdf_utf8_part;
 * for these two calls ONLY, a part with NEITHER pointer set is the NULL literal.  A row is the chosen part's whole row or the
 * literal, copied into every row that takes it; NULL when the chosen part is.  Outputs follow rdf_utf8_trim's sizing rule
 * unchanged: values == NULL / capacity == 0 is the sizing call, a short data capacity gives RDF_MEMORY_ERROR with every length
 * set and nothing written, an output chunk above 2^31-1 bytes is RDF_COMPUTE_ERROR.  out_offsets[c].validity is required when
 * chunk c can be NULL (coalesce: no part is never-NULL in it; case_when: `otherwise` is absent or any value can be NULL).
 * Refused before any device work, in this order, RDF_INVALID_ARGUMENT unless said otherwise: nparts / nbranches outside 1..8; a
 * NULL list with nchunks > 0, or negative nchunks; no column part; a part that sets both pointers; a literal longer than
 * RDF_UTF8_PATTERN_MAX (or of negative length); a condition that is not RDF_BOOL; offsets / data / outputs of the wrong dtype;
 * mixed memory kinds; a missing required bitmap; chunk row counts that differ between parts or conditions (RDF_COMPUTE_ERROR);
 * an offsets capacity below rows + 1 (RDF_MEMORY_ERROR).  nchunks == 0 is RDF_OK. */
rdf_status rdf_utf8_coalesce(const rdf_utf8_part* parts, int32_t nparts, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_case_when(const rdf_array* const* conds, const rdf_utf8_part* values, int32_t nbranches,
                              const rdf_utf8_part* otherwise, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);

rdf_status rdf_utf8_concat(const rdf_utf8_part* parts, int32_t nparts, int64_t nchunks, int32_t with_separator,
                           const uint8_t* sep, int64_t sep_bytes, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_pad(int32_t side /* 0 = lpad, 1 = rpad */, const rdf_utf8_array* chunks, int64_t nchunks, int64_t len,
                        const uint8_t* pad, int64_t pad_bytes, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_repeat(const rdf_utf8_array* chunks, int64_t nchunks, int64_t times, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_reverse(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_substring_index(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* delim, int64_t delim_bytes,
                                    int64_t count, rdf_out* out_offsets, rdf_out* out_data);

/* ------------------------------------------------------------------ Utf8 rewrites */

/* A row's content changed by what the row holds: replace(phone, '-', ''), translate(s, 'áé', 'ae'), initcap(city) before a
 * GROUP BY; split(tags, ',') -> rdf_list_explode -> rdf_utf8_take to turn a delimited cell into rows.  The reference declares
 * initcap, translate and split with empty bodies (src/functions/scalar.rs), so these follow Spark 3; the executable model,
 * with every rule below spelled out, is tests/utf8_rewrite_ref.py (Spark itself was not run).
 * Inputs are taken exactly as rdf_utf8_trim takes them (row `offset`, value offsets that need not start at 0, validity at
 * any bit offset, host or device memory, all one kind).  Outputs are chunked like the inputs under the one sizing rule of
 * rdf_utf8_filter .. _upper (values == NULL, capacity == 0 is the sizing call; a capacity that is too small gives
 * RDF_MEMORY_ERROR with every length set and nothing written; an output chunk above 2^31-1 bytes is RDF_COMPUTE_ERROR).  A
 * NULL row gives a NULL row of zero bytes; an output whose rows can be NULL needs out_offsets[i].validity (split:
 * out_list_offsets[i].validity); null_count is set.  Bytes are not validated and nothing outside a row is read.
 *   replace    occurrences of `search` are found byte-wise from the left, each search resuming at the END of the previous hit
 *              ('aaaaa', 'aa', 'b' -> 'bba'); every hit is replaced.  An empty search gives the row unchanged
 *              (UTF8String.replace); an empty replacement deletes.
 *   translate  both arguments are cut into units (a unit begins at every byte that is not a continuation byte and runs over
 *              the continuation bytes after it; on valid UTF-8: the code points).  A unit of the row equal to unit i of
 *              `matching` becomes unit i of `replace`, and is dropped when `replace` has no unit i; the first position of a
 *              unit in `matching` decides; units of `replace` beyond matching's count are ignored.  A unit whose length is
 *              not what its first byte announces (a stray continuation byte, a lead byte with too few or too many of them)
 *              never matches and is copied.
 *   initcap    title_words(lower(row)): lower is rdf_utf8_lower's mapping (one-to-many mappings, Final_Sigma); a word
 *              begins at the first byte of the row and after every byte 0x20, and at no other white space
 *              (UTF8String.toTitleCase); a word's first code point takes its SIMPLE title mapping (one code point: 'ǆ' ->
 *              'ǅ', 'ß' stays).  Units that are not well-formed are copied.
 *   split      `delim` is a LITERAL (Spark takes a regular expression; a delimiter without metacharacters means the same).
 *              Hits are found as in replace.  limit > 0: only the first limit - 1 hits split, so the last element holds the
 *              rest; limit <= 0: every hit splits.  Trailing empty strings are kept ('a,b,,c,' -> 5 elements), the empty row
 *              gives [''], a NULL row a NULL list.  The result is a List<Utf8>: out_list_offsets[i] is RDF_I32, rows + 1
 *              entries from 0, with the rows' validity: the `offsets` member of an rdf_list_array, as rdf_list_explode
 *              takes it; out_offsets[i] (RDF_I32, elements + 1 entries, no validity) and out_data[i] are the child Utf8
 *              chunk, as rdf_utf8_take takes it.  On return the lengths of all three are set; a capacity of out_offsets or
 *              out_data that is too small, or a NULL `values` there, is RDF_MEMORY_ERROR: all lengths set, nothing written.
 * Errors, all before any device work, in this order, RDF_INVALID_ARGUMENT unless said otherwise: a literal (search,
 * replacement, matching, replace, delim; in argument order) whose length is negative, or above RDF_UTF8_PATTERN_MAX, or a
 * NULL pointer with a positive length; an empty delim; negative nchunks or a NULL list with nchunks > 0 (nchunks == 0 is
 * RDF_OK here); offsets / data of the wrong dtype; outputs of the wrong dtype; mixed memory kinds; a row-offsets output
 * without a buffer, a negative capacity, a data capacity without a buffer (not for split, where that is the sizing call); a
 * missing validity buffer; a row-offsets capacity below rows + 1: RDF_MEMORY_ERROR with that length set; no device:
 * RDF_DEVICE_ERROR. */
rdf_status rdf_utf8_replace(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* search, int64_t search_bytes,
                            const uint8_t* replacement, int64_t replacement_bytes, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_translate(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* matching, int64_t matching_bytes,
                              const uint8_t* replace, int64_t replace_bytes, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_initcap(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_split(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* delim, int64_t delim_bytes, int64_t limit,
                          rdf_out* out_list_offsets, rdf_out* out_offsets, rdf_out* out_data);

/* ------------------------------------------------------------------ regular expressions over Utf8
 *
 * Spark 3's rlike, regexp_count, regexp_extract(s, p, 0), regexp_replace and split(s, regex, limit): java.util.regex, that is
 * LEFTMOST-FIRST matching (a|ab on "ab" matches "a").  The pattern compiles once per call, on the host, into two small DFAs
 * (the forward one finds where the leftmost-first match ends, the reverse one where it starts); the device walks them, a
 * class look-up and a table entry per row byte, a lane a row.  There is no backtracking: a pattern cannot make a kernel run long.
 *
 * accepted: literals; \ \. \t \n \r \f \xhh \uhhhh and a backslash before ASCII punctuation; `.` (every code point but \n \r
 *   U+0085 U+2028 U+2029); classes [abc] [a-z] [^..] with \d \w \s inside; \d \D \w \W \s \S (ASCII definitions, \s is
 *   [ \t\n\x0B\f\r]); ( ) and (?: ), which both only group; |; * + ? {n} {n,} {n,m}, greedy and lazy; ^ \A (row start) and
 *   $ \z (row end); one leading (?i) (?s) (?is) (?si); (?i) folds ASCII letters only.
 * refused with RDF_INVALID_ARGUMENT, rdf_last_error() naming the construct and its byte in the pattern: backreferences,
 *   look-ahead and look-behind, atomic and named groups, possessive quantifiers, \b \B \G \Z \R \X \h \v, \p{..}, POSIX classes,
 *   && and a nested [ in a class, a ] or ^] that opens a class, \Q..\E, octal escapes, flags anywhere but at the front, the
 *   flags m x u d U, a dangling {, a quantifier without an operand, {n,m} with n > m or a count above 1000, counted repetition
 *   past 1000 expanded leaves; and, because their Java meaning is not certain, a quantifier on a quantifier, a quantifier on
 *   an anchor and a quantifier that may repeat more than once over an operand that can match the empty string.  A pattern
 *   whose program passes 4096 instructions, whose DFAs pass 2048 states each or whose tables pass 256 KiB is refused with
 *   the count in the message; it is never run wrong.
 * KNOWN DIFFERENCE FROM SPARK: `$` is Java's \z; Java's `$` also matches before a final line terminator.  After an empty
 *   match the search moves on by a code point, where Java moves by a UTF-16 unit.
 * bytes: rows are not validated; the pattern must be UTF-8.  Every consuming element matches one well-formed UTF-8 sequence
 *   (RFC 3629) and nothing else: a stray or truncated byte is matched by no element, not by `.` and not by [^a].  A match,
 *   the empty one included, begins only at a byte that is not a continuation byte, or at the row's end.
 * matches are found as Matcher.find finds them: from byte 0; after a non-empty match from its end; after an empty match at p
 *   from the next allowed start after p; ^ holds at byte 0 only.  A NULL row gives NULL.
 *
 *   rdf_utf8_regexp_match    rlike: a match exists.  RDF_BOOL masks under the conventions of rdf_utf8_predicate.
 *   rdf_utf8_regexp_count    the matches.  RDF_I32 under the conventions of rdf_utf8_measure.
 *   rdf_utf8_regexp_extract  the first match's bytes, '' when there is none.  group must be 0 ("capture groups are not
 *                            built"); the ABI does not change when they are.  Outputs as rdf_utf8_replace's.
 *   rdf_utf8_regexp_replace  every match replaced.  In the replacement \x stands for x; a trailing backslash and any
 *                            unescaped $ are refused.  Outputs as rdf_utf8_replace's, under the one sizing rule.
 *   rdf_utf8_regexp_split    String.split(regex, limit) as Spark 3 calls it: a zero-width match at byte 0 never splits;
 *                            limit > 0: only the first limit - 1 hits split; limit <= 0: every hit; trailing empty strings
 *                            are kept; the empty row gives ['']; an empty pattern is valid.  Outputs as rdf_utf8_split's.
 *   rdf_utf8_regexp_info     host only, needs no device: the counts the caps are defined on.
 *
 * Order of the checks: pattern_bytes outside 0 .. RDF_UTF8_PATTERN_MAX, a null pattern with bytes; the pattern compiled
 * (syntax, then the caps); group != 0; the replacement's length and pointer, then its escapes; then the checks of
 * rdf_utf8_predicate (match, count) or of rdf_utf8_replace / rdf_utf8_split in their order, nchunks == 0 being RDF_OK
 * there; no device: RDF_DEVICE_ERROR.  Every refusal of the pattern, group or replacement comes before any device work. */
typedef struct {
    int32_t program_len, forward_states, reverse_states, classes;
    int64_t table_bytes;
    int32_t can_match_empty, anchored_start;
} rdf_regexp_info;
rdf_status rdf_utf8_regexp_info(const uint8_t* pattern, int64_t pattern_bytes, rdf_regexp_info* out);
rdf_status rdf_utf8_regexp_match(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes, rdf_out* mask);
rdf_status rdf_utf8_regexp_count(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes, rdf_out* out);
rdf_status rdf_utf8_regexp_extract(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes, int32_t group,
                                   rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_regexp_replace(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes,
                                   const uint8_t* replacement, int64_t replacement_bytes, rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_regexp_split(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes, int64_t limit,
                                 rdf_out* out_list_offsets, rdf_out* out_offsets, rdf_out* out_data);

/* ------------------------------------------------------------------ text to values and back
 *
 * ScalarFunctions::{to_date(s, fmt), to_timestamp, unix_timestamp, from_unix_time, date_format} (src/functions/scalar.rs
 * declares them with empty bodies) and CAST between Utf8 and Boolean / integer / date / timestamp columns, with Spark 3's
 * semantics as far as tests/textconv_ref.py (the executable model) and DESIGN.md state them; no time zones beyond a numeric
 * offset in the text.  Inputs follow the rdf_utf8_array conventions exactly as rdf_utf8_trim takes them; temporal storage
 * follows rdf_datetime_fields (Int32 or Int64 plus its rdf_time_unit, RDF_TIME_DAY is Int32).
 *
 * CAST grammars (pattern == NULL): the bytes 0x09-0x0D, 0x1C-0x1F and 0x20 are trimmed from both ends, nothing else.
 *   INT        [+-]? digit+ ( '.' digit* )?   the fraction is checked and dropped; a value outside the dtype is NULL; for an
 *              unsigned dtype '-0' is 0 and any other negative NULL; a text without a digit before the '.' is NULL
 *   BOOL       t true y yes 1 / f false n no 0, ASCII letters of either case
 *   DATE       [+-]? y{4,7} ( - m{1,2} ( - d{1,2} ( [ T] anything )? )? )?   a missing month or day is 1; a date that
 *              does not exist, or whose day number leaves Int32, is NULL
 *   TIMESTAMP  the date part, optionally [ T] h{1,2} : m{1,2} ( : s{1,2} ( . digit* )? )? after a full date, optionally a
 *              zone Z, UTC or [+-] h{1,2} ( : m{1,2} )? of at most 18:00, which is subtracted; fraction digits beyond the
 *              unit are dropped; a value the unit's Int64 cannot hold is NULL
 * Patterns (DATE / TIMESTAMP): yyyy yy M MM MMM d dd D DDD H HH h hh a m mm s ss S..SSSSSSSSS, EEE (format only), '...'
 * quoted text ('' a quote), any non-letter byte for itself; at most 32 tokens and 64 literal bytes.  A pattern trims nothing
 * and has to consume the whole row.  Two-letter numeric tokens take exactly two digits, one-letter ones one or two (D up to
 * three), greedily; absent fields are those of 1970-01-01 00:00:00; a field given twice with two values, fields that contradict
 * each other (D against M / d, H against h a) or lie outside their range give NULL.
 * CAST to text: shortest decimal; true / false; yyyy-MM-dd; yyyy-MM-dd HH:mm:ss plus '.' and the fraction without trailing
 * zeros when it is not 0.  Years 0..9999 print as four digits, larger ones as '+' and the digits, negative ones as '-' and at
 * least four digits.  parse(format(x)) == x for every integer, every Int32 day number and every timestamp of the years
 * -999999 .. 9999999.
 *
 * Refused with RDF_INVALID_ARGUMENT before any device work and with nothing written: an unknown kind or unit; a pattern with
 * BOOL / INT; a pattern that does not compile or whose output could pass 256 bytes a row (rdf_last_error() names the
 * position); a NULL list with nchunks > 0, negative nchunks; an output of the wrong dtype; two memory kinds in one call; parse:
 * an output without a validity buffer; format: an input with validity but an output without, Int64 storage with RDF_TIME_DAY,
 * chunks of two storage types.  Float dtypes, and temporal storage other than Int32 / Int64, are RDF_COMPUTE_ERROR
 * ("... does not support type").  A capacity below the rows is RDF_MEMORY_ERROR.  nchunks == 0 is RDF_OK.  Without a device
 * a valid call returns RDF_DEVICE_ERROR (no CPU fallback). */
typedef enum { RDF_TEXT_BOOL = 0, RDF_TEXT_INT, RDF_TEXT_DATE, RDF_TEXT_TIMESTAMP } rdf_text_kind;

/* Utf8 -> Boolean / integer / Date32 day number / timestamp.  pattern == NULL: Spark 3's CAST grammar of the kind;
 * else a datetime pattern (DATE, TIMESTAMP only): to_date(s, fmt), to_timestamp(s, fmt), unix_timestamp(s, fmt) is
 * TIMESTAMP with RDF_TIME_SECOND.  A row that does not parse is NULL, never an error, so every output needs a validity
 * buffer.  failed[c] (may be NULL): rows of chunk c that were not NULL and did not parse.
 * out[c]: RDF_BOOL (BOOL), any of the eight integer dtypes taken from out[c].dtype (INT; one dtype for the call), RDF_I32
 * (DATE), RDF_I64 in `unit`, second .. nanosecond (TIMESTAMP).  NULL rows hold 0, bitmaps are written as
 * rdf_datetime_fields writes them, null_count is set. */
rdf_status rdf_utf8_parse(const rdf_utf8_array* chunks, int64_t nchunks, int32_t kind, int32_t unit,
                          const uint8_t* pattern, int64_t pattern_bytes, rdf_out* out, int64_t* failed);

/* The inverse: Boolean / integer / temporal storage (+ unit, as rdf_hour takes it) -> Utf8 under the sizing rule of
 * rdf_utf8_trim.  pattern == NULL: CAST(x AS STRING); else date_format(x, fmt), from_unix_time(x, fmt) is TIMESTAMP with
 * RDF_TIME_SECOND.  Kind DATE prints the date of a temporal value of any unit, TIMESTAMP its date and time; with a pattern
 * the two are the same.  NULL in gives NULL out with an empty row. */
rdf_status rdf_utf8_format(const rdf_array* a, int64_t nchunks, int32_t kind, int32_t unit,
                           const uint8_t* pattern, int64_t pattern_bytes, rdf_out* out_offsets, rdf_out* out_data);

/* Float32 / Float64 columns to and from text (tests/textfloat_ref.py is the executable model, DESIGN.md §30 the account).
 * Parse: after the trim of the CAST grammars, [+-]? ( digit+ ( '.' digit* )? | '.' digit+ ) ( [eE] [+-]? digit+ )?, or in
 * either letter case nan (no sign), [+-]? inf, [+-]? infinity; everything else (hex floats, a trailing d / f, '_') is NULL.
 * The value is the exact decimal rounded once, to nearest and ties to even, into the target type, however many digits the row
 * has (Float32 straight from the decimal); overflow gives an infinity, underflow a zero that keeps the sign; NaN is the
 * canonical quiet NaN.  Format: Java's Double.toString / Float.toString as specified since JDK 19 (the shortest decimal that
 * rounds back, the closest of that length, at least two digits chosen: 4.9E-324; plain for 10^-3 <= |x| < 10^7, else
 * d.dddE[-]n; NaN, Infinity, -Infinity, 0.0, -0.0); at most 24 bytes a row (Float32: 15).  parse(format(x)) has the bits of x.
 * Argument checks, memory kinds, capacities, nchunks == 0 and RDF_DEVICE_ERROR are those of rdf_utf8_parse / rdf_utf8_format;
 * any dtype but RDF_F32 / RDF_F64 is RDF_COMPUTE_ERROR ("... does not support type").
 * rdf_set_option("textfloat_exact", 1) sends every row through the exact (big-integer) path, for tests and measurements.
 *
 * Utf8 -> Float32 / Float64 (the dtype of out[c], one dtype per call): CAST(s AS FLOAT / DOUBLE).  A row that does not
 * parse is NULL and is counted in failed[c]; NULL rows hold 0; bitmaps / null_count as rdf_utf8_parse writes them. */
rdf_status rdf_utf8_parse_float(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out, int64_t* failed);

/* Float32 / Float64 -> Utf8: CAST(x AS STRING), under the sizing rule of rdf_utf8_trim (a first call without data
 * buffers reports the bytes per chunk).  NULL in gives NULL out with an empty row. */
rdf_status rdf_utf8_format_float(const rdf_array* a, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data);

/* DataFrame::sort (src/dataframe.rs:194-222) whose criteria may be Utf8 columns: arrow's lexsort_to_indices over numeric
 * and StringArray columns alike.  keys[k] is criterion k (key 0 most significant) and sets exactly one of
 *   values  nchunks numeric chunks (one dtype), ordered as by rdf_sort_to_indices, or
 *   utf8    nchunks Utf8 chunks (rdf_utf8_array conventions: row `offset`, value offsets that need not start at 0,
 *           validity at any bit offset, Int32 offsets per chunk; the bytes of all chunks together may exceed 2^31).
 * Utf8 values compare byte by byte as unsigned bytes (Rust's str Ord, code-point order); a proper prefix sorts first and
 * 0x00 is an ordinary byte ("a" < "a\0" < "a\0b" < "b"); the bytes are not validated as UTF-8.  `descending` reverses
 * the order of non-NULL values; NULL rows sort last in both directions (nulls_first is ignored, as for the numeric
 * sort).  The sort is stable: rows equal on every key keep ascending row order.  out_indices: ONE RDF_U32 array over the
 * concatenation of the chunks.  Inputs and output all in host memory or all in device memory.  With numeric keys only
 * the result is rdf_sort_to_indices' on the same columns, bit for bit.
 * Errors: no keys RDF_COMPUTE_ERROR; a key setting both pointers or neither, wrong dtypes, mixed memory kinds
 * RDF_INVALID_ARGUMENT; chunk row counts that differ between keys RDF_COMPUTE_ERROR; 2^32 rows or more
 * RDF_INVALID_ARGUMENT; output capacity below the rows RDF_MEMORY_ERROR. */
typedef struct {
    const rdf_array*      values;   /* nchunks numeric chunks of this criterion, or NULL */
    const rdf_utf8_array* utf8;     /* nchunks Utf8 chunks of this criterion, or NULL  */
    rdf_sort_options      options;
} rdf_sort_key;
rdf_status rdf_lexsort_to_indices(const rdf_sort_key* keys, int32_t nkeys, int64_t nchunks, rdf_out* out_indices);

/* ------------------------------------------------------------------ row hashes and digests */

/* hash, xxhash64, crc32, md5, sha1 and sha2 per row.  The reference declares hash, crc32, md5, sha1 and sha2 with empty
 * bodies (src/functions/scalar.rs:205, :265, :338, :389, :390), so these follow Spark 3; the executable model is
 * tests/digest_ref.py.  Inputs follow the rdf_utf8_array conventions exactly as rdf_utf8_trim takes them (row `offset`,
 * value offsets that need not start at 0, validity at any bit offset, host or device memory, all one kind).
 *   rdf_hash_columns   Spark's hash (RDF_HASH_MURMUR3_32: Murmur3_x86_32, out[i] RDF_I32, the seed must fit Int32) or
 *              xxhash64 (RDF_HASH_XXHASH64, out[i] RDF_I64) over 1 .. RDF_HASH_COLS_MAX columns; Spark's default seed is 42.
 *              cols[k] sets exactly one of values (nchunks numeric or RDF_BOOL chunks of one dtype) / utf8, as for
 *              rdf_groupby_agg_keys; `options` is ignored.  h = seed; for each column in order, a row that is not NULL in it
 *              gives h = H(value, h), a NULL leaves h unchanged.  Bool hashes as hashInt(1 / 0); I8 / I16 / I32 as hashInt
 *              of the sign-extended value; U8 / U16 as hashInt of the zero-extended value and U32 as hashInt of its bits
 *              (Spark has no unsigned types: this defines them); I64 / U64 as hashLong of the bits; F32 / F64 as hashInt /
 *              hashLong of the bits with every NaN taken as the canonical quiet NaN and -0.0 as +0.0; Utf8 as
 *              hashUnsafeBytes (Murmur3's tail is Spark's: every byte after the 4-byte words alone, as a SIGNED byte).
 *              Temporal columns hash as their Int32 / Int64 storage.  out[i] has the rows of chunk i; the result is never
 *              NULL: a validity buffer, if given, is written all ones and null_count is 0.  The results are ordinary keys
 *              for rdf_groupby_agg, rdf_uniques, rdf_window and rdf_equijoin_indices.
 *   rdf_utf8_digest    md5 / sha1 / sha2 of every row as lowercase hex text of 32 / 40 / 56 / 64 / 96 / 128 bytes; a NULL
 *              row gives NULL with zero bytes.  Outputs are chunked like the input under the one sizing rule of
 *              rdf_utf8_filter .. _upper: out_data[i].length = non-NULL rows x width (values == NULL, capacity == 0 is the
 *              sizing call; a capacity that is too small gives RDF_MEMORY_ERROR with every length set and nothing written;
 *              an output chunk beyond 2^31-1 bytes is RDF_COMPUTE_ERROR).  out_offsets[i].validity is required when chunk i
 *              has one.  Spark's sha2(col, bits) maps bits 0 and 256 to RDF_DIGEST_SHA256; any other value of `kind` is an
 *              error here where Spark returns NULL.
 *   rdf_utf8_crc32     zlib's CRC-32 of every row as RDF_I64 in 0 .. 2^32-1, under rdf_utf8_measure's output rules: length
 *              == rows, a NULL row gives NULL (value 0), validity required when the chunk has one, null_count set.
 * Errors, all before any device work, in this order: (1) an unknown kind; (2) ncols outside 1 .. RDF_HASH_COLS_MAX, or a
 * column that sets both pointers or neither; (3) a Murmur3 seed outside Int32; (4) wrong dtypes, mixed memory kinds, a
 * missing validity buffer: all RDF_INVALID_ARGUMENT; (5) chunk row counts that differ between columns: RDF_COMPUTE_ERROR;
 * (6) a capacity below the rows (rdf_utf8_digest: offsets below rows + 1): RDF_MEMORY_ERROR with `length` set; (7) no
 * device: RDF_DEVICE_ERROR.  The data capacity of rdf_utf8_digest is judged after the count, on the device.
 * nchunks == 0 is RDF_OK. */
typedef enum { RDF_HASH_MURMUR3_32 = 0, RDF_HASH_XXHASH64 = 1 } rdf_hash_kind;
typedef enum { RDF_DIGEST_MD5 = 0, RDF_DIGEST_SHA1, RDF_DIGEST_SHA224, RDF_DIGEST_SHA256,
               RDF_DIGEST_SHA384, RDF_DIGEST_SHA512 } rdf_digest_kind;
#define RDF_HASH_COLS_MAX 8
rdf_status rdf_hash_columns(int32_t kind, const rdf_sort_key* cols, int32_t ncols, int64_t nchunks,
                            int64_t seed, rdf_out* out);
rdf_status rdf_utf8_digest(int32_t kind, const rdf_utf8_array* chunks, int64_t nchunks,
                           rdf_out* out_offsets, rdf_out* out_data);
rdf_status rdf_utf8_crc32(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out);

/* ------------------------------------------------------------------ Column::hist / Column::uniques */

/* Column::hist (src/table.rs:244-290): the histogram of an Int64 or Float64 column over `nbins` equal-width buckets.  The
 * reference feeds every value `as f64` to the histo_fp crate, whose bucket boundaries it does not pin; the semantics here
 * are numpy.histogram(x, bins = nbins, range = range), counts and edges alike:
 *   - NULL rows and NaN are not counted; *out_counted = the rows that landed in a bucket;
 *   - range == NULL: lo / hi = minimum / maximum of the counted values (rdf_min / rdf_max's rule: NaN never wins); an
 *     infinite one is RDF_COMPUTE_ERROR ("range is not finite"); no counted value at all gives lo, hi = 0, 1.
 *     range = {lo, hi}: both finite, lo <= hi, else RDF_INVALID_ARGUMENT; values outside [lo, hi] are not counted.
 *     lo == hi becomes lo - 0.5, hi + 0.5 either way;
 *   - step = (hi - lo) / nbins, edges[i] = lo + i * step (IEEE double, two roundings), edges[nbins] = hi exactly; x belongs
 *     to bucket i with edges[i] <= x < edges[i + 1], the last bucket also takes x == hi.
 * Other dtypes: RDF_INVALID_ARGUMENT (the reference panics "Unsupported type for histogram").  1 <= nbins <= 2^24.
 * out_counts: ONE RDF_I64 array of nbins, out_edges: ONE RDF_F64 array of nbins + 1; a capacity below that is
 * RDF_MEMORY_ERROR with the needed lengths set and nothing written.  Counts are exact: two runs, and host and device
 * memory, give identical outputs.  With `range` given the call is additive over row ranges (shards can be summed). */
rdf_status rdf_hist(const rdf_array* chunks, int64_t nchunks, int64_t nbins, const double* range, rdf_out* out_counts,
                    rdf_out* out_edges, int64_t* out_counted);

/* Column::uniques (src/table.rs:293-341) for Int64 / UInt64 / Float64 columns: the distinct values of the valid rows, each
 * once, as ONE chunk of the input dtype in unspecified order (the reference's is HashSet iteration order).  NULL rows are
 * skipped.  Float64 values compare numerically: -0.0 and +0.0 are one value, returned as +0.0; all NaNs are one value,
 * returned once as the quiet NaN 0x7FF8000000000000; every other value comes back bit for bit.  *out_count is always set;
 * out_values == NULL counts only; a capacity below the count is RDF_MEMORY_ERROR (out_values->length = the count, nothing
 * written); a capacity of all rows always suffices.  Other dtypes: RDF_INVALID_ARGUMENT ("Datatype not supported for
 * uniques").  The caller passes no cardinality: keys go into a hash set sized from the rows within a memory budget
 * (rdf_set_option "uniques_table_bits"), and a column with more distinct values than the set was sized for is sorted
 * instead (first row of every run of equal keys kept; "uniques_route" 1 forces this route). */
rdf_status rdf_uniques(const rdf_array* chunks, int64_t nchunks, rdf_out* out_values, int64_t* out_count);

/* Column::uniques for Utf8 columns (src/table.rs:311-324): the distinct byte strings of the valid rows, each once, as ONE
 * Utf8 chunk (offsets from 0, no NULLs: no validity buffer needed) in unspecified order.  Equality is byte equality; the
 * empty string is a value, 0x00 an ordinary byte, the bytes are not validated.  Sizing as for rdf_utf8_take: lengths
 * reported in out_offsets->length / out_data->length, RDF_MEMORY_ERROR and nothing written when a capacity is short
 * (out_data with values == NULL, capacity == 0 is the sizing call; out_offsets needs a buffer of at least one entry, and
 * rows + 1 entries / the input's bytes always suffice).  *out_count is always set.  Rows are matched through a 64-bit hash
 * of their bytes and every row is then compared with its hash's representative; two different strings with one hash (or
 * more distinct values than the hash set was sized for, or "uniques_route" 1) send the call to the exact route: the order
 * of rdf_lexsort_to_indices, neighbours compared. */
rdf_status rdf_utf8_uniques(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_offsets, rdf_out* out_data,
                            int64_t* out_count);

/* ------------------------------------------------------------------ text keys: dictionary encoding, GROUP BY, join */

/* Dictionary encoding of a Utf8 column: dense UInt32 codes per row and the dictionary of the distinct values.  The code of
 * a row is the number of distinct values whose first occurrence precedes the first occurrence of the row's value, over
 * the concatenation of the chunks (first-occurrence order: pandas.factorize) — a function of the input alone, whichever
 * route computes it.  Dictionary row k holds the bytes of the value with code k; it has no NULLs (no validity buffer
 * needed) and its offsets start at 0.  A NULL row gives a NULL code: validity bit clear, value 0.  Equality is byte
 * equality; the empty string is a value, 0x00 an ordinary byte, the bytes are not validated.
 * out_codes: nchunks RDF_U32 outputs, out_codes[i] of chunk i's rows (length and null_count set per chunk; a validity
 *   buffer is required when chunk i carries one, and filled with ones when the chunk carries none);
 * out_dict_offsets / out_dict_data: ONE Utf8 chunk; *out_count = the distinct values.
 * rdf_utf8_array conventions as for rdf_utf8_uniques; inputs and outputs all in host memory or all in device memory.
 * Sizing as for rdf_utf8_uniques: *out_count and every needed length (out_codes[i].length, out_dict_offsets->length,
 * out_dict_data->length) are always set; a short out_dict_data, out_dict_offsets or out_codes[i].capacity is
 * RDF_MEMORY_ERROR and nothing is written; out_dict_data with values == NULL, capacity == 0 is the sizing call;
 * out_dict_offsets needs a buffer of at least one entry; rows + 1 entries and the input's bytes always suffice.  2^32 rows
 * or more: RDF_INVALID_ARGUMENT; a dictionary beyond 2^31-1 bytes: RDF_COMPUTE_ERROR.  Rows are matched as in
 * rdf_utf8_uniques (64-bit hash, every row compared with its hash's smallest row); a hash shared by two strings, more
 * values than the table was sized for, or "uniques_route" 1 send the call to the exact route (rdf_lexsort_to_indices'
 * stable order, the first row of every run of equal values), with bit-identical codes and dictionary. */
rdf_status rdf_utf8_dictionary_encode(const rdf_utf8_array* chunks, int64_t nchunks, rdf_out* out_codes,
                                      rdf_out* out_dict_offsets, rdf_out* out_dict_data, int64_t* out_count);

/* One key column of a GROUP BY result: `values` for a numeric grouping column, or the (utf8_offsets, utf8_data) pair —
 * ONE Utf8 chunk — for a Utf8 one.  Exactly one of the two forms is set, matching the key. */
typedef struct { rdf_out* values; rdf_out* utf8_offsets; rdf_out* utf8_data; } rdf_key_out;

/* rdf_groupby_agg over 1..RDF_MAX_GROUP_KEYS grouping columns of which each is integer or Utf8.  keys[k] sets `values`
 * (nchunks integer chunks) or `utf8` (nchunks Utf8 chunks); its `options` are ignored.  Everything rdf_groupby_agg
 * documents holds: a NULL key is a group of its own, NULL values are skipped, the output dtypes, the capacities
 * (>= min(max_groups, rows) + 2 for every numeric output), RDF_MEMORY_ERROR beyond max_groups groups, unspecified group
 * order.  One difference, kept because callers size max_groups by their non-NULL keys: with a Utf8 key among the grouping
 * columns the two groups the kernels set aside — the NULL tuple, and the tuple whose packed code hashes to the LDS free
 * marker — do not count against max_groups, so up to max_groups + 2 groups come back (the capacities above hold them).
 * A Utf8 grouping column comes back as one Utf8 chunk whose row g belongs to out_values[g] / out_counts[g]; it is
 * NULL for the NULL group (validity required when the key carries a validity buffer) and sizes like every Utf8 output:
 * lengths reported, RDF_MEMORY_ERROR and nothing written when short; groups + 1 offsets and the key column's input bytes
 * always suffice.  Utf8 keys are dictionary-encoded (rdf_utf8_dictionary_encode), the codes grouped next to the numeric
 * keys by rdf_groupby_agg, and the dictionary taken by the result's code column.  With numeric keys only the call IS
 * rdf_groupby_agg.  Errors before any device work: a key or key output setting both forms or neither, wrong dtypes, mixed
 * memory kinds, nkeys outside 1..4 RDF_INVALID_ARGUMENT; chunk row counts that differ between columns RDF_COMPUTE_ERROR. */
rdf_status rdf_groupby_agg_keys(const rdf_sort_key* keys, int32_t nkeys, const rdf_array* values, int64_t nchunks,
                                int32_t agg, int64_t max_groups, rdf_key_out* out_keys, rdf_out* out_values,
                                rdf_out* out_counts);

/* Hash GROUP BY with several aggregates from ONE pass over the keys: groupby(k).agg(sum(a), min(b), max(b), count(d), ...)
 * as one call.  The grouping columns are prepared and hashed once (Utf8 keys dictionary-encoded, several keys packed into
 * one 64-bit key exactly as in rdf_groupby_agg_keys), up to RDF_MULTI_MAX_CALLS aggregates over up to
 * RDF_MULTI_MAX_VALUES value columns are folded into one table, and row g of EVERY output belongs to the same group.
 *   keys / out_keys      as rdf_groupby_agg_keys: 1..RDF_MAX_GROUP_KEYS keys, each integer or Utf8; a NULL key is a group of
 *                        its own; validity required in the key output of a nullable key.
 *   values[v]            nchunks chunks of value column v (numeric, one dtype per column), nvalues in 0..8.
 *   calls[c]             {agg (rdf_agg_fn), value}: value indexes `values`; -1 (COUNT only) counts the group's rows.  Two calls
 *                        may name one column.  Avg stays on the caller's side: sum / count of the same call.
 *   outs[c]              the dtype rdf_groupby_agg gives for (agg, dtype of the column): Float64 for float values, UInt64 for
 *                        MIN / MAX of UInt64, Int64 otherwise (integer sums wrap); NULL values are skipped per value column;
 *                        MIN / MAX of a group without a non-NULL value is NULL (validity required when that column is
 *                        nullable); NaN never wins a MIN / MAX unless every value of the group is NaN.  For COUNT the values
 *                        are unspecified (Int64).
 *   out_counts[c]        Int64: the non-NULL values of call c's column in the group; the group's rows when value == -1.
 *   out_group_rows       Int64 rows of the group (may be NULL: not wanted).
 *   *out_groups          the number of groups; 0 rows is a valid call with 0 groups.
 * Group order is unspecified.  Capacities >= min(max_groups, rows) + 2 for every numeric output; more than max_groups groups
 * -> RDF_MEMORY_ERROR and nothing is written (exactly max_groups succeed; with a Utf8 key among the keys the two set-aside
 * groups — the NULL tuple and the tuple whose packed code hashes to the free marker — do not count, as in
 * rdf_groupby_agg_keys); Utf8 key outputs size as there.  f64 sums are accumulated with hardware atomics in any order: a
 * group of n values comes back within gamma(n - 1) * sum|x_i| of the exact sum (the bound stated for rdf_group_pipeline),
 * and inputs whose partial sums are all exactly representable are summed exactly, bit for bit.
 * Routes (rdf_groupby_multi_plan.h): while max_groups <= rdf_groupby_multi_capacity(ncalls) every block folds its rows into
 * a table of hashed keys in LDS — a row finds its slot once and adds into the slot's accumulators — and merges its groups
 * into one table in HBM at the end; beyond that rows go straight to the table in HBM.  rdf_set_option("groupby_multi_route",
 * 0 planned | 1 LDS route | 2 HBM table) forces one (the LDS route hands over to the table when a block's table fills up
 * under a promise beyond its capacity); rdf_set_option("groupby_multi_slots", n) shrinks the LDS table (0 = planned).
 * Before any device work, with the outputs untouched: ncalls outside 1..8, nvalues outside 0..8, an unknown agg, a value
 * index out of range, value == -1 with SUM / MIN / MAX, a non-numeric value dtype, mixed memory kinds, a key or key output
 * in both forms or in neither, a missing validity buffer where one is required -> RDF_INVALID_ARGUMENT; chunk row counts
 * that differ between columns -> RDF_COMPUTE_ERROR.  Host-memory inputs are copied in whole (no streamed slabs). */
typedef struct { int32_t agg; int32_t value; } rdf_multi_agg_call;   /* agg: rdf_agg_fn; value: index into values, -1 = count rows */
#define RDF_MULTI_MAX_CALLS  8
#define RDF_MULTI_MAX_VALUES 8
rdf_status rdf_groupby_multi(const rdf_sort_key* keys, int32_t nkeys, const rdf_array* const* values, int32_t nvalues,
                             int64_t nchunks, const rdf_multi_agg_call* calls, int32_t ncalls, int64_t max_groups,
                             rdf_key_out* out_keys, rdf_out* outs, rdf_out* out_counts, rdf_out* out_group_rows,
                             int64_t* out_groups);
/* The most groups the one-pass LDS route holds for this many calls (table load <= 0.5); 0 for ncalls outside 1..8. */
int64_t rdf_groupby_multi_capacity(int32_t ncalls);

/* rdf_equijoin_indices_multi over 1..4 key pairs of which each is Utf8 on both sides or numeric of one dtype on both
 * sides (anything else: RDF_INVALID_ARGUMENT).  left_keys[k] / right_keys[k] hold left_nchunks / right_nchunks chunks.  A
 * Utf8 pair is encoded against one shared dictionary (the left chunks followed by the right chunks in one
 * rdf_utf8_dictionary_encode call) and the codes are joined.  Everything rdf_equijoin_indices_multi documents is
 * inherited: NULL never matches, the LEFT / RIGHT / INNER / FULL semantics, the pair order, the count-only call with
 * NULL outputs, the capacity rule.  The two sides together hold fewer than 2^32 rows; the key columns of one side agree
 * in their chunks' rows (RDF_COMPUTE_ERROR otherwise). */
rdf_status rdf_equijoin_indices_keys(const rdf_sort_key* left_keys, int64_t left_nchunks, const rdf_sort_key* right_keys,
                                     int64_t right_nchunks, int32_t nkeys, int32_t join_type, rdf_out* out_left,
                                     rdf_out* out_right, int64_t* out_rows);

/* ------------------------------------------------------------------ membership: semi / anti join, is_in, distinct rows */

/* Which of my rows have a partner over there (LEFT SEMI, LEFT ANTI, x IN (...)), and which rows are the first of their kind
 * (distinct, drop_duplicates)?  One primitive: a set of key tuples goes into a hash table, a column of tuples is streamed
 * past it, and every row gives ONE bit.  The answer is an RDF_BOOL mask per chunk — what rdf_filter, rdf_filter_columns,
 * rdf_filter_frame and rdf_utf8_filter take, and rdf_predicate as a Boolean input column.  A mask has no output order: the
 * result is a function of the input alone; the executable model is tests/member_ref.py.
 *
 * Common to both calls.  Keys follow rdf_equijoin_indices_keys: 1..RDF_MEMBER_MAX_KEYS keys, each numeric (one of the ten
 * fixed-width numeric dtypes, or RDF_BOOL) of one dtype on both sides, or Utf8 on both sides; `options` are ignored; the key
 * columns of one side agree in their chunks' rows.  All inputs and outputs in host memory or all in device memory (device
 * bitmaps start on an 8-byte boundary); the two sides together (or the one side) hold fewer than 2^32 rows.
 *   Float keys compare as rdf_uniques and rdf_window compare them — Spark 3's rule for join and grouping keys: -0.0 == +0.0
 *   and every NaN equals every NaN.  This KNOWINGLY DIFFERS from rdf_equijoin_indices, which matches key bits (there -0.0 and
 *   +0.0, and NaNs of different payload, are different keys).
 *   Utf8 keys are byte strings; the empty string is a value, not NULL.  rdf_member_mask encodes a Utf8 pair against ONE shared
 *   dictionary (left chunks then right chunks, codes only), rdf_first_occurrence every Utf8 key against its own.
 * out_mask[i] describes chunk i's rows: bit r = row r, output offset 0, length and null_count set.  *out_rows = the TRUE bits
 * over all chunks, always set (0 when the call is refused).  out_mask == NULL is the count-only call, which sizes a following
 * filter.  Zero rows on either side is a valid call.
 * Errors, all before any device work: NULL pointers, a chunk count below 1, nkeys outside 1..4, an unknown kind / keep, IS_IN
 * with more than one key, a key setting both pointers or neither, wrong dtypes, a Utf8 key paired with a numeric one, key
 * dtypes that differ between the sides, mixed memory kinds, a mask that is not RDF_BOOL, a missing validity buffer (IS_IN), 2^32
 * rows or more, "member_route" 1 on a call the LDS form cannot serve: RDF_INVALID_ARGUMENT.  Key columns of one side that differ in
 * their chunks' rows: RDF_COMPUTE_ERROR.  A capacity below a chunk's rows: RDF_MEMORY_ERROR with every `length` set and nothing
 * written.  Scratch that does not fit — a table that "member_table_bits" made too small for the keys included —:
 * RDF_MEMORY_ERROR, never a partial answer.
 *
 * rdf_member_mask
 *   SEMI   TRUE iff no key of the left row is NULL and some right row holds an equal tuple.  A right row with a NULL in any
 *          key is never in the set.  The result is never NULL: validity is not required and written all-valid where given.
 *   ANTI   the complement of SEMI, bit for bit: a left row with a NULL key is kept (Spark's LEFT ANTI).
 *   IS_IN  SQL's three-valued x IN (right), nkeys == 1: TRUE on a match; otherwise NULL when x is NULL or the right side
 *          holds a NULL row; otherwise FALSE.  Over an empty right side every row is FALSE, NULL rows included.  Validity is
 *          required; the value bit of a NULL slot is 0 (rdf_predicate's rule); *out_rows counts TRUE only.  NOT IN is
 *          rdf_predicate's NOT over this mask.
 *   The right side is built into an open-addressing table in HBM (load <= 0.5 of the build rows); while that table fits the
 *   LDS budget and there is one key column, every probe block copies it into LDS and probes there.
 *   rdf_set_option("member_route", 0 planned | 1 LDS | 2 HBM), ("member_slots", n) shrinks the LDS form's table (tests),
 *   ("member_table_bits", b) caps the table at 2^b slots (4..32, default 30).  rdf_last_kernel names the form that ran.
 *
 * rdf_first_occurrence
 *   Rows are equal iff they agree on every key, NULL equal to NULL, component-wise: a NULL is a key value of its own, as in
 *   GROUP BY.  KEEP_FIRST: TRUE on the row with the smallest index of every distinct tuple (pandas keep='first'); KEEP_LAST:
 *   the largest index; KEEP_NONE: TRUE on tuples that occur exactly once.  For FIRST and LAST *out_rows is the number of
 *   distinct tuples.  The result is never NULL. */
typedef enum { RDF_MEMBER_SEMI = 0, RDF_MEMBER_ANTI = 1, RDF_MEMBER_IS_IN = 2 } rdf_member_kind;
typedef enum { RDF_KEEP_FIRST = 0, RDF_KEEP_LAST = 1, RDF_KEEP_NONE = 2 } rdf_keep;
#define RDF_MEMBER_MAX_KEYS 4

rdf_status rdf_member_mask(const rdf_sort_key* left_keys, int64_t left_nchunks, const rdf_sort_key* right_keys,
                           int64_t right_nchunks, int32_t nkeys, int32_t kind,
                           rdf_out* out_mask /* left_nchunks RDF_BOOL outputs, or NULL */, int64_t* out_rows);

rdf_status rdf_first_occurrence(const rdf_sort_key* keys, int32_t nkeys, int64_t nchunks, int32_t keep,
                                rdf_out* out_mask /* nchunks RDF_BOOL outputs, or NULL */, int64_t* out_rows);

/* ------------------------------------------------------------------ sorted GROUP BY: count_distinct, sum_distinct, first, last */

/* The aggregations of a GROUP BY that need the rows of a group in an order: AggregateFunctions::count_distinct,
 * sum_distinct, first and last (src/functions/aggregate.rs declares them with empty bodies; Dataset::try_aggregate,
 * src/expression.rs:114-221, plans CountDistinct / First / Last), so the semantics are SQL's / Spark's, written down here.
 * One call answers up to 8 functions of ONE value column from ONE sort over (grouping keys, value) — rdf_window's sort and
 * peer rules (see below), with the grouping columns as partition keys and the value column as the one order key.
 *
 * group_by: 0 .. 4 rdf_sort_key (numeric or Utf8 chunks per key, rdf_lexsort_to_indices' conventions); value: ONE
 * rdf_sort_key, numeric or Utf8, NULL iff ncalls == 0.  The `options` of every key are ignored.  Rows are numbered over the
 * concatenation of the chunks.  Inputs and outputs all in host memory or all in device memory.
 *   - Groups: rows that agree on every grouping key; NULL is a key value of its own.  Float keys compare as in rdf_window /
 *     rdf_uniques: -0.0 == +0.0, one NaN.  ngroup == 0: all rows are one group.  Zero rows give zero groups and a valid
 *     call (so does a call with no keys and no value: it has no rows).
 *   - Groups are emitted in ascending key order: key 0 most significant, NULLs last, NaN after +inf.  *out_groups = the
 *     number of groups.
 *   - out_group_rows[g] (RDF_U32, or NULL): the row index of the first row of group g in row order; gather the key columns,
 *     numeric or Utf8, with rdf_take / rdf_utf8_take.  ncalls == 0 returns only this: the distinct key tuples.
 *   - outs[c] is ONE array of one entry per group for calls[c]:
 *       COUNT_DISTINCT  RDF_I64: the distinct non-NULL values of the group, by the sort's peer rule (floats canonical, Utf8
 *                       by bytes, the empty string is a value); 0 for a group without a non-NULL value.
 *       SUM_DISTINCT    RDF_F64 for Float32 / Float64 values (Float32 widened to double before adding), RDF_I64 otherwise
 *                       (wrapping mod 2^64, as rdf_groupby_agg's sums): the sum of the distinct non-NULL values; 0 for a
 *                       group without one, as rdf_groupby_agg — COUNT_DISTINCT tells the two apart.  -0.0 / +0.0 count once,
 *                       as +0.0.  IEEE otherwise: a NaN among the values gives NaN, +inf with -inf gives NaN.  With m
 *                       distinct finite values v the result is within gamma(m - 1) * sum|v| of the exact sum, whatever the
 *                       grouping.  A Utf8 value column: RDF_INVALID_ARGUMENT.
 *       FIRST / LAST    RDF_U32 ROW INDICES, the LAG / LEAD convention: the smallest / largest row index of the group; with
 *                       ignore_nulls != 0 the smallest / largest among the rows whose value is not NULL, NULL when the
 *                       group has none (a validity bitmap is then required if any value chunk carries validity; it is
 *                       written where given).  Without ignore_nulls every index is valid, and rdf_take / rdf_utf8_take of
 *                       the value column returns NULL where that row's value is NULL: SQL's first(x).
 *     ignore_nulls is read by FIRST / LAST only.
 *   - The result is a function of the multiset of rows alone: groups come in key order and a Float64 sum is accumulated in
 *     an order fixed by the sorted distinct values and the group boundaries — no atomics — so row order (after mapping
 *     FIRST / LAST back), chunking, memory kind and repetition do not change a byte.
 * Sizing: *out_groups, out_group_rows->length and every outs[c].length are set once the groups are counted; any given
 * capacity below the group count is RDF_MEMORY_ERROR with nothing written; a capacity of the rows always suffices;
 * out_group_rows == NULL with ncalls == 0 is the count-only call.
 * Errors, all before any device work: an unknown fn, more than 8 calls or 4 keys, a key or the value setting both pointers
 * or neither, wrong dtypes or output dtypes, a missing validity bitmap, mixed memory kinds, 2^32 rows or more
 * RDF_INVALID_ARGUMENT; chunk row counts that differ between columns RDF_COMPUTE_ERROR.
 * RDF_GROUP_SORTED_TILE is the tile of the fold over the distinct (group, value) pairs (rdf_group_sorted.hip): tests place
 * group boundaries around its multiples. */
#define RDF_GROUP_MAX_CALLS 8
#define RDF_GROUP_SORTED_TILE 256
typedef enum { RDF_GRP_COUNT_DISTINCT = 0, RDF_GRP_SUM_DISTINCT = 1, RDF_GRP_FIRST = 2, RDF_GRP_LAST = 3 } rdf_group_fn;
typedef struct { int32_t fn; int32_t ignore_nulls; } rdf_group_call;
rdf_status rdf_groupby_sorted(const rdf_sort_key* group_by, int32_t ngroup, const rdf_sort_key* value, int64_t nchunks,
                              const rdf_group_call* calls, int32_t ncalls, rdf_out* out_group_rows, rdf_out* outs,
                              int64_t* out_groups);

/* ------------------------------------------------------------------ moments per group: variance, stddev, skewness, kurtosis, covar, corr */

/* Up to 8 statistics of ONE value column x — or of ONE pair (x, y) — per group of 0 .. 4 grouping keys: the grouped form of
 * rdf_moments / rdf_comoments (AggregateFunction::Variance / StdDev / Skewness / Kurtosis per group).  ONE sort over the
 * grouping keys alone, then one moment state per group, then the statistics read off the states.
 *
 * Keys, groups, their order (ascending, NULL last, floats canonical), out_group_rows, memory kinds, the 2^32 row limit, the
 * sizing rule and the count-only call (out_group_rows == NULL, ncalls == 0, out_counts == NULL, out_states == NULL) are
 * rdf_groupby_sorted's: any given capacity below the group count is RDF_MEMORY_ERROR with nothing written and the group
 * count in *out_groups and every length.  group_by takes 0 .. 4 keys, each numeric or Utf8; ngroup == 0 makes all rows one
 * group.
 *   - x is nchunks numeric chunks of any of the ten dtypes, every value converted `as f64` like rdf_moments.  y is NULL, or
 *     nchunks numeric chunks of the same lengths; its dtype may differ from x's.  A row counts when its x is valid, and with
 *     y given when both are valid.  There is no mask argument: a caller filters first.  x is NULL exactly when nothing but
 *     the key tuples is asked for (ncalls == 0, out_counts == NULL, out_states == NULL).
 *   - calls[c].stat is an rdf_stat when y == NULL and an rdf_costat otherwise.  outs[c] is RDF_F64, one entry per group, and
 *     a validity bitmap is REQUIRED for every call: a statistic is absent without any NULL input (VAR_SAMP of one row,
 *     SKEWNESS with M2 == 0).  "Absent" is exactly out_is_some == 0 of rdf_moments_stat / rdf_comoments_stat on the
 *     group's state; the value under a NULL is 0 and null_count is set.
 *   - A group whose rows all fail to count still appears: count 0, the all-zero state, every statistic NULL.  A non-finite
 *     counted value makes every statistic of THAT group NaN (valid, not NULL); other groups are untouched.
 *   - out_counts (optional, RDF_I64): the counted rows per group.
 *   - out_states (optional): one rdf_moments_state (y == NULL) or rdf_comoments_state per group, in group order, in the
 *     memory kind of the inputs; states_capacity counts states and follows the sizing rule.  They are what
 *     rdf_moments_merge / rdf_comoments_merge combine across shards and what rdf_*_stat read.  ncalls == 0 with out_states
 *     or out_counts given is valid.
 *   - Accuracy: every group's state is held to rdf_moments' bound with n the GROUP's count: the per-group sums
 *     of x and x^2 are never formed.
 *   - Determinism: no float atomics, no block waits for another.  Chunking, offsets, memory kind and repetition change no
 *     byte of any output.  Row order inside a group is the summation order: a shuffle of the rows may change last bits,
 *     inside the bound, never a count.
 * Errors, all RDF_INVALID_ARGUMENT before any device work with nothing written, in this order: null out_groups; a bad key
 * count or key list; a bad call count or call list; x missing while anything but the key tuples is asked for, or x given
 * with nothing asked (y without x included); an unknown stat for the form; the keys' own rules (rdf_groupby_sorted's); a
 * non-numeric x / y or chunks of mixed dtypes; a wrong output dtype; a missing validity bitmap; a wrong out_counts /
 * out_group_rows dtype; out_states with states_capacity < 0; mixed memory kinds.  Chunk lengths that differ between the
 * columns are RDF_COMPUTE_ERROR.
 * RDF_GROUP_MOMENTS_TILE is the sorted rows of one level-0 tile (rdf_group_moments.hip): tests place group boundaries
 * around its multiples. */
#define RDF_GROUP_MOMENTS_MAX_CALLS 8
#define RDF_GROUP_MOMENTS_TILE 256
typedef struct { int32_t stat; int32_t reserved; } rdf_group_stat_call;   /* rdf_stat when y == NULL, rdf_costat otherwise */
rdf_status rdf_groupby_moments(const rdf_sort_key* group_by, int32_t ngroup, const rdf_array* x, const rdf_array* y,
                               int64_t nchunks, const rdf_group_stat_call* calls, int32_t ncalls, rdf_out* out_group_rows,
                               rdf_out* outs, rdf_out* out_counts, void* out_states, int64_t states_capacity,
                               int64_t* out_groups);

/* ------------------------------------------------------------------ percentiles and median per group */

/* Up to 8 percentiles of ONE value column per group of 0 .. 4 grouping keys, all from ONE sort over (grouping keys, value).
 * The reference's aggregate.rs stops before percentiles; the semantics are Spark 3's `percentile` (its formula restated) for
 * RDF_PCT_CONT and SQL's percentile_disc for RDF_PCT_DISC, and tests/percentile_ref.py is their executable definition.
 * `median` is {RDF_PCT_CONT, 0, 0.5}.
 *
 * Keys, value, groups, their order (ascending, NULL last), out_group_rows, memory kinds, the row limit, the sizing rule and
 * the count-only call (out_group_rows == NULL, ncalls == 0, out_counts == NULL) are rdf_groupby_sorted's.  value is NULL
 * exactly when ncalls == 0 and out_counts == NULL.
 *   - A group's non-NULL values are taken in the sort's order: NaN after +inf, -0.0 and +0.0 peers, Utf8 by unsigned bytes.
 *     m is their count.  out_counts (optional) is ONE RDF_I64 array of m per group.
 *   - m == 0 gives NULL for every call: every outs[c] needs a validity bitmap when any value chunk carries validity; a
 *     bitmap is written wherever one is given, and null_count is set.  The value under a NULL is 0.
 *   - RDF_PCT_CONT: output RDF_F64, numeric values only.  d(v) = (double)v: Float32 widened, integers rounded to nearest
 *     even, -0.0 read as +0.0, every NaN the quiet NaN 0x7FF8000000000000.  pos = (double)(m - 1) * p, lo = floor(pos),
 *     hi = ceil(pos).  If lo == hi or the values at sorted positions lo and hi are peers the result is d(v_lo); otherwise
 *     (hi - pos) * d(v_lo) + (pos - lo) * d(v_hi), two multiplies and one add, each rounded (no FMA).  IEEE otherwise: a
 *     -inf / +inf pair gives NaN.  A NaN result is 0x7FF8000000000000.
 *   - RDF_PCT_DISC: output RDF_U32 ROW INDICES (the FIRST / LAST / LAG convention; gather with rdf_take / rdf_utf8_take), any
 *     value type.  k = max(0, (int64)ceil(p * (double)m) - 1); the result is the smallest row index of the group whose value
 *     is a peer of the k-th sorted value.
 *   - The result is a function of the multiset of rows alone: chunking, offsets, memory kind and repetition change no byte;
 *     shuffling the rows changes only the DISC indices, which map back to the same values.
 * Errors, all before any device work, in this order: null out_groups; a bad key count or key list; a bad call count or call
 * list; a value column missing or unasked for; an unknown kind; p outside [0, 1] or NaN; then the keys' and value's own
 * rules (rdf_groupby_sorted's); CONT of a Utf8 column; a wrong output dtype; a missing validity bitmap; a wrong out_counts
 * or out_group_rows dtype; mixed memory kinds: RDF_INVALID_ARGUMENT.
 * Routes.  The SORTED route serves every call: rdf_window's front over (grouping keys, value), then one thread per (group,
 * call).  The SELECT route serves ngroup == 0 with a numeric value and runs no sort: a radix select over the values' ordered
 * unsigned images, RDF_PCT_SELECT_BITS per pass, candidates re-read under a prefix test until at most RDF_PCT_SELECT_FINISH
 * of them are left (one block sorts those in LDS) or the key's bits are used up — at most ceil(key bits / digit bits) counting
 * reads plus one collecting read, whatever the values hold.  Both routes give the same bytes.
 * Under auto the select route takes every call it can serve: it measured faster for every dtype, size and distribution
 * tried.
 * rdf_set_option("percentile_route", 0 auto | 1 sorted | 2 select); 2 on a call the select route cannot serve is
 * RDF_INVALID_ARGUMENT (refused after the kinds and p, before the keys are looked at); rdf_last_kernel names the route taken.
 * RDF_PERCENTILE_PICK_BLOCK is the block of the kernel that answers one (group, call) per thread, RDF_PCT_SELECT_TILE the
 * rows of one block tile of the select route's streaming passes: tests place group counts and row counts around them. */
#define RDF_PERCENTILE_MAX_CALLS 8
#define RDF_PERCENTILE_PICK_BLOCK 256
#define RDF_PCT_SELECT_BITS 8
#define RDF_PCT_SELECT_TILE 4096
#define RDF_PCT_SELECT_FINISH 2048
typedef enum { RDF_PCT_CONT = 0, RDF_PCT_DISC = 1 } rdf_percentile_kind;
typedef struct { int32_t kind; int32_t reserved; double p; } rdf_percentile_call;
rdf_status rdf_groupby_percentile(const rdf_sort_key* group_by, int32_t ngroup, const rdf_sort_key* value, int64_t nchunks,
                                  const rdf_percentile_call* calls, int32_t ncalls, rdf_out* out_group_rows, rdf_out* outs,
                                  rdf_out* out_counts, int64_t* out_groups);

/* ------------------------------------------------------------------ collect per group and explode: collect_list, collect_set, explode */

/* The three operations that connect rows with lists: ArrayFunction::CollectList / CollectSet (src/expression.rs:691-692,
 * collect_list() / collect_set() in src/functions/array.rs:404-405) and ScalarFunctions::explode() (src/functions/scalar.rs:237).
 * All three have empty bodies in the reference, so the semantics are SQL's / Spark's, written down here.
 *
 * rdf_groupby_collect: ONE List row per group of 0 .. 4 grouping keys, collected from ONE value column; keys and value are
 * rdf_sort_key under rdf_groupby_sorted's conventions (numeric or Utf8 chunks, `options` ignored, rows numbered over the
 * concatenation of the chunks, inputs and outputs all in host memory or all in device memory, fewer than 2^32 rows).
 *   - Groups as in rdf_groupby_sorted: NULL is a key value of its own, floats compare canonically (-0.0 == +0.0, one NaN),
 *     groups come in ascending key order with NULL last, out_group_rows[g] (RDF_U32) is the first row of group g,
 *     ngroup == 0 makes all rows one group.  Zero rows give zero groups and a valid call that writes nothing (every
 *     length 0, out_offsets' included: a List of no rows has no offsets to read).
 *   - out_offsets (RDF_I32): G + 1 entries starting at 0.  Every list is valid; a group without a non-NULL value gets an
 *     EMPTY list, as in Spark.
 *   - kind RDF_COLLECT_LIST: the group's rows whose value is not NULL, in ascending row order.
 *     kind RDF_COLLECT_SET:  the group's distinct non-NULL values by the sort's peer rule (-0.0 == +0.0, one NaN, Utf8 by
 *     bytes, the empty string is a value), each once, in ascending value order (NaN after +inf): no hash order shows.
 *   - The child as row indices: out_child_rows (RDF_U32, E entries, the FIRST / LAG convention) holds the row index of every
 *     element, for SET the smallest row index holding that value.  rdf_take / rdf_utf8_take of the value column by it build
 *     the child array, so one output form serves every value type.
 *   - The child as values: out_values (optional, numeric value columns only; with a Utf8 value RDF_INVALID_ARGUMENT) has the
 *     value's dtype and is written in the same pass.  For SET floats come out canonical: +0.0 for either zero and the quiet
 *     NaN 0x7ff8000000000000 / 0x7fc00000, so out_values is a function of the multiset of rows alone.  LIST copies bits.
 *   - Determinism: no atomics on data.  Chunking, memory kind and repetition change no byte; for SET the row order changes
 *     no byte of out_offsets and out_values, and out_child_rows only through the row mapping.
 * Sizing: *out_groups (G) and *out_elements (E) and every length are set once known; any given capacity that is too small
 * (G for the group rows, G + 1 for the offsets, E for the child) is RDF_MEMORY_ERROR with nothing written; capacities of the
 * rows (rows + 1 for the offsets) always suffice; every output may be NULL, and all four NULL is the count-only call.
 * E > 2^31 - 1 is RDF_COMPUTE_ERROR (Int32 offsets; it takes 2^31 rows, which no test reaches).
 * Errors, all before any device work: an unknown kind, more than 4 keys, a NULL value, a key or the value setting both
 * pointers or neither, wrong dtypes or output dtypes, out_values with a Utf8 value, mixed memory kinds, 2^32 rows or more
 * RDF_INVALID_ARGUMENT; chunk row counts that differ between columns RDF_COMPUTE_ERROR.
 * RDF_COLLECT_TILE: items per tile of the compaction and expansion passes (rdf_collect.hip); tests place boundaries around
 * its multiples.
 *
 * rdf_list_explode: every element of every non-NULL list becomes one output row, ordered by list row, then by position.
 * Only list->offsets (and its validity / offset fields) is read; list->values is the caller's to gather from.
 *   - out_parent_rows (RDF_U32): the list row; it feeds rdf_take_columns for the frame's other columns.
 *     out_child_index (RDF_U32): the element's index into list->values; it feeds rdf_take.
 *     out_pos (optional, RDF_I32): the 0-based position inside the list (posexplode).
 *   - The slice of a NULL list is skipped even where its offsets span elements (Arrow allows that; rdf_list_remove treats
 *     it the same way).  Offsets need not start at 0, and the array may be sliced (`offset` fields).
 *   - outer != 0 (explode_outer): a NULL or empty list yields ONE row whose out_child_index and out_pos are NULL (their
 *     values are 0); validity bitmaps are then required for both, as for FIRST with ignore_nulls.
 * Sizing and errors as above: *out_rows and every length are set once known, a capacity below it is RDF_MEMORY_ERROR with
 * nothing written, all three outputs NULL is the count-only call, zero list rows is a valid call that writes nothing;
 * non-Int32 offsets, wrong output dtypes, a missing bitmap, mixed memory kinds, 2^32 list rows: RDF_INVALID_ARGUMENT. */
#define RDF_COLLECT_TILE 1024
typedef enum { RDF_COLLECT_LIST = 0, RDF_COLLECT_SET = 1 } rdf_collect_kind;
rdf_status rdf_groupby_collect(const rdf_sort_key* group_by, int32_t ngroup, const rdf_sort_key* value, int64_t nchunks,
                               int32_t kind, rdf_out* out_group_rows, rdf_out* out_offsets, rdf_out* out_child_rows,
                               rdf_out* out_values, int64_t* out_groups, int64_t* out_elements);
rdf_status rdf_list_explode(const rdf_list_array* list, int32_t outer, rdf_out* out_parent_rows, rdf_out* out_child_index,
                            rdf_out* out_pos, int64_t* out_rows);

/* ------------------------------------------------------------------ window functions */

/* SQL window functions over partitions: row_number / rank / dense_rank / percent_rank / cume_dist / ntile / lag / lead.
 * The reference declares them (src/functions/window.rs, WindowSpec in src/window.rs, ntile in src/functions/scalar.rs) with
 * empty bodies, so the semantics are SQL's / Spark's, written down here.  One call answers up to 8 functions from ONE sort.
 *
 * partition_by / order_by are rdf_sort_key lists (numeric or Utf8 chunks per key, rdf_lexsort_to_indices' conventions;
 * 0 .. 4 keys each).  The `options` of a partition key are ignored; `descending` of an order key is honoured.  Rows are
 * numbered over the concatenation of the chunks; outs[c] is ONE array of all rows for calls[c] in the ORIGINAL row order
 * (row i's answer at position i).  Inputs and outputs all in host memory or all in device memory.
 *   - Partitions: rows are in one partition iff they agree on every partition key.  NULL is a key value of its own.  No
 *     partition keys: one partition of all rows.
 *   - Order inside a partition: by the order keys, key 0 most significant, `descending` per key; NULLs last in both
 *     directions (nulls_first is ignored); ties keep ascending row order.  No order keys: row order, and every row of a
 *     partition is a peer of every other.
 *   - Peers: rows of one partition that agree on every order key; NULL agrees with NULL.
 *   - Float keys (partition and order alike) compare as rdf_uniques does: -0.0 == +0.0, every NaN equals every NaN, NaN
 *     sorts after +inf (before it when descending).  rdf_sort_to_indices' IEEE total order is not changed by this.
 *   - With k = 0-based position of the row in its ordered partition, n = rows of the partition, f / l = position of the
 *     row's first / last peer, d = number of peer groups before the row's own:
 *       ROW_NUMBER k + 1;  RANK f + 1;  DENSE_RANK d + 1;
 *       PERCENT_RANK n == 1 ? 0.0 : (double)f / (double)(n - 1);  CUME_DIST (double)(l + 1) / (double)n  (one IEEE division
 *       of exact integers each: bit-exact against any CPU);
 *       NTILE(b): q = n / b, r = n % b; k < r(q+1) ? k/(q+1) + 1 : r + (k - r(q+1))/q + 1  (b > n gives k + 1);
 *       LAG(o) / LEAD(o): the ROW INDEX (in the concatenation) of the row at position k - o / k + o of the same partition,
 *       NULL when that position is outside it; offset 0 is the row itself.  Gather any column, numeric or Utf8, with
 *       rdf_take / rdf_utf8_take: their "NULL index -> NULL row" rule gives SQL's default.
 *   - Output dtypes: RDF_I64 for ROW_NUMBER / RANK / DENSE_RANK / NTILE, RDF_F64 for PERCENT_RANK / CUME_DIST, RDF_U32
 *     with a validity bitmap for LAG / LEAD (validity required when the offset is > 0; written where given otherwise).
 * param: NTILE buckets >= 1; LAG / LEAD offset >= 0; not read for the other functions.
 * With no keys at all the row count is nrows_if_no_keys (nchunks is ignored); otherwise nchunks >= 1 and nrows_if_no_keys
 * is 0 or the keys' rows.  Zero rows is a valid call that writes nothing.
 * Errors, all before any device work: no calls, an unknown fn, param out of range, more than 4 keys of a kind or 8 calls,
 * a key setting both pointers or neither, wrong dtypes, a missing validity for LAG / LEAD with offset > 0, mixed memory
 * kinds, nrows_if_no_keys that contradicts the keys, an output with a capacity and no buffer: RDF_INVALID_ARGUMENT;
 * chunk row counts that differ between keys: RDF_COMPUTE_ERROR; 2^32 rows or more: RDF_INVALID_ARGUMENT; an output
 * capacity below the rows: RDF_MEMORY_ERROR with every
 * outs[c].length set to the rows and nothing written. */
typedef enum {
    RDF_WIN_ROW_NUMBER = 0, RDF_WIN_RANK = 1, RDF_WIN_DENSE_RANK = 2, RDF_WIN_PERCENT_RANK = 3, RDF_WIN_CUME_DIST = 4,
    RDF_WIN_NTILE = 5, RDF_WIN_LAG = 6, RDF_WIN_LEAD = 7
} rdf_window_fn;
typedef struct { int32_t fn; int32_t pad; int64_t param; } rdf_window_call;
#define RDF_WINDOW_MAX_KEYS 4
#define RDF_WINDOW_MAX_CALLS 8
rdf_status rdf_window(const rdf_sort_key* partition_by, int32_t npartition, const rdf_sort_key* order_by, int32_t norder,
                      int64_t nchunks, int64_t nrows_if_no_keys, const rdf_window_call* calls, int32_t ncalls, rdf_out* outs);

/* Window FRAMES: sum / min / max / count / avg / first_value / last_value over WindowSpec::rows_between / range_between
 * (src/window.rs; the aggregates are AggregateFunctions' of src/functions/aggregate.rs).  Up to 8 calls, each with its own
 * frame and one of up to 4 value columns, all answered from ONE sort.  Partitions, order, peers, float key
 * canonicalisation, chunk conventions, memory kinds, the 2^32-row cap and "outs[c] is one array in the original row
 * order" are rdf_window's rules above, unchanged; so are zero rows, short capacities and the error codes.
 *
 * values[v]: nchunks chunks of one dtype, Int64 or Float64 (other dtypes RDF_INVALID_ARGUMENT, as rdf_hist), with the keys'
 * rows per chunk.  With no keys at all the value chunks give the rows (no value columns either: nrows_if_no_keys, nchunks
 * ignored); nrows_if_no_keys is 0 or agrees.  calls[c].value indexes `values`; -1 is allowed for COUNT (count the frame's
 * rows) and FIRST_VALUE / LAST_VALUE (they read no values).
 *
 * The frame of a row at position k of n in its ordered partition, with first / last peer f / l, is the closed range [a, b]:
 *   ROWS   UNBOUNDED_PRECEDING 0;  PRECEDING s  k - s;  CURRENT_ROW k;  FOLLOWING s  k + s;  UNBOUNDED_FOLLOWING n - 1
 *   RANGE  the two unbounded kinds as above; CURRENT_ROW is f as a start and l as an end (SQL's default frame, RANGE
 *          BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW, is [0, l]).  RANGE with an offset: RDF_INVALID_ARGUMENT ("range
 *          offsets are not built"): an offset there has the order key's type, see rdf_window_range_agg below.
 * then a = max(a, 0), b = min(b, n - 1); the frame is empty when a > b.
 *
 * Results, with c = the valid (non-NULL) value rows of the frame — NULL rows are skipped:
 *   COUNT        RDF_I64, never NULL: c, or b - a + 1 with value == -1; an empty frame gives 0.
 *   SUM          the value dtype, with validity.  NULL when c == 0: SQL's rule, deliberately NOT rdf_sum's 0.  Int64: the
 *                wrapping sum, bit-exact.  Float64: the partition's running sum is carried as a double-double (Knuth's
 *                TwoSum on both words, relative error <= 3u^2 + 13u^3 per addition, u = 2^-53); the frame's value is the
 *                double-double difference of two prefixes rounded ONCE, a zero comes back as +0.0.  Non-finite values are
 *                counted, not summed: any NaN or both infinities in the frame give NaN, one kind of infinity that
 *                infinity; a frame after them is finite again.  With F = the exact sum of the frame, m = the partition's
 *                rows up to the frame's end and T = the sum of |x| over them: |result - F| <= ulp(F) + 8 (m + 1) 2^-106 T;
 *                integer-valued doubles whose partial sums stay below 2^53 give F bit for bit.  (A partition whose running
 *                sum of |x| itself overflows Float64 returns what IEEE arithmetic gives.)
 *   AVG          RDF_F64, with validity: NULL when c == 0, else the Float64 SUM / (double)c, one IEEE division; Int64
 *                values enter `as f64` and take the Float64 path.
 *   MIN / MAX    the value dtype, with validity: NULL when c == 0.  Float64 follows rdf_min / rdf_max: NaNs are ignored
 *                unless every valid value of the frame is NaN (then the quiet NaN 0x7FF8000000000000); other values
 *                compare in IEEE total order (-0.0 < +0.0), so the result is one of the inputs bit for bit.
 *   FIRST_VALUE / LAST_VALUE   RDF_U32 ROW INDICES with validity, the LAG / LEAD convention: the row at position a / b,
 *                for rdf_take / rdf_utf8_take (any column type; NULL values are not skipped); an empty frame gives NULL.
 * null_count is set on every output.  A validity bitmap is required for every function but COUNT (written all-valid where
 * given).
 * Refused before any device work with RDF_INVALID_ARGUMENT: a start of UNBOUNDED_FOLLOWING, an end of
 * UNBOUNDED_PRECEDING, a start that lies after the end for every row (start kind > end kind; both PRECEDING with
 * start < end; both FOLLOWING with start > end), a negative offset, an unknown unit, kind or fn, a value index out of
 * range or -1 for SUM / MIN / MAX / AVG, more than 4 value columns or 8 calls, a wrong output dtype, a missing validity
 * bitmap.  Scratch that does not fit device memory is RDF_MEMORY_ERROR, never a partial answer. */
typedef enum { RDF_FRAME_ROWS = 0, RDF_FRAME_RANGE = 1 } rdf_frame_unit;
typedef enum {
    RDF_BOUND_UNBOUNDED_PRECEDING = 0, RDF_BOUND_PRECEDING = 1, RDF_BOUND_CURRENT_ROW = 2, RDF_BOUND_FOLLOWING = 3,
    RDF_BOUND_UNBOUNDED_FOLLOWING = 4
} rdf_frame_bound;
typedef struct { int32_t unit, start_kind, end_kind, pad; int64_t start, end; } rdf_window_frame;
typedef enum {
    RDF_WAGG_SUM = 0, RDF_WAGG_MIN = 1, RDF_WAGG_MAX = 2, RDF_WAGG_COUNT = 3, RDF_WAGG_AVG = 4, RDF_WAGG_FIRST_VALUE = 5,
    RDF_WAGG_LAST_VALUE = 6
} rdf_window_agg_fn;
typedef struct { int32_t fn; int32_t value; rdf_window_frame frame; } rdf_window_agg_call;
#define RDF_WINDOW_MAX_VALUES 4
rdf_status rdf_window_agg(const rdf_sort_key* partition_by, int32_t npartition, const rdf_sort_key* order_by, int32_t norder,
                          const rdf_array* const* values, int32_t nvalues, int64_t nchunks, int64_t nrows_if_no_keys,
                          const rdf_window_agg_call* calls, int32_t ncalls, rdf_out* outs);

/* Window frames with VALUE offsets: RANGE BETWEEN s PRECEDING AND e FOLLOWING over ONE numeric order key (Spark's
 * rangeBetween(-s, e), a rolling 7-day sum, "events within 500 us of this one").  rdf_window_agg refuses such frames; this
 * entry point answers them, and every frame without an offset as rdf_window_agg's RANGE unit does.  Inherited unchanged:
 * partitions (0 .. 4 keys, numeric or Utf8), peers and the float canonicalisation of the keys; chunk conventions, memory
 * kinds, "outs[c] is one array in the original row order"; value dtypes (Int64 / Float64, up to 4 columns), up to 8 calls
 * from ONE sort, output dtypes and validity rules; every function's result rules (NULL when no valid row, wrapping Int64
 * sums, the double-double Float64 sum and its bound, MIN / MAX in IEEE total order, FIRST / LAST as row indices); zero
 * rows, short capacities, the 2^32-row cap, the error codes, and "all refusals before any device work, nothing written".
 *
 * Order key: norder must be 1 and the key numeric, RDF_I32, RDF_I64 (dates, timestamps and times are passed as their
 * storage) or RDF_F64; `descending` is honoured.  Anything else: RDF_INVALID_ARGUMENT.
 * Bounds, in positions of the ordered partition of n rows (first / last peer of the row: f / l):
 *   UNBOUNDED_PRECEDING 0;  UNBOUNDED_FOLLOWING n - 1 (the NULL and NaN rows at the partition's end included);
 *   CURRENT_ROW f as a start, l as an end.
 *   An offset bound of an ORDINARY row (key o not NULL and not NaN; the ordinary rows of a partition are one run of
 *   positions: NULLs sort last, NaN after +inf, before it when descending).  With d = +1 ascending, -1 descending the bound
 *   VALUE is v = o - d s for PRECEDING s and o + d s for FOLLOWING s.  A start is the first position of the run whose key is
 *   not before v in the sort direction (none: one past the run's last position); an end is the last position of the run
 *   whose key is not after v (none: one before the run's first position).  It never reaches a NULL or NaN row.
 *     Integer keys (Int32 widens to Int64): v is the mathematical integer, no wrap; INT64_MIN with offset 2^63 - 1 is exact.
 *     Float64 keys: v is ONE IEEE operation, fl(o - s) or fl(o + s), compared with the keys by IEEE < and > (-0.0 == +0.0):
 *     with keys 0.1, 0.3 and offset 0.2, 0.1 lies in 0.3's frame iff 0.1 >= fl(0.3 - 0.2).  +-inf keys follow the arithmetic.
 *   An offset bound of a NULL or NaN row: its own peer group, f as a start, l as an end (Spark's and PostgreSQL's rule).
 * The frame is [a, b]; a > b is an empty frame: COUNT 0, the others NULL.
 * Offsets: start_i / end_i (>= 0) are read when the order key is Int32 / Int64, start_f / end_f (finite, >= 0) when it is
 * Float64, and only for PRECEDING / FOLLOWING.
 * Refused with RDF_INVALID_ARGUMENT: the static frame errors of rdf_window_agg (a start of UNBOUNDED_FOLLOWING, an end of
 * UNBOUNDED_PRECEDING, start kind > end kind, both PRECEDING with start < end, both FOLLOWING with start > end, unknown
 * kinds), a negative integer offset, a Float64 offset that is negative, NaN or infinite, and MIN / MAX with neither side
 * unbounded ("min / max over a range frame bounded on both sides is not built"; with one unbounded side they are the
 * forward / backward scans' F[b] / B[a]).
 * rdf_set_option("window_range_route", v) chooses how the bounds are searched: 0 = auto, 1 = a tile's key window is staged
 * in LDS wherever it fits (what auto decides today as well: 0 and 1 behave alike until auto declines a window that fits),
 * 2 = every lane searches the sorted keys in global memory; no value changes a byte of a result,
 * and rdf_last_kernel() names wrange_bounds_lds_kernel / wrange_bounds_global_kernel as they were used. */
typedef struct { int32_t start_kind, end_kind;      /* rdf_frame_bound */
                 int64_t start_i, end_i;            /* offsets >= 0, read when the order key is Int32 / Int64 */
                 double  start_f, end_f; } rdf_window_range_frame;   /* read when it is Float64; 40 bytes */
typedef struct { int32_t fn; int32_t value; rdf_window_range_frame frame; } rdf_window_range_call;   /* rdf_window_agg_fn; 48 bytes */
rdf_status rdf_window_range_agg(const rdf_sort_key* partition_by, int32_t npartition, const rdf_sort_key* order_by, int32_t norder,
                                const rdf_array* const* values, int32_t nvalues, int64_t nchunks,
                                const rdf_window_range_call* calls, int32_t ncalls, rdf_out* outs);

/* ------------------------------------------------------------------ fused batch loop */

typedef enum {
    RDF_SINK_STORE = 0, /* materialise every value expression as a new column (Evaluate::calculate) */
    RDF_SINK_AGG = 1    /* fold every value expression into {sum,min,max,count} (AggregateFunctions) */
} rdf_sink;

#define RDF_MAX_VALUES 4

/* A maximal run of Calculate / Filter / aggregate steps of Evaluate::evaluate
 * (src/evaluation.rs:66-96) fused into one pass per batch. */
typedef struct {
    const rdf_expr_node* nodes;
    int32_t nnodes;
    int32_t filter_root;                 /* BooleanFilter root or -1: rows where it is false/null are dropped */
    int32_t nvalues;                     /* 1..RDF_MAX_VALUES */
    int32_t value_roots[RDF_MAX_VALUES];
    int32_t sink;                        /* rdf_sink */
} rdf_program;

/* AggregateFunctions results for one value expression.  sum/min/max are returned in the value's
 * class: f64 for F32/F64 values, i64 bit pattern (wrapped to the value's width) otherwise. */
typedef struct {
    double  sum_f64, min_f64, max_f64;
    int64_t sum_i64, min_i64, max_i64;
    int64_t count;    /* valid rows that passed the filter */
    int32_t is_some;  /* count > 0 */
    int32_t dtype;    /* value dtype */
} rdf_agg_result;

/* Host-resident batches (RDF_MEM_HOST) beyond one slab (256 MiB; rdf_set_option("stream_slab_bytes", n), -1 = never) are STREAMED
 * by every entry point that takes chunk lists — rdf_pipeline (both sinks), rdf_binary / rdf_unary / rdf_cast / rdf_hour /
 * rdf_predicate, the column aggregates, rdf_group_pipeline, rdf_groupby_agg (one Int64 / UInt64 key column), rdf_filter_pipeline:
 * slab k + 1 crosses the link while the kernel runs over slab k, results that are columns leave on a third stream, aggregates
 * are folded in slab order.  Float SUMS of a streamed call are therefore folded per slab (f64): their low bits depend on where the
 * slabs are cut (stream_slab_bytes, the batch lengths) and — with the run-time compiler working in the background, jit = 1 —
 * on which slab was the first to run compiled; every such result is within the 1e-6 relative the path promises for f64 sums, but
 * two calls need not agree bit for bit.  Integer results, extrema, counts, columns, masks and filtered rows do not depend on it.
 *
 * cols[c * nchunks + i].  SINK_STORE: outs[v * nchunks + i] receives value v of batch i
 * (filter_root must be -1: filter then store is rdf_predicate + rdf_filter_columns).
 * SINK_AGG: aggs[v] receives the aggregates, outs may be NULL. */
rdf_status rdf_pipeline(const rdf_program* prog, const rdf_array* cols, int32_t ncols, int64_t nchunks,
                        rdf_out* outs, rdf_agg_result* aggs);
/* DataFrame::filter(&BooleanFilter) (src/dataframe.rs:178-189) over HOST-resident RecordBatches in ONE call: the predicate
 * (BooleanFilter::eval_to_array, src/expression.rs:766-861) is evaluated and every column compacted on the device, slab by
 * slab — slab k + 1 crosses the link while slab k is filtered and slab k - 1's kept rows travel back on a third stream —,
 * so a frame of any size (larger than free HBM included) is filtered at the link's rate with two slabs of HBM.  Column
 * index c of the expression = column c of `cols`; cols / outs laid out [c * nchunks + i], RDF_MEM_HOST; outs[c * nchunks + i]
 * needs the capacity of its input batch (and a validity buffer where the column carries one) and receives the kept rows of
 * batch i (ChunkedArray::filter keeps batch boundaries, src/table.rs:97-107).  What rdf_predicate + rdf_filter_columns do in
 * two calls with the mask making a round trip through the host; a device-resident frame is filtered with rdf_filter_frame. */
rdf_status rdf_filter_pipeline(const rdf_expr_node* nodes, int32_t nnodes, int32_t root, const rdf_array* cols, int32_t ncols,
                               int64_t nchunks, rdf_out* outs);
/* Host-resident frames are STREAMED: when the RDF_MEM_HOST arrays of a SINK_AGG call hold more than one slab of bytes
 * (rdf_set_option("stream_slab_bytes", ...), default 256 MiB) the batch list is cut into slabs of whole batches (a longer batch
 * on 64-row boundaries), slab k + 1 crosses the link on the copy stream while the fused kernel runs over slab k, and the
 * slabs' partial aggregates are folded in slab order — the batch loop of Evaluate::evaluate (src/evaluation.rs:66-96) over
 * what a reader produced (DataFrame::from_csv / from_arrow, src/dataframe.rs:349-407), with two slabs of HBM in use whatever
 * the frame's size.  Column buffers in page-locked memory (rdf_host_alloc / rdf_host_register) of at least 256 KiB leave with
 * one asynchronous copy each; pageable memory and the readers' small batches are packed into a page-locked staging buffer by
 * a few host threads first.  rdf_stream_stats: slabs (0 = the last rdf_pipeline call of this thread was not streamed), bytes
 * that went through the staging buffer, bytes copied straight out of the caller's page-locked memory. */
rdf_status rdf_stream_stats(int64_t* slabs, int64_t* bytes_staged, int64_t* bytes_direct);

/* A frame handle for repeated calls over the same device-resident columns.  The reference's DataFrame holds its
 * RecordBatches for its lifetime (src/dataframe.rs:30-48) and every query walks them again; with the reader's 1024-row
 * batches (src/dataframe.rs:352) a 1e9-row frame is a million chunks, and validating / translating a million rdf_array
 * descriptors per call (14 ms) costs ten times the kernel (1.2 ms).  rdf_frame_pin does that work once: dtypes and batch
 * lengths checked, descriptors and tile tables kept in HBM.  cols[c * nchunks + i], RDF_MEM_DEVICE only; the buffers
 * must stay alive and unchanged until rdf_frame_release.  rdf_pipeline_frame = rdf_pipeline over the pinned columns
 * (column index c of the program = column c of the pin call); outputs and results exactly as rdf_pipeline.  A handle
 * belongs to the device it was pinned on and is used by one thread at a time. */
typedef struct rdf_frame rdf_frame;
rdf_status rdf_frame_pin(const rdf_array* cols, int32_t ncols, int64_t nchunks, rdf_frame** out);
rdf_status rdf_frame_release(rdf_frame* frame);
rdf_status rdf_pipeline_frame(const rdf_program* prog, rdf_frame* frame, rdf_out* outs, rdf_agg_result* aggs);

/* ------------------------------------------------------------------ frame-level operators
 *
 * DataFrame::filter / take / sort and GroupAggregate over a pinned frame, returning a NEW frame whose buffers the library
 * owns (rdf_frame_release gives them back).  Nothing per RecordBatch crosses to the host: descriptor tables are built by
 * kernels, so a frame held in the readers' 1024-row batches (src/dataframe.rs:352: 976 563 batches for 1e9 rows) costs what
 * its kernels cost — the list-taking entry points above pay O(batches) host work per call (walking rdf_array / rdf_out lists).
 * Frames returned here are ordinary frames: rdf_pipeline_frame, rdf_filter_frame, ... run over them (<= 8 columns for the
 * program-evaluating entry points), rdf_frame_column exports their descriptors.  Every batch of an owned frame starts on a
 * 64-row boundary of its column buffer (values 16-byte, bitmaps 8-byte aligned); null counts are reported as unknown (-1). */

/* columns, batches, rows of a frame */
rdf_status rdf_frame_info(rdf_frame* frame, int32_t* ncols, int64_t* nchunks, int64_t* rows);
/* The rdf_array descriptors of one column (nchunks entries, RDF_MEM_DEVICE, borrowed from the frame): the bridge back to
 * the list-taking entry points and to arrow::array::ArrayData on the Rust side.  O(batches) host work, once per frame. */
rdf_status rdf_frame_column(rdf_frame* frame, int32_t col, rdf_array* chunks);
/* DataFrame::filter(&BooleanFilter) (src/dataframe.rs:178-189): the predicate is evaluated over every batch
 * (BooleanFilter::eval_to_array, src/expression.rs:766-861) and EVERY column of the frame is compacted with it in one pass
 * (Column::filter per column in the reference); batch boundaries are kept (ChunkedArray::filter, src/table.rs:97-107), a
 * batch may become empty.  `root` must be boolean-typed; column index c of the expression = column c of the frame.  The frame may
 * have up to 64 columns; the predicate reads at most 8 of them. */
rdf_status rdf_filter_frame(rdf_frame* frame, const rdf_expr_node* nodes, int32_t nnodes, int32_t root, rdf_frame** out);
/* DataFrame::take's per-column loop (src/dataframe.rs:216-222; DataFrame::join's, :705-711) as ONE gather pass: the index
 * list is read once, each row is resolved to (batch, element) once, and the gathers of all columns of a row are in flight
 * together.  cols[c * nchunks + i]; indices: ONE RDF_U32 / RDF_U64 array; outs: ncols one-chunk outputs.  Semantics per
 * column exactly rdf_take's (null index -> null, out of range -> RDF_COMPUTE_ERROR). */
rdf_status rdf_take_columns(const rdf_array* cols, int32_t ncols, int64_t nchunks, const rdf_array* indices, rdf_out* outs);
/* The same over a pinned frame -> a one-batch frame of indices->length rows (indices: host or device memory). */
rdf_status rdf_take_frame(rdf_frame* frame, const rdf_array* indices, rdf_frame** out);
/* DataFrame::sort (src/dataframe.rs:194-222): lexsort_to_indices over columns sort_cols[0..nsort) of the frame (criterion 0
 * most significant, rdf_sort_to_indices' rules), then the take of every column by that order in one pass.  out_indices
 * (optional, RDF_U32, device memory) receives the row order; out (optional) the sorted one-batch frame. */
rdf_status rdf_sort_frame(rdf_frame* frame, const int32_t* sort_cols, int32_t nsort, const rdf_sort_options* opts,
                          rdf_out* out_indices, rdf_frame** out);
/* rdf_groupby_agg over columns of a frame: grouping columns key_cols[0..nkeys), ONE aggregation of column value_col
 * (ignored for RDF_AGG_COUNT).  -> a one-batch frame of nkeys + 2 columns: the group keys, the aggregate (rdf_groupby_agg's
 * output type), the counts (Int64).  One grouping column runs on the frame's own tables; several are packed first. */
rdf_status rdf_groupby_agg_frame(rdf_frame* frame, const int32_t* key_cols, int32_t nkeys, int32_t value_col, int32_t agg,
                                 int64_t max_groups, rdf_frame** out);

/* ------------------------------------------------------------------ fused grouped aggregation */

#define RDF_MAX_GROUP_VALUES 8
#define RDF_MAX_GROUP_SLOTS  1024   /* (ngroups + 1) * nvalues must not exceed this */

/* sum/count of one value expression inside one group.  sum in the value's class: f64 for F32/F64
 * values (accumulated in f64), wrapping i64 otherwise (widened, not re-wrapped to the value's width). */
typedef struct {
    double  sum_f64;
    int64_t sum_i64;
    int64_t count;    /* rows of the group that passed the filter and whose value is not NULL */
    int32_t is_some;  /* count > 0 */
    int32_t dtype;    /* value dtype */
} rdf_group_result;

/* Transformation::GroupAggregate(groups, [Sum|Average|Count ...]) after a run of Calculate/Filter steps,
 * for a SMALL DENSE group domain (TPC-H Q1's returnflag x linestatus; BASELINE.json config C5), fused into
 * one pass per batch: rows are dropped by `filter_root` (or kept when -1), `group_root` is an
 * integer-valued expression giving each row's group id in [0, ngroups) (e.g. flag * 2 + status over
 * dictionary codes; a NULL id lands in the extra group `ngroups`), and every value expression is summed
 * and counted per group: out[v * (ngroups + 1) + g].  group_rows[g] (may be NULL) = rows in group g after
 * the filter, i.e. SQL count(*).  An id outside [0, ngroups) at a row that passed the filter ->
 * RDF_COMPUTE_ERROR.  Averages are sum / count on the caller's side (AggregateFunctions::avg,
 * src/functions/aggregate.rs:32-65).  The reference plans this step (Dataset::try_aggregate,
 * src/expression.rs:114-221) but does not execute it (src/evaluation.rs:73 panics): semantics are SQL's,
 * parity unpinned by the reference.  f64 sums: every addition is a correctly rounded f64 addition, their order is not
 * deterministic, so a group of n values x_i comes back within gamma(n - 1) * sum|x_i| of the exact sum (gamma(k) =
 * k u / (1 - k u), u = 2^-53: the bound of any order and tree of additions), products are not contracted into the
 * sums, and inputs whose values and partial sums are all exactly representable (integer-valued or small dyadic
 * measures) are summed exactly, bit for bit in every order (tests/group_ref.py is the executable statement).
 * Large or sparse key domains: rdf_groupby_sum. */
rdf_status rdf_group_pipeline(const rdf_expr_node* nodes, int32_t nnodes, int32_t filter_root, int32_t group_root,
                              int32_t ngroups, const int32_t* value_roots, int32_t nvalues,
                              const rdf_array* cols, int32_t ncols, int64_t nchunks,
                              rdf_group_result* out, int64_t* group_rows);
/* rdf_group_pipeline / rdf_predicate over the pinned columns (same results, same errors). */
rdf_status rdf_group_pipeline_frame(const rdf_expr_node* nodes, int32_t nnodes, int32_t filter_root, int32_t group_root, int32_t ngroups,
                                    const int32_t* value_roots, int32_t nvalues, rdf_frame* frame, rdf_group_result* out,
                                    int64_t* group_rows);
rdf_status rdf_predicate_frame(const rdf_expr_node* nodes, int32_t nnodes, int32_t root, rdf_frame* frame, rdf_out* mask);

/* ------------------------------------------------------------------ multi-GPU: the exchange behind the boundary
 *
 * Where the reference panics (Transformation::GroupAggregate, src/evaluation.rs:73) and everywhere its batch loop is
 * per-chunk independent (src/evaluation.rs:66-96, src/functions/aggregate.rs:88-90), RecordBatches shard over the GPUs of a
 * node by contiguous row ranges.  A communicator is ONE RANK's end of the group: rank r runs on one GPU and is
 * driven by one host thread (one process per GPU, or one thread per GPU inside a single process — the shape a single-process
 * library like the reference needs).  Two transports, same entry points:
 *   RDF_COMM_RCCL  librccl.so (loaded on first use, never linked): ncclAllGather for the split sizes and the partial
 *                  aggregates, grouped ncclSend / ncclRecv over xGMI for the all-to-all(v) of partial groups / rows, on the
 *                  communicator's own stream, ordered against the thread's compute stream by events;
 *   RDF_COMM_PEER  single process only, no RCCL: every rank pulls its share out of the other ranks' send buffers with
 *                  hipMemcpyPeerAsync (xGMI DMA between the devices of one process).  `devices` may name one GPU several
 *                  times (ranks sharing a GPU: how the N > 1 logic is tested on a one-GPU box).
 * Every rank must make the same sequence of collective calls (rdf_comm_barrier / _allgather, rdf_agg_combine,
 * rdf_group_combine, rdf_groupby_agg_dist, rdf_groupby_agg_frame_dist) with matching arguments; an error one rank meets
 * before its exchange is carried to every rank by the exchange itself (all of them return an error, nobody waits for a
 * peer that left).  A communicator belongs to the device it was created for and is used by one thread at a time. */
typedef struct rdf_comm rdf_comm;
#define RDF_COMM_ID_BYTES 128
#define RDF_COMM_MAX_RANKS 64
typedef enum { RDF_COMM_RCCL = 0, RDF_COMM_PEER = 1 } rdf_comm_kind;

/* ncclGetUniqueId: rank 0 makes one and hands it to every rank through whatever channel the host has (a file, a socket,
 * MPI, torch's store); every rank then calls rdf_comm_init_rank on the device it selected with rdf_set_device. */
rdf_status rdf_comm_unique_id(uint8_t id[RDF_COMM_ID_BYTES]);
rdf_status rdf_comm_init_rank(int32_t world, int32_t rank, const uint8_t id[RDF_COMM_ID_BYTES], rdf_comm** out);
/* Single process: all `ndev` communicators at once (ncclCommInitAll / the peer-copy transport); out[i] is then used by the
 * thread that called rdf_set_device(devices[i]). */
rdf_status rdf_comm_init_all(int32_t ndev, const int32_t* devices, int32_t kind, rdf_comm** out);
rdf_status rdf_comm_destroy(rdf_comm* comm);
/* world size, rank, device, transport, RCCL's version code (0 for RDF_COMM_PEER); any pointer may be NULL */
rdf_status rdf_comm_info(rdf_comm* comm, int32_t* world, int32_t* rank, int32_t* device, int32_t* kind, int32_t* rccl_version);
rdf_status rdf_comm_barrier(rdf_comm* comm);
/* `bytes` of host memory from every rank, in rank order, into all_host (world * bytes); bytes <= 1 MiB. */
rdf_status rdf_comm_allgather(rdf_comm* comm, const void* mine_host, int64_t bytes, void* all_host);

/* AggregateFunctions over row-sharded batches: every rank passes the rdf_agg_result of its shard (rdf_pipeline's SINK_AGG
 * output) and gets the aggregates of the whole column back — the partials are all-gathered (world x 72 bytes per value) and
 * folded in rank order on every rank, exactly AggregateFunctions' own left fold over chunks (src/functions/aggregate.rs:82-93)
 * with ranks in place of chunks: identical bits on every rank; integer sums wrap to the value's width; NaN never displaces a
 * number in min / max. */
rdf_status rdf_agg_combine(rdf_comm* comm, rdf_agg_result* aggs, int32_t nvalues);
/* rdf_pipeline (an aggregating program, RDF_SINK_AGG) + rdf_agg_combine in ONE call over this rank's device-resident shard:
 * the shard's partial {sum, min, max, count} never visit the host — they are all-gathered (RCCL, on the communicator's stream,
 * ordered behind the kernel by an event) and folded on the device by the same fixed-order tree on every rank, and the total is
 * the first thing the host reads: one wait per step instead of two (the per-step host round trip of the pair of calls is
 * latency, the same at any number of GPUs).  An error a rank's kernel raises (a zero divisor) is returned on every rank.
 * The peer transport, and host-resident batches (which may stream), run the two calls this replaces.
 * rdf_pipeline_frame_dist: the same over a pinned frame. */
rdf_status rdf_pipeline_dist(rdf_comm* comm, const rdf_program* prog, const rdf_array* cols, int32_t ncols, int64_t nchunks,
                             rdf_agg_result* aggs);
rdf_status rdf_pipeline_frame_dist(rdf_comm* comm, const rdf_program* prog, rdf_frame* frame, rdf_agg_result* aggs);
/* The same for rdf_group_pipeline's output (small dense group domain, TPC-H Q1): out[nvalues * (ngroups + 1)] and
 * group_rows[ngroups + 1] (may be NULL) are replaced by the totals over all ranks. */
rdf_status rdf_group_combine(rdf_comm* comm, rdf_group_result* out, int64_t* group_rows, int32_t ngroups, int32_t nvalues);

typedef enum { RDF_EXCHANGE_AUTO = 0, RDF_EXCHANGE_GROUPS = 1, RDF_EXCHANGE_ROWS = 2 } rdf_exchange_mode;
/* what the last exchange of a rank moved (bench lines, tests) */
typedef struct {
    int32_t exchange;            /* RDF_EXCHANGE_GROUPS or RDF_EXCHANGE_ROWS: what travelled */
    int32_t rounds;              /* grouped send / recv rounds (every rank runs the same number) */
    int64_t local_groups;        /* partial groups of this rank before the exchange (rows, for RDF_EXCHANGE_ROWS) */
    int64_t rows_sent, rows_sent_remote, rows_received;   /* records to all owners / to other ranks / from all ranks */
    int64_t bytes_sent, bytes_sent_remote, bytes_received;
    double  exchange_ms;         /* device time from the start of the pack to the end of the unpack (hipEvents) */
} rdf_exchange_stats;

/* Transformation::GroupAggregate over row-sharded batches (replaces the panic! at src/evaluation.rs:73 for N GPUs; SURVEY.md
 * 8e): this rank's shard is aggregated locally (rdf_groupby_agg), its partial groups are bucketed by owner on the device
 * (owner = ((key * 0x9E3779B97F4A7C15) >> 33) % world, rdf_group_exchange_pack's rule), the (key, partial, count) triples
 * travel to their owners, and every rank merges what it receives (rdf_groupby_merge: sums added, minima / maxima compared,
 * counts added).  The outputs hold the groups THIS RANK OWNS — the union over the ranks is the result, no key twice.
 * RDF_EXCHANGE_ROWS shuffles the shard's rows instead (16 bytes each) and aggregates them once, at their owner: what pays
 * when pre-aggregation cannot shrink a shard (RDF_EXCHANGE_AUTO: when 2 * max_groups * world >= the rows of all ranks,
 * decided from an all-gather of the shard sizes so that every rank takes the same path; needs one chunk per column, no NULLs).
 * ONE grouping column of Int64 / UInt64 without NULLs (cast narrower keys first), device-resident inputs and outputs
 * (RDF_MEM_DEVICE); values / agg / max_groups / output types and capacities as rdf_groupby_agg (max_groups bounds the groups
 * of the whole result; capacity >= min(max_groups, rows of all ranks) + 2 is always enough).  stats may be NULL. */
rdf_status rdf_groupby_agg_dist(rdf_comm* comm, const rdf_array* keys, const rdf_array* values, int64_t nchunks, int32_t agg,
                                int64_t max_groups, int32_t exchange, rdf_out* out_keys, rdf_out* out_values, rdf_out* out_counts,
                                rdf_exchange_stats* stats);
/* The same over a pinned frame: grouping column key_col, ONE aggregation of column value_col -> a one-batch frame of the
 * groups this rank owns: (key, aggregate, count) as rdf_groupby_agg_frame's. */
rdf_status rdf_groupby_agg_frame_dist(rdf_comm* comm, rdf_frame* frame, int32_t key_col, int32_t value_col, int32_t agg,
                                      int64_t max_groups, int32_t exchange, rdf_frame** out, rdf_exchange_stats* stats);

/* ------------------------------------------------------------------ synthetic data (bench/tests) */

/* x[row] = lo + (hi-lo) * u(seed, column_id, first_row + row), u in [0,1) from a counter-based
 * SplitMix64 hash; identical on every rank/device and in the CPU oracle.  Device memory only. */
rdf_status rdf_fill_uniform_f64(double* dev_ptr, int64_t n, uint64_t seed, uint64_t column_id,
                                int64_t first_row, double lo, double hi);
/* x[row] = lo + (hash mod span), span = hi - lo (> 0). */
rdf_status rdf_fill_uniform_i64(int64_t* dev_ptr, int64_t n, uint64_t seed, uint64_t column_id,
                                int64_t first_row, int64_t lo, int64_t hi);
/* validity bit = (hash(seed, column_id, row) mod 2^32) >= null_fraction * 2^32; nbits bits written. */
rdf_status rdf_fill_validity(uint8_t* dev_ptr, int64_t nbits, uint64_t seed, uint64_t column_id,
                             int64_t first_row, double null_fraction);

/* Per-thread tunables, for tests and ablations: "spec" (1 = use the ahead-of-time specialised kernels
 * when the program shape is in the catalogs, default; 0 = always the general evaluator), "fast_filter",
 * "vec_bitmap" (accepted and ignored since round 5: the specialised kernels read bitmap words on the scalar unit only), "gb_partition" (hash GROUP BY: 3 = second
 * generation, default: LDS-table stream <= 2048 groups, line-aligned scatter + LDS tables <= 1.3 M, else one table in HBM;
 * 4 = its scatter path whatever max_groups says; 1 = rdf_groupby_sum runs on the first-generation histogram + scatter + aggregate
 * path — otherwise the fallback for heavily skewed sums / counts of one key column — where that path's range holds
 * (1024 < max_groups <= 1 331 200, at least one row), elsewhere as 3; 2 = accepted, behaves as 3 (it named the retired radix-sort
 * partitioning); 0 = one table in HBM),
 * "gb_debug" (3 = tests: rdf_groupby_sum takes that first-generation path, inside the same range, with its combining scatter
 * forced; every other value is accepted and ignored: no value changes a result),
 * "jit" (a program shape no catalog holds: 1 = the specialised kernel template is compiled for it at run time — `hipcc` as a child
 * process on a helper thread, about half a second; THIS call and the ones until it is ready are answered by the general evaluator,
 * a code object found in the cache directory is loaded at once —, default; 2 = the call waits for the compiler; 0 = always the
 * general evaluator),
 * "gb_compact" (scatter path, keys inside a window of 2^39: 1 = 4-byte records when only rows are counted, default; 2 = also
 * 12-byte records for sum / min / max; 0 = 16-byte records always), "gb_skew_plan" (1 = per-partition capacity plan when the probe finds a few heavy
 * partitions, default; 0 = the first-generation combining path instead; 2 = always),
 * "window_range_route" (rdf_window_range_agg's bounds pass: 0 = auto, 1 = the LDS key window wherever it fits — today auto's own
 * choice —, 2 = the global search for every tile; no value changes a result),
 * "take_rows" (rdf_take_frame / rdf_sort_frame: 1 = gather
 * interleaved row records when the index list is long and the frame wide, default; 0 = always column by column; 2 = always records),
 * "gb_hot" (skewed keys on the scatter path: 1 = the few dozen hash classes that hold the heavy hitters get a pass of their own — folded in
 * LDS per block — and the scatter takes the other rows, default; 0 = capacity plan / first-generation combining path),
 * "gb_bucket" (partition tables of the scatter path's aggregate pass: 0 = one key per probe for keys packed into at most 4 x max_groups
 * values — the multiplicative hash never collides there —, four keys per 32-byte bucket otherwise, default; 1 / 4 force one),
 * "filter_fused" (rdf_filter_frame with a `column CMP literal [AND | OR column CMP literal]` predicate over 4- / 8-byte columns: 1 = the
 * predicate runs inside the compaction kernel, one pass, default; 2 = the same (it forced the kernel on long batches while those took
 * three passes); 0 = predicate -> mask, count, compact),
 * "filter_block" (rdf_filter_frame's one-pass form and rdf_filter / rdf_filter_columns over device-resident chunks, on frames of equally wide 4- / 8-byte columns in LONG batches: 1 = block tiles held in registers, every tile's row count
 * published one iteration before its offset is asked for, offsets from one scanner wave, default; 0 = the wave-tile kernels),
 * "filter_block_rows" (the mean batch length from which that kernel is taken, default 8192),
 * "filter_ends" (the wave-tile one-pass kernel on frames whose batch lengths are not multiples of its 1024-row tile: 1 = the tiles at the end
 * of a batch take the LDS-DMA path too, default; 0 = they load row by row),
 * "filter_short" (the same operators on frames whose batches are no longer than one block tile — the readers' 1024-row RecordBatches,
 * chunks of a few thousand rows: 1 = the block kernel with a batch on 1 / 2 / 4 / 8 waves of one block and no prefix between blocks,
 * default; 0 = the wave-tile kernels; "filter_block" 0 switches both forms off),
 * "interp_lean" (interpreted programs — no specialised kernel, no compiler — over at most 4 columns of 8-byte types whose every step is a
 * comparison, f64 / 64-bit integer arithmetic, a Boolean connective, an integer -> f64 cast or the filter, aggregated or stored: 1 = the
 * interpreter's branch-free kernel with host-assigned step handlers (eval_lean_kernel, 1.4-2.2 x the general kernel on aggregates), default;
 * 2 = the same with one tile per trip of its step loop (the A/B of its two-tile form); 0 = eval_kernel),
 * "filter_gen", "filter_one", "filter_tile", "filter_mixed", "filter_lookback" (accepted and ignored: they selected forms of the compaction
 * kernels that were measured slower and removed — the table-driven block tiles, the two-launch form for frames of 8- and 4-byte columns, the
 * older look-back walks of the wave-tile kernel),
 * "join_table" (equi-join on one key column: 2 = the build side sorted by hash, the table of its distinct keys laid out by a scan,
 * default; 0 = a bucket index over the build keys sorted by key — what joins on several key columns, build sides of 2^31 - 1 rows or
 * more and a table whose placement overflows use in any case; 1 named the retired table with slots claimed by compare-and-swap:
 * accepted, the planner decides as under 2),
 * "sort_msd" (keys that vary in 25 bits or more: 1 = passes over the top bits, buckets finished in LDS, default; 0 = one pass per byte),
 * "sort_gen", "sort_pipe", "sort_super" (accepted and ignored: they selected forms of the digit passes that were measured slower and removed),
 * "sort_sample" (Float64 sort keys: 1 = the value buckets of those passes are planned from a sample of the keys — the range the rows lie
 * in without far outliers / infinities / NaNs, as many bucket bits as the densest region needs —, default; 0 = [min, max], ~500 rows per bucket),
 * "stream_slab_bytes" (rdf_pipeline over host memory: bytes per slab of the streamed batch loop, 0 = 256 MiB, -1 = never stream),
 * "comm_max_bytes" (most bytes one ncclSend / peer copy of the group-by exchange moves, default 256 MiB: larger shares go in
 * several rounds; every rank of a communicator must use the same value),
 * "uniques_route" (rdf_uniques / rdf_utf8_uniques: 0 = the hash route while its set holds the column's distinct values, the sort /
 * exact route otherwise, default; 1 = always the sort / exact route),
 * "uniques_table_bits" (log2 of the most slots that hash set may have, 10..32, default 24: it is filled to half, so up to 2^23
 * distinct values stay on the hash route). 
 * "member_route" (rdf_member_mask: 0 = planned, 1 = probe a copy of the table in LDS — a call it cannot serve is refused —, 2 =
 * probe the table in HBM), "member_slots" (slots of the LDS form's table, 0 = planned: tests), "member_table_bits" (log2 of the
 * most slots the table of rdf_member_mask / rdf_first_occurrence may have, 4..32, 0 = the default 30; a table that then cannot
 * hold the keys is RDF_MEMORY_ERROR). */
rdf_status rdf_set_option(const char* name, int64_t value);
/* Number of program shapes with a specialised kernel. */
int32_t    rdf_spec_catalog_size(void);
/* One line about the run-time compiler of shapes outside the catalogs: whether `hipcc` and the kernel sources were found (and
 * where), the code-object cache directory ($RDF_JIT_CACHE, else $XDG_CACHE_HOME/rdf_mi355x/jit, else ~/.cache/rdf_mi355x/jit;
 * RDF_JIT_CACHE=off disables it), and how many kernels were compiled / read from the cache / failed / are being compiled.
 * Without a compiler such programs run on the interpreter (same results; 1.4-2.5 x slower on its lean kernel's class, 3-20 x otherwise) unless the cache holds them. */
const char* rdf_jit_status(void);
/* Name of the dominant kernel the last rdf_pipeline-family call of this thread launched.
 *
 * After rdf_sort_to_indices / rdf_sort_frame over numeric criteria the name is "os_scatter_kernel", or
 * "os_scatter_kernel+os_local_kernel" when at least one column was finished by the LDS bucket sort, followed by a route note
 * " (sort routes: <entry>; <entry>; ...)" with one entry per numeric column in the order the columns were SORTED (the last
 * criterion first).  An entry is one of
 *   none                                                            nothing varies and no row is NULL: no pass
 *   bytes passes=P nulls=N                                          P passes over the low bytes of (key - min)
 *   top+lds B=b top=t map=M nulls=N bucket=L lds=C                  t stable passes over the top b bits, then every bucket
 *                                                                   sorted in LDS; C = the largest LDS class launched (rows:
 *                                                                   the power of two >= L, at least 256)
 *   top+bytes B=b top=t map=M bucket=L then passes=P nulls=N        the top passes ran, a bucket of L > 4096 rows turned up,
 *                                                                   the byte passes sorted the column (the late fall-back)
 *   crowded+bytes B=b top=t map=M digit=D then passes=P nulls=N     D rows share their top digit, more than the buckets
 *                                                                   under it could hold: byte passes before any top pass
 *                                                                   (the early fall-back)
 * M names where the top bits come from: bits (the key's own bits), linear (Float64 value buckets over [min, max]:
 * "sort_sample" 0), flat or segments (Float64 value buckets planned from a sample of the keys: one linear map between the
 * tails, or shares per segment).  N is 1 when a NULLs-last pass ran.  L is the largest bucket the boundary search found.
 * The words before the note keep their meaning: "os_local_kernel" appears iff some entry is top+lds. */
const char* rdf_last_kernel(void);

/* Average duration (ms) and launch count of the dominant kernel launched by this thread since the
 * last reset, from hipEvents recorded on the stream the kernels run on (bench.py's roofline leg). */
rdf_status rdf_kernel_timing_reset(int32_t enable);
rdf_status rdf_kernel_timing_get(double* total_ms, int64_t* launches);

/* Measurement helper, not an operator: what BARE streaming kernels reach on this device, GB/s of bytes moved — kind 0: read `bytes`
 * of a (xor fold, the cheapest consumer), 1: copy a -> b, 2: a, b -> c (two reads, one write).  Several loop shapes and grids are
 * timed with HIP events on the library's stream, `reps` launches each after one warm-up; the best is returned with its description
 * in `shape` (may be NULL).  These are the denominators bench.py's `roofline.peak_measured` and DESIGN.md's memory model use; the
 * reference has no counterpart (its benches time kernels on the CPU, src/functions/scalar.rs:621-671). */
rdf_status rdf_probe_stream(int32_t kind, const void* a, void* b, void* c, int64_t bytes, int32_t reps, double* best_gbps, char* shape, int32_t shape_len);

#ifdef __cplusplus
}
#endif
#endif /* RDF_MI355X_H */
