//! rdf_shim.rs — the binding a rust-dataframe maintainer would add (e.g. as `src/gpu/mod.rs`) to run the Arrow compute
//! hot path on an MI355X through `librdf_mi355x.so` (C ABI: `include/rdf_mi355x.h`).
//!
//! SOURCE ONLY: the build image has no Rust toolchain, so this file is neither compiled nor tested here.  The same ABI is
//! exercised end to end from C (`tests/test_abi.py` compiles the header with gcc and checks every export), from C++
//! (`include/rdf_frame.hpp`, `tests/cpp/`) and from Python / ctypes (`rust_dataframe_amd/_abi.py`).  Written against the
//! reference's pinned-era `arrow` crate (no `arrow::ffi`): raw buffer pointers are passed.
//!
//! Layout: (1) `sys` — the declarations, one per export of the header; (2) views over Arrow arrays and output buffers;
//! (3) replacement bodies with the reference's own signatures for the functions of SURVEY.md section 8b.
#![allow(non_camel_case_types, dead_code)]

pub mod sys {
    use std::os::raw::{c_char, c_void};

    // rdf_dtype / rdf_mem / rdf_status (include/rdf_mi355x.h)
    pub const RDF_I8: i32 = 0;  pub const RDF_I16: i32 = 1; pub const RDF_I32: i32 = 2;  pub const RDF_I64: i32 = 3;
    pub const RDF_U8: i32 = 4;  pub const RDF_U16: i32 = 5; pub const RDF_U32: i32 = 6;  pub const RDF_U64: i32 = 7;
    pub const RDF_F32: i32 = 8; pub const RDF_F64: i32 = 9; pub const RDF_BOOL: i32 = 10; pub const RDF_NULLTYPE: i32 = 11;
    pub const RDF_MEM_HOST: i32 = 0; pub const RDF_MEM_DEVICE: i32 = 1;
    pub const RDF_OK: i32 = 0; pub const RDF_COMPUTE_ERROR: i32 = 1; pub const RDF_DIVIDE_BY_ZERO: i32 = 2;
    pub const RDF_INVALID_ARGUMENT: i32 = 3; pub const RDF_MEMORY_ERROR: i32 = 4; pub const RDF_DEVICE_ERROR: i32 = 5;
    // rdf_op
    pub const RDF_OP_ADD: i32 = 1; pub const RDF_OP_SUB: i32 = 2; pub const RDF_OP_MUL: i32 = 3; pub const RDF_OP_DIV: i32 = 4;
    pub const RDF_OP_ATAN2: i32 = 5; pub const RDF_OP_HYPOT: i32 = 6; pub const RDF_OP_LOG: i32 = 7;
    pub const RDF_OP_ABS: i32 = 8; pub const RDF_OP_ACOS: i32 = 9; pub const RDF_OP_ASIN: i32 = 10; pub const RDF_OP_ATAN: i32 = 11;
    pub const RDF_OP_CBRT: i32 = 12; pub const RDF_OP_CEIL: i32 = 13; pub const RDF_OP_COS: i32 = 14; pub const RDF_OP_COSH: i32 = 15;
    pub const RDF_OP_DEGREES: i32 = 16; pub const RDF_OP_EXP: i32 = 17; pub const RDF_OP_EXPM1: i32 = 18; pub const RDF_OP_FLOOR: i32 = 19;
    pub const RDF_OP_LOG10: i32 = 20; pub const RDF_OP_LOG2: i32 = 21; pub const RDF_OP_RADIANS: i32 = 22; pub const RDF_OP_ROUND: i32 = 23;
    pub const RDF_OP_SIN: i32 = 24; pub const RDF_OP_SINH: i32 = 25; pub const RDF_OP_SQRT: i32 = 26; pub const RDF_OP_TAN: i32 = 27;
    pub const RDF_OP_TANH: i32 = 28; pub const RDF_OP_CAST: i32 = 29;
    pub const RDF_OP_GT: i32 = 30; pub const RDF_OP_GE: i32 = 31; pub const RDF_OP_EQ: i32 = 32; pub const RDF_OP_NE: i32 = 33;
    pub const RDF_OP_LT: i32 = 34; pub const RDF_OP_LE: i32 = 35; pub const RDF_OP_NOT: i32 = 36; pub const RDF_OP_AND: i32 = 37; pub const RDF_OP_OR: i32 = 38;
    pub const RDF_OP_HOUR_S: i32 = 39; pub const RDF_OP_HOUR_MS: i32 = 40; pub const RDF_OP_HOUR_US: i32 = 41; pub const RDF_OP_HOUR_NS: i32 = 42; pub const RDF_OP_HOUR_DAY: i32 = 43;
    pub const RDF_OP_COT: i32 = 44; pub const RDF_OP_SEC: i32 = 45; pub const RDF_OP_CSC: i32 = 46;
    pub const RDF_NODE_COLUMN: i32 = 0; pub const RDF_NODE_SCALAR: i32 = 1; pub const RDF_NODE_OP: i32 = 2;
    pub const RDF_SINK_STORE: i32 = 0; pub const RDF_SINK_AGG: i32 = 1;
    pub const RDF_JOIN_LEFT: i32 = 0; pub const RDF_JOIN_RIGHT: i32 = 1; pub const RDF_JOIN_INNER: i32 = 2; pub const RDF_JOIN_FULL: i32 = 3;
    pub const RDF_AGG_SUM: i32 = 0; pub const RDF_AGG_MIN: i32 = 1; pub const RDF_AGG_MAX: i32 = 2; pub const RDF_AGG_COUNT: i32 = 3;
    pub const RDF_MAX_VALUES: usize = 4; pub const RDF_MAX_GROUP_KEYS: usize = 4;

    #[repr(C)] #[derive(Clone, Copy)]
    pub struct rdf_array { pub values: *const c_void, pub validity: *const u8, pub offset: i64, pub length: i64,
                           pub null_count: i64, pub dtype: i32, pub mem: i32 }
    #[repr(C)] #[derive(Clone, Copy)]
    pub struct rdf_out { pub values: *mut c_void, pub validity: *mut u8, pub capacity: i64, pub length: i64,
                         pub null_count: i64, pub dtype: i32, pub mem: i32 }
    #[repr(C)] #[derive(Clone, Copy)]
    pub struct rdf_expr_node { pub kind: i32, pub op: i32, pub dtype: i32, pub lhs: i32, pub rhs: i32, pub column: i32,
                               pub f64_: f64, pub i64_: i64 }
    #[repr(C)] pub struct rdf_program { pub nodes: *const rdf_expr_node, pub nnodes: i32, pub filter_root: i32, pub nvalues: i32,
                                        pub value_roots: [i32; RDF_MAX_VALUES], pub sink: i32 }
    #[repr(C)] #[derive(Clone, Copy, Default)]
    pub struct rdf_agg_result { pub sum_f64: f64, pub min_f64: f64, pub max_f64: f64, pub sum_i64: i64, pub min_i64: i64,
                                pub max_i64: i64, pub count: i64, pub is_some: i32, pub dtype: i32 }
    #[repr(C)] #[derive(Clone, Copy, Default)]
    pub struct rdf_group_result { pub sum_f64: f64, pub sum_i64: i64, pub count: i64, pub is_some: i32, pub dtype: i32 }
    #[repr(C)] #[derive(Clone, Copy)] pub struct rdf_sort_options { pub descending: i32, pub nulls_first: i32 }
    #[repr(C)] #[derive(Clone, Copy)] pub struct rdf_list_array { pub offsets: rdf_array, pub values: rdf_array }
    #[repr(C)] #[derive(Clone, Copy)] pub struct rdf_utf8_array { pub offsets: rdf_array, pub data: rdf_array }
    // one part of rdf_utf8_concat: exactly one of utf8 (nchunks chunks) / literal (literal_bytes bytes) is set
    #[repr(C)] #[derive(Clone, Copy)]
    pub struct rdf_utf8_part { pub utf8: *const rdf_utf8_array, pub literal: *const u8, pub literal_bytes: i64 }
    pub const RDF_UTF8_PARTS_MAX: i32 = 8;
    // what rdf_utf8_regexp_info reports of a compiled pattern: the counts the size caps are defined on
    #[repr(C)] #[derive(Clone, Copy)]
    pub struct rdf_regexp_info { pub program_len: i32, pub forward_states: i32, pub reverse_states: i32, pub classes: i32,
                                 pub table_bytes: i64, pub can_match_empty: i32, pub anchored_start: i32 }
    // one criterion of rdf_lexsort_to_indices: exactly one of values / utf8 points at nchunks chunks
    #[repr(C)] #[derive(Clone, Copy)]
    pub struct rdf_sort_key { pub values: *const rdf_array, pub utf8: *const rdf_utf8_array, pub options: rdf_sort_options }
    // one key column of rdf_groupby_agg_keys' result: `values` for a numeric key, the (utf8_offsets, utf8_data) pair for a Utf8 one
    #[repr(C)] #[derive(Clone, Copy)]
    pub struct rdf_key_out { pub values: *mut rdf_out, pub utf8_offsets: *mut rdf_out, pub utf8_data: *mut rdf_out }
    // one call of rdf_groupby_multi: agg = RDF_AGG_*, value = index into `values` (-1: COUNT of the group's rows)
    #[repr(C)] #[derive(Clone, Copy)] pub struct rdf_multi_agg_call { pub agg: i32, pub value: i32 }
    // one call of rdf_window: fn = RDF_WIN_*, param = ntile buckets / lag, lead offset
    #[repr(C)] #[derive(Clone, Copy)] pub struct rdf_window_call { pub fn_: i32, pub pad: i32, pub param: i64 }
    pub const RDF_WIN_ROW_NUMBER: i32 = 0; pub const RDF_WIN_RANK: i32 = 1; pub const RDF_WIN_DENSE_RANK: i32 = 2;
    pub const RDF_WIN_PERCENT_RANK: i32 = 3; pub const RDF_WIN_CUME_DIST: i32 = 4; pub const RDF_WIN_NTILE: i32 = 5;
    pub const RDF_WIN_LAG: i32 = 6; pub const RDF_WIN_LEAD: i32 = 7;
    // one call of rdf_window_agg: fn = RDF_WAGG_*, value = index into `values` (-1: COUNT of rows, FIRST / LAST_VALUE), its frame
    #[repr(C)] #[derive(Clone, Copy)]
    pub struct rdf_window_frame { pub unit: i32, pub start_kind: i32, pub end_kind: i32, pub pad: i32, pub start: i64, pub end: i64 }
    #[repr(C)] #[derive(Clone, Copy)] pub struct rdf_window_agg_call { pub fn_: i32, pub value: i32, pub frame: rdf_window_frame }
    // one call of rdf_window_range_agg: a RANGE frame whose offsets are in the order key's units (start_i / end_i for Int32 / Int64
    // keys, start_f / end_f for Float64 keys; read for RDF_BOUND_PRECEDING / RDF_BOUND_FOLLOWING only)
    #[repr(C)] #[derive(Clone, Copy)]
    pub struct rdf_window_range_frame { pub start_kind: i32, pub end_kind: i32, pub start_i: i64, pub end_i: i64, pub start_f: f64, pub end_f: f64 }
    #[repr(C)] #[derive(Clone, Copy)] pub struct rdf_window_range_call { pub fn_: i32, pub value: i32, pub frame: rdf_window_range_frame }
    pub const RDF_FRAME_ROWS: i32 = 0; pub const RDF_FRAME_RANGE: i32 = 1;
    pub const RDF_BOUND_UNBOUNDED_PRECEDING: i32 = 0; pub const RDF_BOUND_PRECEDING: i32 = 1; pub const RDF_BOUND_CURRENT_ROW: i32 = 2;
    pub const RDF_BOUND_FOLLOWING: i32 = 3; pub const RDF_BOUND_UNBOUNDED_FOLLOWING: i32 = 4;
    pub const RDF_WAGG_SUM: i32 = 0; pub const RDF_WAGG_MIN: i32 = 1; pub const RDF_WAGG_MAX: i32 = 2; pub const RDF_WAGG_COUNT: i32 = 3;
    pub const RDF_WAGG_AVG: i32 = 4; pub const RDF_WAGG_FIRST_VALUE: i32 = 5; pub const RDF_WAGG_LAST_VALUE: i32 = 6;
    // one call of rdf_groupby_sorted: fn = RDF_GRP_*, ignore_nulls read by FIRST / LAST
    #[repr(C)] #[derive(Clone, Copy)] pub struct rdf_group_call { pub fn_: i32, pub ignore_nulls: i32 }
    pub const RDF_GRP_COUNT_DISTINCT: i32 = 0; pub const RDF_GRP_SUM_DISTINCT: i32 = 1; pub const RDF_GRP_FIRST: i32 = 2; pub const RDF_GRP_LAST: i32 = 3;
    pub const RDF_GROUP_MAX_CALLS: i32 = 8;
    // one call of rdf_groupby_moments: stat = RDF_STAT_* without y, RDF_COSTAT_* with y
    #[repr(C)] #[derive(Clone, Copy)] pub struct rdf_group_stat_call { pub stat: i32, pub reserved: i32 }
    pub const RDF_GROUP_MOMENTS_MAX_CALLS: i32 = 8; pub const RDF_GROUP_MOMENTS_TILE: i32 = 256;
    // one call of rdf_groupby_percentile: kind = RDF_PCT_*, p in [0, 1]; the median is { RDF_PCT_CONT, 0, 0.5 }
    #[repr(C)] #[derive(Clone, Copy)] pub struct rdf_percentile_call { pub kind: i32, pub reserved: i32, pub p: f64 }
    pub const RDF_PCT_CONT: i32 = 0; pub const RDF_PCT_DISC: i32 = 1; pub const RDF_PERCENTILE_MAX_CALLS: i32 = 8;
    // rdf_groupby_collect's kind, and the tile of its compaction / of explode's expansion
    pub const RDF_COLLECT_LIST: i32 = 0; pub const RDF_COLLECT_SET: i32 = 1; pub const RDF_COLLECT_TILE: i32 = 1024;
    // the state of rdf_moments / rdf_comoments: count, the mean(s) as two doubles each, the central sums
    #[repr(C)] #[derive(Clone, Copy, Default)]
    pub struct rdf_moments_state { pub count: i64, pub mean: f64, pub mean_lo: f64, pub m2: f64, pub m3: f64, pub m4: f64 }
    #[repr(C)] #[derive(Clone, Copy, Default)]
    pub struct rdf_comoments_state { pub count: i64, pub mean_x: f64, pub mean_x_lo: f64, pub mean_y: f64, pub mean_y_lo: f64,
                                     pub m2x: f64, pub m2y: f64, pub cxy: f64 }
    pub const RDF_STAT_MEAN: i32 = 0; pub const RDF_STAT_VAR_POP: i32 = 1; pub const RDF_STAT_VAR_SAMP: i32 = 2; pub const RDF_STAT_STDDEV_POP: i32 = 3;
    pub const RDF_STAT_STDDEV_SAMP: i32 = 4; pub const RDF_STAT_SKEWNESS: i32 = 5; pub const RDF_STAT_KURTOSIS: i32 = 6;
    pub const RDF_COSTAT_COVAR_POP: i32 = 0; pub const RDF_COSTAT_COVAR_SAMP: i32 = 1; pub const RDF_COSTAT_CORR: i32 = 2;
    #[repr(C)] #[derive(Clone, Copy)]
    pub struct rdf_value_part { pub column: *const rdf_array, pub literal_bits: u64, pub literal_is_null: i32 }   // column == null: a literal
    pub const RDF_IS_NULL: i32 = 0; pub const RDF_IS_NOT_NULL: i32 = 1; pub const RDF_IS_NAN: i32 = 2;
    pub const RDF_SELECT_PARTS_MAX: i32 = 8;
    #[repr(C)] pub struct rdf_frame { _opaque: [u8; 0] }
    #[repr(C)] pub struct rdf_comm { _opaque: [u8; 0] }
    #[repr(C)] #[derive(Clone, Copy, Default)]
    pub struct rdf_exchange_stats { pub exchange: i32, pub rounds: i32, pub local_groups: i64, pub rows_sent: i64, pub rows_sent_remote: i64,
                                    pub rows_received: i64, pub bytes_sent: i64, pub bytes_sent_remote: i64, pub bytes_received: i64, pub exchange_ms: f64 }
    pub const RDF_COMM_RCCL: i32 = 0; pub const RDF_COMM_PEER: i32 = 1;
    pub const RDF_EXCHANGE_AUTO: i32 = 0; pub const RDF_EXCHANGE_GROUPS: i32 = 1; pub const RDF_EXCHANGE_ROWS: i32 = 2;

    #[link(name = "rdf_mi355x")]
    extern "C" {
        // plumbing
        pub fn rdf_version() -> *const c_char;
        pub fn rdf_last_error() -> *const c_char;
        pub fn rdf_device_count(count: *mut i32) -> i32;
        pub fn rdf_set_device(device: i32) -> i32;
        pub fn rdf_set_stream(hip_stream: *mut c_void) -> i32;
        pub fn rdf_synchronize() -> i32;
        pub fn rdf_dev_alloc(ptr: *mut *mut c_void, bytes: i64) -> i32;
        pub fn rdf_dev_free(ptr: *mut c_void) -> i32;
        pub fn rdf_copy_h2d(dst_dev: *mut c_void, src_host: *const c_void, bytes: i64) -> i32;
        pub fn rdf_copy_d2h(dst_host: *mut c_void, src_dev: *const c_void, bytes: i64) -> i32;
        // ScalarFunctions (src/functions/scalar.rs)
        pub fn rdf_binary(op: i32, a: *const rdf_array, b: *const rdf_array, nchunks: i64, out: *mut rdf_out) -> i32;
        pub fn rdf_unary(op: i32, a: *const rdf_array, nchunks: i64, out: *mut rdf_out) -> i32;
        pub fn rdf_cast(a: *const rdf_array, nchunks: i64, out: *mut rdf_out) -> i32;
        pub fn rdf_hour(a: *const rdf_array, nchunks: i64, unit: i32, out: *mut rdf_out) -> i32;
        // year .. date_diff (scalar.rs declares them with empty bodies): Spark 3's semantics, see rdf_mi355x.h.  fields: rdf_datetime_field
        // codes (0 = year .. 10 = date), level: rdf_trunc_level (0 = year .. 7 = second), op: rdf_date_shift_op (0 = days .. 3 = next_day)
        pub fn rdf_datetime_fields(a: *const rdf_array, nchunks: i64, unit: i32, fields: *const i32, nfields: i32, outs: *mut rdf_out) -> i32;
        pub fn rdf_datetime_trunc(a: *const rdf_array, nchunks: i64, unit: i32, level: i32, out: *mut rdf_out) -> i32;
        pub fn rdf_date_shift(a: *const rdf_array, nchunks: i64, unit: i32, op: i32, amounts: *const rdf_array, amount: i32, out: *mut rdf_out) -> i32;
        pub fn rdf_date_diff(end: *const rdf_array, end_unit: i32, start: *const rdf_array, start_unit: i32, nchunks: i64, out: *mut rdf_out) -> i32;
        // coalesce / greatest / least / nanv1 / when (scalar.rs declares them with empty bodies) and is_null / is_not_null / isnan as masks:
        // Spark 3's semantics, see rdf_mi355x.h.  A value part is a column's chunks or a literal (its bits in the call's dtype, or NULL); all
        // parts and the output share one numeric dtype; op: rdf_null_test_op (0 = is_null, 1 = is_not_null, 2 = is_nan); conds[k]: nchunks
        // Boolean chunks; otherwise may be null (NULL).  Outputs need a bitmap unless some part can never be NULL (see the header).
        pub fn rdf_null_test(op: i32, a: *const rdf_array, nchunks: i64, mask: *mut rdf_out) -> i32;
        pub fn rdf_coalesce(parts: *const rdf_value_part, nparts: i32, nchunks: i64, out: *mut rdf_out) -> i32;
        pub fn rdf_case_when(conds: *const *const rdf_array, values: *const rdf_value_part, nbranches: i32, otherwise: *const rdf_value_part,
                             nchunks: i64, out: *mut rdf_out) -> i32;
        pub fn rdf_extremum(greatest: i32, parts: *const rdf_value_part, nparts: i32, nchunks: i64, out: *mut rdf_out) -> i32;
        pub fn rdf_nanvl(a: *const rdf_value_part, b: *const rdf_value_part, nchunks: i64, out: *mut rdf_out) -> i32;
        // coalesce / when over StringArrays: rdf_utf8_part as in rdf_utf8_concat, but a part with neither pointer set is the NULL literal;
        // outputs under the sizing rule of rdf_utf8_trim (call once with data capacity 0, then with the lengths reported)
        pub fn rdf_utf8_coalesce(parts: *const rdf_utf8_part, nparts: i32, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_case_when(conds: *const *const rdf_array, values: *const rdf_utf8_part, nbranches: i32, otherwise: *const rdf_utf8_part,
                                  nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        // AggregateFunctions (src/functions/aggregate.rs)
        pub fn rdf_sum(a: *const rdf_array, nchunks: i64, out_scalar: *mut c_void, out_is_some: *mut i32) -> i32;
        pub fn rdf_min(a: *const rdf_array, nchunks: i64, out_scalar: *mut c_void, out_is_some: *mut i32) -> i32;
        pub fn rdf_max(a: *const rdf_array, nchunks: i64, out_scalar: *mut c_void, out_is_some: *mut i32) -> i32;
        pub fn rdf_count(a: *const rdf_array, nchunks: i64, out_count: *mut i64, out_is_some: *mut i32) -> i32;
        pub fn rdf_avg(a: *const rdf_array, nchunks: i64, out_mean: *mut f64, out_is_some: *mut i32) -> i32;
        // variance / stddev / skewness / kurtosis (aggregate.rs:94-102) and corr (scalar.rs:184): one pass -> a state, statistics off the state
        pub fn rdf_moments(a: *const rdf_array, mask: *const rdf_array, nchunks: i64, out: *mut rdf_moments_state) -> i32;
        pub fn rdf_comoments(x: *const rdf_array, y: *const rdf_array, mask: *const rdf_array, nchunks: i64, out: *mut rdf_comoments_state) -> i32;
        pub fn rdf_moments_merge(into: *mut rdf_moments_state, other: *const rdf_moments_state) -> i32;
        pub fn rdf_comoments_merge(into: *mut rdf_comoments_state, other: *const rdf_comoments_state) -> i32;
        pub fn rdf_moments_stat(s: *const rdf_moments_state, stat: i32, out: *mut f64, out_is_some: *mut i32) -> i32;
        pub fn rdf_comoments_stat(s: *const rdf_comoments_state, stat: i32, out: *mut f64, out_is_some: *mut i32) -> i32;
        // BooleanFilter / filter / take (src/expression.rs:766-861, src/table.rs:97-107,213-241)
        pub fn rdf_predicate(nodes: *const rdf_expr_node, nnodes: i32, root: i32, cols: *const rdf_array, ncols: i32,
                             nchunks: i64, mask: *mut rdf_out) -> i32;
        pub fn rdf_filter_count(mask: *const rdf_array, nchunks: i64, counts: *mut i64) -> i32;
        pub fn rdf_filter(col: *const rdf_array, mask: *const rdf_array, nchunks: i64, out: *mut rdf_out) -> i32;
        pub fn rdf_filter_columns(cols: *const rdf_array, ncols: i32, mask: *const rdf_array, nchunks: i64, outs: *mut rdf_out) -> i32;
        // DataFrame::filter over host-resident batches in one streamed call (src/dataframe.rs:178-189)
        pub fn rdf_filter_pipeline(nodes: *const rdf_expr_node, nnodes: i32, root: i32, cols: *const rdf_array, ncols: i32,
                                   nchunks: i64, outs: *mut rdf_out) -> i32;
        pub fn rdf_take(chunks: *const rdf_array, nchunks: i64, indices: *const rdf_array, out: *mut rdf_out) -> i32;
        // sort / join (src/dataframe.rs:194-222, src/functions/join.rs:19-137)
        pub fn rdf_sort_to_indices(cols: *const rdf_array, ncols: i32, nchunks: i64, opts: *const rdf_sort_options,
                                   out_indices: *mut rdf_out) -> i32;
        // DataFrame::sort whose criteria may be StringArray columns (byte order, NULLs last, stable)
        pub fn rdf_lexsort_to_indices(keys: *const rdf_sort_key, nkeys: i32, nchunks: i64, out_indices: *mut rdf_out) -> i32;
        pub fn rdf_hist(chunks: *const rdf_array, nchunks: i64, nbins: i64, range: *const f64, out_counts: *mut rdf_out,
                        out_edges: *mut rdf_out, out_counted: *mut i64) -> i32;
        pub fn rdf_uniques(chunks: *const rdf_array, nchunks: i64, out_values: *mut rdf_out, out_count: *mut i64) -> i32;
        pub fn rdf_utf8_uniques(chunks: *const rdf_utf8_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out,
                                out_count: *mut i64) -> i32;
        // text keys: dictionary codes in first-occurrence order, GROUP BY and join whose keys may be StringArray columns
        pub fn rdf_utf8_dictionary_encode(chunks: *const rdf_utf8_array, nchunks: i64, out_codes: *mut rdf_out,
                                          out_dict_offsets: *mut rdf_out, out_dict_data: *mut rdf_out, out_count: *mut i64) -> i32;
        pub fn rdf_groupby_agg_keys(keys: *const rdf_sort_key, nkeys: i32, values: *const rdf_array, nchunks: i64, agg: i32,
                                    max_groups: i64, out_keys: *mut rdf_key_out, out_values: *mut rdf_out, out_counts: *mut rdf_out) -> i32;
        pub fn rdf_equijoin_indices_keys(left_keys: *const rdf_sort_key, left_nchunks: i64, right_keys: *const rdf_sort_key,
                                         right_nchunks: i64, nkeys: i32, join_type: i32, out_left: *mut rdf_out,
                                         out_right: *mut rdf_out, out_rows: *mut i64) -> i32;
        // LEFT SEMI / LEFT ANTI / x IN (..) and distinct rows as one RDF_BOOL mask per chunk (kind: 0 semi, 1 anti, 2 is_in;
        // keep: 0 first, 1 last, 2 none); out_mask NULL = count only
        pub fn rdf_member_mask(left_keys: *const rdf_sort_key, left_nchunks: i64, right_keys: *const rdf_sort_key,
                               right_nchunks: i64, nkeys: i32, kind: i32, out_mask: *mut rdf_out, out_rows: *mut i64) -> i32;
        pub fn rdf_first_occurrence(keys: *const rdf_sort_key, nkeys: i32, nchunks: i64, keep: i32, out_mask: *mut rdf_out,
                                    out_rows: *mut i64) -> i32;
        // several aggregates of one GROUP BY from one pass over the keys; row g of every output is one group
        pub fn rdf_groupby_multi(keys: *const rdf_sort_key, nkeys: i32, values: *const *const rdf_array, nvalues: i32, nchunks: i64,
                                 calls: *const rdf_multi_agg_call, ncalls: i32, max_groups: i64, out_keys: *mut rdf_key_out,
                                 outs: *mut rdf_out, out_counts: *mut rdf_out, out_group_rows: *mut rdf_out, out_groups: *mut i64) -> i32;
        pub fn rdf_groupby_multi_capacity(ncalls: i32) -> i64;
        // AggregateFunctions::count_distinct / sum_distinct / first / last (aggregate.rs, declared with empty bodies) per group
        pub fn rdf_groupby_sorted(group_by: *const rdf_sort_key, ngroup: i32, value: *const rdf_sort_key, nchunks: i64,
                                  calls: *const rdf_group_call, ncalls: i32, out_group_rows: *mut rdf_out, outs: *mut rdf_out,
                                  out_groups: *mut i64) -> i32;
        // AggregateFunction::Variance / StdDev / Skewness / Kurtosis (and covar / corr) per group: one moment state per group
        pub fn rdf_groupby_moments(group_by: *const rdf_sort_key, ngroup: i32, x: *const rdf_array, y: *const rdf_array, nchunks: i64,
                                   calls: *const rdf_group_stat_call, ncalls: i32, out_group_rows: *mut rdf_out, outs: *mut rdf_out,
                                   out_counts: *mut rdf_out, out_states: *mut c_void, states_capacity: i64, out_groups: *mut i64) -> i32;
        // percentile / median / percentile_disc per group (Spark's aggregates; aggregate.rs stops before them)
        pub fn rdf_groupby_percentile(group_by: *const rdf_sort_key, ngroup: i32, value: *const rdf_sort_key, nchunks: i64,
                                      calls: *const rdf_percentile_call, ncalls: i32, out_group_rows: *mut rdf_out, outs: *mut rdf_out,
                                      out_counts: *mut rdf_out, out_groups: *mut i64) -> i32;
        // ArrayFunction::CollectList / CollectSet (expression.rs:691-692; collect_list() / collect_set(), array.rs:404-405) per group,
        // and ScalarFunctions::explode (scalar.rs:237): all declared with empty bodies
        pub fn rdf_groupby_collect(group_by: *const rdf_sort_key, ngroup: i32, value: *const rdf_sort_key, nchunks: i64, kind: i32,
                                   out_group_rows: *mut rdf_out, out_offsets: *mut rdf_out, out_child_rows: *mut rdf_out,
                                   out_values: *mut rdf_out, out_groups: *mut i64, out_elements: *mut i64) -> i32;
        pub fn rdf_list_explode(list: *const rdf_list_array, outer: i32, out_parent_rows: *mut rdf_out, out_child_index: *mut rdf_out,
                                out_pos: *mut rdf_out, out_rows: *mut i64) -> i32;
        // WindowSpec / WindowFunctions (src/window.rs, src/functions/window.rs: declared, bodies empty) + ntile (scalar.rs:345)
        pub fn rdf_window(partition_by: *const rdf_sort_key, npartition: i32, order_by: *const rdf_sort_key, norder: i32,
                          nchunks: i64, nrows_if_no_keys: i64, calls: *const rdf_window_call, ncalls: i32, outs: *mut rdf_out) -> i32;
        // WindowSpec::rows_between / range_between (src/window.rs) + AggregateFunctions over the frame
        pub fn rdf_window_agg(partition_by: *const rdf_sort_key, npartition: i32, order_by: *const rdf_sort_key, norder: i32,
                              values: *const *const rdf_array, nvalues: i32, nchunks: i64, nrows_if_no_keys: i64,
                              calls: *const rdf_window_agg_call, ncalls: i32, outs: *mut rdf_out) -> i32;
        // RANGE BETWEEN s PRECEDING AND e FOLLOWING over one Int32 / Int64 / Float64 order key (Spark's rangeBetween)
        pub fn rdf_window_range_agg(partition_by: *const rdf_sort_key, npartition: i32, order_by: *const rdf_sort_key, norder: i32,
                                    values: *const *const rdf_array, nvalues: i32, nchunks: i64,
                                    calls: *const rdf_window_range_call, ncalls: i32, outs: *mut rdf_out) -> i32;
        pub fn rdf_equijoin_indices(left_keys: *const rdf_array, left_nchunks: i64, right_keys: *const rdf_array, right_nchunks: i64,
                                    join_type: i32, out_left: *mut rdf_out, out_right: *mut rdf_out, out_rows: *mut i64) -> i32;
        pub fn rdf_equijoin_indices_multi(left_keys: *const rdf_array, left_nchunks: i64, right_keys: *const rdf_array,
                                          right_nchunks: i64, nkeys: i32, join_type: i32, out_left: *mut rdf_out,
                                          out_right: *mut rdf_out, out_rows: *mut i64) -> i32;
        // Transformation::GroupAggregate (planned by Dataset::try_aggregate, src/expression.rs:114-221; evaluation.rs:73 panics)
        pub fn rdf_groupby_sum(keys: *const rdf_array, values: *const rdf_array, nchunks: i64, max_groups: i64,
                               out_keys: *mut rdf_out, out_sums: *mut rdf_out, out_counts: *mut rdf_out) -> i32;
        pub fn rdf_groupby_agg(keys: *const rdf_array, nkeys: i32, values: *const rdf_array, nchunks: i64, agg: i32, max_groups: i64,
                               out_keys: *mut rdf_out, out_values: *mut rdf_out, out_counts: *mut rdf_out) -> i32;
        pub fn rdf_groupby_merge(keys: *const rdf_array, partial: *const rdf_array, counts: *const rdf_array, agg: i32, max_groups: i64,
                                 out_keys: *mut rdf_out, out_values: *mut rdf_out, out_counts: *mut rdf_out) -> i32;
        pub fn rdf_group_exchange_pack(keys: *const rdf_array, partial: *const rdf_array, counts: *const rdf_array, world: i32,
                                       packed_dev: *mut c_void, owner_counts: *mut i64) -> i32;
        pub fn rdf_group_exchange_unpack(packed_dev: *const c_void, n: i64, keys: *mut rdf_out, partial: *mut rdf_out,
                                         counts: *mut rdf_out) -> i32;
        pub fn rdf_row_exchange_pack(keys: *const rdf_array, values: *const rdf_array, world: i32, packed_dev: *mut c_void,
                                     owner_counts: *mut i64) -> i32;
        pub fn rdf_row_exchange_unpack(packed_dev: *const c_void, n: i64, keys: *mut rdf_out, values: *mut rdf_out) -> i32;
        // several GPUs: the communicator and every collective of the path live behind the boundary —
        // the library loads RCCL itself; Evaluate::evaluate's GroupAggregate arm (src/evaluation.rs:73) calls rdf_groupby_agg_dist
        pub fn rdf_comm_unique_id(id: *mut u8) -> i32;                                   // 128 bytes (ncclUniqueId)
        pub fn rdf_comm_init_rank(world: i32, rank: i32, id: *const u8, out: *mut *mut rdf_comm) -> i32;
        pub fn rdf_comm_init_all(ndev: i32, devices: *const i32, kind: i32, out: *mut *mut rdf_comm) -> i32;
        pub fn rdf_comm_destroy(comm: *mut rdf_comm) -> i32;
        pub fn rdf_comm_info(comm: *mut rdf_comm, world: *mut i32, rank: *mut i32, device: *mut i32, kind: *mut i32, rccl_version: *mut i32) -> i32;
        pub fn rdf_comm_barrier(comm: *mut rdf_comm) -> i32;
        pub fn rdf_comm_allgather(comm: *mut rdf_comm, mine_host: *const c_void, bytes: i64, all_host: *mut c_void) -> i32;
        pub fn rdf_agg_combine(comm: *mut rdf_comm, aggs: *mut rdf_agg_result, nvalues: i32) -> i32;
        pub fn rdf_pipeline_dist(comm: *mut rdf_comm, prog: *const rdf_program, cols: *const rdf_array, ncols: i32, nchunks: i64,
                                 aggs: *mut rdf_agg_result) -> i32;
        pub fn rdf_pipeline_frame_dist(comm: *mut rdf_comm, prog: *const rdf_program, frame: *mut rdf_frame, aggs: *mut rdf_agg_result) -> i32;
        pub fn rdf_group_combine(comm: *mut rdf_comm, out: *mut rdf_group_result, group_rows: *mut i64, ngroups: i32, nvalues: i32) -> i32;
        pub fn rdf_groupby_agg_dist(comm: *mut rdf_comm, keys: *const rdf_array, values: *const rdf_array, nchunks: i64, agg: i32,
                                    max_groups: i64, exchange: i32, out_keys: *mut rdf_out, out_values: *mut rdf_out,
                                    out_counts: *mut rdf_out, stats: *mut rdf_exchange_stats) -> i32;
        pub fn rdf_groupby_agg_frame_dist(comm: *mut rdf_comm, frame: *mut rdf_frame, key_col: i32, value_col: i32, agg: i32,
                                          max_groups: i64, exchange: i32, out: *mut *mut rdf_frame, stats: *mut rdf_exchange_stats) -> i32;
        pub fn rdf_group_pipeline(nodes: *const rdf_expr_node, nnodes: i32, filter_root: i32, group_root: i32, ngroups: i32,
                                  value_roots: *const i32, nvalues: i32, cols: *const rdf_array, ncols: i32, nchunks: i64,
                                  out: *mut rdf_group_result, group_rows: *mut i64) -> i32;
        // ArrayFunctions over List<primitive> (src/functions/array.rs:15-399)
        pub fn rdf_list_contains(list: *const rdf_list_array, value: *const c_void, out: *mut rdf_out) -> i32;
        pub fn rdf_list_position(list: *const rdf_list_array, value: *const c_void, out: *mut rdf_out) -> i32;
        pub fn rdf_list_max(list: *const rdf_list_array, out: *mut rdf_out) -> i32;
        pub fn rdf_list_min(list: *const rdf_list_array, out: *mut rdf_out) -> i32;
        pub fn rdf_list_remove(list: *const rdf_list_array, value: *const c_void, out_offsets: *mut rdf_out, out_values: *mut rdf_out) -> i32;
        pub fn rdf_list_sort(list: *const rdf_list_array, out_values: *mut rdf_out) -> i32;
        pub fn rdf_list_distinct(list: *const rdf_list_array, out_offsets: *mut rdf_out, out_values: *mut rdf_out) -> i32;
        pub fn rdf_list_except(a: *const rdf_list_array, b: *const rdf_list_array, out_offsets: *mut rdf_out, out_values: *mut rdf_out) -> i32;
        pub fn rdf_list_intersect(a: *const rdf_list_array, b: *const rdf_list_array, out_offsets: *mut rdf_out, out_values: *mut rdf_out) -> i32;
        pub fn rdf_list_union(a: *const rdf_list_array, b: *const rdf_list_array, out_offsets: *mut rdf_out, out_values: *mut rdf_out) -> i32;
        pub fn rdf_list_repeat(list: *const rdf_list_array, count: i32, out_offsets: *mut rdf_out, out_values: *mut rdf_out) -> i32;
        // Utf8 (StringArray) columns: Column::filter / take and the string ScalarFunctions; one sizing rule for all (header)
        pub fn rdf_utf8_filter(chunks: *const rdf_utf8_array, mask: *const rdf_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_take(chunks: *const rdf_utf8_array, nchunks: i64, indices: *const rdf_array, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_trim(chunks: *const rdf_utf8_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_ltrim(chunks: *const rdf_utf8_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_rtrim(chunks: *const rdf_utf8_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_substring(chunks: *const rdf_utf8_array, nchunks: i64, pos: i64, len: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_lower(chunks: *const rdf_utf8_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_upper(chunks: *const rdf_utf8_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_predicate(op: i32, chunks: *const rdf_utf8_array, nchunks: i64, pattern: *const u8, pattern_bytes: i64, escape: i32, mask: *mut rdf_out) -> i32;
        pub fn rdf_utf8_compare(op: i32, a: *const rdf_utf8_array, b: *const rdf_utf8_array, nchunks: i64, mask: *mut rdf_out) -> i32;
        pub fn rdf_utf8_measure(what: i32, chunks: *const rdf_utf8_array, nchunks: i64, pattern: *const u8, pattern_bytes: i64, pos: i64, out: *mut rdf_out) -> i32;
        // Utf8 builders (concat / concat_ws, lpad / rpad, repeat, reverse, substring_index): the sizing rule of rdf_utf8_trim
        pub fn rdf_utf8_concat(parts: *const rdf_utf8_part, nparts: i32, nchunks: i64, with_separator: i32, sep: *const u8, sep_bytes: i64,
                               out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_pad(side: i32, chunks: *const rdf_utf8_array, nchunks: i64, len: i64, pad: *const u8, pad_bytes: i64,
                            out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_repeat(chunks: *const rdf_utf8_array, nchunks: i64, times: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_reverse(chunks: *const rdf_utf8_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_substring_index(chunks: *const rdf_utf8_array, nchunks: i64, delim: *const u8, delim_bytes: i64, count: i64,
                                        out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        // Utf8 rewrites (ScalarFunctions::initcap / translate / split, declared with empty bodies, and replace): the sizing rule of
        // rdf_utf8_trim.  split takes a LITERAL delimiter and returns a List<Utf8>: out_list_offsets (rows + 1 entries, with the rows'
        // validity) is the `offsets` member of an rdf_list_array; out_offsets / out_data are the child Utf8 chunk, both sized in two calls.
        pub fn rdf_utf8_replace(chunks: *const rdf_utf8_array, nchunks: i64, search: *const u8, search_bytes: i64,
                                replacement: *const u8, replacement_bytes: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_translate(chunks: *const rdf_utf8_array, nchunks: i64, matching: *const u8, matching_bytes: i64,
                                  replace: *const u8, replace_bytes: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_initcap(chunks: *const rdf_utf8_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_split(chunks: *const rdf_utf8_array, nchunks: i64, delim: *const u8, delim_bytes: i64, limit: i64,
                              out_list_offsets: *mut rdf_out, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        // regular expressions (src/functions/scalar.rs declares regexp_extract and regexp_replace next to split, with empty bodies):
        // java.util.regex's leftmost-first matching, compiled per call into two DFAs on the host; a pattern the library does not
        // take is RDF_INVALID_ARGUMENT with the construct and its byte in rdf_last_error().
        pub fn rdf_utf8_regexp_info(pattern: *const u8, pattern_bytes: i64, out: *mut rdf_regexp_info) -> i32;
        pub fn rdf_utf8_regexp_match(chunks: *const rdf_utf8_array, nchunks: i64, pattern: *const u8, pattern_bytes: i64, mask: *mut rdf_out) -> i32;
        pub fn rdf_utf8_regexp_count(chunks: *const rdf_utf8_array, nchunks: i64, pattern: *const u8, pattern_bytes: i64, out: *mut rdf_out) -> i32;
        pub fn rdf_utf8_regexp_extract(chunks: *const rdf_utf8_array, nchunks: i64, pattern: *const u8, pattern_bytes: i64, group: i32,
                                       out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_regexp_replace(chunks: *const rdf_utf8_array, nchunks: i64, pattern: *const u8, pattern_bytes: i64,
                                       replacement: *const u8, replacement_bytes: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_regexp_split(chunks: *const rdf_utf8_array, nchunks: i64, pattern: *const u8, pattern_bytes: i64, limit: i64,
                                     out_list_offsets: *mut rdf_out, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        // text to values and back (src/functions/scalar.rs: date_format :209, from_unix_time :262, to_date :459, to_timestamp :461,
        // unix_timestamp :473, and CAST between Utf8 and Boolean / integer / date / timestamp): kind 0 .. 3 = bool, int, date,
        // timestamp; pattern null = the CAST grammar, else a datetime pattern.  parse: a row that does not parse is NULL, so every
        // output carries a validity buffer; failed (may be null) counts such rows per chunk.  format: rdf_utf8_trim's sizing rule.
        pub fn rdf_utf8_parse(chunks: *const rdf_utf8_array, nchunks: i64, kind: i32, unit: i32, pattern: *const u8, pattern_bytes: i64,
                              out: *mut rdf_out, failed: *mut i64) -> i32;
        pub fn rdf_utf8_format(a: *const rdf_array, nchunks: i64, kind: i32, unit: i32, pattern: *const u8, pattern_bytes: i64,
                               out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        // CAST between Utf8 and Float32 / Float64 (the dtype of the outputs / inputs): correctly rounded parsing, a row that does not
        // parse is NULL; Java's Double.toString / Float.toString under rdf_utf8_trim's sizing rule.
        pub fn rdf_utf8_parse_float(chunks: *const rdf_utf8_array, nchunks: i64, out: *mut rdf_out, failed: *mut i64) -> i32;
        pub fn rdf_utf8_format_float(a: *const rdf_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        // row hashes and digests (src/functions/scalar.rs: hash :265, crc32 :205, md5 :338, sha1 :389, sha2 :390): kind 0 = Spark's
        // Murmur3_x86_32 (Int32 out, seed 42 by default), 1 = xxhash64 (Int64 out); digests 0 .. 5 = md5, sha1, sha224, sha256, sha384,
        // sha512 as lowercase hex text under the sizing rule of rdf_utf8_trim; crc32 as Int64
        pub fn rdf_hash_columns(kind: i32, cols: *const rdf_sort_key, ncols: i32, nchunks: i64, seed: i64, out: *mut rdf_out) -> i32;
        pub fn rdf_utf8_digest(kind: i32, chunks: *const rdf_utf8_array, nchunks: i64, out_offsets: *mut rdf_out, out_data: *mut rdf_out) -> i32;
        pub fn rdf_utf8_crc32(chunks: *const rdf_utf8_array, nchunks: i64, out: *mut rdf_out) -> i32;
        // the fused batch loop (src/evaluation.rs:66-96); host-resident frames above one slab are streamed (rdf_stream_stats says how)
        pub fn rdf_jit_status() -> *const c_char;          // the run-time compiler: found or not, cache directory, counts
        pub fn rdf_stream_stats(slabs: *mut i64, bytes_staged: *mut i64, bytes_direct: *mut i64) -> i32;
        pub fn rdf_pipeline(prog: *const rdf_program, cols: *const rdf_array, ncols: i32, nchunks: i64, outs: *mut rdf_out,
                            aggs: *mut rdf_agg_result) -> i32;
        // a frame pinned for repeated queries: descriptors validated once, tables kept in HBM (device-resident columns)
        pub fn rdf_frame_pin(cols: *const rdf_array, ncols: i32, nchunks: i64, out: *mut *mut rdf_frame) -> i32;
        pub fn rdf_frame_release(frame: *mut rdf_frame) -> i32;
        pub fn rdf_pipeline_frame(prog: *const rdf_program, frame: *mut rdf_frame, outs: *mut rdf_out, aggs: *mut rdf_agg_result) -> i32;
        pub fn rdf_group_pipeline_frame(nodes: *const rdf_expr_node, nnodes: i32, filter_root: i32, group_root: i32, ngroups: i32,
                                        value_roots: *const i32, nvalues: i32, frame: *mut rdf_frame, out: *mut rdf_group_result,
                                        group_rows: *mut i64) -> i32;
        pub fn rdf_predicate_frame(nodes: *const rdf_expr_node, nnodes: i32, root: i32, frame: *mut rdf_frame, mask: *mut rdf_out) -> i32;
        // frame in, frame out: DataFrame::filter / take / sort (src/dataframe.rs:178-222) and GroupAggregate without walking the batch list
        pub fn rdf_frame_info(frame: *mut rdf_frame, ncols: *mut i32, nchunks: *mut i64, rows: *mut i64) -> i32;
        pub fn rdf_frame_column(frame: *mut rdf_frame, col: i32, chunks: *mut rdf_array) -> i32;
        pub fn rdf_filter_frame(frame: *mut rdf_frame, nodes: *const rdf_expr_node, nnodes: i32, root: i32, out: *mut *mut rdf_frame) -> i32;
        pub fn rdf_take_columns(cols: *const rdf_array, ncols: i32, nchunks: i64, indices: *const rdf_array, outs: *mut rdf_out) -> i32;
        pub fn rdf_take_frame(frame: *mut rdf_frame, indices: *const rdf_array, out: *mut *mut rdf_frame) -> i32;
        pub fn rdf_sort_frame(frame: *mut rdf_frame, sort_cols: *const i32, nsort: i32, opts: *const rdf_sort_options,
                              out_indices: *mut rdf_out, out: *mut *mut rdf_frame) -> i32;
        pub fn rdf_groupby_agg_frame(frame: *mut rdf_frame, key_cols: *const i32, nkeys: i32, value_col: i32, agg: i32,
                                     max_groups: i64, out: *mut *mut rdf_frame) -> i32;
        // ingestion: pinned reader buffers, uploads that do not block the reader, one fence per load (src/dataframe.rs:349-407)
        pub fn rdf_host_alloc(ptr: *mut *mut c_void, bytes: i64) -> i32;
        pub fn rdf_host_free(ptr: *mut c_void) -> i32;
        pub fn rdf_host_register(ptr: *mut c_void, bytes: i64) -> i32;
        pub fn rdf_host_unregister(ptr: *mut c_void) -> i32;
        pub fn rdf_copy_h2d_async(dst_dev: *mut c_void, src_host_pinned: *const c_void, bytes: i64) -> i32;
        pub fn rdf_copy_fence() -> i32;
        // synthetic data, switches, introspection (bench / tests)
        pub fn rdf_fill_uniform_f64(dev_ptr: *mut f64, n: i64, seed: u64, column_id: u64, first_row: i64, lo: f64, hi: f64) -> i32;
        pub fn rdf_fill_uniform_i64(dev_ptr: *mut i64, n: i64, seed: u64, column_id: u64, first_row: i64, lo: i64, hi: i64) -> i32;
        pub fn rdf_fill_validity(dev_ptr: *mut u8, nbits: i64, seed: u64, column_id: u64, first_row: i64, null_fraction: f64) -> i32;
        pub fn rdf_set_option(name: *const c_char, value: i64) -> i32;
        pub fn rdf_spec_catalog_size() -> i32;
        pub fn rdf_last_kernel() -> *const c_char;
        pub fn rdf_kernel_timing_reset(enable: i32) -> i32;
        pub fn rdf_kernel_timing_get(total_ms: *mut f64, launches: *mut i64) -> i32;
        pub fn rdf_probe_stream(kind: i32, a: *const c_void, b: *mut c_void, c: *mut c_void, bytes: i64, reps: i32, best_gbps: *mut f64, shape: *mut c_char, shape_len: i32) -> i32;
    }
}

// ------------------------------------------------------------------------------------------------
// (2) views over Arrow arrays, output buffers, error mapping

use self::sys::*;
use arrow::array::{Array, ArrayData, ArrayRef, BooleanArray, Float64Array, Int64Array, ListArray, PrimitiveArray, StringArray, UInt32Array};
use arrow::buffer::MutableBuffer;
use arrow::datatypes::{ArrowNumericType, ArrowPrimitiveType, DataType};
use arrow::error::ArrowError;
use std::ffi::CStr;
use std::os::raw::c_void;

/// DataType -> rdf_dtype for the types the hot path computes on (src/evaluation.rs:107-293).
pub fn rdf_dtype(dt: &DataType) -> i32 {
    match dt {
        DataType::Int8 => RDF_I8, DataType::Int16 => RDF_I16, DataType::Int32 => RDF_I32, DataType::Int64 => RDF_I64,
        DataType::UInt8 => RDF_U8, DataType::UInt16 => RDF_U16, DataType::UInt32 => RDF_U32, DataType::UInt64 => RDF_U64,
        DataType::Float32 => RDF_F32, DataType::Float64 => RDF_F64, DataType::Boolean => RDF_BOOL,
        // temporal arrays pass as their storage (rdf_hour takes the unit separately)
        DataType::Date32(_) | DataType::Time32(_) => RDF_I32,
        DataType::Date64(_) | DataType::Time64(_) | DataType::Timestamp(_, _) => RDF_I64,
        _ => RDF_NULLTYPE,
    }
}

/// A chunk as the library sees it: pointers into the array's own buffers, nothing copied.
pub fn view(a: &dyn Array) -> rdf_array {
    let d = a.data();
    rdf_array {
        values: d.buffers()[0].raw_data() as *const c_void,
        validity: d.null_buffer().map_or(std::ptr::null(), |b| b.raw_data()),
        offset: d.offset() as i64,
        length: d.len() as i64,
        null_count: d.null_count() as i64,
        dtype: rdf_dtype(d.data_type()),
        mem: RDF_MEM_HOST,
    }
}
pub fn views<T: ArrowPrimitiveType>(chunks: &[&PrimitiveArray<T>]) -> Vec<rdf_array> { chunks.iter().map(|c| view(*c)).collect() }

/// Caller-allocated output chunk (values + optional validity), 64-byte padded like every Arrow buffer.
pub struct OutBuf { values: MutableBuffer, validity: Option<MutableBuffer>, dtype: DataType, capacity: usize }
impl OutBuf {
    pub fn new(dtype: DataType, capacity: usize, nullable: bool) -> Self {
        let width = match rdf_dtype(&dtype) { RDF_BOOL => 0, RDF_I8 | RDF_U8 => 1, RDF_I16 | RDF_U16 => 2, RDF_I32 | RDF_U32 | RDF_F32 => 4, _ => 8 };
        let vbytes = if width == 0 { (capacity + 7) / 8 + 8 } else { capacity * width + 16 };
        let mut values = MutableBuffer::new(vbytes);
        values.resize(vbytes).unwrap();
        let validity = if nullable { let mut b = MutableBuffer::new((capacity + 7) / 8 + 8); b.resize((capacity + 7) / 8 + 8).unwrap(); Some(b) } else { None };
        OutBuf { values, validity, dtype, capacity }
    }
    pub fn as_out(&mut self) -> rdf_out {
        rdf_out { values: self.values.raw_data_mut() as *mut c_void,
                  validity: self.validity.as_mut().map_or(std::ptr::null_mut(), |b| b.raw_data_mut()),
                  capacity: self.capacity as i64, length: 0, null_count: 0, dtype: rdf_dtype(&self.dtype), mem: RDF_MEM_HOST }
    }
    /// Wrap what the library wrote (`length`, `null_count` come back in the rdf_out).
    pub fn finish(self, out: &rdf_out) -> ArrayRef {
        let mut b = ArrayData::builder(self.dtype).len(out.length as usize).null_count(out.null_count as usize).add_buffer(self.values.freeze());
        if let Some(v) = self.validity { b = b.null_bit_buffer(v.freeze()); }
        arrow::array::make_array(b.build())
    }
}

fn last_error() -> String { unsafe { CStr::from_ptr(rdf_last_error()).to_string_lossy().into_owned() } }
/// rdf_status -> ArrowError / DataFrameError (src/error.rs:6-21).
pub fn status(code: i32) -> Result<(), ArrowError> {
    match code {
        RDF_OK => Ok(()),
        RDF_DIVIDE_BY_ZERO => Err(ArrowError::DivideByZero),
        RDF_INVALID_ARGUMENT => Err(ArrowError::InvalidArgumentError(last_error())),
        RDF_MEMORY_ERROR => Err(ArrowError::MemoryError(last_error())),
        _ => Err(ArrowError::ComputeError(last_error())),
    }
}

// ------------------------------------------------------------------------------------------------
// (3) replacement bodies, same signatures as the reference

/// ScalarFunctions::add (src/functions/scalar.rs:16-34); subtract / multiply / divide / par_multiply alike.
pub fn add<T: ArrowNumericType>(left: Vec<&PrimitiveArray<T>>, right: Vec<&PrimitiveArray<T>>) -> Result<Vec<ArrayRef>, ArrowError> {
    binary_op(RDF_OP_ADD, &left, &right)
}
fn binary_op<T: ArrowNumericType>(op: i32, left: &[&PrimitiveArray<T>], right: &[&PrimitiveArray<T>]) -> Result<Vec<ArrayRef>, ArrowError> {
    let (a, b) = (views(left), views(right));
    let mut bufs: Vec<OutBuf> = left.iter().zip(right.iter())
        .map(|(l, r)| OutBuf::new(T::get_data_type(), l.len(), l.null_count() + r.null_count() > 0)).collect();
    let mut outs: Vec<rdf_out> = bufs.iter_mut().map(|b| b.as_out()).collect();
    status(unsafe { rdf_binary(op, a.as_ptr(), b.as_ptr(), a.len() as i64, outs.as_mut_ptr()) })?;
    Ok(bufs.into_iter().zip(outs.iter()).map(|(b, o)| b.finish(o)).collect())
}

/// ScalarFunctions::sin ... tanh, abs (src/functions/scalar.rs:106-452): `scalar_op(array, |x| x.sin())` per chunk.
pub fn unary_op<T: ArrowNumericType>(op: i32, array: Vec<&PrimitiveArray<T>>) -> Result<Vec<ArrayRef>, ArrowError> {
    let a = views(&array);
    let mut bufs: Vec<OutBuf> = array.iter().map(|x| OutBuf::new(T::get_data_type(), x.len(), x.null_count() > 0)).collect();
    let mut outs: Vec<rdf_out> = bufs.iter_mut().map(|b| b.as_out()).collect();
    status(unsafe { rdf_unary(op, a.as_ptr(), a.len() as i64, outs.as_mut_ptr()) })?;
    Ok(bufs.into_iter().zip(outs.iter()).map(|(b, o)| b.finish(o)).collect())
}

/// AggregateFunctions::sum (src/functions/aggregate.rs:82-93); min / max / count / avg alike.
pub fn sum<T: ArrowNumericType>(chunks: &[&PrimitiveArray<T>]) -> Result<Option<T::Native>, ArrowError> where T::Native: Default {
    let a = views(chunks);
    let (mut value, mut is_some) = (T::Native::default(), 0i32);
    status(unsafe { rdf_sum(a.as_ptr(), a.len() as i64, &mut value as *mut T::Native as *mut c_void, &mut is_some) })?;
    Ok(if is_some != 0 { Some(value) } else { None })
}

/// AggregateFunctions::variance / stddev / skewness / kurtosis (src/functions/aggregate.rs:94-102, empty there): one pass for the
/// state, any number of statistics off it.  `stat` = RDF_STAT_*; variance and stddev are the sample forms (VAR_SAMP, STDDEV_SAMP).
pub fn moments<T: ArrowNumericType>(chunks: &[&PrimitiveArray<T>], mask: Option<&[&BooleanArray]>) -> Result<rdf_moments_state, ArrowError> {
    let a = views(chunks);
    let m = mask.map(|m| m.iter().map(|x| view(*x)).collect::<Vec<_>>());
    let mut st = rdf_moments_state::default();
    status(unsafe { rdf_moments(a.as_ptr(), m.as_ref().map_or(std::ptr::null(), |v| v.as_ptr()), a.len() as i64, &mut st) })?;
    Ok(st)
}
pub fn moments_stat(st: &rdf_moments_state, stat: i32) -> Result<Option<f64>, ArrowError> {
    let (mut v, mut is_some) = (0f64, 0i32);
    status(unsafe { rdf_moments_stat(st, stat, &mut v, &mut is_some) })?;
    Ok(if is_some != 0 { Some(v) } else { None })
}
/// shards, ranks or slabs: `into` becomes the state of both row sets
pub fn moments_merge(into: &mut rdf_moments_state, other: &rdf_moments_state) -> Result<(), ArrowError> {
    status(unsafe { rdf_moments_merge(into, other) })
}
/// ScalarFunctions::corr (src/functions/scalar.rs:184, empty there) and the covariances; `stat` = RDF_COSTAT_*.
pub fn comoments<T: ArrowNumericType, U: ArrowNumericType>(x: &[&PrimitiveArray<T>], y: &[&PrimitiveArray<U>], stat: i32) -> Result<Option<f64>, ArrowError> {
    let (a, b) = (views(x), views(y));
    let mut st = rdf_comoments_state::default();
    status(unsafe { rdf_comoments(a.as_ptr(), b.as_ptr(), std::ptr::null(), a.len() as i64, &mut st) })?;
    let (mut v, mut is_some) = (0f64, 0i32);
    status(unsafe { rdf_comoments_stat(&st, stat, &mut v, &mut is_some) })?;
    Ok(if is_some != 0 { Some(v) } else { None })
}
pub fn comoments_merge(into: &mut rdf_comoments_state, other: &rdf_comoments_state) -> Result<(), ArrowError> {
    status(unsafe { rdf_comoments_merge(into, other) })
}

/// ChunkedArray::filter / Column::filter (src/table.rs:97-107, 213-215): chunk boundaries are kept.
/// NOTE: this per-call form marshals one descriptor per chunk on the host: on a column held in the readers' 1024-row batches
/// (1e9 rows = a million chunks) the call is host-bound (1 s of marshalling around a 2.5 ms kernel).  A DataFrame-level caller
/// (`DataFrame::filter`, `::take`, `::sort`) should pin the frame once and use `GpuFrame::filter / take / sort` below, which cost
/// what their kernels cost whatever the batch size; these two bodies are for one-off calls on a few large chunks.
pub fn filter_chunks<T: ArrowNumericType>(chunks: &[&PrimitiveArray<T>], mask: &[&BooleanArray]) -> Result<Vec<ArrayRef>, ArrowError> {
    let (c, m) = (views(chunks), mask.iter().map(|x| view(*x)).collect::<Vec<_>>());
    let mut counts = vec![0i64; m.len()];
    status(unsafe { rdf_filter_count(m.as_ptr(), m.len() as i64, counts.as_mut_ptr()) })?;
    let mut bufs: Vec<OutBuf> = chunks.iter().zip(counts.iter()).map(|(x, n)| OutBuf::new(T::get_data_type(), *n as usize, x.null_count() > 0)).collect();
    let mut outs: Vec<rdf_out> = bufs.iter_mut().map(|b| b.as_out()).collect();
    status(unsafe { rdf_filter(c.as_ptr(), m.as_ptr(), c.len() as i64, outs.as_mut_ptr()) })?;
    Ok(bufs.into_iter().zip(outs.iter()).map(|(b, o)| b.finish(o)).collect())
}

/// Column::take (src/table.rs:218-241): no `to_array()` concatenation copy; ONE output chunk.
pub fn take_chunks<T: ArrowNumericType>(chunks: &[&PrimitiveArray<T>], indices: &UInt32Array) -> Result<ArrayRef, ArrowError> {
    let (c, i) = (views(chunks), view(indices));
    let nullable = indices.null_count() > 0 || chunks.iter().any(|x| x.null_count() > 0);
    let mut buf = OutBuf::new(T::get_data_type(), indices.len(), nullable);
    let mut out = buf.as_out();
    status(unsafe { rdf_take(c.as_ptr(), c.len() as i64, &i, &mut out) })?;
    Ok(buf.finish(&out))
}

/// One rank's shard of a DataFrame sharded over the GPUs of a node by row ranges: what Evaluate::evaluate's
/// GroupAggregate arm (src/evaluation.rs:73, a panic in the reference) and AggregateFunctions run on when N > 1.
pub struct ShardedFrame { pub local: GpuFrame, comm: *mut rdf_comm }
impl ShardedFrame {
    /// `id`: rdf_comm_unique_id of rank 0, handed over by the host (file, socket, ...); the calling thread drives `local`'s device.
    pub fn new(local: GpuFrame, world: i32, rank: i32, id: &[u8; 128]) -> Result<ShardedFrame, ArrowError> {
        let mut comm: *mut rdf_comm = std::ptr::null_mut();
        status(unsafe { rdf_comm_init_rank(world, rank, id.as_ptr(), &mut comm) })?;
        Ok(ShardedFrame { local, comm })
    }
    /// GroupAggregate(group column, [agg(value column)]) over all shards -> the groups THIS rank owns (key, aggregate, count).
    pub fn group_aggregate(&self, key_col: i32, value_col: i32, agg: i32, max_groups: i64) -> Result<(GpuFrame, rdf_exchange_stats), ArrowError> {
        let (mut out, mut st) = (std::ptr::null_mut(), rdf_exchange_stats::default());
        status(unsafe { rdf_groupby_agg_frame_dist(self.comm, self.local.handle, key_col, value_col, agg, max_groups, RDF_EXCHANGE_AUTO, &mut out, &mut st) })?;
        Ok((GpuFrame { handle: out }, st))
    }
    /// AggregateFunctions::{sum, min, max, count} of a fused program over the whole sharded column: partials of the shard in,
    /// totals out, identical on every rank (rank-order fold).
    pub fn aggregate(&self, prog: &rdf_program, nvalues: usize) -> Result<Vec<rdf_agg_result>, ArrowError> {
        let mut aggs = vec![rdf_agg_result::default(); RDF_MAX_VALUES];
        // (kernel, all-gather of the partials and their fold stay on the device: one host wait per call)
        status(unsafe { rdf_pipeline_frame_dist(self.comm, prog, self.local.handle, aggs.as_mut_ptr()) })?;
        aggs.truncate(nvalues);
        Ok(aggs)
    }
}
impl Drop for ShardedFrame { fn drop(&mut self) { unsafe { rdf_comm_destroy(self.comm); } } }

/// A DataFrame resident in HBM: the handle is pinned once and every operator returns a new handle (released in Drop).
pub struct GpuFrame { handle: *mut rdf_frame }
impl Drop for GpuFrame { fn drop(&mut self) { unsafe { rdf_frame_release(self.handle); } } }
impl GpuFrame {
    /// DataFrame::filter (src/dataframe.rs:178-189): predicate over every batch, every column compacted in one pass.
    pub fn filter(&self, nodes: &[rdf_expr_node], root: i32) -> Result<GpuFrame, ArrowError> {
        let mut out: *mut rdf_frame = std::ptr::null_mut();
        status(unsafe { rdf_filter_frame(self.handle, nodes.as_ptr(), nodes.len() as i32, root, &mut out) })?;
        Ok(GpuFrame { handle: out })
    }
    /// DataFrame::sort (src/dataframe.rs:194-222): lexsort_to_indices + Column::take of every column.
    pub fn sort(&self, sort_cols: &[i32], opts: &[rdf_sort_options]) -> Result<GpuFrame, ArrowError> {
        let mut out: *mut rdf_frame = std::ptr::null_mut();
        status(unsafe { rdf_sort_frame(self.handle, sort_cols.as_ptr(), sort_cols.len() as i32, opts.as_ptr(), std::ptr::null_mut(), &mut out) })?;
        Ok(GpuFrame { handle: out })
    }
    /// DataFrame::take (src/dataframe.rs:216-222).
    pub fn take(&self, indices: &UInt32Array) -> Result<GpuFrame, ArrowError> {
        let (i, mut out) = (view(indices), std::ptr::null_mut());
        status(unsafe { rdf_take_frame(self.handle, &i, &mut out) })?;
        Ok(GpuFrame { handle: out })
    }
    /// (columns, batches, rows); rdf_frame_column(handle, c, views) then gives the device views of a column.
    pub fn shape(&self) -> (i32, i64, i64) {
        let (mut c, mut b, mut r) = (0i32, 0i64, 0i64);
        unsafe { rdf_frame_info(self.handle, &mut c, &mut b, &mut r) };
        (c, b, r)
    }
}

/// Transformation::GroupAggregate(groups, [aggregation]) — `Evaluate::evaluate` panics here today (src/evaluation.rs:73).
/// One aggregation over 1..4 integer grouping columns of any cardinality; keys[k][chunk].
pub fn group_aggregate(keys: &[Vec<rdf_array>], key_types: &[DataType], values: Option<&[rdf_array]>, agg: i32, value_out: DataType,
                       max_groups: usize) -> Result<(Vec<ArrayRef>, ArrayRef, ArrayRef), ArrowError> {
    let nchunks = keys[0].len();
    let flat: Vec<rdf_array> = keys.iter().flat_map(|k| k.iter().cloned()).collect();
    let cap = max_groups + 2;
    let mut kbufs: Vec<OutBuf> = key_types.iter().map(|t| OutBuf::new(t.clone(), cap, true)).collect();
    let mut kouts: Vec<rdf_out> = kbufs.iter_mut().map(|b| b.as_out()).collect();
    let (mut vbuf, mut cbuf) = (OutBuf::new(value_out, cap, true), OutBuf::new(DataType::Int64, cap, false));
    let (mut vout, mut cout) = (vbuf.as_out(), cbuf.as_out());
    status(unsafe { rdf_groupby_agg(flat.as_ptr(), keys.len() as i32, values.map_or(std::ptr::null(), |v| v.as_ptr()), nchunks as i64,
                                    agg, max_groups as i64, kouts.as_mut_ptr(), &mut vout, &mut cout) })?;
    Ok((kbufs.into_iter().zip(kouts.iter()).map(|(b, o)| b.finish(o)).collect(), vbuf.finish(&vout), cbuf.finish(&cout)))
}

/// ArrayFunctions::array_contains (src/functions/array.rs:15-37): a ListArray travels as two views.
pub fn list_view<T: ArrowNumericType>(array: &ListArray) -> rdf_list_array {
    let data = array.data();
    let child = array.values();
    let child = child.as_any().downcast_ref::<PrimitiveArray<T>>().unwrap();
    rdf_list_array {
        offsets: rdf_array { values: data.buffers()[0].raw_data() as *const c_void,            // i32 value_offsets, len + 1
                             validity: data.null_buffer().map_or(std::ptr::null(), |b| b.raw_data()),
                             offset: data.offset() as i64, length: array.len() as i64 + 1, null_count: -1, dtype: RDF_I32, mem: RDF_MEM_HOST },
        values: view(child),
    }
}
pub fn array_contains<T: ArrowNumericType>(array: &ListArray, val: T::Native) -> Result<ArrayRef, ArrowError> {
    let l = list_view::<T>(array);
    let mut buf = OutBuf::new(DataType::Boolean, array.len(), true);
    let mut out = buf.as_out();
    status(unsafe { rdf_list_contains(&l, &val as *const T::Native as *const c_void, &mut out) })?;
    Ok(buf.finish(&out))
}

/// A StringArray travels as two views, nothing copied: its value_offsets (Int32, len + 1, carrying the row validity and the
/// row offset of a slice) and its value bytes.
pub fn utf8_view(array: &StringArray) -> rdf_utf8_array {
    let data = array.data();
    let bytes = data.buffers()[1].len();
    rdf_utf8_array {
        offsets: rdf_array { values: data.buffers()[0].raw_data() as *const c_void,
                             validity: data.null_buffer().map_or(std::ptr::null(), |b| b.raw_data()),
                             offset: data.offset() as i64, length: array.len() as i64 + 1, null_count: -1, dtype: RDF_I32, mem: RDF_MEM_HOST },
        data: rdf_array { values: data.buffers()[1].raw_data() as *const c_void, validity: std::ptr::null(), offset: 0,
                          length: bytes as i64, null_count: 0, dtype: RDF_U8, mem: RDF_MEM_HOST },
    }
}
/// One rdf_utf8_* call made twice: the sizing call (no data buffers), then into buffers of exactly the reported sizes.
fn utf8_call(rows: &[usize], nullable: &[bool], call: &dyn Fn(*mut rdf_out, *mut rdf_out) -> i32) -> Result<Vec<ArrayRef>, ArrowError> {
    let mut obufs: Vec<OutBuf> = rows.iter().zip(nullable).map(|(r, n)| OutBuf::new(DataType::Int32, r + 1, *n)).collect();
    let mut oo: Vec<rdf_out> = obufs.iter_mut().map(|b| b.as_out()).collect();
    let mut od: Vec<rdf_out> = rows.iter().map(|_| rdf_out { values: std::ptr::null_mut(), validity: std::ptr::null_mut(), capacity: 0,
                                                           length: 0, null_count: 0, dtype: RDF_U8, mem: RDF_MEM_HOST }).collect();
    let code = call(oo.as_mut_ptr(), od.as_mut_ptr());
    if code != RDF_OK && code != RDF_MEMORY_ERROR { status(code)?; }
    let mut dbufs: Vec<OutBuf> = od.iter().map(|o| OutBuf::new(DataType::UInt8, o.length as usize, false)).collect();
    if code == RDF_MEMORY_ERROR {
        let mut oo2: Vec<rdf_out> = obufs.iter_mut().map(|b| b.as_out()).collect();
        let mut od2: Vec<rdf_out> = dbufs.iter_mut().map(|b| b.as_out()).collect();
        status(call(oo2.as_mut_ptr(), od2.as_mut_ptr()))?;
        oo = oo2; od = od2;
    }
    Ok(obufs.into_iter().zip(dbufs).zip(oo.iter().zip(od.iter())).map(|((ob, db), (o, d))| {
        let offs = ob.finish(o);
        let bytes = db.finish(d);
        let b = ArrayData::builder(DataType::Utf8).len(o.length as usize - 1).null_count(o.null_count as usize)
            .add_buffer(offs.data().buffers()[0].clone()).add_buffer(bytes.data().buffers()[0].clone());
        let b = match offs.data().null_buffer() { Some(v) => b.null_bit_buffer(v.clone()), None => b };
        arrow::array::make_array(b.build())
    }).collect())
}
/// ScalarFunctions::{lower, upper, trim, ltrim, rtrim} (src/functions/scalar.rs:315-427) over the chunks of a column.
pub fn utf8_unary(op: &str, chunks: &[&StringArray]) -> Result<Vec<ArrayRef>, ArrowError> {
    let v: Vec<rdf_utf8_array> = chunks.iter().map(|c| utf8_view(c)).collect();
    let f = match op { "lower" => rdf_utf8_lower, "upper" => rdf_utf8_upper, "trim" => rdf_utf8_trim, "ltrim" => rdf_utf8_ltrim,
                       "rtrim" => rdf_utf8_rtrim, _ => return Err(ArrowError::ComputeError(format!("no Utf8 function {}", op))) };
    let rows: Vec<usize> = chunks.iter().map(|c| c.len()).collect();
    let nullable: Vec<bool> = chunks.iter().map(|c| c.null_count() > 0 || c.data().null_buffer().is_some()).collect();
    utf8_call(&rows, &nullable, &|oo, od| unsafe { f(v.as_ptr(), v.len() as i64, oo, od) })
}
/// substring (scalar.rs:428-441): chars().skip(pos).take(len).
pub fn utf8_substring(chunks: &[&StringArray], pos: usize, len: usize) -> Result<Vec<ArrayRef>, ArrowError> {
    let v: Vec<rdf_utf8_array> = chunks.iter().map(|c| utf8_view(c)).collect();
    let rows: Vec<usize> = chunks.iter().map(|c| c.len()).collect();
    let nullable: Vec<bool> = chunks.iter().map(|c| c.data().null_buffer().is_some()).collect();
    utf8_call(&rows, &nullable, &|oo, od| unsafe { rdf_utf8_substring(v.as_ptr(), v.len() as i64, pos as i64, len as i64, oo, od) })
}
/// Column::filter (src/table.rs:97-107) of a Utf8 column by one BooleanArray per chunk.
pub fn utf8_filter(chunks: &[&StringArray], masks: &[&BooleanArray]) -> Result<Vec<ArrayRef>, ArrowError> {
    let v: Vec<rdf_utf8_array> = chunks.iter().map(|c| utf8_view(c)).collect();
    let m: Vec<rdf_array> = masks.iter().map(|b| view(*b)).collect();
    let rows: Vec<usize> = chunks.iter().map(|c| c.len()).collect();
    let nullable: Vec<bool> = chunks.iter().map(|c| c.data().null_buffer().is_some()).collect();
    utf8_call(&rows, &nullable, &|oo, od| unsafe { rdf_utf8_filter(v.as_ptr(), m.as_ptr(), v.len() as i64, oo, od) })
}
/// Column::take (src/table.rs:213-241) of a Utf8 column: one output chunk.
pub fn utf8_take(chunks: &[&StringArray], indices: &UInt32Array) -> Result<ArrayRef, ArrowError> {
    let v: Vec<rdf_utf8_array> = chunks.iter().map(|c| utf8_view(c)).collect();
    let idx = view(indices);
    let nullable = indices.data().null_buffer().is_some() || chunks.iter().any(|c| c.data().null_buffer().is_some());
    Ok(utf8_call(&[indices.len()], &[nullable], &|oo, od| unsafe { rdf_utf8_take(v.as_ptr(), v.len() as i64, &idx, oo, od) })?.remove(0))
}

/// DataFrame::sort (src/dataframe.rs:194-222) when criteria are StringArray columns: lexsort_to_indices over the chunks of
/// every criterion (`None` for a Utf8 column's numeric views, and the other way round), byte order, NULLs last, stable.
pub fn lexsort_to_indices(criteria: &[(Vec<&dyn Array>, bool)]) -> Result<ArrayRef, ArrowError> {   // (a UInt32Array)
    let nchunks = criteria.first().map_or(0, |c| c.0.len());
    let rows: usize = criteria.first().map_or(0, |c| c.0.iter().map(|a| a.len()).sum());
    let mut num: Vec<Vec<rdf_array>> = Vec::new();
    let mut txt: Vec<Vec<rdf_utf8_array>> = Vec::new();
    for (chunks, _) in criteria {
        match chunks.first().map(|a| a.data_type()) {
            Some(DataType::Utf8) => { txt.push(chunks.iter().map(|a| utf8_view(a.as_any().downcast_ref::<StringArray>().unwrap())).collect()); num.push(Vec::new()); }
            _ => { num.push(chunks.iter().map(|a| view(*a)).collect()); txt.push(Vec::new()); }
        }
    }
    let keys: Vec<rdf_sort_key> = criteria.iter().enumerate().map(|(k, (_, desc))| rdf_sort_key {
        values: if num[k].is_empty() { std::ptr::null() } else { num[k].as_ptr() },
        utf8: if txt[k].is_empty() { std::ptr::null() } else { txt[k].as_ptr() },
        options: rdf_sort_options { descending: *desc as i32, nulls_first: 0 },
    }).collect();
    let mut buf = OutBuf::new(DataType::UInt32, rows, false);
    let mut out = buf.as_out();
    status(unsafe { rdf_lexsort_to_indices(keys.as_ptr(), keys.len() as i32, nchunks as i64, &mut out) })?;
    Ok(buf.finish(&out))
}

/// AggregateFunctions::count_distinct / sum_distinct / first / last (src/functions/aggregate.rs, empty there) per group of 0 .. 4
/// grouping columns, and the CountDistinct / First / Last a GroupAggregate plans (src/expression.rs:114-221): `calls` are
/// (RDF_GRP_*, ignore_nulls) over ONE value column, numeric or Utf8, all answered from one sort.  -> (row index of every group's
/// first row as a UInt32Array, groups in ascending key order with the NULL group last: `take` / `utf8_take` the key columns
/// with it; one array per call): Int64Array for COUNT_DISTINCT, Float64Array / Int64Array for SUM_DISTINCT of a float / an
/// integer column, UInt32Array of ROW INDICES for FIRST / LAST (NULL with ignore_nulls where the group has no non-NULL value).
/// No calls and `value` = None: the distinct key tuples.  The result does not depend on row order, chunking or memory kind.
pub fn groupby_sorted(group_by: &[Vec<&dyn Array>], value: Option<&Vec<&dyn Array>>, calls: &[(i32, bool)]) -> Result<(ArrayRef, Vec<ArrayRef>), ArrowError> {
    let cols: Vec<&Vec<&dyn Array>> = group_by.iter().chain(value.into_iter()).collect();
    let nchunks = cols.first().map_or(0, |c| c.len());
    let rows: usize = cols.first().map_or(0, |c| c.iter().map(|a| a.len()).sum());
    let mut num: Vec<Vec<rdf_array>> = Vec::new();
    let mut txt: Vec<Vec<rdf_utf8_array>> = Vec::new();
    for chunks in cols.iter() {
        match chunks.first().map(|a| a.data_type()) {
            Some(DataType::Utf8) => { txt.push(chunks.iter().map(|a| utf8_view(a.as_any().downcast_ref::<StringArray>().unwrap())).collect()); num.push(Vec::new()); }
            _ => { num.push(chunks.iter().map(|a| view(*a)).collect()); txt.push(Vec::new()); }
        }
    }
    let keys: Vec<rdf_sort_key> = (0..cols.len()).map(|k| rdf_sort_key {
        values: if num[k].is_empty() { std::ptr::null() } else { num[k].as_ptr() },
        utf8: if txt[k].is_empty() { std::ptr::null() } else { txt[k].as_ptr() },
        options: rdf_sort_options { descending: 0, nulls_first: 0 },
    }).collect();
    let ng = group_by.len();
    let float_value = value.and_then(|v| v.first()).map_or(false, |a| matches!(a.data_type(), DataType::Float32 | DataType::Float64));
    let ccalls: Vec<rdf_group_call> = calls.iter().map(|(f, ign)| rdf_group_call { fn_: *f, ignore_nulls: *ign as i32 }).collect();
    let mut bufs: Vec<OutBuf> = calls.iter().map(|(f, ign)| match *f {
        RDF_GRP_COUNT_DISTINCT => OutBuf::new(DataType::Int64, rows, false),
        RDF_GRP_SUM_DISTINCT => OutBuf::new(if float_value { DataType::Float64 } else { DataType::Int64 }, rows, false),
        _ => OutBuf::new(DataType::UInt32, rows, *ign),
    }).collect();
    let mut outs: Vec<rdf_out> = bufs.iter_mut().map(|b| b.as_out()).collect();
    let mut rbuf = OutBuf::new(DataType::UInt32, rows, false);
    let mut rout = rbuf.as_out();
    let mut groups = 0i64;
    status(unsafe { rdf_groupby_sorted(if ng > 0 { keys.as_ptr() } else { std::ptr::null() }, ng as i32,
                                       if value.is_some() { keys[ng..].as_ptr() } else { std::ptr::null() }, nchunks as i64,
                                       if ccalls.is_empty() { std::ptr::null() } else { ccalls.as_ptr() }, ccalls.len() as i32,
                                       &mut rout, if outs.is_empty() { std::ptr::null_mut() } else { outs.as_mut_ptr() }, &mut groups) })?;
    Ok((rbuf.finish(&rout), bufs.into_iter().zip(outs.iter()).map(|(b, o)| b.finish(o)).collect()))
}

/// percentile / median / percentile_disc (Spark's aggregates; aggregate.rs stops before them) per group of 0 .. 4 grouping
/// columns over ONE value column: `calls` = (RDF_PCT_CONT | RDF_PCT_DISC, p), the median is (RDF_PCT_CONT, 0.5).  -> (row index
/// of every group's first row, groups in ascending key order with the NULL group last; one array per call: Float64Array for
/// CONT, UInt32Array of ROW INDICES into the value column for DISC, NULL where the group has no non-NULL value; Int64Array of
/// the non-NULL values per group).  Without grouping columns a numeric column is answered by a radix select, no sort.
pub fn groupby_percentile(group_by: &[Vec<&dyn Array>], value: &Vec<&dyn Array>, calls: &[(i32, f64)]) -> Result<(ArrayRef, Vec<ArrayRef>, ArrayRef), ArrowError> {
    let cols: Vec<&Vec<&dyn Array>> = group_by.iter().chain(std::iter::once(value)).collect();
    let nchunks = value.len();
    let rows: usize = value.iter().map(|a| a.len()).sum();
    let mut num: Vec<Vec<rdf_array>> = Vec::new();
    let mut txt: Vec<Vec<rdf_utf8_array>> = Vec::new();
    for chunks in &cols {
        match chunks.first().map(|a| a.data_type()) {
            Some(DataType::Utf8) => { txt.push(chunks.iter().map(|a| utf8_view(a.as_any().downcast_ref::<StringArray>().unwrap())).collect()); num.push(Vec::new()); }
            _ => { num.push(chunks.iter().map(|a| view(*a)).collect()); txt.push(Vec::new()); }
        }
    }
    let keys: Vec<rdf_sort_key> = (0..cols.len()).map(|k| rdf_sort_key {
        values: if num[k].is_empty() { std::ptr::null() } else { num[k].as_ptr() },
        utf8: if txt[k].is_empty() { std::ptr::null() } else { txt[k].as_ptr() },
        options: rdf_sort_options { descending: 0, nulls_first: 0 },
    }).collect();
    let ng = group_by.len();
    let ccalls: Vec<rdf_percentile_call> = calls.iter().map(|(k, p)| rdf_percentile_call { kind: *k, reserved: 0, p: *p }).collect();
    let mut bufs: Vec<OutBuf> = calls.iter().map(|(k, _)| OutBuf::new(if *k == RDF_PCT_CONT { DataType::Float64 } else { DataType::UInt32 }, rows, true)).collect();
    let mut outs: Vec<rdf_out> = bufs.iter_mut().map(|b| b.as_out()).collect();
    let mut rbuf = OutBuf::new(DataType::UInt32, rows, false);
    let mut rout = rbuf.as_out();
    let mut cbuf = OutBuf::new(DataType::Int64, rows, false);
    let mut cout = cbuf.as_out();
    let mut groups = 0i64;
    status(unsafe { rdf_groupby_percentile(if ng > 0 { keys.as_ptr() } else { std::ptr::null() }, ng as i32, keys[ng..].as_ptr(), nchunks as i64,
                                           if ccalls.is_empty() { std::ptr::null() } else { ccalls.as_ptr() }, ccalls.len() as i32,
                                           &mut rout, if outs.is_empty() { std::ptr::null_mut() } else { outs.as_mut_ptr() }, &mut cout, &mut groups) })?;
    Ok((rbuf.finish(&rout), bufs.into_iter().zip(outs.iter()).map(|(b, o)| b.finish(o)).collect(), cbuf.finish(&cout)))
}

/// collect_list() / collect_set() (src/functions/array.rs:404-405, ArrayFunction::CollectList / CollectSet, empty there) per
/// group of 0 .. 4 grouping columns over ONE value column, numeric or Utf8; `kind` = RDF_COLLECT_LIST (the non-NULL values in
/// row order) or RDF_COLLECT_SET (the distinct non-NULL values ascending).  -> (row index of every group's first row, groups in
/// ascending key order with the NULL group last; Int32 offsets, groups + 1 entries; UInt32 row index of every element): `take`
/// / `utf8_take` the key columns by the first and the value column by the third, and wrap offsets + child as a ListArray.
pub fn groupby_collect(group_by: &[Vec<&dyn Array>], value: &Vec<&dyn Array>, kind: i32) -> Result<(ArrayRef, ArrayRef, ArrayRef), ArrowError> {
    let cols: Vec<&Vec<&dyn Array>> = group_by.iter().chain(std::iter::once(value)).collect();
    let nchunks = value.len();
    let rows: usize = value.iter().map(|a| a.len()).sum();
    let mut num: Vec<Vec<rdf_array>> = Vec::new();
    let mut txt: Vec<Vec<rdf_utf8_array>> = Vec::new();
    for chunks in cols.iter() {
        match chunks.first().map(|a| a.data_type()) {
            Some(DataType::Utf8) => { txt.push(chunks.iter().map(|a| utf8_view(a.as_any().downcast_ref::<StringArray>().unwrap())).collect()); num.push(Vec::new()); }
            _ => { num.push(chunks.iter().map(|a| view(*a)).collect()); txt.push(Vec::new()); }
        }
    }
    let keys: Vec<rdf_sort_key> = (0..cols.len()).map(|k| rdf_sort_key {
        values: if num[k].is_empty() { std::ptr::null() } else { num[k].as_ptr() },
        utf8: if txt[k].is_empty() { std::ptr::null() } else { txt[k].as_ptr() },
        options: rdf_sort_options { descending: 0, nulls_first: 0 },
    }).collect();
    let ng = group_by.len();
    let (mut rbuf, mut obuf, mut cbuf) = (OutBuf::new(DataType::UInt32, rows, false), OutBuf::new(DataType::Int32, rows + 1, false), OutBuf::new(DataType::UInt32, rows, false));
    let (mut rout, mut oout, mut cout) = (rbuf.as_out(), obuf.as_out(), cbuf.as_out());
    let (mut groups, mut elements) = (0i64, 0i64);
    status(unsafe { rdf_groupby_collect(if ng > 0 { keys.as_ptr() } else { std::ptr::null() }, ng as i32, keys[ng..].as_ptr(), nchunks as i64, kind,
                                        &mut rout, &mut oout, &mut cout, std::ptr::null_mut(), &mut groups, &mut elements) })?;
    Ok((rbuf.finish(&rout), obuf.finish(&oout), cbuf.finish(&cout)))
}

/// ScalarFunctions::explode (src/functions/scalar.rs:237, empty there) of a ListArray with primitive children; `outer` keeps a
/// NULL or empty list as one row with a NULL element.  -> (UInt32 list row of every output row: `take` the frame's other
/// columns by it; UInt32 index into the list's child values: `take` the child by it; Int32 position inside the list).
pub fn list_explode<T: ArrowNumericType>(array: &ListArray, outer: bool) -> Result<(ArrayRef, ArrayRef, ArrayRef), ArrowError> {
    let l = list_view::<T>(array);
    let mut rows = 0i64;
    status(unsafe { rdf_list_explode(&l, outer as i32, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), &mut rows) })?;   // the count-only call
    let (mut pbuf, mut cbuf, mut sbuf) = (OutBuf::new(DataType::UInt32, rows as usize, false), OutBuf::new(DataType::UInt32, rows as usize, true),
                                          OutBuf::new(DataType::Int32, rows as usize, true));
    let (mut pout, mut cout, mut sout) = (pbuf.as_out(), cbuf.as_out(), sbuf.as_out());
    status(unsafe { rdf_list_explode(&l, outer as i32, &mut pout, &mut cout, &mut sout, &mut rows) })?;
    Ok((pbuf.finish(&pout), cbuf.finish(&cout), sbuf.finish(&sout)))
}

/// WindowSpec { partition_by, order_by } (src/window.rs) + one WindowFunctions entry (src/functions/window.rs; `ntile` of
/// scalar.rs:345): the function's value for every row, in row order, as one array — Int64Array for row_number / rank /
/// dense_rank / ntile, Float64Array for percent_rank / cume_dist, and for lag / lead a UInt32Array of ROW INDICES (NULL
/// where the partition ends) to gather any column with `take` / `utf8_take`.  Keys as for `lexsort_to_indices`; the
/// `bool` of a partition key is not read.  Several functions over one spec: pass them all, they share the sort.
pub fn window(partition_by: &[(Vec<&dyn Array>, bool)], order_by: &[(Vec<&dyn Array>, bool)], rows: usize,
              calls: &[(i32, i64)]) -> Result<Vec<ArrayRef>, ArrowError> {
    let nchunks = partition_by.first().or(order_by.first()).map_or(0, |c| c.0.len());
    let mut num: Vec<Vec<rdf_array>> = Vec::new();
    let mut txt: Vec<Vec<rdf_utf8_array>> = Vec::new();
    for (chunks, _) in partition_by.iter().chain(order_by.iter()) {
        match chunks.first().map(|a| a.data_type()) {
            Some(DataType::Utf8) => { txt.push(chunks.iter().map(|a| utf8_view(a.as_any().downcast_ref::<StringArray>().unwrap())).collect()); num.push(Vec::new()); }
            _ => { num.push(chunks.iter().map(|a| view(*a)).collect()); txt.push(Vec::new()); }
        }
    }
    let keys: Vec<rdf_sort_key> = partition_by.iter().chain(order_by.iter()).enumerate().map(|(k, (_, desc))| rdf_sort_key {
        values: if num[k].is_empty() { std::ptr::null() } else { num[k].as_ptr() },
        utf8: if txt[k].is_empty() { std::ptr::null() } else { txt[k].as_ptr() },
        options: rdf_sort_options { descending: *desc as i32, nulls_first: 0 },
    }).collect();
    let (np, no) = (partition_by.len(), order_by.len());
    let ccalls: Vec<rdf_window_call> = calls.iter().map(|(f, p)| rdf_window_call { fn_: *f, pad: 0, param: *p }).collect();
    let mut bufs: Vec<OutBuf> = calls.iter().map(|(f, _)| match *f {
        RDF_WIN_PERCENT_RANK | RDF_WIN_CUME_DIST => OutBuf::new(DataType::Float64, rows, false),
        RDF_WIN_LAG | RDF_WIN_LEAD => OutBuf::new(DataType::UInt32, rows, true),
        _ => OutBuf::new(DataType::Int64, rows, false),
    }).collect();
    let mut outs: Vec<rdf_out> = bufs.iter_mut().map(|b| b.as_out()).collect();
    status(unsafe { rdf_window(if np > 0 { keys.as_ptr() } else { std::ptr::null() }, np as i32,
                               if no > 0 { keys[np..].as_ptr() } else { std::ptr::null() }, no as i32,
                               nchunks as i64, if np + no == 0 { rows as i64 } else { 0 },
                               ccalls.as_ptr(), ccalls.len() as i32, outs.as_mut_ptr()) })?;
    Ok(bufs.into_iter().zip(outs.iter()).map(|(b, o)| b.finish(o)).collect())
}

/// WindowSpec { partition_by, order_by, rows_between | range_between } + one AggregateFunctions entry over the frame: `calls`
/// are (RDF_WAGG_*, value column index or -1, frame).  SUM / MIN / MAX come back in the value column's type (Int64Array /
/// Float64Array), AVG as Float64Array, COUNT as Int64Array (never NULL), FIRST_VALUE / LAST_VALUE as a UInt32Array of ROW
/// INDICES for `take` / `utf8_take`; everything but COUNT is NULL where the frame holds no valid row.  `values`: Int64 /
/// Float64 columns, chunked like the keys.  Several calls over one spec share the sort.
pub fn window_agg(partition_by: &[(Vec<&dyn Array>, bool)], order_by: &[(Vec<&dyn Array>, bool)], values: &[Vec<&dyn Array>], rows: usize,
                  calls: &[(i32, i32, rdf_window_frame)]) -> Result<Vec<ArrayRef>, ArrowError> {
    let nchunks = partition_by.first().or(order_by.first()).map(|c| c.0.len()).or(values.first().map(|v| v.len())).unwrap_or(0);
    let mut num: Vec<Vec<rdf_array>> = Vec::new();
    let mut txt: Vec<Vec<rdf_utf8_array>> = Vec::new();
    for (chunks, _) in partition_by.iter().chain(order_by.iter()) {
        match chunks.first().map(|a| a.data_type()) {
            Some(DataType::Utf8) => { txt.push(chunks.iter().map(|a| utf8_view(a.as_any().downcast_ref::<StringArray>().unwrap())).collect()); num.push(Vec::new()); }
            _ => { num.push(chunks.iter().map(|a| view(*a)).collect()); txt.push(Vec::new()); }
        }
    }
    let keys: Vec<rdf_sort_key> = partition_by.iter().chain(order_by.iter()).enumerate().map(|(k, (_, desc))| rdf_sort_key {
        values: if num[k].is_empty() { std::ptr::null() } else { num[k].as_ptr() },
        utf8: if txt[k].is_empty() { std::ptr::null() } else { txt[k].as_ptr() },
        options: rdf_sort_options { descending: *desc as i32, nulls_first: 0 },
    }).collect();
    let vviews: Vec<Vec<rdf_array>> = values.iter().map(|v| v.iter().map(|a| view(*a)).collect()).collect();
    let vptrs: Vec<*const rdf_array> = vviews.iter().map(|v| v.as_ptr()).collect();
    let vtype = |i: i32| if i >= 0 { values[i as usize][0].data_type().clone() } else { DataType::Int64 };
    let (np, no) = (partition_by.len(), order_by.len());
    let ccalls: Vec<rdf_window_agg_call> = calls.iter().map(|(f, v, fr)| rdf_window_agg_call { fn_: *f, value: *v, frame: *fr }).collect();
    let mut bufs: Vec<OutBuf> = calls.iter().map(|(f, v, _)| match *f {
        RDF_WAGG_COUNT => OutBuf::new(DataType::Int64, rows, false),
        RDF_WAGG_AVG => OutBuf::new(DataType::Float64, rows, true),
        RDF_WAGG_FIRST_VALUE | RDF_WAGG_LAST_VALUE => OutBuf::new(DataType::UInt32, rows, true),
        _ => OutBuf::new(vtype(*v), rows, true),
    }).collect();
    let mut outs: Vec<rdf_out> = bufs.iter_mut().map(|b| b.as_out()).collect();
    status(unsafe { rdf_window_agg(if np > 0 { keys.as_ptr() } else { std::ptr::null() }, np as i32,
                                   if no > 0 { keys[np..].as_ptr() } else { std::ptr::null() }, no as i32,
                                   if vptrs.is_empty() { std::ptr::null() } else { vptrs.as_ptr() }, vptrs.len() as i32,
                                   nchunks as i64, if np + no + values.len() == 0 { rows as i64 } else { 0 },
                                   ccalls.as_ptr(), ccalls.len() as i32, outs.as_mut_ptr()) })?;
    Ok(bufs.into_iter().zip(outs.iter()).map(|(b, o)| b.finish(o)).collect())
}

/// window_agg over RANGE frames with VALUE offsets: `order_by` is ONE Int32 / Int64 (dates and timestamps as their storage) or
/// Float64 column, `calls` are (RDF_WAGG_*, value column index or -1, frame) with the frame's offsets in that column's units — a
/// rolling 7-day sum over a Date32 column is { RDF_BOUND_PRECEDING, RDF_BOUND_CURRENT_ROW, start_i: 7, .. }.  Results as window_agg's;
/// MIN / MAX need one unbounded side.
pub fn window_range_agg(partition_by: &[(Vec<&dyn Array>, bool)], order_by: &(Vec<&dyn Array>, bool), values: &[Vec<&dyn Array>], rows: usize,
                        calls: &[(i32, i32, rdf_window_range_frame)]) -> Result<Vec<ArrayRef>, ArrowError> {
    let nchunks = order_by.0.len();
    let mut num: Vec<Vec<rdf_array>> = Vec::new();
    let mut txt: Vec<Vec<rdf_utf8_array>> = Vec::new();
    for (chunks, _) in partition_by.iter().chain(std::iter::once(order_by)) {
        match chunks.first().map(|a| a.data_type()) {
            Some(DataType::Utf8) => { txt.push(chunks.iter().map(|a| utf8_view(a.as_any().downcast_ref::<StringArray>().unwrap())).collect()); num.push(Vec::new()); }
            _ => { num.push(chunks.iter().map(|a| view(*a)).collect()); txt.push(Vec::new()); }
        }
    }
    let keys: Vec<rdf_sort_key> = partition_by.iter().chain(std::iter::once(order_by)).enumerate().map(|(k, (_, desc))| rdf_sort_key {
        values: if num[k].is_empty() { std::ptr::null() } else { num[k].as_ptr() },
        utf8: if txt[k].is_empty() { std::ptr::null() } else { txt[k].as_ptr() },
        options: rdf_sort_options { descending: *desc as i32, nulls_first: 0 },
    }).collect();
    let vviews: Vec<Vec<rdf_array>> = values.iter().map(|v| v.iter().map(|a| view(*a)).collect()).collect();
    let vptrs: Vec<*const rdf_array> = vviews.iter().map(|v| v.as_ptr()).collect();
    let vtype = |i: i32| if i >= 0 { values[i as usize][0].data_type().clone() } else { DataType::Int64 };
    let np = partition_by.len();
    let ccalls: Vec<rdf_window_range_call> = calls.iter().map(|(f, v, fr)| rdf_window_range_call { fn_: *f, value: *v, frame: *fr }).collect();
    let mut bufs: Vec<OutBuf> = calls.iter().map(|(f, v, _)| match *f {
        RDF_WAGG_COUNT => OutBuf::new(DataType::Int64, rows, false),
        RDF_WAGG_AVG => OutBuf::new(DataType::Float64, rows, true),
        RDF_WAGG_FIRST_VALUE | RDF_WAGG_LAST_VALUE => OutBuf::new(DataType::UInt32, rows, true),
        _ => OutBuf::new(vtype(*v), rows, true),
    }).collect();
    let mut outs: Vec<rdf_out> = bufs.iter_mut().map(|b| b.as_out()).collect();
    status(unsafe { rdf_window_range_agg(if np > 0 { keys.as_ptr() } else { std::ptr::null() }, np as i32, keys[np..].as_ptr(), 1,
                                         if vptrs.is_empty() { std::ptr::null() } else { vptrs.as_ptr() }, vptrs.len() as i32,
                                         nchunks as i64, ccalls.as_ptr(), ccalls.len() as i32, outs.as_mut_ptr()) })?;
    Ok(bufs.into_iter().zip(outs.iter()).map(|(b, o)| b.finish(o)).collect())
}

/// Column::hist (src/table.rs:244-290) of an Int64 / Float64 column: (bucket start, bucket end, count[, count / counted])
/// per bucket.  The buckets are numpy.histogram's over [min, max] (the reference's histo_fp buckets are not pinned by its
/// test); NULL rows and NaN are not counted.
pub fn column_hist(chunks: &[&dyn Array], nbins: usize, density: bool) -> Result<Vec<(f64, f64, u64, Option<f64>)>, ArrowError> {
    let v: Vec<rdf_array> = chunks.iter().map(|a| view(*a)).collect();
    let (mut cbuf, mut ebuf) = (OutBuf::new(DataType::Int64, nbins, false), OutBuf::new(DataType::Float64, nbins + 1, false));
    let (mut oc, mut oe) = (cbuf.as_out(), ebuf.as_out());
    let mut counted = 0i64;
    status(unsafe { rdf_hist(v.as_ptr(), v.len() as i64, nbins as i64, std::ptr::null(), &mut oc, &mut oe, &mut counted) })?;
    let (counts, edges) = (cbuf.finish(&oc), ebuf.finish(&oe));
    let counts = counts.as_any().downcast_ref::<Int64Array>().unwrap();
    let edges = edges.as_any().downcast_ref::<Float64Array>().unwrap();
    Ok((0..nbins).map(|i| (edges.value(i), edges.value(i + 1), counts.value(i) as u64,
                           if density && counted > 0 { Some(counts.value(i) as f64 / counted as f64) } else { None })).collect())
}
/// Column::uniques (src/table.rs:293-341): the distinct values of the valid rows as one array (Int64Array / Float64Array /
/// StringArray -> GenericVector::I / F / S), in unspecified order.
pub fn column_uniques(chunks: &[&dyn Array]) -> Result<ArrayRef, ArrowError> {
    if let Some(DataType::Utf8) = chunks.first().map(|a| a.data_type()) {
        let v: Vec<rdf_utf8_array> = chunks.iter().map(|a| utf8_view(a.as_any().downcast_ref::<StringArray>().unwrap())).collect();
        let rows: usize = chunks.iter().map(|a| a.len()).sum();
        let count = 0i64;   // written by the library; the row count of the result says the same
        return Ok(utf8_call(&[rows], &[false], &|oo, od| unsafe { rdf_utf8_uniques(v.as_ptr(), v.len() as i64, oo, od, &count as *const i64 as *mut i64) })?.remove(0));
    }
    let v: Vec<rdf_array> = chunks.iter().map(|a| view(*a)).collect();
    let mut count = 0i64;
    status(unsafe { rdf_uniques(v.as_ptr(), v.len() as i64, std::ptr::null_mut(), &mut count) })?;
    let mut buf = OutBuf::new(chunks[0].data_type().clone(), count as usize, false);
    let mut out = buf.as_out();
    status(unsafe { rdf_uniques(v.as_ptr(), v.len() as i64, &mut out, &mut count) })?;
    Ok(buf.finish(&out))
}

// Evaluate::evaluate (src/evaluation.rs:66-96): fuse each maximal run of Calculate / Filter steps into ONE rdf_pipeline call —
// flatten the Calculations into [rdf_expr_node] (Column -> COLUMN index, ScalarFunction -> OP, Cast -> OP CAST with the
// target dtype), SINK_STORE for a projection, SINK_AGG when the run ends in an aggregate; `include/rdf_frame.hpp`
// (`rdf::Evaluate`) is the C++ statement of exactly that lowering.
