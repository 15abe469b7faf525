"""ctypes mirror of include/rdf_mi355x.h and a thin, symmetric call layer.

`Api(lib, prefix)` wraps any shared library that exports `<prefix>binary`, `<prefix>unary`, ... with the
signatures of the header over these structs.  The product is librdf_mi355x.so with prefix ``rdf_``
(rust_dataframe_amd.lib); the tests bind their CPU checker through the same class, so a parity test is
the same call made twice.  Nothing in this module computes anything.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

# ---------------------------------------------------------------- enums (include/rdf_mi355x.h)
RDF_OK, RDF_COMPUTE_ERROR, RDF_DIVIDE_BY_ZERO, RDF_INVALID_ARGUMENT, RDF_MEMORY_ERROR, RDF_DEVICE_ERROR = range(6)
STATUS_NAMES = ["OK", "ComputeError", "DivideByZero", "InvalidArgument", "MemoryError", "DeviceError"]

I8, I16, I32, I64, U8, U16, U32, U64, F32, F64, BOOL, NULLTYPE = range(12)
MEM_HOST, MEM_DEVICE = 0, 1
# rdf_member_kind, rdf_keep
MEMBER_SEMI, MEMBER_ANTI, MEMBER_IS_IN = 0, 1, 2
KEEP_FIRST, KEEP_LAST, KEEP_NONE = 0, 1, 2
MEMBER_MAX_KEYS = 4

(OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_ATAN2, OP_HYPOT, OP_LOG, OP_ABS, OP_ACOS, OP_ASIN, OP_ATAN, OP_CBRT,
 OP_CEIL, OP_COS, OP_COSH, OP_DEGREES, OP_EXP, OP_EXPM1, OP_FLOOR, OP_LOG10, OP_LOG2, OP_RADIANS, OP_ROUND,
 OP_SIN, OP_SINH, OP_SQRT, OP_TAN, OP_TANH, OP_CAST, OP_GT, OP_GE, OP_EQ, OP_NE, OP_LT, OP_LE, OP_NOT,
 OP_AND, OP_OR) = range(1, 39)
OP_HOUR_S, OP_HOUR_MS, OP_HOUR_US, OP_HOUR_NS, OP_HOUR_DAY = range(39, 44)
OP_COT, OP_SEC, OP_CSC = range(44, 47)
TIME_SECOND, TIME_MILLISECOND, TIME_MICROSECOND, TIME_NANOSECOND, TIME_DAY = range(5)
# rdf_datetime_field / rdf_trunc_level / rdf_date_shift_op
(DT_YEAR, DT_QUARTER, DT_MONTH, DT_DAY_OF_MONTH, DT_DAY_OF_WEEK, DT_DAY_OF_YEAR, DT_WEEK_OF_YEAR, DT_HOUR, DT_MINUTE, DT_SECOND,
 DT_DATE) = range(11)
DT_FIELDS = {"year": DT_YEAR, "quarter": DT_QUARTER, "month": DT_MONTH, "day_of_month": DT_DAY_OF_MONTH, "day_of_week": DT_DAY_OF_WEEK,
             "day_of_year": DT_DAY_OF_YEAR, "week_of_year": DT_WEEK_OF_YEAR, "hour": DT_HOUR, "minute": DT_MINUTE, "second": DT_SECOND,
             "date": DT_DATE}
TRUNC_YEAR, TRUNC_QUARTER, TRUNC_MONTH, TRUNC_WEEK, TRUNC_DAY, TRUNC_HOUR, TRUNC_MINUTE, TRUNC_SECOND = range(8)
TRUNC_LEVELS = {"year": TRUNC_YEAR, "quarter": TRUNC_QUARTER, "month": TRUNC_MONTH, "week": TRUNC_WEEK, "day": TRUNC_DAY,
                "hour": TRUNC_HOUR, "minute": TRUNC_MINUTE, "second": TRUNC_SECOND}
SHIFT_DAYS, SHIFT_MONTHS, SHIFT_LAST_DAY, SHIFT_NEXT_DAY = range(4)
DATE_SHIFTS = {"days": SHIFT_DAYS, "months": SHIFT_MONTHS, "last_day": SHIFT_LAST_DAY, "next_day": SHIFT_NEXT_DAY}
# rdf_null_test_op, RDF_SELECT_PARTS_MAX
IS_NULL, IS_NOT_NULL, IS_NAN = range(3)
NULL_TESTS = {"is_null": IS_NULL, "is_not_null": IS_NOT_NULL, "is_nan": IS_NAN}
SELECT_PARTS_MAX = 8

OP_NAMES = {
    "add": OP_ADD, "subtract": OP_SUB, "multiply": OP_MUL, "divide": OP_DIV, "atan2": OP_ATAN2,
    "hypot": OP_HYPOT, "log": OP_LOG, "abs": OP_ABS, "acos": OP_ACOS, "asin": OP_ASIN, "atan": OP_ATAN,
    "cbrt": OP_CBRT, "ceil": OP_CEIL, "cos": OP_COS, "cosh": OP_COSH, "degrees": OP_DEGREES, "exp": OP_EXP,
    "expm1": OP_EXPM1, "floor": OP_FLOOR, "log10": OP_LOG10, "log2": OP_LOG2, "radians": OP_RADIANS,
    "round": OP_ROUND, "sin": OP_SIN, "sinh": OP_SINH, "sqrt": OP_SQRT, "tan": OP_TAN, "tanh": OP_TANH,
    "cast": OP_CAST, "gt": OP_GT, "ge": OP_GE, "eq": OP_EQ, "ne": OP_NE, "lt": OP_LT, "le": OP_LE,
    "not": OP_NOT, "and": OP_AND, "or": OP_OR,
    "cot": OP_COT, "sec": OP_SEC, "csc": OP_CSC,
    "hour_s": OP_HOUR_S, "hour_ms": OP_HOUR_MS, "hour_us": OP_HOUR_US, "hour_ns": OP_HOUR_NS, "hour_day": OP_HOUR_DAY,
}
UNARY_OPS = [n for n, v in OP_NAMES.items() if OP_ABS <= v <= OP_TANH or OP_COT <= v <= OP_CSC]

NODE_COLUMN, NODE_SCALAR, NODE_OP = 0, 1, 2
SINK_STORE, SINK_AGG = 0, 1
MAX_VALUES = 4

NP_OF = {I8: np.int8, I16: np.int16, I32: np.int32, I64: np.int64, U8: np.uint8, U16: np.uint16,
         U32: np.uint32, U64: np.uint64, F32: np.float32, F64: np.float64}
DT_OF = {np.dtype(v): k for k, v in NP_OF.items()}
DT_OF[np.dtype(np.bool_)] = BOOL


def dtype_code(np_dtype) -> int:
    return DT_OF[np.dtype(np_dtype)]


# ---------------------------------------------------------------- structs
class rdf_array(C.Structure):
    _fields_ = [("values", C.c_void_p), ("validity", C.c_void_p), ("offset", C.c_int64), ("length", C.c_int64),
                ("null_count", C.c_int64), ("dtype", C.c_int32), ("mem", C.c_int32)]


class rdf_out(C.Structure):
    _fields_ = [("values", C.c_void_p), ("validity", C.c_void_p), ("capacity", C.c_int64), ("length", C.c_int64),
                ("null_count", C.c_int64), ("dtype", C.c_int32), ("mem", C.c_int32)]


class rdf_expr_node(C.Structure):
    _fields_ = [("kind", C.c_int32), ("op", C.c_int32), ("dtype", C.c_int32), ("lhs", C.c_int32), ("rhs", C.c_int32),
                ("column", C.c_int32), ("f64", C.c_double), ("i64", C.c_int64)]


class rdf_sort_options(C.Structure):
    _fields_ = [("descending", C.c_int32), ("nulls_first", C.c_int32)]


class rdf_program(C.Structure):
    _fields_ = [("nodes", C.POINTER(rdf_expr_node)), ("nnodes", C.c_int32), ("filter_root", C.c_int32),
                ("nvalues", C.c_int32), ("value_roots", C.c_int32 * MAX_VALUES), ("sink", C.c_int32)]


class rdf_agg_result(C.Structure):
    _fields_ = [("sum_f64", C.c_double), ("min_f64", C.c_double), ("max_f64", C.c_double), ("sum_i64", C.c_int64),
                ("min_i64", C.c_int64), ("max_i64", C.c_int64), ("count", C.c_int64), ("is_some", C.c_int32),
                ("dtype", C.c_int32)]


class rdf_group_result(C.Structure):
    _fields_ = [("sum_f64", C.c_double), ("sum_i64", C.c_int64), ("count", C.c_int64), ("is_some", C.c_int32), ("dtype", C.c_int32)]


MAX_GROUP_VALUES = 8
MAX_GROUP_SLOTS = 1024


class rdf_list_array(C.Structure):
    _fields_ = [("offsets", rdf_array), ("values", rdf_array)]


class rdf_utf8_array(C.Structure):
    _fields_ = [("offsets", rdf_array), ("data", rdf_array)]


class rdf_regexp_info(C.Structure):
    _fields_ = [("program_len", C.c_int32), ("forward_states", C.c_int32), ("reverse_states", C.c_int32), ("classes", C.c_int32),
                ("table_bytes", C.c_int64), ("can_match_empty", C.c_int32), ("anchored_start", C.c_int32)]


class rdf_utf8_part(C.Structure):
    _fields_ = [("utf8", C.POINTER(rdf_utf8_array)), ("literal", C.POINTER(C.c_uint8)), ("literal_bytes", C.c_int64)]


class rdf_value_part(C.Structure):
    _fields_ = [("column", C.POINTER(rdf_array)), ("literal_bits", C.c_uint64), ("literal_is_null", C.c_int32)]


class rdf_sort_key(C.Structure):
    _fields_ = [("values", C.POINTER(rdf_array)), ("utf8", C.POINTER(rdf_utf8_array)), ("options", rdf_sort_options)]


class rdf_key_out(C.Structure):
    _fields_ = [("values", C.POINTER(rdf_out)), ("utf8_offsets", C.POINTER(rdf_out)), ("utf8_data", C.POINTER(rdf_out))]


class rdf_multi_agg_call(C.Structure):
    _fields_ = [("agg", C.c_int32), ("value", C.c_int32)]


MULTI_MAX_CALLS, MULTI_MAX_VALUES = 8, 8


class rdf_window_call(C.Structure):
    _fields_ = [("fn", C.c_int32), ("pad", C.c_int32), ("param", C.c_int64)]


# rdf_window_fn
WIN_ROW_NUMBER, WIN_RANK, WIN_DENSE_RANK, WIN_PERCENT_RANK, WIN_CUME_DIST, WIN_NTILE, WIN_LAG, WIN_LEAD = range(8)
WINDOW_FNS = {"row_number": WIN_ROW_NUMBER, "rank": WIN_RANK, "dense_rank": WIN_DENSE_RANK, "percent_rank": WIN_PERCENT_RANK,
              "cume_dist": WIN_CUME_DIST, "ntile": WIN_NTILE, "lag": WIN_LAG, "lead": WIN_LEAD}
WINDOW_MAX_KEYS, WINDOW_MAX_CALLS = 4, 8


def window_out_dtype(fn: int) -> int:
    return F64 if fn in (WIN_PERCENT_RANK, WIN_CUME_DIST) else U32 if fn in (WIN_LAG, WIN_LEAD) else I64


class rdf_group_call(C.Structure):
    _fields_ = [("fn", C.c_int32), ("ignore_nulls", C.c_int32)]


# rdf_group_fn
GRP_COUNT_DISTINCT, GRP_SUM_DISTINCT, GRP_FIRST, GRP_LAST = range(4)
GROUP_FNS = {"count_distinct": GRP_COUNT_DISTINCT, "sum_distinct": GRP_SUM_DISTINCT, "first": GRP_FIRST, "last": GRP_LAST}
GROUP_MAX_CALLS = 8
GROUP_SORTED_TILE = 256   # RDF_GROUP_SORTED_TILE: the fold's tile over the distinct (group, value) pairs


class rdf_percentile_call(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double)]


PCT_CONT, PCT_DISC = 0, 1
PERCENTILE_KINDS = {"cont": PCT_CONT, "disc": PCT_DISC}
PERCENTILE_MAX_CALLS = 8
PERCENTILE_PICK_BLOCK = 256   # RDF_PERCENTILE_PICK_BLOCK: one (group, call) per thread of the pick kernel
PCT_SELECT_BITS, PCT_SELECT_TILE, PCT_SELECT_FINISH = 8, 4096, 2048   # RDF_PCT_SELECT_*: digit bits, rows per block tile, candidates of the LDS finish


def percentile_calls(calls: Sequence):
    """[("cont", p) | ("disc", p) | "median" | (kind number, p), ...] -> [(kind, p), ...]"""
    out = []
    for c in calls:
        if isinstance(c, str):
            if c != "median":
                raise ValueError(f"unknown percentile call {c!r}")
            out.append((PCT_CONT, 0.5))
        else:
            kind, p = c
            out.append((PERCENTILE_KINDS[kind] if isinstance(kind, str) else int(kind), float(p)))
    return out


def group_sorted_out_dtype(fn: int, value_dtype: int = I64) -> int:
    if fn == GRP_COUNT_DISTINCT:
        return I64
    if fn == GRP_SUM_DISTINCT:
        return F64 if value_dtype in (F32, F64) else I64
    return U32


# rdf_collect_kind
COLLECT_LIST, COLLECT_SET = 0, 1
COLLECT_KINDS = {"list": COLLECT_LIST, "set": COLLECT_SET}
COLLECT_TILE = 1024   # RDF_COLLECT_TILE: items per tile of the compaction (collect) and expansion (explode) passes


class rdf_window_frame(C.Structure):
    _fields_ = [("unit", C.c_int32), ("start_kind", C.c_int32), ("end_kind", C.c_int32), ("pad", C.c_int32), ("start", C.c_int64), ("end", C.c_int64)]


class rdf_window_agg_call(C.Structure):
    _fields_ = [("fn", C.c_int32), ("value", C.c_int32), ("frame", rdf_window_frame)]


FRAME_ROWS, FRAME_RANGE = 0, 1
BOUND_UNBOUNDED_PRECEDING, BOUND_PRECEDING, BOUND_CURRENT_ROW, BOUND_FOLLOWING, BOUND_UNBOUNDED_FOLLOWING = range(5)
WAGG_SUM, WAGG_MIN, WAGG_MAX, WAGG_COUNT, WAGG_AVG, WAGG_FIRST_VALUE, WAGG_LAST_VALUE = range(7)
WINDOW_AGG_FNS = {"sum": WAGG_SUM, "min": WAGG_MIN, "max": WAGG_MAX, "count": WAGG_COUNT, "avg": WAGG_AVG,
                  "first_value": WAGG_FIRST_VALUE, "last_value": WAGG_LAST_VALUE}
WINDOW_MAX_VALUES = 4
UNBOUNDED_PRECEDING, CURRENT_ROW, UNBOUNDED_FOLLOWING = "unbounded_preceding", 0, "unbounded_following"


def window_agg_out_dtype(fn: int, value_dtype: int = I64) -> int:
    return I64 if fn == WAGG_COUNT else F64 if fn == WAGG_AVG else U32 if fn in (WAGG_FIRST_VALUE, WAGG_LAST_VALUE) else value_dtype


def window_frame(unit, start, end) -> rdf_window_frame:
    """("rows" | "range", start, end) in WindowSpec's spelling: UNBOUNDED_PRECEDING / UNBOUNDED_FOLLOWING, 0 = the current row, a
    negative number = that many rows preceding, a positive one = following."""
    def bound(b):
        if b == UNBOUNDED_PRECEDING:
            return BOUND_UNBOUNDED_PRECEDING, 0
        if b == UNBOUNDED_FOLLOWING:
            return BOUND_UNBOUNDED_FOLLOWING, 0
        b = int(b)
        return (BOUND_CURRENT_ROW, 0) if b == 0 else (BOUND_PRECEDING, -b) if b < 0 else (BOUND_FOLLOWING, b)
    (sk, so), (ek, eo) = bound(start), bound(end)
    return rdf_window_frame({"rows": FRAME_ROWS, "range": FRAME_RANGE}[unit], sk, ek, 0, so, eo)


class rdf_window_range_frame(C.Structure):
    _fields_ = [("start_kind", C.c_int32), ("end_kind", C.c_int32), ("start_i", C.c_int64), ("end_i", C.c_int64),
                ("start_f", C.c_double), ("end_f", C.c_double)]


class rdf_window_range_call(C.Structure):
    _fields_ = [("fn", C.c_int32), ("value", C.c_int32), ("frame", rdf_window_range_frame)]


WINDOW_RANGE_TILE = 1024       # kWRangeTile of csrc/rdf_window_range.h: sorted positions per block of the bounds pass
WINDOW_RANGE_LDS_KEYS = 4096   # kWRangeLdsKeys: the keys of a tile's window that are staged in LDS; a wider window is searched in global memory


def window_range_frame(start, end) -> rdf_window_range_frame:
    """(start, end) of a RANGE frame over one numeric order key: UNBOUNDED_PRECEDING / UNBOUNDED_FOLLOWING or a number in the key's
    units, 0 = the current row, -s = s preceding, +s = s following; ints for Int32 / Int64 keys, floats for Float64 keys (both
    fields are filled, the library reads the pair of the key's type).  A bound may also be spelled (kind, offset) with a
    BOUND_* kind, which is how "0 PRECEDING" is said."""
    def bound(b):
        if isinstance(b, tuple):
            kind, off = b
        elif isinstance(b, str):
            kind, off = {UNBOUNDED_PRECEDING: BOUND_UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING: BOUND_UNBOUNDED_FOLLOWING}[b], 0
        else:
            kind, off = (BOUND_CURRENT_ROW, 0) if b == 0 else (BOUND_PRECEDING, -b) if b < 0 else (BOUND_FOLLOWING, b)
        exact = isinstance(off, (int, np.integer)) or (float(off).is_integer() and abs(float(off)) < 2.0 ** 63)
        return int(kind), (int(off) if exact else 0), float(off)
    (sk, si, sf), (ek, ei, ef) = bound(start), bound(end)
    return rdf_window_range_frame(sk, ek, si, ei, sf, ef)


class rdf_moments_state(C.Structure):
    _fields_ = [("count", C.c_int64), ("mean", C.c_double), ("mean_lo", C.c_double), ("m2", C.c_double), ("m3", C.c_double), ("m4", C.c_double)]


class rdf_comoments_state(C.Structure):
    _fields_ = [("count", C.c_int64), ("mean_x", C.c_double), ("mean_x_lo", C.c_double), ("mean_y", C.c_double), ("mean_y_lo", C.c_double),
                ("m2x", C.c_double), ("m2y", C.c_double), ("cxy", C.c_double)]


# rdf_stat / rdf_costat
STAT_MEAN, STAT_VAR_POP, STAT_VAR_SAMP, STAT_STDDEV_POP, STAT_STDDEV_SAMP, STAT_SKEWNESS, STAT_KURTOSIS = range(7)
STATS = {"mean": STAT_MEAN, "var_pop": STAT_VAR_POP, "var_samp": STAT_VAR_SAMP, "stddev_pop": STAT_STDDEV_POP,
         "stddev_samp": STAT_STDDEV_SAMP, "skewness": STAT_SKEWNESS, "kurtosis": STAT_KURTOSIS}
COSTAT_COVAR_POP, COSTAT_COVAR_SAMP, COSTAT_CORR = range(3)
COSTATS = {"covar_pop": COSTAT_COVAR_POP, "covar_samp": COSTAT_COVAR_SAMP, "corr": COSTAT_CORR}


class rdf_group_stat_call(C.Structure):
    _fields_ = [("stat", C.c_int32), ("reserved", C.c_int32)]


GROUP_MOMENTS_MAX_CALLS = 8
GROUP_MOMENTS_TILE = 256   # RDF_GROUP_MOMENTS_TILE: the sorted rows of one level-0 tile of rdf_groupby_moments


class rdf_exchange_stats(C.Structure):
    _fields_ = [("exchange", C.c_int32), ("rounds", C.c_int32), ("local_groups", C.c_int64), ("rows_sent", C.c_int64),
                ("rows_sent_remote", C.c_int64), ("rows_received", C.c_int64), ("bytes_sent", C.c_int64),
                ("bytes_sent_remote", C.c_int64), ("bytes_received", C.c_int64), ("exchange_ms", C.c_double)]


COMM_ID_BYTES = 128
COMM_RCCL, COMM_PEER = 0, 1
EXCHANGE_AUTO, EXCHANGE_GROUPS, EXCHANGE_ROWS = 0, 1, 2


class RdfError(Exception):
    """A non-OK rdf_status: DataFrameError / ArrowError as values (src/error.rs:6-15)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES[status] if 0 <= status < len(STATUS_NAMES) else status}: {message}")
        self.status = status
        self.message = message


# ---------------------------------------------------------------- host arrays (numpy-backed Arrow arrays)
def pack_bits(bits: np.ndarray, pad_words: bool = True) -> np.ndarray:
    """LSB-first bitmap of a bool vector, padded to whole 8-byte words (Arrow pads to 64 bytes)."""
    b = np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")
    n = len(b)
    want = ((n + 7) // 8) * 8 + 8 if pad_words else n
    out = np.zeros(want, dtype=np.uint8)
    out[:n] = b
    return out


def unpack_bits(buf: np.ndarray, offset: int, length: int) -> np.ndarray:
    if length == 0:
        return np.zeros(0, dtype=bool)
    bits = np.unpackbits(np.asarray(buf, dtype=np.uint8), bitorder="little")
    return bits[offset:offset + length].astype(bool)


@dataclass
class HostArray:
    """One Arrow array in host memory: values buffer (+ validity bitmap) with an element offset."""
    values: np.ndarray               # primitive: typed vector incl. `offset` leading elements; BOOL: uint8 bitmap
    validity: Optional[np.ndarray]   # uint8 bitmap or None
    offset: int
    length: int
    dtype: int
    null_count: int = -1

    @staticmethod
    def from_numpy(data, valid=None, offset: int = 0, dtype: Optional[int] = None, rng=None) -> "HostArray":
        """Build an array whose logical content is `data` (`valid`: bool vector, True = valid).  With
        offset > 0 the buffers get `offset` leading junk elements/bits, like a sliced Arrow array."""
        data = np.asarray(data)
        dt = dtype if dtype is not None else dtype_code(data.dtype)
        n = len(data)
        rng = rng or np.random.default_rng(1234)
        if dt == BOOL:
            junk = rng.integers(0, 2, size=offset).astype(bool)
            vals = pack_bits(np.concatenate([junk, data.astype(bool)]))
        else:
            npdt = NP_OF[dt]
            junk = rng.integers(0, 100, size=offset).astype(npdt)
            vals = np.ascontiguousarray(np.concatenate([junk, data.astype(npdt)]))
            if len(vals) == 0:
                vals = np.zeros(1, dtype=npdt)
        vbuf = None
        nulls = 0
        if valid is not None:
            valid = np.asarray(valid, dtype=bool)
            assert len(valid) == n
            junkv = rng.integers(0, 2, size=offset).astype(bool)
            vbuf = pack_bits(np.concatenate([junkv, valid]))
            nulls = int(n - valid.sum())
        return HostArray(vals, vbuf, offset, n, dt, nulls)

    def valid_mask(self) -> np.ndarray:
        if self.validity is None:
            return np.ones(self.length, dtype=bool)
        return unpack_bits(self.validity, self.offset, self.length)

    def to_numpy(self) -> np.ndarray:
        """Logical values (null slots included, whatever they hold)."""
        if self.dtype == BOOL:
            return unpack_bits(self.values, self.offset, self.length)
        return self.values[self.offset:self.offset + self.length]

    def to_pylist(self) -> list:
        v, m = self.to_numpy(), self.valid_mask()
        return [x.item() if ok else None for x, ok in zip(v, m)]

    def slice(self, offset: int, length: int) -> "HostArray":
        """Zero-copy slice (Array::slice, used by ChunkedArray::slice src/table.rs:77-95)."""
        length = max(0, min(length, self.length - offset))
        return HostArray(self.values, self.validity, self.offset + offset, length, self.dtype, -1)

    def _pointers(self):
        """(values address, validity address): looked up once per buffer pair — `ndarray.ctypes.data` costs about a
        microsecond, which is most of the per-chunk marshalling time of a frame in 1024-row batches."""
        cached = self.__dict__.get("_ptrs")
        if cached is None or cached[0] is not self.values or cached[1] is not self.validity:
            cached = (self.values, self.validity, self.values.ctypes.data, self.validity.ctypes.data if self.validity is not None else None)
            self.__dict__["_ptrs"] = cached
        return cached[2], cached[3]

    def c_struct(self, unknown_null_count: bool = False) -> rdf_array:
        vp, bp = self._pointers()
        return rdf_array(vp, bp, self.offset, self.length, -1 if unknown_null_count else self.null_count, self.dtype, MEM_HOST)

    @staticmethod
    def empty_out(dtype: int, capacity: int, with_validity: bool) -> "HostArray":
        if dtype == BOOL:
            vals = np.zeros(((capacity + 63) // 64) * 8 + 8, dtype=np.uint8)
        else:
            vals = np.zeros(max(capacity, 1), dtype=NP_OF[dtype])
        vbuf = np.zeros(((capacity + 63) // 64) * 8 + 8, dtype=np.uint8) if with_validity else None
        return HostArray(vals, vbuf, 0, capacity, dtype, 0)

    def out_struct(self) -> rdf_out:
        vp, bp = self._pointers()
        return rdf_out(vp, bp, self.length, 0, 0, self.dtype, MEM_HOST)


@dataclass
class DeviceArray:
    """One Arrow array resident in HBM; `keep` holds whatever owns the memory (torch tensors)."""
    values_ptr: int
    validity_ptr: Optional[int]
    offset: int
    length: int
    dtype: int
    null_count: int = -1
    keep: object = None
    capacity: int = -1     # for outputs: element capacity of the buffers (defaults to the initial length)

    def __post_init__(self):
        if self.capacity < 0:
            self.capacity = self.length

    @property
    def validity(self):
        return self.validity_ptr

    def c_struct(self, unknown_null_count: bool = False) -> rdf_array:
        return rdf_array(self.values_ptr, self.validity_ptr, self.offset, self.length,
                         -1 if unknown_null_count else self.null_count, self.dtype, MEM_DEVICE)

    def out_struct(self) -> rdf_out:
        return rdf_out(self.values_ptr, self.validity_ptr, self.capacity, 0, 0, self.dtype, MEM_DEVICE)


@dataclass
class HostList:
    """A ListArray with primitive children on the host: value_offsets (int32, rows + 1, possibly behind a row offset),
    optional list validity, child values (a HostArray)."""
    offsets: np.ndarray
    values: "HostArray"
    validity: Optional[np.ndarray] = None   # packed bits
    offset: int = 0
    length: int = 0

    @staticmethod
    def from_lists(rows, dtype: int, row_offset: int = 0, rng=None) -> "HostList":
        """rows: list of (list of numbers | None)."""
        pre = [[0] * 3] * row_offset     # dummy rows in front when a slice offset is requested
        allrows = pre + list(rows)
        offs = np.zeros(len(allrows) + 1, dtype=np.int32)
        flat = []
        for i, r in enumerate(allrows):
            flat.extend([] if r is None else list(r))
            offs[i + 1] = len(flat)
        vals = HostArray.from_numpy(np.array(flat, dtype=NP_OF[dtype]) if flat else np.zeros(0, dtype=NP_OF[dtype]), dtype=dtype)
        valid = None
        if any(r is None for r in rows):
            bits = np.array([True] * row_offset + [r is not None for r in rows])
            valid = pack_bits(bits)
        return HostList(offs, vals, valid, row_offset, len(rows))

    def c_struct(self) -> "rdf_list_array":
        o = rdf_array(self.offsets.ctypes.data, self.validity.ctypes.data if self.validity is not None else None, self.offset,
                      self.length + 1, -1 if self.validity is not None else 0, I32, MEM_HOST)
        return rdf_list_array(o, self.values.c_struct())

    def row_slices(self):
        o = self.offsets[self.offset:self.offset + self.length + 1]
        return [(int(o[i]), int(o[i + 1])) for i in range(self.length)]


@dataclass
class DeviceList:
    """A ListArray resident in HBM: device pointers of the int32 value_offsets (rows + 1) and of the child values."""
    offsets_ptr: int
    length: int
    values: "DeviceArray"
    validity_ptr: Optional[int] = None
    offset: int = 0
    keep: object = None

    def c_struct(self) -> "rdf_list_array":
        o = rdf_array(self.offsets_ptr, self.validity_ptr, self.offset, self.length + 1, -1 if self.validity_ptr else 0, I32, MEM_DEVICE)
        return rdf_list_array(o, self.values.c_struct())


# ---------------------------------------------------------------- expression trees

@dataclass
class HostUtf8:
    """A StringArray (Utf8, Int32 offsets) in host memory: value_offsets (rows + 1 from row `offset` on), optional row
    validity sharing that offset, and the value bytes, whose byte 0 is `data[data_offset]`."""
    offsets: np.ndarray                # int32
    data: np.ndarray                   # uint8
    validity: Optional[np.ndarray] = None
    offset: int = 0
    length: int = 0
    data_offset: int = 0
    null_count: int = -1

    @staticmethod
    def from_pylist(rows, row_offset: int = 0, data_offset: int = 0) -> "HostUtf8":
        """rows: list of (str | None).  row_offset leading junk rows and data_offset leading junk bytes make it look like
        a sliced Arrow array (the first value offset is then not 0)."""
        pre = ["j" * (i % 3 + 1) for i in range(row_offset)]
        enc = [b"" if r is None else r.encode("utf-8") for r in pre + list(rows)]
        offs = np.zeros(len(enc) + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(b) for b in enc]) if enc else []
        if offs[-1] > 2**31 - 1:
            raise ValueError("more than 2^31-1 bytes: not a Utf8 (Int32 offsets) array")
        data = np.frombuffer(b"\xff" * data_offset + b"".join(enc) + b"\0" * 8, dtype=np.uint8).copy()
        valid = None
        nulls = sum(r is None for r in rows)
        if nulls:
            valid = pack_bits(np.array([True] * row_offset + [r is not None for r in rows], dtype=bool))
        return HostUtf8(offs.astype(np.int32), data, valid, row_offset, len(rows), data_offset, nulls)

    @staticmethod
    def from_arrow(arr) -> "HostUtf8":
        """A pyarrow.StringArray (sliced arrays included: their row offset is kept, nothing is copied but the buffers' views)."""
        vbuf, obuf, dbuf = arr.buffers()[:3]
        offs = np.frombuffer(obuf, dtype=np.int32)
        data = np.frombuffer(dbuf, dtype=np.uint8) if dbuf is not None and dbuf.size else np.zeros(8, dtype=np.uint8)
        valid = None
        if vbuf is not None and arr.null_count:
            vb = np.frombuffer(vbuf, dtype=np.uint8)
            valid = np.zeros(((len(vb) + 7) // 8) * 8 + 8, dtype=np.uint8)   # readable to the next 8-byte boundary
            valid[:len(vb)] = vb
        return HostUtf8(offs, data, valid, arr.offset, len(arr), 0, arr.null_count)

    def c_struct(self) -> "rdf_utf8_array":
        o = rdf_array(self.offsets.ctypes.data, self.validity.ctypes.data if self.validity is not None else None, self.offset,
                      self.length + 1, self.null_count if self.validity is not None else 0, I32, MEM_HOST)
        d = rdf_array(self.data.ctypes.data, None, self.data_offset, len(self.data) - self.data_offset, 0, U8, MEM_HOST)
        return rdf_utf8_array(o, d)

    def valid_mask(self) -> np.ndarray:
        if self.validity is None:
            return np.ones(self.length, dtype=bool)
        return unpack_bits(self.validity, self.offset, self.length)

    def to_pylist(self) -> list:
        o = self.offsets[self.offset:self.offset + self.length + 1].astype(np.int64) + self.data_offset
        raw = self.data.tobytes()
        return [raw[o[i]:o[i + 1]].decode("utf-8") if ok else None for i, ok in enumerate(self.valid_mask())]

    def to_arrow(self):
        import pyarrow as pa
        o = self.offsets[self.offset:self.offset + self.length + 1].astype(np.int64)
        first, last = int(o[0]) if len(o) else 0, int(o[-1]) if len(o) else 0
        offs = (o - first).astype(np.int32)
        data = self.data[self.data_offset + first:self.data_offset + last]
        valid = None
        if self.validity is not None:
            valid = pa.py_buffer(pack_bits(self.valid_mask(), pad_words=False).tobytes())
        return pa.StringArray.from_buffers(self.length, pa.py_buffer(offs.tobytes()), pa.py_buffer(data.tobytes()), valid)


@dataclass
class DeviceUtf8:
    """A StringArray resident in HBM (offsets / validity / data device pointers); `keep` holds whatever owns the memory."""
    offsets_ptr: int
    data_ptr: int
    data_length: int
    length: int
    validity_ptr: Optional[int] = None
    offset: int = 0
    data_offset: int = 0
    null_count: int = -1
    keep: object = None

    @staticmethod
    def from_host(h: "HostUtf8", device: str = "cuda") -> "DeviceUtf8":
        """Copies the buffers of a HostUtf8 to the device with torch (tests and tools)."""
        import torch
        ot = torch.from_numpy(np.ascontiguousarray(h.offsets)).to(device)
        dt = torch.from_numpy(np.ascontiguousarray(h.data)).to(device)
        vt = torch.from_numpy(np.ascontiguousarray(h.validity)).to(device) if h.validity is not None else None
        return DeviceUtf8(ot.data_ptr(), dt.data_ptr(), len(h.data) - h.data_offset, h.length, vt.data_ptr() if vt is not None else None,
                          h.offset, h.data_offset, h.null_count, keep=(ot, dt, vt))

    def c_struct(self) -> "rdf_utf8_array":
        o = rdf_array(self.offsets_ptr, self.validity_ptr, self.offset, self.length + 1,
                      self.null_count if self.validity_ptr else 0, I32, MEM_DEVICE)
        d = rdf_array(self.data_ptr, None, self.data_offset, self.data_length, 0, U8, MEM_DEVICE)
        return rdf_utf8_array(o, d)

    def to_host(self) -> "HostUtf8":
        t_off, t_data, t_valid = self.keep[:3]
        offs = t_off.cpu().numpy()[:self.offset + self.length + 1].copy()
        data = t_data.cpu().numpy().copy() if t_data is not None else np.zeros(8, dtype=np.uint8)
        valid = t_valid.cpu().numpy().copy() if t_valid is not None and self.validity_ptr else None
        return HostUtf8(offs, data, valid, self.offset, self.length, self.data_offset, self.null_count)


UTF8_UNARY = ("trim", "ltrim", "rtrim", "substring", "lower", "upper")
# rdf_utf8_pred_op / rdf_utf8_measure_op
UTF8_PRED_OPS = {"eq": 0, "ne": 1, "lt": 2, "le": 3, "gt": 4, "ge": 5, "starts_with": 6, "ends_with": 7, "contains": 8, "like": 9}
UTF8_MEASURE_OPS = {"length": 0, "octet_length": 1, "locate": 2}
UTF8_PATTERN_MAX = 1024
UTF8_PARTS_MAX = 8
# rdf_hash_kind / rdf_digest_kind
HASH_KINDS = {"hash": 0, "murmur3": 0, "xxhash64": 1}
TEXT_BOOL, TEXT_INT, TEXT_DATE, TEXT_TIMESTAMP = range(4)
TEXT_KINDS = {"bool": TEXT_BOOL, "int": TEXT_INT, "date": TEXT_DATE, "timestamp": TEXT_TIMESTAMP}
DIGEST_KINDS = {"md5": 0, "sha1": 1, "sha224": 2, "sha256": 3, "sha384": 4, "sha512": 5}
DIGEST_HEX_BYTES = (32, 40, 56, 64, 96, 128)
HASH_COLS_MAX = 8


class Expr:
    """Builder for rdf_expr_node arrays; mirrors BooleanFilter / Scalar (src/expression.rs:718-763)."""

    def __init__(self):
        self.nodes: List[rdf_expr_node] = []

    def _add(self, **kw) -> int:
        n = rdf_expr_node(kind=kw.get("kind", 0), op=kw.get("op", 0), dtype=kw.get("dtype", 0), lhs=kw.get("lhs", -1),
                          rhs=kw.get("rhs", -1), column=kw.get("column", 0), f64=kw.get("f64", 0.0), i64=kw.get("i64", 0))
        self.nodes.append(n)
        return len(self.nodes) - 1

    def col(self, index: int) -> int:
        return self._add(kind=NODE_COLUMN, column=index)

    def scalar(self, value, dtype: Optional[int] = None) -> int:
        if value is None:
            return self._add(kind=NODE_SCALAR, dtype=NULLTYPE)
        if dtype is None:
            dtype = BOOL if isinstance(value, (bool, np.bool_)) else F64 if isinstance(value, (float, np.floating)) else I64
        if dtype in (F32, F64):
            return self._add(kind=NODE_SCALAR, dtype=dtype, f64=float(value))
        iv = int(value)
        if iv >= 2 ** 63:
            iv -= 2 ** 64
        return self._add(kind=NODE_SCALAR, dtype=dtype, i64=iv)

    def op(self, name, lhs: int, rhs: int = -1, dtype: int = 0) -> int:
        code = OP_NAMES[name] if isinstance(name, str) else int(name)
        return self._add(kind=NODE_OP, op=code, lhs=lhs, rhs=rhs, dtype=dtype)

    def cast(self, child: int, to: int) -> int:
        return self.op("cast", child, -1, to)

    def c_array(self):
        arr = (rdf_expr_node * max(1, len(self.nodes)))()
        for i, n in enumerate(self.nodes):
            arr[i] = n
        return arr


@dataclass
class AggResult:
    sum: object
    min: object
    max: object
    count: int
    is_some: bool
    dtype: int


# ---------------------------------------------------------------- the call layer
class Prepared:
    """A frame's columns (cols[c][i]) marshalled into the C descriptor array ONCE: a frame held in the reference's 1024-row
    batches has ~1e6 of them per 1e9 rows, and a benchmark loop hands the same immutable frame over many times."""

    def __init__(self, cols: Sequence[Sequence]):
        self.cols = cols
        self.carr = _flat(cols, len(cols[0]) if cols else 0)

    def __len__(self):
        return len(self.cols)

    def __getitem__(self, i):
        return self.cols[i]

    def __iter__(self):
        return iter(self.cols)


class Frame:
    """A frame the library returned (rdf_filter_frame, rdf_take_frame, rdf_sort_frame, rdf_groupby_agg_frame): its buffers live
    in HBM and belong to the handle.  Usable wherever a PinnedFrame is (Api.pipeline, the frame operators)."""

    def __init__(self, api, handle, parents=()):
        self.api = api
        self.handle = handle
        self.parents = parents      # frames whose buffers must outlive this one (none today: outputs are copies)

    def info(self):
        nc, nch, rows = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        fn = self.api._fn("frame_info")
        fn.restype = C.c_int
        self.api._check(fn(self.handle, C.byref(nc), C.byref(nch), C.byref(rows)))
        return nc.value, nch.value, rows.value

    def column(self, c: int) -> List["DeviceArray"]:
        """The column's batches as DeviceArrays borrowed from the frame."""
        _, nch, _ = self.info()
        arr = (rdf_array * max(1, nch))()
        fn = self.api._fn("frame_column")
        fn.restype = C.c_int
        self.api._check(fn(self.handle, C.c_int32(c), arr))
        return [DeviceArray(arr[i].values, arr[i].validity, arr[i].offset, arr[i].length, arr[i].dtype, arr[i].null_count, keep=self) for i in range(nch)]

    def column_to_host(self, c: int) -> List["HostArray"]:
        """Download a column batch by batch (tests)."""
        out = []
        d2h = self.api._fn("copy_d2h")
        d2h.restype = C.c_int
        d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        for a in self.column(c):
            es = np.dtype(NP_OF[a.dtype]).itemsize
            vals = np.zeros(max(a.length, 1), dtype=NP_OF[a.dtype])
            if a.length:
                self.api._check(d2h(vals.ctypes.data, a.values_ptr + a.offset * es, a.length * es))
            valid = None
            if a.validity_ptr:
                assert a.offset % 8 == 0
                valid = np.zeros((a.length + 7) // 8 + 8, dtype=np.uint8)
                if a.length:
                    self.api._check(d2h(valid.ctypes.data, a.validity_ptr + a.offset // 8, (a.length + 7) // 8))
            out.append(HostArray(vals[:a.length] if a.length else vals[:0], valid, 0, a.length, a.dtype, -1))
        return out

    def release(self):
        if self.handle is not None and self.handle.value:
            fn = self.api._fn("frame_release")
            fn.restype = C.c_int
            fn(self.handle)
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def __del__(self):
        try:
            self.release()
        except Exception:   # noqa: BLE001 - interpreter shutdown
            pass


class PinnedFrame(Frame):
    """rdf_frame_pin: device-resident columns validated once, their descriptors and tile tables kept in HBM; hand it to
    Api.pipeline in place of the column lists.  The arrays are kept alive by the handle; release() (or the context
    manager) frees the device tables."""

    def __init__(self, api, cols: Sequence[Sequence]):
        self.api = api
        self.cols = cols            # keeps the device buffers alive
        nchunks = len(cols[0])
        carr = _flat(cols, nchunks)
        h = C.c_void_p(0)
        fn = api._fn("frame_pin")
        fn.restype = C.c_int
        api._check(fn(carr, C.c_int32(len(cols)), C.c_int64(nchunks), C.byref(h)))
        self.handle = h
        api._fn("pipeline_frame").restype = C.c_int

    def release(self):
        if self.handle is not None and self.handle.value:
            fn = self.api._fn("frame_release")
            fn.restype = C.c_int
            fn(self.handle)
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def __del__(self):
        try:
            self.release()
        except Exception:   # noqa: BLE001 - interpreter shutdown
            pass


class PreparedCol(list):
    """ONE column (its chunk list) with its descriptor array marshalled once, for the entry points that take a column."""

    def __init__(self, chunks: Sequence):
        super().__init__(chunks)
        self.carr = _flat([list(chunks)], len(chunks))


def _flat(cols: Sequence[Sequence], nchunks: int):
    """cols[c][i] -> C array laid out [c * nchunks + i]."""
    if isinstance(cols, Prepared):
        return cols.carr
    if len(cols) == 1 and isinstance(cols[0], PreparedCol):   # one prepared column handed over as `[col]`
        return cols[0].carr
    n = len(cols) * nchunks
    arr = (rdf_array * max(1, n))()
    for c, col in enumerate(cols):
        assert len(col) == nchunks, "every column of a frame has the same chunking"
        for i, a in enumerate(col):
            arr[c * nchunks + i] = a.c_struct(getattr(a, "_unknown_nc", False))
    return arr


class Api:
    """Symmetric wrapper over `<prefix>binary`, `<prefix>unary`, ... of one shared library."""

    def __init__(self, lib: C.CDLL, prefix: str):
        self.lib = lib
        self.prefix = prefix
        self._err = getattr(lib, prefix + "last_error")
        self._err.restype = C.c_char_p
        for name in ("binary", "unary", "cast", "hour", "sum", "min", "max", "count", "avg", "predicate", "filter_count",
                     "filter", "filter_columns", "take", "pipeline", "group_pipeline", "groupby_sum", "groupby_agg", "groupby_merge", "list_contains", "list_position", "list_max", "list_min", "list_remove", "list_sort", "list_distinct", "list_except", "list_intersect", "list_union", "list_repeat", "sort_to_indices", "equijoin_indices", "equijoin_indices_multi", "fill_uniform_f64",
                     "fill_uniform_i64", "fill_validity"):
            fn = getattr(lib, prefix + name)
            fn.restype = C.c_int
        getattr(lib, prefix + "fill_uniform_f64").argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_int64, C.c_double, C.c_double]
        getattr(lib, prefix + "fill_uniform_i64").argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_int64]
        getattr(lib, prefix + "fill_validity").argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_int64, C.c_double]

    def _fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def _check(self, status: int):
        if status != RDF_OK:
            raise RdfError(status, (self._err() or b"").decode("utf-8", "replace"))

    # ---- outputs
    @staticmethod
    def _mk_outs(dtype: int, lens: Sequence[int], with_validity: Sequence[bool], like=None):
        outs = [HostArray.empty_out(dtype, n, wv) for n, wv in zip(lens, with_validity)]
        carr = (rdf_out * max(1, len(outs)))()
        for i, o in enumerate(outs):
            carr[i] = o.out_struct()
        return outs, carr

    @staticmethod
    def _finish(outs, carr):
        for i, o in enumerate(outs):
            o.length = carr[i].length
            o.null_count = carr[i].null_count
        return outs

    # ---- scalar kernels (ScalarFunctions, src/functions/scalar.rs)
    def binary(self, op, a: Sequence, b: Sequence, outs=None):
        code = OP_NAMES[op] if isinstance(op, str) else op
        n = len(a)
        ca, cb = _flat([a], n), _flat([b], len(b)) if len(b) == n else None
        if cb is None:
            raise ValueError("chunk lists differ in length")
        if outs is None:
            outs, carr = self._mk_outs(a[0].dtype if n else F64, [x.length for x in a],
                                       [x.validity is not None or y.validity is not None for x, y in zip(a, b)])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        self._check(self._fn("binary")(C.c_int32(code), ca, cb, C.c_int64(n), carr))
        return self._finish(outs, carr)

    def unary(self, op, a: Sequence, outs=None):
        code = OP_NAMES[op] if isinstance(op, str) else op
        n = len(a)
        ca = _flat([a], n)
        if outs is None:
            outs, carr = self._mk_outs(a[0].dtype if n else F64, [x.length for x in a], [x.validity is not None for x in a])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        self._check(self._fn("unary")(C.c_int32(code), ca, C.c_int64(n), carr))
        return self._finish(outs, carr)

    def cast(self, a: Sequence, to: int, outs=None):
        n = len(a)
        ca = _flat([a], n)
        if outs is None:   # a lossy cast yields NULL where the value does not fit: always hand over a validity buffer
            outs, carr = self._mk_outs(to, [x.length for x in a], [True for x in a])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        self._check(self._fn("cast")(ca, C.c_int64(n), carr))
        return self._finish(outs, carr)

    def hour(self, a: Sequence, unit: int, outs=None):
        """ScalarFunctions::hour over the Int32 / Int64 storage of a temporal column with time unit `unit` -> Int32 chunks."""
        n = len(a)
        ca = _flat([a], n)
        if outs is None:
            outs, carr = self._mk_outs(I32, [x.length for x in a], [x.validity is not None for x in a])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        self._check(self._fn("hour")(ca, C.c_int64(n), C.c_int32(unit), carr))
        return self._finish(outs, carr)

    # ---- date and time functions (ScalarFunctions::year .. date_diff: declared by the reference, empty there)
    def _dt_outs(self, dtype: int, a: Sequence, nullable: Sequence[bool], nout: int = 1):
        """nout outputs per chunk of `a`, laid out [f * nchunks + c], in the memory the inputs live in."""
        device = any(isinstance(x, DeviceArray) for x in a)
        outs = [self._window_out(dtype, x.length, device, nl) for _ in range(nout) for x, nl in zip(a, nullable)]
        return outs, (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])

    def _dt_fn(self, name):
        fn = self._fn(name)
        fn.restype = C.c_int
        return fn

    def datetime_fields(self, a: Sequence, unit: int, fields: Sequence, outs=None):
        """rdf_datetime_fields: the calendar fields (names of DT_FIELDS or their codes) of a temporal column given as its Int32 /
        Int64 storage with time unit `unit`, from ONE read of it -> one Int32 chunk list per field."""
        codes = [DT_FIELDS[f] if isinstance(f, str) else int(f) for f in fields]
        n = len(a)
        if outs is None:
            outs, carr = self._dt_outs(I32, a, [x.validity is not None for x in a], len(codes))
        else:
            outs = [o for per_field in outs for o in per_field]
            carr = (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])
        cf = (C.c_int32 * max(1, len(codes)))(*codes)
        self._check(self._dt_fn("datetime_fields")(_flat([a], n), C.c_int64(n), C.c_int32(unit), cf, C.c_int32(len(codes)), carr))
        self._finish(outs, carr)
        return [outs[f * n:(f + 1) * n] for f in range(len(codes))]

    def datetime_trunc(self, a: Sequence, unit: int, level, outs=None):
        """rdf_datetime_trunc: date_trunc(level, column) (a name of TRUNC_LEVELS or its code); trunc(date, level) with
        unit = TIME_DAY -> chunks of the input's storage type and unit."""
        code = TRUNC_LEVELS[level] if isinstance(level, str) else int(level)
        n = len(a)
        if outs is None:
            outs, carr = self._dt_outs(a[0].dtype if n else I64, a, [x.validity is not None for x in a])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        self._check(self._dt_fn("datetime_trunc")(_flat([a], n), C.c_int64(n), C.c_int32(unit), C.c_int32(code), carr))
        return self._finish(outs, carr)

    def date_shift(self, a: Sequence, unit: int, op, amount=0, outs=None):
        """rdf_date_shift: date_add / add_months / last_day / next_day (a name of DATE_SHIFTS or its code) -> Int32 day numbers.
        amount: an int for every row, or an Int32 chunk list chunked like `a`."""
        code = DATE_SHIFTS[op] if isinstance(op, str) else int(op)
        n = len(a)
        column = not isinstance(amount, (int, np.integer))
        if outs is None:
            per_row = column and code == SHIFT_NEXT_DAY
            outs, carr = self._dt_outs(I32, a, [per_row or x.validity is not None or (column and k.validity is not None)
                                                for x, k in zip(a, amount if column else a)])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        if column and len(amount) != n:
            raise ValueError("chunk lists differ in length")
        self._check(self._dt_fn("date_shift")(_flat([a], n), C.c_int64(n), C.c_int32(unit), C.c_int32(code), _flat([amount], n) if column else None,
                                              C.c_int32(0 if column else int(amount)), carr))
        return self._finish(outs, carr)

    def date_diff(self, end: Sequence, end_unit: int, start: Sequence, start_unit: int, outs=None):
        """rdf_date_diff: day(end) - day(start) -> Int32 chunks; each column has its own storage type and unit."""
        n = len(end)
        if len(start) != n:
            raise ValueError("chunk lists differ in length")
        if outs is None:
            outs, carr = self._dt_outs(I32, end, [x.validity is not None or y.validity is not None for x, y in zip(end, start)])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        self._check(self._dt_fn("date_diff")(_flat([end], n), C.c_int32(end_unit), _flat([start], n), C.c_int32(start_unit), C.c_int64(n), carr))
        return self._finish(outs, carr)

    # ---- conditional and NULL functions (ScalarFunctions::coalesce / greatest / least / nanv1 / when: declared by the reference, empty there)
    @staticmethod
    def _is_chunks(p) -> bool:
        return isinstance(p, (list, tuple))

    def _value_parts(self, parts: Sequence):
        """parts: chunk lists, Python scalars or None (the NULL literal) -> (rdf_value_part array, dtype, the first column, objects to keep alive)."""
        first = next((p for p in parts if self._is_chunks(p)), None)
        if first is None:
            raise ValueError("at least one part must be a column")
        n = len(first)
        dt = first[0].dtype if n else F64
        arr = (rdf_value_part * max(1, len(parts)))()
        keep = []
        for i, p in enumerate(parts):
            if self._is_chunks(p):
                if len(p) != n:
                    raise ValueError("chunk lists differ in length")
                ca = _flat([p], n)
                keep.append(ca)
                arr[i] = rdf_value_part(C.cast(ca, C.POINTER(rdf_array)), 0, 0)
            elif p is None:
                arr[i] = rdf_value_part(None, 0, 1)
            else:
                npdt = np.dtype(NP_OF[dt])
                bits = int(np.array([p], dtype=npdt).view(f"u{npdt.itemsize}")[0])
                arr[i] = rdf_value_part(None, bits, 0)
        return arr, dt, first, keep

    @staticmethod
    def _never_null(p, c: int) -> bool:
        return p[c].validity is None if Api._is_chunks(p) else p is not None

    def null_test(self, op, a: Sequence, outs=None):
        """rdf_null_test: is_null / is_not_null / is_nan (a name of NULL_TESTS or its code) -> RDF_BOOL chunks, never NULL.  A Utf8
        column is tested through its offsets array's validity, row offset and row count."""
        code = NULL_TESTS[op] if isinstance(op, str) else int(op)
        n = len(a)
        arr = (rdf_array * max(1, n))()
        for i, x in enumerate(a):
            if isinstance(x, (HostUtf8, DeviceUtf8)):
                o = x.c_struct().offsets
                arr[i] = rdf_array(None, o.validity, o.offset, x.length, o.null_count, I32, o.mem)
            else:
                arr[i] = x.c_struct(getattr(x, "_unknown_nc", False))
        if outs is None:
            device = any(isinstance(x, (DeviceArray, DeviceUtf8)) for x in a)
            outs = [self._window_out(BOOL, x.length, device, False) for x in a]
        carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        self._check(self._dt_fn("null_test")(C.c_int32(code), arr, C.c_int64(n), carr))
        return self._finish(outs, carr)

    def coalesce(self, parts: Sequence, outs=None):
        """rdf_coalesce: per row the first part that is not NULL.  parts: 1..8 chunk lists of one dtype, Python scalars or None."""
        arr, dt, first, keep = self._value_parts(parts)
        n = len(first)
        if outs is None:
            outs, carr = self._dt_outs(dt, first, [not any(self._never_null(p, c) for p in parts) for c in range(n)])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        self._check(self._dt_fn("coalesce")(arr, C.c_int32(len(parts)), C.c_int64(n), carr))
        return self._finish(outs, carr)

    def case_when(self, conds: Sequence, values: Sequence, otherwise=None, outs=None):
        """rdf_case_when: conds[k] (RDF_BOOL chunk lists) choose values[k]; rows no condition holds for take `otherwise` (None: NULL).
        values / otherwise: chunk lists of one dtype, Python scalars or None."""
        if len(conds) != len(values):
            raise ValueError("one value per condition")
        arr, dt, first, keep = self._value_parts(list(values) + [otherwise])
        n = len(first)
        cc = [_flat([c], n) for c in conds]
        cptr = (C.POINTER(rdf_array) * max(1, len(cc)))(*[C.cast(c, C.POINTER(rdf_array)) for c in cc])
        if outs is None:
            every = list(values) + [otherwise]
            outs, carr = self._dt_outs(dt, first, [not all(self._never_null(p, c) for p in every) for c in range(n)])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        other = None if otherwise is None else C.byref(arr, len(values) * C.sizeof(rdf_value_part))
        self._check(self._dt_fn("case_when")(cptr, arr, C.c_int32(len(values)), other, C.c_int64(n), carr))
        return self._finish(outs, carr)

    def extremum(self, greatest: bool, parts: Sequence, outs=None):
        """rdf_extremum: greatest / least of 2..8 parts under Spark's ordering; NULL parts are skipped."""
        arr, dt, first, keep = self._value_parts(parts)
        n = len(first)
        if outs is None:
            outs, carr = self._dt_outs(dt, first, [not any(self._never_null(p, c) for p in parts) for c in range(n)])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        self._check(self._dt_fn("extremum")(C.c_int32(1 if greatest else 0), arr, C.c_int32(len(parts)), C.c_int64(n), carr))
        return self._finish(outs, carr)

    def greatest(self, parts: Sequence, outs=None):
        return self.extremum(True, parts, outs)

    def least(self, parts: Sequence, outs=None):
        return self.extremum(False, parts, outs)

    def nanvl(self, a, b, outs=None):
        """rdf_nanvl: a where it is not NaN, else b (Float32 / Float64; chunk lists, Python scalars or None)."""
        arr, dt, first, keep = self._value_parts([a, b])
        n = len(first)
        if outs is None:
            outs, carr = self._dt_outs(dt, first, [not (self._never_null(a, c) and self._never_null(b, c)) for c in range(n)])
        else:
            carr = (rdf_out * max(1, n))(*[o.out_struct() for o in outs])
        self._check(self._dt_fn("nanvl")(C.byref(arr, 0), C.byref(arr, C.sizeof(rdf_value_part)), C.c_int64(n), carr))
        return self._finish(outs, carr)

    # ---- aggregates (AggregateFunctions, src/functions/aggregate.rs)
    def _agg(self, name: str, a: Sequence):
        n = len(a)
        ca = _flat([a], n)
        buf = (C.c_uint8 * 16)()
        some = C.c_int32(0)
        self._check(self._fn(name)(ca, C.c_int64(n), buf, C.byref(some)))
        if not some.value:
            return None
        dt = a[0].dtype
        return np.frombuffer(bytes(buf), dtype=NP_OF[dt], count=1)[0].item()

    def sum(self, a):
        return self._agg("sum", a)

    def min(self, a):
        return self._agg("min", a)

    def max(self, a):
        return self._agg("max", a)

    def count(self, a: Sequence):
        ca = _flat([a], len(a))
        out, some = C.c_int64(0), C.c_int32(0)
        self._check(self._fn("count")(ca, C.c_int64(len(a)), C.byref(out), C.byref(some)))
        return out.value if some.value else None

    def avg(self, a: Sequence):
        ca = _flat([a], len(a))
        out, some = C.c_double(0), C.c_int32(0)
        self._check(self._fn("avg")(ca, C.c_int64(len(a)), C.byref(out), C.byref(some)))
        return out.value if some.value else None

    # ---- moments (variance, stddev, skewness, kurtosis; covariance and corr): a state per call, statistics read off it
    def moments(self, chunks: Sequence, mask: Optional[Sequence] = None) -> rdf_moments_state:
        """rdf_moments: the state (count, mean as two doubles, m2, m3, m4) of the rows that count."""
        n = len(chunks)
        st = rdf_moments_state()
        fn = self._fn("moments")
        fn.restype = C.c_int
        self._check(fn(_flat([chunks], n), _flat([mask], n) if mask is not None else None, C.c_int64(n), C.byref(st)))
        return st

    def comoments(self, x: Sequence, y: Sequence, mask: Optional[Sequence] = None) -> rdf_comoments_state:
        n = len(x)
        if len(y) != n:
            raise ValueError("chunk lists differ in length")
        st = rdf_comoments_state()
        fn = self._fn("comoments")
        fn.restype = C.c_int
        self._check(fn(_flat([x], n), _flat([y], n), _flat([mask], n) if mask is not None else None, C.c_int64(n), C.byref(st)))
        return st

    def moments_merge(self, into, other):
        """into <- the state of both row sets (rdf_moments_merge / rdf_comoments_merge by the state's type); returns `into`."""
        fn = self._fn("comoments_merge" if isinstance(into, rdf_comoments_state) else "moments_merge")
        fn.restype = C.c_int
        self._check(fn(C.byref(into), C.byref(other)))
        return into

    def _stat(self, name: str, state, stat: int):
        out, some = C.c_double(0), C.c_int32(0)
        fn = self._fn(name)
        fn.restype = C.c_int
        self._check(fn(C.byref(state), C.c_int32(stat), C.byref(out), C.byref(some)))
        return out.value if some.value else None

    def moments_stat(self, state: rdf_moments_state, stat):
        """A statistic of the state ("mean", "var_pop", "var_samp", "stddev_pop", "stddev_samp", "skewness", "kurtosis"), or None."""
        return self._stat("moments_stat", state, STATS[stat] if isinstance(stat, str) else stat)

    def comoments_stat(self, state: rdf_comoments_state, stat):
        """"covar_pop", "covar_samp" or "corr" of the state, or None."""
        return self._stat("comoments_stat", state, COSTATS[stat] if isinstance(stat, str) else stat)

    # ---- expressions
    def predicate(self, expr: Expr, root: int, cols: Sequence[Sequence], outs=None):
        frame = cols if isinstance(cols, Frame) else None
        if frame is not None:
            cols = frame.cols
        nchunks = len(cols[0]) if cols else 0
        cc = None if frame is not None else _flat(cols, nchunks)
        if outs is None:
            lens = [cols[0][i].length for i in range(nchunks)]
            nullable = [any(col[i].validity is not None for col in cols) for i in range(nchunks)]
            outs, carr = self._mk_outs(BOOL, lens, nullable)
        else:
            carr = (rdf_out * max(1, nchunks))(*[o.out_struct() for o in outs])
        nodes = expr.c_array()
        if frame is not None:   # rdf_predicate_frame
            fn = self._fn("predicate_frame")
            fn.restype = C.c_int
            self._check(fn(nodes, C.c_int32(len(expr.nodes)), C.c_int32(root), frame.handle, carr))
        else:
            self._check(self._fn("predicate")(nodes, C.c_int32(len(expr.nodes)), C.c_int32(root), cc, C.c_int32(len(cols)),
                                              C.c_int64(nchunks), carr))
        return self._finish(outs, carr)

    # ---- filter / take
    def filter_count(self, mask: Sequence) -> List[int]:
        n = len(mask)
        cm = _flat([mask], n)
        counts = (C.c_int64 * max(1, n))()
        self._check(self._fn("filter_count")(cm, C.c_int64(n), counts))
        return [counts[i] for i in range(n)]

    def filter_columns(self, cols: Sequence[Sequence], mask: Sequence, outs=None):
        nchunks = len(mask)
        if outs is None:
            counts = self.filter_count(mask) if nchunks else []
            outs_all, flat = [], []
            for col in cols:
                o, _ = self._mk_outs(col[0].dtype if nchunks else F64, counts, [x.validity is not None for x in col])
                outs_all.append(o)
                flat.extend(o)
        else:
            outs_all = outs
            flat = [o for col in outs for o in col]
        carr = (rdf_out * max(1, len(flat)))(*[o.out_struct() for o in flat])
        cc = _flat(cols, nchunks)
        cm = _flat([mask], nchunks)
        self._check(self._fn("filter_columns")(cc, C.c_int32(len(cols)), cm, C.c_int64(nchunks), carr))
        self._finish(flat, carr)
        return outs_all

    def filter_pipeline(self, expr: Expr, root: int, cols: Sequence[Sequence], outs=None):
        """DataFrame::filter over host-resident batches in one streamed call (rdf_filter_pipeline): -> outs[c][i] = kept rows of batch i."""
        nchunks = len(cols[0]) if cols else 0
        if outs is None:
            outs = [[HostArray.empty_out(col[i].dtype, col[i].length, col[i].validity is not None) for i in range(nchunks)] for col in cols]
        flat = [o for col in outs for o in col]
        carr = (rdf_out * max(1, len(flat)))(*[o.out_struct() for o in flat])
        nodes = expr.c_array()
        fn = self._fn("filter_pipeline")
        fn.restype = C.c_int
        self._check(fn(nodes, C.c_int32(len(expr.nodes)), C.c_int32(root), _flat(cols, nchunks), C.c_int32(len(cols)), C.c_int64(nchunks), carr))
        self._finish(flat, carr)
        return outs

    def filter(self, col: Sequence, mask: Sequence, outs=None):
        nchunks = len(mask)
        if outs is None:
            counts = self.filter_count(mask) if nchunks else []
            outs, carr = self._mk_outs(col[0].dtype if nchunks else F64, counts, [x.validity is not None for x in col])
        else:
            carr = (rdf_out * max(1, nchunks))(*[o.out_struct() for o in outs])
        self._check(self._fn("filter")(_flat([col], nchunks), _flat([mask], nchunks), C.c_int64(nchunks), carr))
        return self._finish(outs, carr)

    def take(self, chunks: Sequence, indices, out=None):
        n = len(chunks)
        nullable = indices.validity is not None or any(c.validity is not None for c in chunks)
        if out is None:
            out = HostArray.empty_out(chunks[0].dtype, indices.length, nullable)
        carr = (rdf_out * 1)(out.out_struct())
        idx = (rdf_array * 1)(indices.c_struct())
        self._check(self._fn("take")(_flat([chunks], n), C.c_int64(n), idx, carr))
        return self._finish([out], carr)[0]

    def take_columns(self, cols: Sequence[Sequence], indices, outs=None):
        """DataFrame::take's per-column loop as one gather pass: cols[c][chunk] -> one array per column."""
        nchunks = len(cols[0])
        if outs is None:
            outs = [HostArray.empty_out(col[0].dtype, indices.length, indices.validity is not None or any(c.validity is not None for c in col)) for col in cols]
        carr = (rdf_out * len(cols))(*[o.out_struct() for o in outs])
        idx = (rdf_array * 1)(indices.c_struct())
        fn = self._fn("take_columns")
        fn.restype = C.c_int
        self._check(fn(_flat(cols, nchunks), C.c_int32(len(cols)), C.c_int64(nchunks), idx, carr))
        return self._finish(outs, carr)

    # ---- frame-level operators (a frame in, a frame out; nothing per batch on the host)
    def _new_frame(self, fn_name, *args):
        h = C.c_void_p(0)
        fn = self._fn(fn_name)
        fn.restype = C.c_int
        self._check(fn(*args, C.byref(h)))
        return Frame(self, h)

    def filter_frame(self, frame, expr: "Expr", root: int) -> "Frame":
        return self._new_frame("filter_frame", frame.handle, expr.c_array(), C.c_int32(len(expr.nodes)), C.c_int32(root))

    def take_frame(self, frame, indices) -> "Frame":
        return self._new_frame("take_frame", frame.handle, (rdf_array * 1)(indices.c_struct()))

    def sort_frame(self, frame, sort_cols: Sequence[int], descending: Sequence[bool], out_indices=None, want_frame=True):
        """-> (sorted frame or None, out_indices)."""
        sc = (C.c_int32 * len(sort_cols))(*sort_cols)
        opts = (rdf_sort_options * len(sort_cols))(*[rdf_sort_options(int(d), 0) for d in descending])
        carr = (rdf_out * 1)(out_indices.out_struct()) if out_indices is not None else None
        h = C.c_void_p(0)
        fn = self._fn("sort_frame")
        fn.restype = C.c_int
        self._check(fn(frame.handle, sc, C.c_int32(len(sort_cols)), opts, carr, C.byref(h) if want_frame else None))
        if out_indices is not None:
            out_indices.length = carr[0].length
        return (Frame(self, h) if want_frame else None), out_indices

    def groupby_agg_frame(self, frame, key_cols: Sequence[int], value_col: int, agg, max_groups: int) -> "Frame":
        code = self.AGGS[agg] if isinstance(agg, str) else int(agg)
        kc = (C.c_int32 * len(key_cols))(*key_cols)
        return self._new_frame("groupby_agg_frame", frame.handle, kc, C.c_int32(len(key_cols)), C.c_int32(value_col), C.c_int32(code), C.c_int64(max_groups))

    # ---- sort (DataFrame::sort -> lexsort_to_indices)
    def sort_to_indices(self, cols: Sequence[Sequence], descending: Sequence[bool], out=None):
        nchunks = len(cols[0])
        n = sum(a.length for a in cols[0])
        if out is None:
            out = HostArray.empty_out(U32, n, False)
        opts = (rdf_sort_options * len(cols))(*[rdf_sort_options(int(d), 0) for d in descending])
        carr = (rdf_out * 1)(out.out_struct())
        self._check(self._fn("sort_to_indices")(_flat(cols, nchunks), C.c_int32(len(cols)), C.c_int64(nchunks), opts, carr))
        return self._finish([out], carr)[0]

    def lexsort_to_indices(self, keys: Sequence, out=None):
        """DataFrame::sort over numeric and Utf8 criteria (rdf_lexsort_to_indices).  keys[k] = (chunks, descending): the
        chunks are HostArray / DeviceArray (numeric) or HostUtf8 / DeviceUtf8 (Utf8), one kind per key; key 0 is the most
        significant.  -> ONE UInt32 array of row numbers over the concatenation of the chunks."""
        keys = [(k, False) if not isinstance(k, tuple) else k for k in keys]
        nchunks = len(keys[0][0]) if keys else 0
        first = keys[0][0] if keys else []
        n = sum(c.length for c in first)
        if out is None:
            out = HostArray.empty_out(U32, n, False)
        ck = (rdf_sort_key * max(1, len(keys)))()
        keep = []
        for i, (chunks, desc) in enumerate(keys):
            utf8 = len(chunks) > 0 and all(isinstance(c, (HostUtf8, DeviceUtf8)) for c in chunks)
            if utf8:
                arr = (rdf_utf8_array * max(1, len(chunks)))(*[c.c_struct() for c in chunks])
                ck[i] = rdf_sort_key(None, C.cast(arr, C.POINTER(rdf_utf8_array)), rdf_sort_options(int(desc), 0))
            else:
                arr = (rdf_array * max(1, len(chunks)))(*[c.c_struct(getattr(c, "_unknown_nc", False)) for c in chunks])
                ck[i] = rdf_sort_key(C.cast(arr, C.POINTER(rdf_array)), None, rdf_sort_options(int(desc), 0))
            keep.append(arr)
        carr = (rdf_out * 1)(out.out_struct())
        fn = self._fn("lexsort_to_indices")
        fn.restype = C.c_int
        self._check(fn(ck if keys else None, C.c_int32(len(keys)), C.c_int64(nchunks), carr))
        return self._finish([out], carr)[0]

    # ---- join (calc_equijoin_indices)
    JOIN_TYPES = {"left": 0, "right": 1, "inner": 2, "full": 3}

    def equijoin_indices(self, left_keys: Sequence, right_keys: Sequence, how: str, outs=None):
        """-> (left_indices, right_indices): UInt32 arrays with None where a side has no partner.  `outs` = caller-allocated
        (left, right) outputs (device-resident runs): the sizing call is skipped."""
        jt = self.JOIN_TYPES[how]
        rows = C.c_int64(0)
        lk, rk = _flat([left_keys], len(left_keys)), _flat([right_keys], len(right_keys))
        if outs is not None:
            ol, orr = outs
            cl, cr = (rdf_out * 1)(ol.out_struct()), (rdf_out * 1)(orr.out_struct())
            self._check(self._fn("equijoin_indices")(lk, C.c_int64(len(left_keys)), rk, C.c_int64(len(right_keys)), C.c_int32(jt), cl, cr, C.byref(rows)))
            ol.length = orr.length = rows.value
            return ol, orr
        self._check(self._fn("equijoin_indices")(lk, C.c_int64(len(left_keys)), rk, C.c_int64(len(right_keys)), C.c_int32(jt), None, None, C.byref(rows)))
        ol, orr = HostArray.empty_out(U32, rows.value, True), HostArray.empty_out(U32, rows.value, True)
        cl, cr = (rdf_out * 1)(ol.out_struct()), (rdf_out * 1)(orr.out_struct())
        self._check(self._fn("equijoin_indices")(lk, C.c_int64(len(left_keys)), rk, C.c_int64(len(right_keys)), C.c_int32(jt), cl, cr, C.byref(rows)))
        self._finish([ol], cl)
        self._finish([orr], cr)
        return ol, orr

    def equijoin_indices_multi(self, left_cols: Sequence[Sequence], right_cols: Sequence[Sequence], how: str):
        """Several key columns per side: left_cols[k][chunk] pairs with right_cols[k][chunk]."""
        jt = self.JOIN_TYPES[how]
        rows = C.c_int64(0)
        nk, lnc, rnc = len(left_cols), len(left_cols[0]), len(right_cols[0])
        lk, rk = _flat(left_cols, lnc), _flat(right_cols, rnc)
        fn = self._fn("equijoin_indices_multi")
        self._check(fn(lk, C.c_int64(lnc), rk, C.c_int64(rnc), C.c_int32(nk), C.c_int32(jt), None, None, C.byref(rows)))
        ol, orr = HostArray.empty_out(U32, rows.value, True), HostArray.empty_out(U32, rows.value, True)
        cl, cr = (rdf_out * 1)(ol.out_struct()), (rdf_out * 1)(orr.out_struct())
        self._check(fn(lk, C.c_int64(lnc), rk, C.c_int64(rnc), C.c_int32(nk), C.c_int32(jt), cl, cr, C.byref(rows)))
        self._finish([ol], cl)
        self._finish([orr], cr)
        return ol, orr

    # ---- group-by (Transformation::GroupAggregate with one integer key; SQL semantics)
    def groupby_sum(self, keys: Sequence, values: Optional[Sequence], max_groups: int, outs=None):
        """-> (keys, sums, counts) as three one-chunk arrays in unspecified group order."""
        n = len(keys)
        kdt = keys[0].dtype
        sdt = F64 if values is not None and values[0].dtype in (F32, F64) else I64
        if outs is None:
            cap = max_groups + 2
            outs = (HostArray.empty_out(kdt, cap, any(k.validity is not None for k in keys)),
                    HostArray.empty_out(sdt, cap, False), HostArray.empty_out(I64, cap, False))
        carr = [(rdf_out * 1)(o.out_struct()) for o in outs]
        cv = _flat([values], n) if values is not None else None
        self._check(self._fn("groupby_sum")(_flat([keys], n), cv, C.c_int64(n), C.c_int64(max_groups), carr[0], carr[1], carr[2]))
        for o, cc in zip(outs, carr):
            o.length = cc[0].length
            o.null_count = cc[0].null_count
        return outs

    AGGS = {"sum": 0, "min": 1, "max": 2, "count": 3}

    @staticmethod
    def _agg_out_dtype(agg: int, vdt) -> int:
        if vdt is None:
            return I64
        if vdt in (F32, F64):
            return F64
        return U64 if (agg in (1, 2) and vdt == U64) else I64

    def groupby_agg(self, key_cols: Sequence[Sequence], values: Optional[Sequence], agg, max_groups: int, outs=None):
        """GroupAggregate(groups, [agg]) over 1..4 grouping columns: key_cols[k][chunk].  -> ([key arrays], values, counts)."""
        code = self.AGGS[agg] if isinstance(agg, str) else int(agg)
        nk, n = len(key_cols), len(key_cols[0])
        vdt = values[0].dtype if values is not None and code != 3 else None
        if outs is None:
            cap = max_groups + 2
            nullable_v = values is not None and any(v.validity is not None for v in values)
            outs = ([HostArray.empty_out(col[0].dtype, cap, any(k.validity is not None for k in col)) for col in key_cols],
                    HostArray.empty_out(self._agg_out_dtype(code, vdt), cap, nullable_v and code in (1, 2)), HostArray.empty_out(I64, cap, False))
        ok, ov, oc = outs
        ck = (rdf_out * nk)(*[o.out_struct() for o in ok])
        cv, cc = (rdf_out * 1)(ov.out_struct()), (rdf_out * 1)(oc.out_struct())
        cvals = _flat([values], n) if values is not None else None
        self._check(self._fn("groupby_agg")(_flat(key_cols, n), C.c_int32(nk), cvals, C.c_int64(n), C.c_int32(code), C.c_int64(max_groups), ck, cv, cc))
        for i, o in enumerate(ok):
            o.length, o.null_count = ck[i].length, ck[i].null_count
        ov.length, ov.null_count = cv[0].length, cv[0].null_count
        oc.length, oc.null_count = cc[0].length, cc[0].null_count
        return ok, ov, oc

    def groupby_merge(self, keys, partial, counts, agg, max_groups: int, outs=None):
        """(key, partial aggregate, count) triples (one array each) -> one row per key.  -> (keys, values, counts)."""
        code = self.AGGS[agg] if isinstance(agg, str) else int(agg)
        if outs is None:
            cap = max_groups + 2
            outs = (HostArray.empty_out(keys.dtype, cap, keys.validity is not None),
                    HostArray.empty_out(partial.dtype if partial is not None else I64, cap, code in (1, 2)), HostArray.empty_out(I64, cap, False))
        carr = [(rdf_out * 1)(o.out_struct()) for o in outs]
        ck = (rdf_array * 1)(keys.c_struct())
        cp = (rdf_array * 1)(partial.c_struct()) if partial is not None else None
        cc = (rdf_array * 1)(counts.c_struct())
        self._check(self._fn("groupby_merge")(ck, cp, cc, C.c_int32(code), C.c_int64(max_groups), carr[0], carr[1], carr[2]))
        for o, c_ in zip(outs, carr):
            o.length, o.null_count = c_[0].length, c_[0].null_count
        return outs

    def group_exchange_pack(self, keys, partial, counts, world: int, packed_ptr: int) -> List[int]:
        """Device-resident partial groups -> `packed_ptr` ([n][3] int64 words grouped by owning rank); returns rows per rank."""
        oc = (C.c_int64 * world)()
        fn = self._fn("group_exchange_pack")
        fn.restype = C.c_int
        self._check(fn((rdf_array * 1)(keys.c_struct()), (rdf_array * 1)(partial.c_struct()), (rdf_array * 1)(counts.c_struct()),
                       C.c_int32(world), C.c_void_p(packed_ptr), oc))
        return [oc[r] for r in range(world)]

    def group_exchange_unpack(self, packed_ptr: int, n: int, keys, partial, counts):
        fn = self._fn("group_exchange_unpack")
        fn.restype = C.c_int
        carr = [(rdf_out * 1)(o.out_struct()) for o in (keys, partial, counts)]
        self._check(fn(C.c_void_p(packed_ptr), C.c_int64(n), carr[0], carr[1], carr[2]))
        for o in (keys, partial, counts):
            o.length = n
        return keys, partial, counts

    def row_exchange_pack(self, keys, values, world: int, packed_ptr: int) -> List[int]:
        """Device-resident ROWS (key, value) -> `packed_ptr` ([n][2] int64 words grouped by owning rank); returns rows per rank."""
        oc = (C.c_int64 * world)()
        fn = self._fn("row_exchange_pack")
        fn.restype = C.c_int
        self._check(fn((rdf_array * 1)(keys.c_struct()), (rdf_array * 1)(values.c_struct()), C.c_int32(world), C.c_void_p(packed_ptr), oc))
        return [oc[r] for r in range(world)]

    def row_exchange_unpack(self, packed_ptr: int, n: int, keys, values):
        fn = self._fn("row_exchange_unpack")
        fn.restype = C.c_int
        carr = [(rdf_out * 1)(o.out_struct()) for o in (keys, values)]
        self._check(fn(C.c_void_p(packed_ptr), C.c_int64(n), carr[0], carr[1]))
        for o in (keys, values):
            o.length = n
        return keys, values

    # ---- ArrayFunctions over List<primitive> (src/functions/array.rs)
    def _scalar(self, value, dtype: int):
        return np.array([value], dtype=NP_OF.get(dtype, np.int64))   # an unsupported child dtype is the library's to reject

    def list_contains(self, lst, value, out=None):
        out = out if out is not None else HostArray.empty_out(BOOL, lst.length, True)
        carr = (rdf_out * 1)(out.out_struct())
        v = self._scalar(value, lst.values.dtype)
        self._check(self._fn("list_contains")(C.byref(lst.c_struct()), C.c_void_p(v.ctypes.data), carr))
        return self._finish([out], carr)[0]

    def list_position(self, lst, value, out=None):
        out = out if out is not None else HostArray.empty_out(I32, lst.length, False)
        carr = (rdf_out * 1)(out.out_struct())
        v = self._scalar(value, lst.values.dtype)
        self._check(self._fn("list_position")(C.byref(lst.c_struct()), C.c_void_p(v.ctypes.data), carr))
        return self._finish([out], carr)[0]

    def list_extreme(self, lst, want_max: bool, out=None):
        out = out if out is not None else HostArray.empty_out(lst.values.dtype, lst.length, True)
        carr = (rdf_out * 1)(out.out_struct())
        self._check(self._fn("list_max" if want_max else "list_min")(C.byref(lst.c_struct()), carr))
        return self._finish([out], carr)[0]

    def list_remove(self, lst, value, outs=None):
        """-> (offsets int32 [rows + 1], values)"""
        oo, ov = outs if outs is not None else (HostArray.empty_out(I32, lst.length + 1, False),
                                                HostArray.empty_out(lst.values.dtype, max(1, lst.values.length), False))
        co, cv = (rdf_out * 1)(oo.out_struct()), (rdf_out * 1)(ov.out_struct())
        v = self._scalar(value, lst.values.dtype)
        self._check(self._fn("list_remove")(C.byref(lst.c_struct()), C.c_void_p(v.ctypes.data), co, cv))
        self._finish([oo], co)
        self._finish([ov], cv)
        return oo, ov

    def list_set(self, op: str, lst, other=None, count: int = 0, outs=None):
        """array_distinct / array_except / array_intersect / array_union / array_repeat -> (offsets int32 [rows + 1], values)"""
        cap = {"distinct": lst.values.length, "except": lst.values.length, "intersect": lst.values.length,
               "union": lst.values.length + (other.values.length if other is not None else 0),
               "repeat": lst.values.length * max(0, count)}[op]
        oo, ov = outs if outs is not None else (HostArray.empty_out(I32, lst.length + 1, False),
                                                HostArray.empty_out(lst.values.dtype, max(1, cap), False))
        co, cv = (rdf_out * 1)(oo.out_struct()), (rdf_out * 1)(ov.out_struct())
        fn = self._fn("list_" + op)
        if op == "distinct":
            st = fn(C.byref(lst.c_struct()), co, cv)
        elif op == "repeat":
            st = fn(C.byref(lst.c_struct()), C.c_int32(count), co, cv)
        else:
            st = fn(C.byref(lst.c_struct()), C.byref(other.c_struct()) if other is not None else None, co, cv)
        self._check(st)
        self._finish([oo], co)
        self._finish([ov], cv)
        return oo, ov

    def list_sort(self, lst, out=None):
        ov = out if out is not None else HostArray.empty_out(lst.values.dtype, max(1, lst.values.length), False)
        cv = (rdf_out * 1)(ov.out_struct())
        self._check(self._fn("list_sort")(C.byref(lst.c_struct()), cv))
        return self._finish([ov], cv)[0]

    # ---- Utf8 columns (Column::filter / Column::take, the string ScalarFunctions); bound lazily: only the product has them
    def _utf8_fn(self, name):
        fn = self._fn(name)
        fn.restype = C.c_int
        return fn

    @staticmethod
    def _utf8_outs(chunks, rows_out, nullable, device: bool, caps=None):
        """Output buffers for one call: offsets of rows + 1 entries, data of caps[i] bytes (0: the sizing call)."""
        outs, keep = [], []
        for i, (r, nl) in enumerate(zip(rows_out, nullable)):
            cap = caps[i] if caps is not None else 0
            if device:
                import torch
                ot = torch.zeros(r + 1, dtype=torch.int32, device="cuda")
                vt = torch.zeros(((r + 63) // 64) * 8 + 8, dtype=torch.uint8, device="cuda") if nl else None
                dt = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda") if cap else None
                o_off = rdf_out(ot.data_ptr(), vt.data_ptr() if vt is not None else None, r + 1, 0, 0, I32, MEM_DEVICE)
                o_dat = rdf_out(dt.data_ptr() if dt is not None else None, None, cap, 0, 0, U8, MEM_DEVICE)
                keep.append((ot, dt, vt))
            else:
                ob = np.zeros(r + 1, dtype=np.int32)
                vb = np.zeros(((r + 63) // 64) * 8 + 8, dtype=np.uint8) if nl else None
                db = np.zeros(max(cap, 1), dtype=np.uint8) if cap else None
                o_off = rdf_out(ob.ctypes.data, vb.ctypes.data if vb is not None else None, r + 1, 0, 0, I32, MEM_HOST)
                o_dat = rdf_out(db.ctypes.data if db is not None else None, None, cap, 0, 0, U8, MEM_HOST)
                keep.append((ob, db, vb))
            outs.append((o_off, o_dat))
        co = (rdf_out * max(1, len(outs)))(*[o[0] for o in outs])
        cd = (rdf_out * max(1, len(outs)))(*[o[1] for o in outs])
        return co, cd, keep

    def _utf8_run(self, call, chunks, rows_out, nullable, as_arrow=False):
        """The sizing call, then the call into exactly sized buffers -> one HostUtf8 / DeviceUtf8 per output chunk
        (python lists / pyarrow arrays with as_arrow="pylist" / True)."""
        device = any(isinstance(c, (DeviceUtf8, DeviceArray)) for c in chunks)   # (rdf_utf8_format: the inputs are value chunks)
        co, cd, keep = self._utf8_outs(chunks, rows_out, nullable, device)
        st = call(co, cd)
        if st not in (RDF_OK, RDF_MEMORY_ERROR):
            self._check(st)
        if st == RDF_MEMORY_ERROR and all(cd[i].capacity >= cd[i].length for i in range(len(rows_out))):
            self._check(st)   # not the data buffers: a genuine error
        caps = [cd[i].length for i in range(len(rows_out))]
        if st == RDF_MEMORY_ERROR:
            co, cd, keep = self._utf8_outs(chunks, rows_out, nullable, device, caps)
            self._check(call(co, cd))
        res = []
        for i in range(len(rows_out)):
            rows = co[i].length - 1
            if device:
                ot, dt, vt = keep[i]
                r = DeviceUtf8(ot.data_ptr(), dt.data_ptr() if dt is not None else 0, cd[i].length, rows,
                               vt.data_ptr() if vt is not None else None, 0, 0, co[i].null_count, keep=(ot, dt, vt))
            else:
                ob, db, vb = keep[i]
                r = HostUtf8(ob, db if db is not None else np.zeros(8, dtype=np.uint8), vb, 0, rows, 0, co[i].null_count)
            if as_arrow:
                h = r.to_host() if device else r
                r = h.to_pylist() if as_arrow == "pylist" else h.to_arrow()
            res.append(r)
        return res

    def utf8_filter(self, chunks: Sequence, mask: Sequence, as_arrow=False):
        """Column::filter over StringArray chunks: one result per chunk."""
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        marr = _flat([mask], n)
        fn = self._utf8_fn("utf8_filter")
        return self._utf8_run(lambda co, cd: fn(carr, marr, C.c_int64(n), co, cd), chunks,
                              [c.length for c in chunks], [c.validity is not None if isinstance(c, HostUtf8) else bool(c.validity_ptr) for c in chunks], as_arrow)

    def utf8_take(self, chunks: Sequence, indices, as_arrow=False):
        """Column::take: ONE result chunk of indices.length rows."""
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        idx = (rdf_array * 1)(indices.c_struct())
        nullable = indices.validity is not None or any((c.validity is not None) if isinstance(c, HostUtf8) else bool(c.validity_ptr) for c in chunks)
        fn = self._utf8_fn("utf8_take")
        return self._utf8_run(lambda co, cd: fn(carr, C.c_int64(n), idx, co, cd), chunks, [indices.length], [nullable], as_arrow)[0]

    def utf8_unary(self, op: str, chunks: Sequence, pos: int = 0, length: int = 0, as_arrow=False):
        """trim / ltrim / rtrim / substring(pos, length) / lower / upper: one result per chunk."""
        if op not in UTF8_UNARY:
            raise ValueError(f"unknown Utf8 function {op!r}")
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        fn = self._utf8_fn("utf8_" + op)
        if op == "substring":
            call = lambda co, cd: fn(carr, C.c_int64(n), C.c_int64(pos), C.c_int64(length), co, cd)  # noqa: E731
        else:
            call = lambda co, cd: fn(carr, C.c_int64(n), co, cd)  # noqa: E731
        return self._utf8_run(call, chunks, [c.length for c in chunks],
                              [c.validity is not None if isinstance(c, HostUtf8) else bool(c.validity_ptr) for c in chunks], as_arrow)

    # ---- Utf8 predicates and measures: masks and integers from text (rdf_utf8_predicate / _compare / _measure)
    @staticmethod
    def _utf8_nullable(c) -> bool:
        return c.validity is not None if isinstance(c, HostUtf8) else bool(c.validity_ptr)

    def _utf8_pred_outs(self, dtype: int, chunks: Sequence, nullable: Sequence[bool], outs):
        if outs is None:
            device = any(isinstance(c, DeviceUtf8) for c in chunks)
            outs = [self._window_out(dtype, c.length, device, nl) for c, nl in zip(chunks, nullable)]
        return outs, (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])

    @staticmethod
    def _utf8_pattern(pattern):
        raw = b"" if pattern is None else (pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern))
        return raw, (C.c_uint8 * max(1, len(raw))).from_buffer_copy(raw or b"\0")

    def utf8_predicate(self, op, chunks: Sequence, pattern, escape=None, outs=None):
        """rdf_utf8_predicate: every row against a literal or a LIKE pattern (a name of UTF8_PRED_OPS or its code; `pattern`
        is str, encoded as UTF-8, or bytes; `escape` a one-character str, a byte value or None) -> one Boolean array per chunk."""
        code = UTF8_PRED_OPS[op] if isinstance(op, str) else int(op)
        esc = -1 if escape is None else (escape if isinstance(escape, (int, np.integer)) else ord(escape))
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        raw, cp = self._utf8_pattern(pattern)
        outs, co = self._utf8_pred_outs(BOOL, chunks, [self._utf8_nullable(c) for c in chunks], outs)
        self._check(self._utf8_fn("utf8_predicate")(C.c_int32(code), carr, C.c_int64(n), cp, C.c_int64(len(raw)), C.c_int32(int(esc)), co))
        return self._finish(outs, co)

    def utf8_compare(self, op, a: Sequence, b: Sequence, outs=None):
        """rdf_utf8_compare: column against column, one of the six comparisons -> one Boolean array per chunk."""
        code = UTF8_PRED_OPS[op] if isinstance(op, str) else int(op)
        n = len(a)
        if len(b) != n:
            raise ValueError("chunk lists differ in length")
        ca = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in a])
        cb = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in b])
        outs, co = self._utf8_pred_outs(BOOL, a, [self._utf8_nullable(x) or self._utf8_nullable(y) for x, y in zip(a, b)], outs)
        self._check(self._utf8_fn("utf8_compare")(C.c_int32(code), ca, cb, C.c_int64(n), co))
        return self._finish(outs, co)

    def utf8_measure(self, what, chunks: Sequence, pattern=None, pos: int = 1, outs=None):
        """rdf_utf8_measure: "length" (code points), "octet_length" (bytes) or "locate" (1-based code-point position of
        `pattern` at or after `pos`, 0 = none; instr is pos = 1) -> one Int32 array per chunk."""
        code = UTF8_MEASURE_OPS[what] if isinstance(what, str) else int(what)
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        raw, cp = self._utf8_pattern(pattern)
        outs, co = self._utf8_pred_outs(I32, chunks, [self._utf8_nullable(c) for c in chunks], outs)
        self._check(self._utf8_fn("utf8_measure")(C.c_int32(code), carr, C.c_int64(n), cp, C.c_int64(len(raw)), C.c_int64(int(pos)), co))
        return self._finish(outs, co)

    # ---- Utf8 builders: text columns made of more than one source (rdf_utf8_concat / _pad / _repeat / _reverse / _substring_index)
    def utf8_build_call(self, op: str, chunks, *args):
        """-> (call(out_offsets, out_data) -> status, the column chunks that give the row counts, nullable per chunk) of one
        builder call; utf8_build runs it under the sizing rule, tests call it with buffers of their own.
          ("concat", parts) / ("concat_ws", parts, sep): parts = chunk lists and str / bytes literals (chunks = None)
          ("lpad" | "rpad", chunks, len, pad), ("repeat", chunks, times), ("reverse", chunks), ("substring_index", chunks, delim, count)"""
        if op in ("concat", "concat_ws"):
            parts = args[0]
            raw, cp = self._utf8_pattern(args[1] if op == "concat_ws" else None)
            cols = [p for p in parts if not isinstance(p, (str, bytes, bytearray))]
            n = len(cols[0]) if cols else 0
            keep, cparts = [raw, cp], (rdf_utf8_part * max(1, len(parts)))()
            for k, p in enumerate(parts):
                if isinstance(p, (str, bytes, bytearray)):
                    lraw, lp = self._utf8_pattern(p)
                    keep.append(lp)
                    cparts[k] = rdf_utf8_part(None, C.cast(lp, C.POINTER(C.c_uint8)), len(lraw))
                else:
                    if len(p) != n:
                        raise ValueError("chunk lists differ in length")
                    carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in p])
                    keep.append(carr)
                    cparts[k] = rdf_utf8_part(carr, None, 0)
            fn = self._utf8_fn("utf8_concat")
            ws = op == "concat_ws"
            call = lambda co, cd, keep=keep: fn(cparts, C.c_int32(len(parts)), C.c_int64(n), C.c_int32(int(ws)), cp, C.c_int64(len(raw)), co, cd)  # noqa: E731
            nullable = [False if ws else any(self._utf8_nullable(col[i]) for col in cols) for i in range(n)]
            return call, (cols[0] if cols else []), nullable
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        nullable = [self._utf8_nullable(c) for c in chunks]
        if op in ("lpad", "rpad"):
            raw, cp = self._utf8_pattern(args[1])
            fn = self._utf8_fn("utf8_pad")
            call = lambda co, cd: fn(C.c_int32(int(op == "rpad")), carr, C.c_int64(n), C.c_int64(int(args[0])), cp, C.c_int64(len(raw)), co, cd)  # noqa: E731
        elif op == "repeat":
            fn = self._utf8_fn("utf8_repeat")
            call = lambda co, cd: fn(carr, C.c_int64(n), C.c_int64(int(args[0])), co, cd)  # noqa: E731
        elif op == "reverse":
            fn = self._utf8_fn("utf8_reverse")
            call = lambda co, cd: fn(carr, C.c_int64(n), co, cd)  # noqa: E731
        elif op == "substring_index":
            raw, cp = self._utf8_pattern(args[0])
            fn = self._utf8_fn("utf8_substring_index")
            call = lambda co, cd: fn(carr, C.c_int64(n), cp, C.c_int64(len(raw)), C.c_int64(int(args[1])), co, cd)  # noqa: E731
        else:
            raise ValueError(f"unknown Utf8 builder {op!r}")
        return call, chunks, nullable

    def utf8_build(self, op: str, chunks, *args, as_arrow=False):
        """One builder call under the sizing rule (the sizing call, then the call into exactly sized buffers): one result per
        chunk.  Arguments as for utf8_build_call."""
        call, shape, nullable = self.utf8_build_call(op, chunks, *args)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    def utf8_concat(self, parts: Sequence, sep=None, as_arrow=False):
        """concat (sep is None) / concat_ws of chunk lists and str / bytes literals."""
        return self.utf8_build("concat", None, parts, as_arrow=as_arrow) if sep is None else self.utf8_build("concat_ws", None, parts, sep, as_arrow=as_arrow)

    # ---- regular expressions over Utf8 (rdf_utf8_regexp_info / _match / _count / _extract / _replace / _split): Spark 3's
    # rlike, regexp_count, regexp_extract(s, p, 0), regexp_replace and split with a regular expression.  `pattern` is str
    # (encoded as UTF-8) or bytes; a pattern the library does not take raises with the construct and its byte position.
    def utf8_regexp_info(self, pattern) -> dict:
        """rdf_utf8_regexp_info (host only, needs no device): the sizes the caps are defined on."""
        raw, cp = self._utf8_pattern(pattern)
        info = rdf_regexp_info()
        self._check(self._utf8_fn("utf8_regexp_info")(cp, C.c_int64(len(raw)), C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in rdf_regexp_info._fields_}

    def _utf8_regexp_measure(self, name, dtype, chunks, pattern, outs):
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        raw, cp = self._utf8_pattern(pattern)
        outs, co = self._utf8_pred_outs(dtype, chunks, [self._utf8_nullable(c) for c in chunks], outs)
        self._check(self._utf8_fn(name)(carr, C.c_int64(n), cp, C.c_int64(len(raw)), co))
        return self._finish(outs, co)

    def utf8_regexp_match(self, chunks: Sequence, pattern, outs=None):
        """rlike: a match exists anywhere in the row -> one Boolean array per chunk."""
        return self._utf8_regexp_measure("utf8_regexp_match", BOOL, chunks, pattern, outs)

    def utf8_regexp_count(self, chunks: Sequence, pattern, outs=None):
        """regexp_count: the matches Matcher.find finds -> one Int32 array per chunk."""
        return self._utf8_regexp_measure("utf8_regexp_count", I32, chunks, pattern, outs)

    def utf8_regexp_extract_call(self, chunks: Sequence, pattern, group: int = 0):
        return self._utf8_rewrite_call("utf8_regexp_extract", chunks, [pattern], (C.c_int32(int(group)),))

    def utf8_regexp_replace_call(self, chunks: Sequence, pattern, replacement):
        return self._utf8_rewrite_call("utf8_regexp_replace", chunks, [pattern, replacement])

    def utf8_regexp_split_call(self, chunks: Sequence, pattern, limit: int = -1):
        return self._utf8_rewrite_call("utf8_regexp_split", chunks, [pattern], (C.c_int64(int(limit)),))

    def utf8_regexp_extract(self, chunks: Sequence, pattern, group: int = 0, as_arrow=False):
        """regexp_extract(row, pattern, 0): the first match's bytes, '' when there is none; group != 0 is refused."""
        call, shape, nullable = self.utf8_regexp_extract_call(chunks, pattern, group)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    def utf8_regexp_replace(self, chunks: Sequence, pattern, replacement, as_arrow=False):
        """regexp_replace(row, pattern, replacement): every match replaced; in the replacement \\x stands for x."""
        call, shape, nullable = self.utf8_regexp_replace_call(chunks, pattern, replacement)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    def utf8_regexp_split(self, chunks: Sequence, pattern, limit: int = -1, as_arrow=False):
        """split(row, regex, limit) as String.split -> what utf8_split returns."""
        return self._utf8_split_run(self.utf8_regexp_split_call(chunks, pattern, limit), chunks, as_arrow)

    # ---- Utf8 rewrites: a row's content changed by what it holds (rdf_utf8_replace / _translate / _initcap / _split)
    def _utf8_rewrite_call(self, name, chunks, lits, tail=()):
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        args = []
        for lit in lits:
            raw, cp = self._utf8_pattern(lit)
            args += [cp, C.c_int64(len(raw))]
        fn = self._utf8_fn(name)
        call = lambda *outs, keep=(carr, args): fn(carr, C.c_int64(n), *args, *tail, *outs)  # noqa: E731
        return call, chunks, [self._utf8_nullable(c) for c in chunks]

    def utf8_replace_call(self, chunks: Sequence, search, replacement):
        """-> (call(out_offsets, out_data) -> status, chunks, nullable per chunk), as utf8_build_call returns them."""
        return self._utf8_rewrite_call("utf8_replace", chunks, [search, replacement])

    def utf8_translate_call(self, chunks: Sequence, matching, replace):
        return self._utf8_rewrite_call("utf8_translate", chunks, [matching, replace])

    def utf8_initcap_call(self, chunks: Sequence):
        return self._utf8_rewrite_call("utf8_initcap", chunks, [])

    def utf8_split_call(self, chunks: Sequence, delim, limit: int = -1):
        """-> (call(out_list_offsets, out_offsets, out_data) -> status, chunks, nullable per chunk)"""
        return self._utf8_rewrite_call("utf8_split", chunks, [delim], (C.c_int64(int(limit)),))

    def utf8_replace(self, chunks: Sequence, search, replacement, as_arrow=False):
        """replace(row, search, replacement): every non-overlapping occurrence from the left; one result per chunk."""
        call, shape, nullable = self.utf8_replace_call(chunks, search, replacement)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    def utf8_translate(self, chunks: Sequence, matching, replace, as_arrow=False):
        """translate(row, matching, replace): code point i of matching becomes code point i of replace, or is dropped."""
        call, shape, nullable = self.utf8_translate_call(chunks, matching, replace)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    def utf8_initcap(self, chunks: Sequence, as_arrow=False):
        """initcap(row): lower-cased, the first code point after every space (and the first of the row) title-cased."""
        call, shape, nullable = self.utf8_initcap_call(chunks)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    def utf8_split(self, chunks: Sequence, delim, limit: int = -1, as_arrow=False):
        """split(row, delim, limit) with a literal delimiter -> per chunk a List<Utf8> as (list, child): a HostList /
        DeviceList that holds the list offsets and validity (rdf_list_explode takes it as it is; its `values` member is the
        child's Int32 offsets array, which that call never reads) and the child HostUtf8 / DeviceUtf8 with one row per
        element (rdf_utf8_take takes it).  as_arrow=True: pyarrow ListArrays of strings ("pylist": python lists).  The
        sizing call, then the call into exactly sized buffers."""
        return self._utf8_split_run(self.utf8_split_call(chunks, delim, limit), chunks, as_arrow)

    def _utf8_split_run(self, split_call, chunks, as_arrow):
        """utf8_split's and utf8_regexp_split's shared tail: one *_split_call under the sizing rule -> what utf8_split returns"""
        call, shape, nullable = split_call
        device = any(isinstance(c, DeviceUtf8) for c in chunks)
        rows = [c.length for c in shape]

        def outs(ecaps, dcaps):
            lists = [self._window_out(I32, r + 1, device, nl) for r, nl in zip(rows, nullable)]
            offs = [self._window_out(I32, e, device, False) if e else None for e in ecaps]
            co, cd, keep = self._utf8_outs(shape, rows, [False] * len(rows), device, dcaps)
            mem = MEM_DEVICE if device else MEM_HOST
            cl = (rdf_out * max(1, len(rows)))(*[x.out_struct() for x in lists])
            ce = (rdf_out * max(1, len(rows)))(*[x.out_struct() if x is not None else rdf_out(None, None, 0, 0, 0, I32, mem) for x in offs])
            return cl, ce, cd, lists, offs, keep

        n = len(rows)
        cl, ce, cd, lists, offs, keep = outs([0] * n, [0] * n)
        st = call(cl, ce, cd)
        if st != RDF_MEMORY_ERROR:
            self._check(st)
        if n and st == RDF_MEMORY_ERROR:
            cl, ce, cd, lists, offs, keep = outs([ce[i].length for i in range(n)], [cd[i].length for i in range(n)])
            self._check(call(cl, ce, cd))
        res = []
        for i in range(n):
            elems = ce[i].length - 1
            lists[i].length = rows[i] + 1
            lists[i].null_count = cl[i].null_count
            offs[i].length = elems + 1
            if device:
                import torch
                _, dt, _ = keep[i]
                lst = DeviceList(lists[i].values_ptr, rows[i], offs[i], lists[i].validity_ptr if nullable[i] else None, 0, keep=lists[i].keep)
                child = DeviceUtf8(offs[i].values_ptr, dt.data_ptr() if dt is not None else 0, cd[i].length, elems, None, 0, 0, 0,
                                   keep=(offs[i].keep[0].view(torch.int32), dt, None))
            else:
                _, db, _ = keep[i]
                lst = HostList(lists[i].values, offs[i], lists[i].validity if nullable[i] else None, 0, rows[i])
                child = HostUtf8(offs[i].values, db if db is not None else np.zeros(8, dtype=np.uint8), None, 0, elems, 0, 0)
            if as_arrow:
                hl = lst if not device else HostList(lst.keep[0].cpu().numpy().view(np.int32).copy(), None,
                                                    lst.keep[1].cpu().numpy().copy() if nullable[i] else None, 0, rows[i])
                hc = child.to_host() if device else child
                lo = hl.offsets[:rows[i] + 1]
                valid = unpack_bits(hl.validity, 0, rows[i]) if hl.validity is not None else np.ones(rows[i], dtype=bool)
                if as_arrow == "pylist":
                    flat = hc.to_pylist()
                    res.append([flat[lo[r]:lo[r + 1]] if valid[r] else None for r in range(rows[i])])
                else:
                    import pyarrow as pa
                    mask = pa.array(~valid) if hl.validity is not None else None
                    res.append(pa.ListArray.from_arrays(pa.array(lo, type=pa.int32()), hc.to_arrow(), mask=mask))
            else:
                res.append((lst, child))
        return res

    # ---- text to values and back (rdf_utf8_parse / rdf_utf8_format)
    @staticmethod
    def _text_kind(kind, unit):
        code = TEXT_KINDS[kind] if isinstance(kind, str) else int(kind)
        return code, (TIME_SECOND if unit is None else int(unit))

    def utf8_parse(self, chunks: Sequence, kind, unit=None, pattern=None, dtype=None, outs=None):
        """rdf_utf8_parse: "bool" / "int" / "date" / "timestamp" (or the code) from text, by the kind's CAST grammar or, with
        `pattern` (str / bytes), to_date / to_timestamp / unix_timestamp -> (one array per chunk, failed rows per chunk).
        dtype: the integer dtype of an "int" call (default Int64); unit: of a "timestamp" call (default seconds)."""
        code, unit = self._text_kind(kind, unit)
        out_dt = {TEXT_BOOL: BOOL, TEXT_DATE: I32, TEXT_TIMESTAMP: I64}.get(code, I64 if dtype is None else int(dtype))
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        raw, cp = self._utf8_pattern(pattern)
        outs, co = self._utf8_pred_outs(out_dt, chunks, [True] * n, outs)
        failed = (C.c_int64 * max(1, n))()
        self._check(self._utf8_fn("utf8_parse")(carr, C.c_int64(n), C.c_int32(code), C.c_int32(unit), cp if pattern is not None else None,
                                                C.c_int64(len(raw)), co, failed))
        return self._finish(outs, co), [int(failed[i]) for i in range(n)]

    def utf8_format_call(self, chunks: Sequence, kind, unit=None, pattern=None):
        """-> (call(out_offsets, out_data) -> status, chunks, nullable per chunk) of one rdf_utf8_format call; utf8_format runs it
        under the sizing rule, tests call it with buffers of their own."""
        code, unit = self._text_kind(kind, unit)
        n = len(chunks)
        carr = _flat([chunks], n)
        raw, cp = self._utf8_pattern(pattern)
        fn = self._utf8_fn("utf8_format")
        call = lambda co, cd: fn(carr, C.c_int64(n), C.c_int32(code), C.c_int32(unit), cp if pattern is not None else None, C.c_int64(len(raw)), co, cd)  # noqa: E731
        return call, chunks, [(c.validity is not None) if isinstance(c, HostArray) else bool(c.validity_ptr) for c in chunks]

    def utf8_format(self, chunks: Sequence, kind, unit=None, pattern=None, as_arrow=False):
        """rdf_utf8_format: CAST(x AS STRING) of Boolean / integer / temporal chunks or, with `pattern`, date_format /
        from_unix_time: one Utf8 result per chunk.  unit: the time unit of temporal storage (default seconds)."""
        call, shape, nullable = self.utf8_format_call(chunks, kind, unit, pattern)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    # ---- Float32 / Float64 to and from text (rdf_utf8_parse_float / rdf_utf8_format_float)
    def _textfloat_fn(self, name):
        fn = self._utf8_fn(name)
        if name == "utf8_parse_float":
            fn.argtypes = [C.POINTER(rdf_utf8_array), C.c_int64, C.POINTER(rdf_out), C.POINTER(C.c_int64)]
        else:
            fn.argtypes = [C.POINTER(rdf_array), C.c_int64, C.POINTER(rdf_out), C.POINTER(rdf_out)]
        return fn

    def utf8_parse_float(self, chunks: Sequence, dtype=F64, outs=None):
        """rdf_utf8_parse_float: CAST(s AS FLOAT / DOUBLE), correctly rounded -> (one Float32 / Float64 array per chunk, failed
        rows per chunk).  A row that does not parse is NULL."""
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        outs, co = self._utf8_pred_outs(int(dtype), chunks, [True] * n, outs)
        failed = (C.c_int64 * max(1, n))()
        self._check(self._textfloat_fn("utf8_parse_float")(carr, C.c_int64(n), co, failed))
        return self._finish(outs, co), [int(failed[i]) for i in range(n)]

    def utf8_format_float_call(self, chunks: Sequence):
        """-> (call(out_offsets, out_data) -> status, chunks, nullable per chunk) of one rdf_utf8_format_float call;
        utf8_format_float runs it under the sizing rule, tests call it with buffers of their own."""
        n = len(chunks)
        carr = _flat([chunks], n)
        fn = self._textfloat_fn("utf8_format_float")
        call = lambda co, cd: fn(carr, C.c_int64(n), co, cd)  # noqa: E731
        return call, chunks, [(c.validity is not None) if isinstance(c, HostArray) else bool(c.validity_ptr) for c in chunks]

    def utf8_format_float(self, chunks: Sequence, as_arrow=False):
        """rdf_utf8_format_float: CAST(x AS STRING) of Float32 / Float64 chunks (Java's Double.toString): one Utf8 result per chunk."""
        call, shape, nullable = self.utf8_format_float_call(chunks)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    # ---- coalesce / case_when over text (rdf_utf8_coalesce / rdf_utf8_case_when)
    def utf8_select_call(self, parts: Sequence, conds=None):
        """-> (call(out_offsets, out_data) -> status, the first column part, nullable per chunk) of one rdf_utf8_coalesce
        (conds is None) or rdf_utf8_case_when call (parts = the branches' values, then `otherwise`, None for an absent one).
        parts: chunk lists, str / bytes literals, None for the NULL literal."""
        cols = [p for p in parts if isinstance(p, (list, tuple))]
        if not cols:
            raise ValueError("at least one part must be a column")
        n = len(cols[0])
        keep, cparts = [], (rdf_utf8_part * max(1, len(parts)))()
        for k, p in enumerate(parts):
            if p is None:
                cparts[k] = rdf_utf8_part(None, None, 0)
            elif isinstance(p, (str, bytes, bytearray)):
                lraw, lp = self._utf8_pattern(p)
                keep.append(lp)
                cparts[k] = rdf_utf8_part(None, C.cast(lp, C.POINTER(C.c_uint8)), len(lraw))
            else:
                if len(p) != n:
                    raise ValueError("chunk lists differ in length")
                carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in p])
                keep.append(carr)
                cparts[k] = rdf_utf8_part(carr, None, 0)
        can_be_null = lambda p, i: p is None or (isinstance(p, (list, tuple)) and self._utf8_nullable(p[i]))  # noqa: E731
        if conds is None:
            fn = self._utf8_fn("utf8_coalesce")
            call = lambda co, cd, keep=keep: fn(cparts, C.c_int32(len(parts)), C.c_int64(n), co, cd)  # noqa: E731
            nullable = [all(can_be_null(p, i) for p in parts) for i in range(n)]
        else:
            nb = len(parts) - 1
            if len(conds) != nb:
                raise ValueError("one value per condition")
            cc = [_flat([c], n) for c in conds]
            cptr = (C.POINTER(rdf_array) * max(1, nb))(*[C.cast(c, C.POINTER(rdf_array)) for c in cc])
            other = None if parts[nb] is None else C.byref(cparts, nb * C.sizeof(rdf_utf8_part))
            fn = self._utf8_fn("utf8_case_when")
            call = lambda co, cd, keep=(keep, cc): fn(cptr, cparts, C.c_int32(nb), other, C.c_int64(n), co, cd)  # noqa: E731
            nullable = [any(can_be_null(p, i) for p in parts) for i in range(n)]
        return call, cols[0], nullable

    def utf8_coalesce(self, parts: Sequence, as_arrow=False):
        """rdf_utf8_coalesce: per row the first part that is not NULL (chunk lists, str / bytes literals, None): one result per chunk."""
        call, shape, nullable = self.utf8_select_call(parts)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    def utf8_case_when(self, conds: Sequence, values: Sequence, otherwise=None, as_arrow=False):
        """rdf_utf8_case_when: conds[k] (RDF_BOOL chunk lists) choose values[k]; rows no condition holds for take `otherwise` (None: NULL)."""
        call, shape, nullable = self.utf8_select_call(list(values) + [otherwise], conds)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    # ---- row hashes and digests (rdf_hash_columns / rdf_utf8_digest / rdf_utf8_crc32)
    def hash_columns(self, kind, cols: Sequence[Sequence], seed: int = 42, outs=None):
        """rdf_hash_columns: Spark's hash ("hash" / "murmur3") or "xxhash64" over 1..8 columns, each a list of numeric /
        Boolean or Utf8 chunks -> one Int32 / Int64 array per chunk, never NULL."""
        code = HASH_KINDS[kind] if isinstance(kind, str) else int(kind)
        ck, keep = self._sort_keys([list(c) for c in cols])
        shape = cols[0] if len(cols) else []
        n = len(shape)
        if outs is None:
            device = any(isinstance(c, (DeviceArray, DeviceUtf8)) for c in shape)
            outs = [self._window_out(I64 if code == 1 else I32, c.length, device, False) for c in shape]
        co = (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])
        self._check(self._utf8_fn("hash_columns")(C.c_int32(code), ck, C.c_int32(len(cols)), C.c_int64(n), C.c_int64(int(seed)), co))
        return self._finish(outs, co)

    def utf8_crc32(self, chunks: Sequence, outs=None):
        """rdf_utf8_crc32: zlib's CRC-32 of every row -> one Int64 array per chunk."""
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        outs, co = self._utf8_pred_outs(I64, chunks, [self._utf8_nullable(c) for c in chunks], outs)
        self._check(self._utf8_fn("utf8_crc32")(carr, C.c_int64(n), co))
        return self._finish(outs, co)

    def utf8_digest_call(self, kind, chunks: Sequence):
        """-> (call(out_offsets, out_data) -> status, chunks, nullable per chunk) of one rdf_utf8_digest call; utf8_digest runs
        it under the sizing rule, tests call it with buffers of their own."""
        code = DIGEST_KINDS[kind] if isinstance(kind, str) else int(kind)
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        fn = self._utf8_fn("utf8_digest")
        call = lambda co, cd: fn(C.c_int32(code), carr, C.c_int64(n), co, cd)  # noqa: E731
        return call, chunks, [self._utf8_nullable(c) for c in chunks]

    def utf8_digest(self, kind, chunks: Sequence, as_arrow=False):
        """md5 / sha1 / sha224 / sha256 / sha384 / sha512 of every row as lowercase hex text: one result per chunk."""
        call, shape, nullable = self.utf8_digest_call(kind, chunks)
        return self._utf8_run(call, shape, [c.length for c in shape], nullable, as_arrow)

    # ---- Column::hist / Column::uniques (bound lazily: only the product has them)
    @staticmethod
    def _stats_out(dtype: int, capacity: int, device: bool):
        """One output array of `capacity` elements in host or device memory (device buffers padded to 64 elements)."""
        if not device:
            return HostArray.empty_out(dtype, capacity, False)
        import torch
        t = torch.zeros(((capacity + 63) // 64) * 64 + 64, dtype=torch.int64, device="cuda")
        return DeviceArray(t.data_ptr(), None, 0, capacity, dtype, 0, keep=t, capacity=capacity)

    @staticmethod
    def stats_to_numpy(arr) -> np.ndarray:
        """The logical values of an output of hist / uniques, whichever memory it lives in."""
        if isinstance(arr, HostArray):
            return arr.to_numpy().copy()
        return arr.keep.cpu().numpy().view(NP_OF[arr.dtype])[:arr.length].copy()

    def hist(self, chunks: Sequence, nbins: int, range=None, outs=None):
        """Column::hist with numpy.histogram's buckets -> (counts, edges, counted): an Int64 array of nbins, a Float64 array of
        nbins + 1 (HostArray / DeviceArray like the input; `outs` = caller-allocated (counts, edges)) and the rows counted."""
        n = len(chunks)
        device = any(isinstance(c, DeviceArray) for c in chunks) or (outs is not None and isinstance(outs[0], DeviceArray))
        if outs is None:
            outs = (self._stats_out(I64, nbins, device), self._stats_out(F64, nbins + 1, device))
        cc, ce = (rdf_out * 1)(outs[0].out_struct()), (rdf_out * 1)(outs[1].out_struct())
        rng = (C.c_double * 2)(float(range[0]), float(range[1])) if range is not None else None
        counted = C.c_int64(-1)
        fn = self._fn("hist")
        fn.restype = C.c_int
        self._check(fn(_flat([chunks], n), C.c_int64(n), C.c_int64(nbins), rng, cc, ce, C.byref(counted)))
        self._finish([outs[0]], cc)
        self._finish([outs[1]], ce)
        return outs[0], outs[1], counted.value

    def uniques(self, chunks: Sequence, out=None, count_only: bool = False):
        """Column::uniques of an Int64 / UInt64 / Float64 column -> ONE array of the distinct values (unspecified order).
        Without `out` the count-only call sizes the buffer; count_only=True returns just the count."""
        n = len(chunks)
        carr = _flat([chunks], n)
        fn = self._fn("uniques")
        fn.restype = C.c_int
        count = C.c_int64(-1)
        if out is None:
            self._check(fn(carr, C.c_int64(n), None, C.byref(count)))
            if count_only:
                return count.value
            device = any(isinstance(c, DeviceArray) for c in chunks)
            out = self._stats_out(chunks[0].dtype if n else F64, count.value, device)
        co = (rdf_out * 1)(out.out_struct())
        self._check(fn(carr, C.c_int64(n), co, C.byref(count)))
        return self._finish([out], co)[0]

    # ---- window functions (src/functions/window.rs, src/window.rs: declared by the reference, empty there)
    @staticmethod
    def _window_out(dtype: int, n: int, device: bool, with_validity: bool):
        if not device:
            return HostArray.empty_out(dtype, n, with_validity)
        import torch
        cap = ((n + 63) // 64) * 64 + 64
        t = torch.zeros(cap, dtype=torch.int64, device="cuda")   # (8 bytes per element cover every output dtype)
        v = torch.zeros(cap // 8, dtype=torch.uint8, device="cuda") if with_validity else None
        return DeviceArray(t.data_ptr(), v.data_ptr() if with_validity else None, 0, n, dtype, 0, keep=(t, v), capacity=n)

    @staticmethod
    def _sort_keys(keys: Sequence):
        """[(chunks, descending) | chunks] -> (rdf_sort_key array, objects to keep alive)"""
        keys = [(k, False) if not isinstance(k, tuple) else k for k in keys]
        ck = (rdf_sort_key * max(1, len(keys)))()
        keep = []
        for i, (chunks, desc) in enumerate(keys):
            utf8 = len(chunks) > 0 and all(isinstance(c, (HostUtf8, DeviceUtf8)) for c in chunks)
            if utf8:
                arr = (rdf_utf8_array * max(1, len(chunks)))(*[c.c_struct() for c in chunks])
                ck[i] = rdf_sort_key(None, C.cast(arr, C.POINTER(rdf_utf8_array)), rdf_sort_options(int(desc), 0))
            else:
                arr = (rdf_array * max(1, len(chunks)))(*[c.c_struct(getattr(c, "_unknown_nc", False)) for c in chunks])
                ck[i] = rdf_sort_key(C.cast(arr, C.POINTER(rdf_array)), None, rdf_sort_options(int(desc), 0))
            keep.append(arr)
        return ck, keep

    @staticmethod
    def window_to_numpy(out):
        """One output of window(raw=True) as numpy: an array, or for lag / lead the masked pair (row indices, valid)."""
        if isinstance(out, HostArray):
            vals = out.values[:out.length].copy()
            valid = unpack_bits(out.validity, 0, out.length) if out.validity is not None else None
        else:
            t, v = out.keep
            vals = t.cpu().numpy().view(NP_OF[out.dtype])[:out.length].copy()
            valid = unpack_bits(v.cpu().numpy(), 0, out.length) if v is not None else None
        if out.dtype != U32:
            return vals
        return vals, (valid if valid is not None else np.ones(out.length, dtype=bool))

    def window(self, partition_by: Sequence, order_by: Sequence, calls: Sequence, mem: Optional[str] = None, nrows: int = 0,
               outs=None, raw: bool = False):
        """rdf_window: SQL window functions over partitions, every call answered from one sort.  partition_by = [chunks, ...],
        order_by = [(chunks, descending) | chunks, ...] (chunks: HostArray / DeviceArray or HostUtf8 / DeviceUtf8 lists);
        calls = [name | (name, param), ...] with the names of WINDOW_FNS (param: ntile buckets, lag / lead offset).  mem
        ("host" / "device") is needed only when there are no keys, and nrows gives the rows then.  -> one numpy array per call
        in the original row order, lag / lead as (row indices, valid); raw=True returns the output arrays as they are."""
        pk, keep_p = self._sort_keys(partition_by)
        ok, keep_o = self._sort_keys(order_by)
        all_keys = [k[0] if isinstance(k, tuple) else k for k in list(partition_by) + list(order_by)]
        nchunks = len(all_keys[0]) if all_keys else 0
        n = sum(c.length for c in all_keys[0]) if all_keys else int(nrows)
        device = mem == "device" if mem is not None else any(isinstance(c, (DeviceArray, DeviceUtf8)) for k in all_keys for c in k)
        cc = (rdf_window_call * max(1, len(calls)))()
        for i, c in enumerate(calls):
            name, param = c if isinstance(c, tuple) else (c, 0)
            cc[i] = rdf_window_call(WINDOW_FNS[name] if isinstance(name, str) else int(name), 0, int(param))
        if outs is None:
            outs = [self._window_out(window_out_dtype(cc[i].fn), n, device, cc[i].fn in (WIN_LAG, WIN_LEAD)) for i in range(len(calls))]
        carr = (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])
        fn = self._fn("window")
        fn.restype = C.c_int
        self._check(fn(pk if partition_by else None, C.c_int32(len(partition_by)), ok if order_by else None, C.c_int32(len(order_by)),
                       C.c_int64(nchunks), C.c_int64(nrows), cc if calls else None, C.c_int32(len(calls)), carr))
        self._finish(outs, carr)
        return outs if raw else [self.window_to_numpy(o) for o in outs]

    def window_agg(self, partition_by: Sequence, order_by: Sequence, values: Sequence, calls: Sequence, mem: Optional[str] = None,
                   nrows: int = 0, outs=None, raw: bool = False):
        """rdf_window_agg: sum / min / max / count / avg / first_value / last_value over window frames, every call answered
        from one sort.  partition_by / order_by as for window(); values = [chunks, ...] (Int64 or Float64 columns);
        calls = [(name, value index, frame), ...] with the names of WINDOW_AGG_FNS, frame = ("rows" | "range", start, end) in
        window_frame's spelling or an rdf_window_frame.  -> per call (values, valid) as numpy in the original row order
        (count: valid all True); raw=True returns the output arrays as they are."""
        pk, keep_p = self._sort_keys(partition_by)
        ok, keep_o = self._sort_keys(order_by)
        cols = [k[0] if isinstance(k, tuple) else k for k in list(partition_by) + list(order_by)] + list(values)
        nchunks = len(cols[0]) if cols else 0
        n = sum(c.length for c in cols[0]) if cols else int(nrows)
        device = mem == "device" if mem is not None else any(isinstance(c, (DeviceArray, DeviceUtf8)) for k in cols for c in k)
        varrs = [(rdf_array * max(1, len(v)))(*[c.c_struct(getattr(c, "_unknown_nc", False)) for c in v]) for v in values]
        vptr = (C.POINTER(rdf_array) * max(1, len(values)))(*[C.cast(a, C.POINTER(rdf_array)) for a in varrs])
        cc = (rdf_window_agg_call * max(1, len(calls)))()
        for i, (name, value, frame) in enumerate(calls):
            fr = frame if isinstance(frame, rdf_window_frame) else window_frame(*frame)
            cc[i] = rdf_window_agg_call(WINDOW_AGG_FNS[name] if isinstance(name, str) else int(name), int(value), fr)
        if outs is None:
            vdt = [v[0].dtype if len(v) else I64 for v in values]
            outs = [self._window_out(window_agg_out_dtype(cc[i].fn, vdt[cc[i].value] if 0 <= cc[i].value < len(vdt) else I64), n, device,
                                     cc[i].fn != WAGG_COUNT) for i in range(len(calls))]
        carr = (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])
        fn = self._fn("window_agg")
        fn.restype = C.c_int
        self._check(fn(pk if partition_by else None, C.c_int32(len(partition_by)), ok if order_by else None, C.c_int32(len(order_by)),
                       vptr if values else None, C.c_int32(len(values)), C.c_int64(nchunks), C.c_int64(nrows),
                       cc if calls else None, C.c_int32(len(calls)), carr))
        self._finish(outs, carr)
        return outs if raw else [self.window_agg_to_numpy(o) for o in outs]

    def window_range_agg(self, partition_by: Sequence, order_by: Sequence, values: Sequence, calls: Sequence, mem: Optional[str] = None,
                         outs=None, raw: bool = False):
        """rdf_window_range_agg: window_agg's functions over RANGE frames whose offsets are in the units of ONE numeric order
        key (Int32 / Int64 / Float64): a rolling 7-day sum is ("sum", 0, (-7, 0)) over a day-number key.  calls = [(name, value
        index, (start, end)), ...] in window_range_frame's spelling, or with an rdf_window_range_frame.  -> per call (values,
        valid) as numpy in the original row order; raw=True returns the output arrays as they are."""
        pk, keep_p = self._sort_keys(partition_by)
        ok, keep_o = self._sort_keys(order_by)
        cols = [k[0] if isinstance(k, tuple) else k for k in list(partition_by) + list(order_by)] + list(values)
        nchunks = len(cols[0]) if cols else 0
        n = sum(c.length for c in cols[0]) if cols else 0
        device = mem == "device" if mem is not None else any(isinstance(c, (DeviceArray, DeviceUtf8)) for k in cols for c in k)
        varrs = [(rdf_array * max(1, len(v)))(*[c.c_struct(getattr(c, "_unknown_nc", False)) for c in v]) for v in values]
        vptr = (C.POINTER(rdf_array) * max(1, len(values)))(*[C.cast(a, C.POINTER(rdf_array)) for a in varrs])
        cc = (rdf_window_range_call * max(1, len(calls)))()
        for i, (name, value, frame) in enumerate(calls):
            fr = frame if isinstance(frame, rdf_window_range_frame) else window_range_frame(*frame)
            cc[i] = rdf_window_range_call(WINDOW_AGG_FNS[name] if isinstance(name, str) else int(name), int(value), fr)
        if outs is None:
            vdt = [v[0].dtype if len(v) else I64 for v in values]
            outs = [self._window_out(window_agg_out_dtype(cc[i].fn, vdt[cc[i].value] if 0 <= cc[i].value < len(vdt) else I64), n, device,
                                     cc[i].fn != WAGG_COUNT) for i in range(len(calls))]
        carr = (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])
        fn = self._fn("window_range_agg")
        fn.restype = C.c_int
        status = fn(pk if partition_by else None, C.c_int32(len(partition_by)), ok if order_by else None, C.c_int32(len(order_by)),
                    vptr if values else None, C.c_int32(len(values)), C.c_int64(nchunks),
                    cc if calls else None, C.c_int32(len(calls)), carr)
        if status == RDF_MEMORY_ERROR:
            self._finish(outs, carr)   # a short capacity: the lengths say how many rows the caller's outputs need
        self._check(status)
        self._finish(outs, carr)
        return outs if raw else [self.window_agg_to_numpy(o) for o in outs]

    @staticmethod
    def window_agg_to_numpy(out):
        """One output of window_agg(raw=True) as (values, valid)."""
        if isinstance(out, HostArray):
            vals = out.values[:out.length].copy()
            valid = unpack_bits(out.validity, 0, out.length) if out.validity is not None else None
        else:
            t, v = out.keep
            vals = t.cpu().numpy().view(NP_OF[out.dtype])[:out.length].copy()
            valid = unpack_bits(v.cpu().numpy(), 0, out.length) if v is not None else None
        return vals, (valid if valid is not None else np.ones(out.length, dtype=bool))

    # ---- sorted GROUP BY: count_distinct / sum_distinct / first / last per group
    def groupby_sorted(self, group_by: Sequence, value, calls: Sequence, group_rows: bool = True, outs=None, rows_out=None,
                       raw: bool = False):
        """rdf_groupby_sorted: group_by = [chunks, ...] (0 .. 4 numeric or Utf8 columns), value = chunks of ONE numeric or Utf8
        column (None with no calls), calls = [name | (name, ignore_nulls), ...] with the names of GROUP_FNS.  Groups come in
        ascending key order, NULL last.  -> (groups, group_rows, results): the number of groups, the UInt32 row index of every
        group's first row (None with group_rows=False) and per call a numpy array, first / last as (row indices, valid).
        Without `outs` / `rows_out` the buffers hold one entry per row, which always suffices; raw=True returns the output
        arrays as they are."""
        cols = list(group_by) + ([value] if value is not None else [])
        gk, keep_g = self._sort_keys(group_by)
        vk, keep_v = self._sort_keys([value] if value is not None else [])
        nchunks = len(cols[0]) if cols else 0
        n = sum(c.length for c in cols[0]) if cols else 0
        device = any(isinstance(c, (DeviceArray, DeviceUtf8)) for k in cols for c in k)
        vdt = value[0].dtype if value is not None and len(value) and not self._is_utf8(value) else I64
        cc = (rdf_group_call * max(1, len(calls)))()
        for i, c in enumerate(calls):
            name, ign = c if isinstance(c, tuple) else (c, 0)
            cc[i] = rdf_group_call(GROUP_FNS[name] if isinstance(name, str) else int(name), int(ign))
        if outs is None:
            outs = [self._window_out(group_sorted_out_dtype(cc[i].fn, vdt), n, device, cc[i].fn in (GRP_FIRST, GRP_LAST)) for i in range(len(calls))]
        if rows_out is None and group_rows:
            rows_out = self._window_out(U32, n, device, False)
        carr = (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])
        crow = (rdf_out * 1)(rows_out.out_struct()) if rows_out is not None else None
        groups = C.c_int64(-1)
        fn = self._fn("groupby_sorted")
        fn.restype = C.c_int
        try:
            self._check(fn(gk if group_by else None, C.c_int32(len(group_by)), vk if value is not None else None, C.c_int64(nchunks),
                           cc if calls else None, C.c_int32(len(calls)), crow, carr if calls else None, C.byref(groups)))
        finally:
            self._finish(outs, carr)
            if rows_out is not None:
                self._finish([rows_out], crow)
            self.last_groups = groups.value
        if raw:
            return groups.value, rows_out, outs
        rows = self.window_to_numpy(rows_out)[0] if rows_out is not None else None
        return groups.value, rows, [self.window_to_numpy(o) for o in outs]

    # ---- percentiles and median per group
    def groupby_percentile(self, group_by: Sequence, value, calls: Sequence, group_rows: bool = True, counts: bool = False,
                           outs=None, rows_out=None, counts_out=None, raw: bool = False):
        """rdf_groupby_percentile: group_by = [chunks, ...] (0 .. 4 numeric or Utf8 columns), value = chunks of ONE numeric or
        Utf8 column (None with no calls and no counts), calls = [("cont", p) | ("disc", p) | "median", ...].  Groups come in
        ascending key order, NULL last.  -> (groups, group_rows, results, counts): the number of groups, the UInt32 row index
        of every group's first row (None with group_rows=False), per call the pair (values, valid) — Float64 for "cont", UInt32
        row indices for "disc" — and the Int64 count of non-NULL values per group (None with counts=False).  Without `outs` /
        `rows_out` / `counts_out` the buffers hold one entry per row, which always suffices, and every call gets a validity
        bitmap; raw=True returns the output arrays as they are."""
        cols = list(group_by) + ([value] if value is not None else [])
        gk, keep_g = self._sort_keys(group_by)
        vk, keep_v = self._sort_keys([value] if value is not None else [])
        nchunks = len(cols[0]) if cols else 0
        n = sum(c.length for c in cols[0]) if cols else 0
        device = any(isinstance(c, (DeviceArray, DeviceUtf8)) for k in cols for c in k)
        kp = percentile_calls(calls)
        cc = (rdf_percentile_call * max(1, len(kp)))()
        for i, (kind, p) in enumerate(kp):
            cc[i] = rdf_percentile_call(kind, 0, p)
        if outs is None:
            outs = [self._window_out(F64 if kind == PCT_CONT else U32, n, device, True) for kind, _ in kp]
        if rows_out is None and group_rows:
            rows_out = self._window_out(U32, n, device, False)
        if counts_out is None and counts:
            counts_out = self._window_out(I64, n, device, False)
        carr = (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])
        crow = (rdf_out * 1)(rows_out.out_struct()) if rows_out is not None else None
        ccnt = (rdf_out * 1)(counts_out.out_struct()) if counts_out is not None else None
        groups = C.c_int64(-1)
        fn = self._fn("groupby_percentile")
        fn.restype = C.c_int
        try:
            self._check(fn(gk if group_by else None, C.c_int32(len(group_by)), vk if value is not None else None, C.c_int64(nchunks),
                           cc if kp else None, C.c_int32(len(kp)), crow, carr if kp else None, ccnt, C.byref(groups)))
        finally:
            self._finish(outs, carr)
            if rows_out is not None:
                self._finish([rows_out], crow)
            if counts_out is not None:
                self._finish([counts_out], ccnt)
            self.last_groups = groups.value
        if raw:
            return groups.value, rows_out, outs, counts_out
        return (groups.value, self._out_values(rows_out), [self.window_agg_to_numpy(o) for o in outs], self._out_values(counts_out))

    # ---- moments per group: variance, stddev, skewness, kurtosis, covar, corr
    def groupby_moments(self, group_by: Sequence, x, y=None, stats: Sequence = (), group_rows: bool = True, counts: bool = True,
                        states: bool = False, outs=None, rows_out=None, counts_out=None, states_capacity: Optional[int] = None,
                        raw: bool = False):
        """rdf_groupby_moments: group_by = [chunks, ...] (0 .. 4 numeric or Utf8 columns), x = chunks of ONE numeric column
        (None when only the key tuples are asked for), y = None or chunks of a second numeric column, stats = names of STATS
        (without y) or COSTATS (with y), or their numbers.  Groups come in ascending key order, NULL last.
        -> (groups, group_rows, results, counts, states): the number of groups, the UInt32 row index of every group's first
        row (None with group_rows=False), per statistic the pair (Float64 values, valid), the Int64 count of counted rows per
        group (None with counts=False) and, with states=True, a ctypes array of one rdf_moments_state / rdf_comoments_state
        per group (else None).  Without `outs` / `rows_out` / `counts_out` / `states_capacity` the buffers hold one entry per
        row, which always suffices; raw=True returns the output arrays as they are."""
        cols = list(group_by) + [c for c in (x, y) if c is not None]
        gk, keep_g = self._sort_keys(group_by)
        nchunks = len(cols[0]) if cols else 0
        n = sum(c.length for c in cols[0]) if cols else 0
        device = any(isinstance(c, (DeviceArray, DeviceUtf8)) for k in cols for c in k)
        names = COSTATS if y is not None else STATS
        cc = (rdf_group_stat_call * max(1, len(stats)))()
        for i, st in enumerate(stats):
            cc[i] = rdf_group_stat_call(names[st] if isinstance(st, str) else int(st), 0)
        cx = _flat([x], nchunks) if x is not None else None
        cy = _flat([y], nchunks) if y is not None else None
        if outs is None:
            outs = [self._window_out(F64, n, device, True) for _ in stats]
        if rows_out is None and group_rows:
            rows_out = self._window_out(U32, n, device, False)
        if counts_out is None and counts and x is not None:
            counts_out = self._window_out(I64, n, device, False)
        state_t = rdf_comoments_state if y is not None else rdf_moments_state
        cap = n if states_capacity is None else int(states_capacity)
        sbuf = sptr = None
        if states:
            if device:
                import torch
                sbuf = torch.zeros(max(1, cap) * C.sizeof(state_t), dtype=torch.uint8, device="cuda")
                sptr = C.c_void_p(sbuf.data_ptr())
            else:
                sbuf = (state_t * max(1, cap))()
                sptr = C.cast(sbuf, C.c_void_p)
        carr = (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])
        crow = (rdf_out * 1)(rows_out.out_struct()) if rows_out is not None else None
        ccnt = (rdf_out * 1)(counts_out.out_struct()) if counts_out is not None else None
        groups = C.c_int64(-1)
        fn = self._fn("groupby_moments")
        fn.restype = C.c_int
        try:
            self._check(fn(gk if group_by else None, C.c_int32(len(group_by)), cx, cy, C.c_int64(nchunks),
                           cc if len(stats) else None, C.c_int32(len(stats)), crow, carr if len(stats) else None, ccnt,
                           sptr, C.c_int64(cap if states else 0), C.byref(groups)))
        finally:
            self._finish(outs, carr)
            if rows_out is not None:
                self._finish([rows_out], crow)
            if counts_out is not None:
                self._finish([counts_out], ccnt)
            self.last_groups = groups.value
        got = None
        if states:
            g = groups.value
            if device:
                got = (state_t * g).from_buffer_copy(sbuf[:g * C.sizeof(state_t)].cpu().numpy().tobytes()) if g else (state_t * 0)()
            else:
                got = (state_t * g).from_buffer_copy(bytes(sbuf)[:g * C.sizeof(state_t)])
        if raw:
            return groups.value, rows_out, outs, counts_out, got
        return (groups.value, self._out_values(rows_out), [self.window_agg_to_numpy(o) for o in outs], self._out_values(counts_out), got)

    # ---- collect per group and explode: collect_list / collect_set / explode
    @staticmethod
    def _out_values(out):
        """The values of one output array as numpy, `length` entries."""
        if out is None:
            return None
        if isinstance(out, HostArray):
            return out.values[:out.length].copy()
        return out.keep[0].cpu().numpy().view(NP_OF[out.dtype])[:out.length].copy()

    def groupby_collect(self, group_by: Sequence, value, kind, values: bool = True, group_rows: bool = True, outs=None,
                        raw: bool = False):
        """rdf_groupby_collect: group_by = [chunks, ...] (0 .. 4 numeric or Utf8 columns), value = chunks of ONE numeric or Utf8
        column, kind = "list" | "set" (COLLECT_KINDS).  One List row per group, groups in ascending key order, NULL last.
        -> (groups, group_rows, offsets, child_rows, values | None): the number of groups, the UInt32 row index of every
        group's first row (None with group_rows=False), the Int32 offsets (groups + 1 entries), the UInt32 row index of every
        element and the elements themselves (numeric value columns with values=True, else None).  Without `outs` the buffers
        hold one entry per row (rows + 1 offsets), which always suffices; `outs` = (group_rows, offsets, child_rows, values)
        are the caller's output arrays, None where one is not wanted, and (None, None, None, None) is the count-only call
        (the counts are then in last_groups / last_elements).  raw=True returns the output arrays as they are."""
        cols = list(group_by) + [value]
        gk, keep_g = self._sort_keys(group_by)
        vk, keep_v = self._sort_keys([value])
        nchunks = len(value)
        n = sum(c.length for c in value)
        device = any(isinstance(c, (DeviceArray, DeviceUtf8)) for k in cols for c in k)
        if outs is None:
            numeric = len(value) > 0 and not self._is_utf8(value)
            outs = (self._window_out(U32, n, device, False) if group_rows else None,
                    self._window_out(I32, n + 1, device, False),
                    self._window_out(U32, n, device, False),
                    self._window_out(value[0].dtype, n, device, False) if values and numeric else None)
        cs = [(rdf_out * 1)(o.out_struct()) if o is not None else None for o in outs]
        groups, elements = C.c_int64(-1), C.c_int64(-1)
        fn = self._fn("groupby_collect")
        fn.restype = C.c_int
        try:
            self._check(fn(gk if group_by else None, C.c_int32(len(group_by)), vk, C.c_int64(nchunks),
                           C.c_int32(COLLECT_KINDS[kind] if isinstance(kind, str) else int(kind)), cs[0], cs[1], cs[2], cs[3],
                           C.byref(groups), C.byref(elements)))
        finally:
            for o, c in zip(outs, cs):
                if o is not None:
                    self._finish([o], c)
            self.last_groups, self.last_elements = groups.value, elements.value
        if raw:
            return (groups.value,) + tuple(outs)
        return (groups.value,) + tuple(self._out_values(o) for o in outs)

    def list_explode(self, lst, outer: bool = False, pos: bool = False, outs=None, raw: bool = False):
        """rdf_list_explode of a HostList / DeviceList: one output row per element of every non-NULL list (outer=True: one
        row with a NULL element for a NULL or empty list).  -> (parent_rows, (child_index, valid), pos | None): the list row
        of every output row, the element's index into the list's child values with its validity (all True without outer),
        and with pos=True the 0-based position inside the list as (pos, valid).  Without `outs` one count-only call sizes
        the buffers; `outs` = (parent_rows, child_index, pos) are the caller's arrays, None where one is not wanted.
        raw=True returns the output arrays as they are.  The row count is in last_rows."""
        fn = self._fn("list_explode")
        fn.restype = C.c_int
        ls = lst.c_struct()
        rows = C.c_int64(-1)
        device = isinstance(lst, DeviceList)
        if outs is None:
            self._check(fn(C.byref(ls), C.c_int32(int(outer)), None, None, None, C.byref(rows)))
            r = rows.value
            outs = (self._window_out(U32, r, device, False), self._window_out(U32, r, device, True),
                    self._window_out(I32, r, device, True) if pos else None)
        cs = [(rdf_out * 1)(o.out_struct()) if o is not None else None for o in outs]
        try:
            self._check(fn(C.byref(ls), C.c_int32(int(outer)), cs[0], cs[1], cs[2], C.byref(rows)))
        finally:
            for o, c in zip(outs, cs):
                if o is not None:
                    self._finish([o], c)
            self.last_rows = rows.value
        if raw:
            return tuple(outs)

        def masked(o):
            if o is None:
                return None
            if isinstance(o, HostArray):
                valid = unpack_bits(o.validity, 0, o.length) if o.validity is not None else None
            else:
                valid = unpack_bits(o.keep[1].cpu().numpy(), 0, o.length) if o.keep[1] is not None else None
            return self._out_values(o), (valid if valid is not None else np.ones(o.length, dtype=bool))
        return self._out_values(outs[0]), masked(outs[1]), masked(outs[2])

    def utf8_uniques(self, chunks: Sequence, as_arrow=False):
        """Column::uniques of a Utf8 column -> ONE Utf8 chunk of the distinct strings (no NULLs, unspecified order).  The
        output can never need more bytes than the input, so the buffers are sized from the input and one call is made."""
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        fn = self._utf8_fn("utf8_uniques")
        count = C.c_int64(-1)
        rows = sum(c.length for c in chunks)
        device = any(isinstance(c, DeviceUtf8) for c in chunks)
        nbytes = sum(c.data_length if isinstance(c, DeviceUtf8) else len(c.data) - c.data_offset for c in chunks)
        co, cd, keep = self._utf8_outs(chunks, [rows], [False], device, [max(1, nbytes)])
        self._check(fn(carr, C.c_int64(n), co, cd, C.byref(count)))
        got = co[0].length - 1
        if device:
            ot, dt, vt = keep[0]
            r = DeviceUtf8(ot.data_ptr(), dt.data_ptr(), cd[0].length, got, None, 0, 0, 0, keep=(ot, dt, vt))
        else:
            ob, db, vb = keep[0]
            r = HostUtf8(ob, db, None, 0, got, 0, 0)
        if as_arrow:
            h = r.to_host() if device else r
            r = h.to_pylist() if as_arrow == "pylist" else h.to_arrow()
        return r

    # ---- text keys: dictionary encoding, GROUP BY and join whose keys may be Utf8 columns
    @staticmethod
    def _is_utf8(chunks) -> bool:
        return len(chunks) > 0 and all(isinstance(c, (HostUtf8, DeviceUtf8)) for c in chunks)

    @staticmethod
    def _utf8_bytes(chunks) -> int:
        return sum(c.data_length if isinstance(c, DeviceUtf8) else len(c.data) - c.data_offset for c in chunks)

    @staticmethod
    def _utf8_result(co, cd, keep, device: bool, nullable: bool):
        """Output 0 of _utf8_outs after a call, as a HostUtf8 / DeviceUtf8."""
        rows = co[0].length - 1
        if device:
            ot, dt, vt = keep[0]
            return DeviceUtf8(ot.data_ptr(), dt.data_ptr() if dt is not None else 0, cd[0].length, rows,
                              vt.data_ptr() if (vt is not None and nullable) else None, 0, 0, co[0].null_count if nullable else 0, keep=(ot, dt, vt))
        ob, db, vb = keep[0]
        return HostUtf8(ob, db if db is not None else np.zeros(8, dtype=np.uint8), vb if nullable else None, 0, rows, 0, co[0].null_count if nullable else 0)

    def utf8_dictionary_encode(self, chunks: Sequence):
        """rdf_utf8_dictionary_encode -> (codes, dictionary, count): one UInt32 array per input chunk (with validity; NULL rows
        give NULL codes), ONE Utf8 chunk of the distinct values in first-occurrence order, and their number.  The buffers
        are sized from the input (rows + 1 offsets, the input's bytes), so one call is made."""
        n = len(chunks)
        carr = (rdf_utf8_array * max(1, n))(*[c.c_struct() for c in chunks])
        device = any(isinstance(c, DeviceUtf8) for c in chunks)
        codes = [self._window_out(U32, c.length, device, True) for c in chunks]
        cc = (rdf_out * max(1, n))(*[o.out_struct() for o in codes])
        co, cd, keep = self._utf8_outs(chunks, [sum(c.length for c in chunks)], [False], device, [max(1, self._utf8_bytes(chunks))])
        count = C.c_int64(-1)
        fn = self._utf8_fn("utf8_dictionary_encode")
        self._check(fn(carr, C.c_int64(n), cc, co, cd, C.byref(count)))
        self._finish(codes, cc)
        return codes, self._utf8_result(co, cd, keep, device, False), count.value

    def groupby_agg_keys(self, key_cols: Sequence[Sequence], values: Optional[Sequence], agg, max_groups: int):
        """rdf_groupby_agg_keys: GROUP BY over 1..4 grouping columns, each a list of numeric chunks or of Utf8 chunks.
        -> ([key column: array | HostUtf8 / DeviceUtf8], values, counts), one chunk each, in unspecified group order."""
        code = self.AGGS[agg] if isinstance(agg, str) else int(agg)
        nk, n = len(key_cols), len(key_cols[0])
        ck, keep_k = self._sort_keys(list(key_cols))
        device = any(isinstance(c, (DeviceArray, DeviceUtf8)) for col in key_cols for c in col)
        vdt = values[0].dtype if values is not None and code != 3 else None
        cap = max_groups + 2
        kouts = (rdf_key_out * max(1, nk))()
        holders = []
        for k, col in enumerate(key_cols):
            nullable = any((c.validity is not None) if isinstance(c, (HostArray, HostUtf8)) else bool(c.validity_ptr) for c in col)
            if self._is_utf8(col):
                co, cd, keep = self._utf8_outs(col, [cap], [nullable], device, [max(1, self._utf8_bytes(col))])
                kouts[k] = rdf_key_out(None, C.cast(co, C.POINTER(rdf_out)), C.cast(cd, C.POINTER(rdf_out)))
                holders.append(("utf8", co, cd, keep, nullable))
            else:
                o = self._window_out(col[0].dtype, cap, device, nullable)
                co = (rdf_out * 1)(o.out_struct())
                kouts[k] = rdf_key_out(C.cast(co, C.POINTER(rdf_out)), None, None)
                holders.append(("num", o, co))
        nullable_v = values is not None and any(v.validity is not None for v in values)
        ov = self._window_out(self._agg_out_dtype(code, vdt), cap, device, nullable_v and code in (1, 2))
        oc = self._window_out(I64, cap, device, False)
        cv, ccnt = (rdf_out * 1)(ov.out_struct()), (rdf_out * 1)(oc.out_struct())
        cvals = _flat([values], n) if values is not None else None
        fn = self._fn("groupby_agg_keys")
        fn.restype = C.c_int
        self._check(fn(ck, C.c_int32(nk), cvals, C.c_int64(n), C.c_int32(code), C.c_int64(max_groups), kouts, cv, ccnt))
        keys = []
        for h in holders:
            if h[0] == "utf8":
                keys.append(self._utf8_result(h[1], h[2], h[3], device, h[4]))
            else:
                keys.append(self._finish([h[1]], h[2])[0])
        self._finish([ov], cv)
        self._finish([oc], ccnt)
        return keys, ov, oc

    def groupby_multi_capacity(self, ncalls: int) -> int:
        """rdf_groupby_multi_capacity: the most groups the one-pass LDS route of rdf_groupby_multi holds for this many calls."""
        fn = self._fn("groupby_multi_capacity")
        fn.restype = C.c_int64
        return int(fn(C.c_int32(ncalls)))

    def groupby_multi(self, key_cols: Sequence[Sequence], values: Sequence[Sequence], calls: Sequence, max_groups: int, with_rows: bool = True):
        """rdf_groupby_multi: GROUP BY over 1..4 grouping columns (numeric or Utf8 chunk lists) with several aggregates from one
        pass: values[v] = the chunks of value column v, calls = [(agg, value index | -1)].
        -> ([key column], [outs[c]], [counts[c]], group rows | None), one chunk each; row g of every output is one group."""
        calls = [((self.AGGS[a] if isinstance(a, str) else int(a)), int(v)) for a, v in calls]
        nk, n, nv, nc = len(key_cols), len(key_cols[0]), len(values), len(calls)
        ck, keep_k = self._sort_keys(list(key_cols))
        device = any(isinstance(c, (DeviceArray, DeviceUtf8)) for col in key_cols for c in col)
        cap = max_groups + 2
        kouts = (rdf_key_out * max(1, nk))()
        holders = []
        for k, col in enumerate(key_cols):
            nullable = any((c.validity is not None) if isinstance(c, (HostArray, HostUtf8)) else bool(c.validity_ptr) for c in col)
            if self._is_utf8(col):
                co, cd, keep = self._utf8_outs(col, [cap], [nullable], device, [max(1, self._utf8_bytes(col))])
                kouts[k] = rdf_key_out(None, C.cast(co, C.POINTER(rdf_out)), C.cast(cd, C.POINTER(rdf_out)))
                holders.append(("utf8", co, cd, keep, nullable))
            else:
                o = self._window_out(col[0].dtype, cap, device, nullable)
                co = (rdf_out * 1)(o.out_struct())
                kouts[k] = rdf_key_out(C.cast(co, C.POINTER(rdf_out)), None, None)
                holders.append(("num", o, co))
        carrs = [_flat([v], n) for v in values]
        cvals = (C.POINTER(rdf_array) * max(1, nv))(*[C.cast(a, C.POINTER(rdf_array)) for a in carrs])
        ccalls = (rdf_multi_agg_call * max(1, nc))(*[rdf_multi_agg_call(a, v) for a, v in calls])
        ovs, ocs = [], []
        for a, v in calls:
            vdt = values[v][0].dtype if (a != 3 and 0 <= v < nv) else None
            ovs.append(self._window_out(self._agg_out_dtype(a, vdt), cap, device, True))
            ocs.append(self._window_out(I64, cap, device, False))
        cv = (rdf_out * max(1, nc))(*[o.out_struct() for o in ovs])
        cc = (rdf_out * max(1, nc))(*[o.out_struct() for o in ocs])
        orow = self._window_out(I64, cap, device, False) if with_rows else None
        crow = (rdf_out * 1)(orow.out_struct()) if with_rows else None
        groups = C.c_int64(-1)
        fn = self._fn("groupby_multi")
        fn.restype = C.c_int
        self._check(fn(ck, C.c_int32(nk), cvals, C.c_int32(nv), C.c_int64(n), ccalls, C.c_int32(nc), C.c_int64(max_groups),
                       kouts, cv, cc, crow, C.byref(groups)))
        keys = []
        for h in holders:
            if h[0] == "utf8":
                keys.append(self._utf8_result(h[1], h[2], h[3], device, h[4]))
            else:
                keys.append(self._finish([h[1]], h[2])[0])
        self._finish(ovs, cv)
        self._finish(ocs, cc)
        if with_rows:
            self._finish([orow], crow)
        assert groups.value == ocs[0].length
        return keys, ovs, ocs, orow

    def equijoin_indices_keys(self, left_cols: Sequence[Sequence], right_cols: Sequence[Sequence], how: str, count_only: bool = False, outs=None):
        """rdf_equijoin_indices_keys: left_cols[k] pairs with right_cols[k]; a pair is Utf8 on both sides or numeric of one
        dtype on both sides.  -> (left_indices, right_indices) as UInt32 arrays with validity, or the row count alone.
        `outs` = caller-allocated (left, right) outputs: the sizing call is skipped."""
        jt = self.JOIN_TYPES[how] if isinstance(how, str) else int(how)
        lk, keep_l = self._sort_keys(list(left_cols))
        rk, keep_r = self._sort_keys(list(right_cols))
        nk, lnc, rnc = len(left_cols), len(left_cols[0]), len(right_cols[0])
        device = any(isinstance(c, (DeviceArray, DeviceUtf8)) for col in list(left_cols) + list(right_cols) for c in col)
        rows = C.c_int64(-1)
        fn = self._fn("equijoin_indices_keys")
        fn.restype = C.c_int
        if outs is not None:
            ol, orr = outs
            cl, cr = (rdf_out * 1)(ol.out_struct()), (rdf_out * 1)(orr.out_struct())
            self._check(fn(lk, C.c_int64(lnc), rk, C.c_int64(rnc), C.c_int32(nk), C.c_int32(jt), cl, cr, C.byref(rows)))
            self._finish([ol], cl)
            self._finish([orr], cr)
            return ol, orr
        self._check(fn(lk, C.c_int64(lnc), rk, C.c_int64(rnc), C.c_int32(nk), C.c_int32(jt), None, None, C.byref(rows)))
        if count_only:
            return rows.value
        ol, orr = self._window_out(U32, rows.value, device, True), self._window_out(U32, rows.value, device, True)
        cl, cr = (rdf_out * 1)(ol.out_struct()), (rdf_out * 1)(orr.out_struct())
        self._check(fn(lk, C.c_int64(lnc), rk, C.c_int64(rnc), C.c_int32(nk), C.c_int32(jt), cl, cr, C.byref(rows)))
        self._finish([ol], cl)
        self._finish([orr], cr)
        return ol, orr

    # ---- membership: semi / anti join, is_in, distinct rows
    MEMBER_KINDS = {"semi": MEMBER_SEMI, "anti": MEMBER_ANTI, "is_in": MEMBER_IS_IN}
    KEEPS = {"first": KEEP_FIRST, "last": KEEP_LAST, "none": KEEP_NONE, False: KEEP_NONE}

    @staticmethod
    def _key_rows(col):
        return [c.length for c in col]

    def _mask_call(self, call, lens, device, with_validity, count_only, outs):
        """call(carr | None, byref(rows)) -> status; -> the row count (count_only) or (mask outputs, TRUE rows)"""
        rows = C.c_int64(-1)
        if count_only:
            self._check(call(None, C.byref(rows)))
            return rows.value
        if outs is None:
            outs = [self._window_out(BOOL, n, device, with_validity) for n in lens]
        carr = (rdf_out * max(1, len(outs)))(*[o.out_struct() for o in outs])
        st = call(carr, C.byref(rows))
        self._finish(outs, carr)
        self.last_out_rows = rows.value
        self._check(st)
        return outs, rows.value

    def member_mask(self, left_cols: Sequence[Sequence], right_cols: Sequence[Sequence], kind, count_only: bool = False, outs=None):
        """rdf_member_mask: left_cols[k] pairs with right_cols[k] (HostArray / DeviceArray / HostUtf8 / DeviceUtf8 chunk lists);
        kind = "semi" | "anti" | "is_in".  -> (one BOOL mask per left chunk, TRUE rows), or the TRUE rows alone."""
        kd = self.MEMBER_KINDS[kind] if isinstance(kind, str) else int(kind)
        lk, keep_l = self._sort_keys(list(left_cols))
        rk, keep_r = self._sort_keys(list(right_cols))
        nk, lnc, rnc = len(left_cols), len(left_cols[0]), len(right_cols[0])
        device = any(isinstance(c, (DeviceArray, DeviceUtf8)) for col in list(left_cols) + list(right_cols) for c in col)
        fn = self._fn("member_mask")
        fn.restype = C.c_int
        return self._mask_call(lambda carr, rows: fn(lk, C.c_int64(lnc), rk, C.c_int64(rnc), C.c_int32(nk), C.c_int32(kd), carr, rows),
                               self._key_rows(left_cols[0]), device, kd == MEMBER_IS_IN, count_only, outs)

    def first_occurrence(self, key_cols: Sequence[Sequence], keep="first", count_only: bool = False, outs=None):
        """rdf_first_occurrence: keep = "first" | "last" | "none" (pandas' keep=False).  -> (one BOOL mask per chunk, TRUE
        rows), or the TRUE rows alone."""
        kp = self.KEEPS[keep] if isinstance(keep, (str, bool)) else int(keep)
        ck, keep_k = self._sort_keys(list(key_cols))
        nk, nc = len(key_cols), len(key_cols[0])
        device = any(isinstance(c, (DeviceArray, DeviceUtf8)) for col in key_cols for c in col)
        fn = self._fn("first_occurrence")
        fn.restype = C.c_int
        return self._mask_call(lambda carr, rows: fn(ck, C.c_int32(nk), C.c_int64(nc), C.c_int32(kp), carr, rows),
                               self._key_rows(key_cols[0]), device, False, count_only, outs)

    # ---- fused grouped aggregation over a small dense domain (TPC-H Q1 shape)
    def group_pipeline(self, expr: Expr, cols: Sequence[Sequence], value_roots: Sequence[int], group_root: int, ngroups: int,
                       filter_root: int = -1, with_some: bool = False):
        """-> (res, rows): res[v][g] = (sum, count) of value v in group g (g == ngroups: the NULL group), rows[g] = count(*).
        with_some: (sum, count, is_some) instead."""
        nchunks = 0 if isinstance(cols, Frame) or not cols else len(cols[0])
        nodes = expr.c_array()
        nv = len(value_roots)
        S = ngroups + 1
        out = (rdf_group_result * max(1, nv * S))()
        rows = (C.c_int64 * max(1, S))()
        roots = (C.c_int32 * max(1, nv))(*value_roots)
        if isinstance(cols, Frame):   # rdf_group_pipeline_frame
            fn = self._fn("group_pipeline_frame")
            fn.restype = C.c_int
            self._check(fn(nodes, C.c_int32(len(expr.nodes)), C.c_int32(filter_root), C.c_int32(group_root), C.c_int32(ngroups),
                           roots, C.c_int32(nv), cols.handle, out, rows))
        else:
            self._check(self._fn("group_pipeline")(nodes, C.c_int32(len(expr.nodes)), C.c_int32(filter_root), C.c_int32(group_root),
                                                   C.c_int32(ngroups), roots, C.c_int32(nv), _flat(cols, nchunks), C.c_int32(len(cols)),
                                                   C.c_int64(nchunks), out, rows))
        res = []
        for v in range(nv):
            row = []
            for g in range(S):
                r = out[v * S + g]
                row.append((r.sum_f64 if r.dtype in (F32, F64) else r.sum_i64, r.count) + ((r.is_some,) if with_some else ()))
            res.append(row)
        return res, [rows[g] for g in range(S)]

    # ---- fused batch loop
    def pipeline(self, expr: Expr, cols: Sequence[Sequence], value_roots: Sequence[int], filter_root: int = -1,
                 sink: int = SINK_AGG, outs=None):
        nodes = expr.c_array()
        prog = rdf_program(C.cast(nodes, C.POINTER(rdf_expr_node)), len(expr.nodes), filter_root, len(value_roots),
                           (C.c_int32 * MAX_VALUES)(*(list(value_roots) + [0] * (MAX_VALUES - len(value_roots)))), sink)
        if isinstance(cols, Frame):   # rdf_pipeline_frame: descriptors validated and kept on the device once
            def call(carr, aggs):
                return self._fn("pipeline_frame")(C.byref(prog), cols.handle, carr, aggs)
        else:
            nchunks = len(cols[0]) if cols else 0
            cc = _flat(cols, nchunks)

            def call(carr, aggs):
                return self._fn("pipeline")(C.byref(prog), cc, C.c_int32(len(cols)), C.c_int64(nchunks), carr, aggs)
        aggs = (rdf_agg_result * MAX_VALUES)()
        if sink == SINK_STORE:
            assert outs is not None, "SINK_STORE needs caller-allocated outputs: outs[v][chunk]"
            flat = [o for v in outs for o in v]
            carr = (rdf_out * max(1, len(flat)))(*[o.out_struct() for o in flat])
            self._check(call(carr, aggs))
            self._finish(flat, carr)
            return outs
        self._check(call(None, aggs))
        res = []
        for v in range(len(value_roots)):
            r = aggs[v]
            if r.dtype in (F32, F64):
                res.append(AggResult(r.sum_f64, r.min_f64, r.max_f64, r.count, bool(r.is_some), r.dtype))
            else:
                fix = (lambda x: x + 2 ** 64 if x < 0 else x) if r.dtype == U64 else (lambda x: x)
                res.append(AggResult(fix(r.sum_i64), fix(r.min_i64), fix(r.max_i64), r.count, bool(r.is_some), r.dtype))
        return res


# ---------------------------------------------------------------- multi-GPU: one rank's end of a communicator
class Comm:
    """rdf_comm: the exchange of the N > 1 path behind the C ABI (RCCL loaded by the library itself, or peer copies between
    the threads of one process).  One Comm per rank, used by the thread that drives the rank's device."""

    EXCHANGES = {"auto": EXCHANGE_AUTO, "groups": EXCHANGE_GROUPS, "rows": EXCHANGE_ROWS}

    def __init__(self, api: "Api", handle):
        self.api, self.handle = api, handle
        self.stats = {}

    # -- construction
    @staticmethod
    def unique_id(api: "Api") -> bytes:
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        fn = api._fn("comm_unique_id")
        fn.restype = C.c_int
        api._check(fn(buf))
        return bytes(buf)

    @staticmethod
    def init_rank(api: "Api", world: int, rank: int, uid: bytes) -> "Comm":
        assert len(uid) == COMM_ID_BYTES
        h = C.c_void_p(0)
        fn = api._fn("comm_init_rank")
        fn.restype = C.c_int
        api._check(fn(C.c_int32(world), C.c_int32(rank), (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid), C.byref(h)))
        return Comm(api, h)

    @staticmethod
    def init_all(api: "Api", devices: Sequence[int], kind: int = COMM_RCCL) -> List["Comm"]:
        n = len(devices)
        hs = (C.c_void_p * n)()
        fn = api._fn("comm_init_all")
        fn.restype = C.c_int
        api._check(fn(C.c_int32(n), (C.c_int32 * n)(*devices), C.c_int32(kind), hs))
        return [Comm(api, C.c_void_p(hs[i])) for i in range(n)]

    def destroy(self):
        if self.handle is not None:
            fn = self.api._fn("comm_destroy")
            fn.restype = C.c_int
            fn(self.handle)
            self.handle = None

    def info(self) -> dict:
        v = [C.c_int32(0) for _ in range(5)]
        fn = self.api._fn("comm_info")
        fn.restype = C.c_int
        self.api._check(fn(self.handle, *[C.byref(x) for x in v]))
        ver = v[4].value
        return {"world": v[0].value, "rank": v[1].value, "device": v[2].value, "kind": "rccl" if v[3].value == COMM_RCCL else "peer",
                "rccl_version": (f"{ver // 10000}.{ver // 100 % 100}.{ver % 100}" if ver else None)}

    # -- collectives
    def barrier(self):
        fn = self.api._fn("comm_barrier")
        fn.restype = C.c_int
        self.api._check(fn(self.handle))

    def allgather(self, mine: bytes) -> List[bytes]:
        world = self.info()["world"]
        out = (C.c_uint8 * (len(mine) * world))()
        fn = self.api._fn("comm_allgather")
        fn.restype = C.c_int
        self.api._check(fn(self.handle, (C.c_uint8 * len(mine)).from_buffer_copy(mine), C.c_int64(len(mine)), out))
        raw = bytes(out)
        return [raw[r * len(mine):(r + 1) * len(mine)] for r in range(world)]

    def agg_combine(self, local: Sequence[AggResult]) -> List[AggResult]:
        """Per-rank partial aggregates (Api.pipeline's results) -> the aggregates over all ranks, folded in rank order."""
        n = len(local)
        arr = (rdf_agg_result * n)()
        for i, p in enumerate(local):
            r = arr[i]
            r.dtype, r.count, r.is_some = p.dtype, p.count, int(p.is_some)
            if p.dtype in (F32, F64):
                r.sum_f64, r.min_f64, r.max_f64 = p.sum, p.min, p.max
            else:
                wrap = lambda x: x - (1 << 64) if x >= (1 << 63) else x
                r.sum_i64, r.min_i64, r.max_i64 = wrap(int(p.sum)), wrap(int(p.min)), wrap(int(p.max))
        fn = self.api._fn("agg_combine")
        fn.restype = C.c_int
        self.api._check(fn(self.handle, arr, C.c_int32(n)))
        out = []
        for i in range(n):
            r = arr[i]
            if r.dtype in (F32, F64):
                out.append(AggResult(r.sum_f64, r.min_f64, r.max_f64, r.count, bool(r.is_some), r.dtype))
            else:
                fix = (lambda x: x + 2 ** 64 if x < 0 else x) if r.dtype == U64 else (lambda x: x)
                out.append(AggResult(fix(r.sum_i64), fix(r.min_i64), fix(r.max_i64), r.count, bool(r.is_some), r.dtype))
        return out

    def pipeline_dist(self, expr: Expr, cols, value_roots: Sequence[int], filter_root: int = -1) -> List[AggResult]:
        """Api.pipeline (aggregating) + agg_combine in one call (rdf_pipeline_dist / rdf_pipeline_frame_dist): this rank's shard in,
        the aggregates over all ranks out — the partials are all-gathered and folded on the device, the host waits once."""
        nodes = expr.c_array()
        prog = rdf_program(C.cast(nodes, C.POINTER(rdf_expr_node)), len(expr.nodes), filter_root, len(value_roots),
                           (C.c_int32 * MAX_VALUES)(*(list(value_roots) + [0] * (MAX_VALUES - len(value_roots)))), SINK_AGG)
        aggs = (rdf_agg_result * MAX_VALUES)()
        if isinstance(cols, Frame):
            fn = self.api._fn("pipeline_frame_dist")
            fn.restype = C.c_int
            self.api._check(fn(self.handle, C.byref(prog), cols.handle, aggs))
        else:
            nchunks = len(cols[0]) if cols else 0
            cc = cols.carr if isinstance(cols, Prepared) else _flat(cols, nchunks)
            fn = self.api._fn("pipeline_dist")
            fn.restype = C.c_int
            self.api._check(fn(self.handle, C.byref(prog), cc, C.c_int32(len(cols)), C.c_int64(nchunks), aggs))
        out = []
        for i in range(len(value_roots)):
            r = aggs[i]
            if r.dtype in (F32, F64):
                out.append(AggResult(r.sum_f64, r.min_f64, r.max_f64, r.count, bool(r.is_some), r.dtype))
            else:
                fix = (lambda x: x + 2 ** 64 if x < 0 else x) if r.dtype == U64 else (lambda x: x)
                out.append(AggResult(fix(r.sum_i64), fix(r.min_i64), fix(r.max_i64), r.count, bool(r.is_some), r.dtype))
        return out

    def group_combine(self, local):
        """(res, rows) of Api.group_pipeline on this rank -> the same over all ranks."""
        res, rows = local
        nv, S = len(res), len(rows)
        isf = [isinstance(res[v][0][0], float) for v in range(nv)]
        out = (rdf_group_result * (nv * S))()
        for v in range(nv):
            for g in range(S):
                s_, c_ = res[v][g]
                r = out[v * S + g]
                r.dtype = F64 if isf[v] else I64
                r.count, r.is_some = c_, int(c_ > 0)
                if isf[v]:
                    r.sum_f64 = s_
                else:
                    r.sum_i64 = s_
        crow = (C.c_int64 * S)(*rows)
        fn = self.api._fn("group_combine")
        fn.restype = C.c_int
        self.api._check(fn(self.handle, out, crow, C.c_int32(S - 1), C.c_int32(nv)))
        return ([[((out[v * S + g].sum_f64 if isf[v] else out[v * S + g].sum_i64), out[v * S + g].count) for g in range(S)] for v in range(nv)],
                [crow[g] for g in range(S)])

    def _stats(self, st):
        self.stats = {"exchange": {EXCHANGE_GROUPS: "partial groups", EXCHANGE_ROWS: "rows"}.get(st.exchange, "none"), "rounds": st.rounds,
                      "local_groups": st.local_groups, "exchange_ms": st.exchange_ms, "exchange_bytes_sent": st.bytes_sent,
                      "exchange_bytes_sent_remote": st.bytes_sent_remote, "exchange_bytes_received": st.bytes_received}

    def groupby_agg(self, keys: Sequence, values: Optional[Sequence], agg, max_groups: int, outs, exchange="auto"):
        """GROUP BY over this rank's shard (device arrays) + the exchange + the merge: -> (keys, values, counts) of the groups
        this rank owns, in the caller's device outputs `outs`."""
        code = self.api.AGGS[agg] if isinstance(agg, str) else int(agg)
        n = len(keys)
        ok, ov, oc = outs
        carr = [(rdf_out * 1)(o.out_struct()) for o in (ok, ov, oc)]
        st = rdf_exchange_stats()
        fn = self.api._fn("groupby_agg_dist")
        fn.restype = C.c_int
        cv = _flat([values], n) if values is not None else None
        self.api._check(fn(self.handle, _flat([keys], n), cv, C.c_int64(n), C.c_int32(code), C.c_int64(max_groups),
                           C.c_int32(self.EXCHANGES[exchange] if isinstance(exchange, str) else int(exchange)), carr[0], carr[1], carr[2], C.byref(st)))
        for o, c_ in zip((ok, ov, oc), carr):
            o.length, o.null_count = c_[0].length, c_[0].null_count
        self._stats(st)
        return ok, ov, oc

    def groupby_agg_frame(self, frame, key_col: int, value_col: int, agg, max_groups: int, exchange="auto") -> "Frame":
        code = self.api.AGGS[agg] if isinstance(agg, str) else int(agg)
        st = rdf_exchange_stats()
        h = C.c_void_p(0)
        fn = self.api._fn("groupby_agg_frame_dist")
        fn.restype = C.c_int
        self.api._check(fn(self.handle, frame.handle, C.c_int32(key_col), C.c_int32(value_col), C.c_int32(code), C.c_int64(max_groups),
                           C.c_int32(self.EXCHANGES[exchange] if isinstance(exchange, str) else int(exchange)), C.byref(h), C.byref(st)))
        self._stats(st)
        return Frame(self.api, h)
