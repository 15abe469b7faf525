"""A numpy evaluator of rdf_program trees, written from include/rdf_mi355x.h and independent of the C oracle.

It walks the `A.Expr` node array itself (not the catalog model's trees), over whole columns:

  * arithmetic in the node's dtype, one rounding per operation (numpy does not contract); integers wrap at the value's width,
    integer division truncates toward zero and MIN / -1 wraps; a zero divisor where both operands are valid raises ZeroDivisor
    (RDF_DIVIDE_BY_ZERO in the product);
  * comparisons in f64: both sides cast to f64; and / or are NULL where either side is NULL;
  * a value is NULL where any input is NULL; a NULL or false predicate drops the row;
  * casts as rdf_cast documents them: a value the target cannot hold (NaN or out of range into an integer) is NULL, floats
    truncate toward zero when the truncated value fits, int -> float and float -> float always succeed;
  * a unary math function at the root of a value is carried EXACTLY (tests/exact_ref.py: hi + lo), with the value rounded once
    to the dtype next to it, so a caller can hold the device to an ulp bound;
  * the aggregating sink returns count / sum / min / max as rdf_agg_result documents: integer sums wrapped to the value's
    width, float sums as the correctly rounded sum (math.fsum) of the selected values, together with those values.
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from rust_dataframe_amd import _abi as A

import exact_ref as X

FLOATS = (A.F32, A.F64)
SIGNED = (A.I8, A.I16, A.I32, A.I64)
UNSIGNED = (A.U8, A.U16, A.U32, A.U64)
OP_NAME = {v: k for k, v in A.OP_NAMES.items()}
ARITH = (A.OP_ADD, A.OP_SUB, A.OP_MUL, A.OP_DIV)
CMP = {A.OP_GT: np.greater, A.OP_GE: np.greater_equal, A.OP_EQ: np.equal, A.OP_NE: np.not_equal, A.OP_LT: np.less,
       A.OP_LE: np.less_equal}


class ZeroDivisor(Exception):
    """A zero divisor at a row where both operands are valid."""


@dataclass
class Val:
    dt: int
    v: np.ndarray                    # values (bool for RDF_BOOL); whatever at NULL rows
    valid: np.ndarray                # bool
    op: Optional[str] = None         # a unary math function at the root: its name, and the exact result hi + lo
    hi: Optional[np.ndarray] = None
    lo: Optional[np.ndarray] = None


@dataclass
class Agg:
    dt: int
    count: int
    sum: object                      # int (wrapped to the value's width) or float (math.fsum of `values`, exact parts included)
    min: object
    max: object
    values: np.ndarray               # the selected values, in the value's dtype (rounded once where `op` is set)
    op: Optional[str] = None
    hi: Optional[np.ndarray] = None  # exact parts of the selected values where `op` is set
    lo: Optional[np.ndarray] = None


def int_range(dt):
    info = np.iinfo(A.NP_OF[dt])
    return int(info.min), int(info.max)


def wrap_int(x: int, dt: int) -> int:
    bits = 8 * np.dtype(A.NP_OF[dt]).itemsize
    x &= (1 << bits) - 1
    if dt in SIGNED and x >= 1 << (bits - 1):
        x -= 1 << bits
    return x


def infer(nodes, cdt, idx):
    nd = nodes[idx]
    if nd.kind == A.NODE_COLUMN:
        return cdt[nd.column]
    if nd.kind == A.NODE_SCALAR:
        return nd.dtype
    if nd.op in ARITH or nd.op in (A.OP_ATAN2, A.OP_HYPOT, A.OP_LOG):
        return infer(nodes, cdt, nd.lhs)
    if nd.op in CMP or nd.op in (A.OP_AND, A.OP_OR, A.OP_NOT):
        return A.BOOL
    if nd.op == A.OP_CAST:
        return nd.dtype
    return infer(nodes, cdt, nd.lhs)      # unary math


def _literal(nd, dom, n):
    """A scalar node's payload converted to `dom` (the tests' literals are written in the domain they are used in, or as f64
    thresholds of comparisons)."""
    if nd.dtype == A.NULLTYPE:
        raise NotImplementedError("NULL literal")
    payload = (float(np.float32(nd.f64)) if nd.dtype == A.F32 else float(nd.f64)) if nd.dtype in FLOATS else wrap_int(int(nd.i64), nd.dtype)
    if dom in FLOATS:
        return np.full(n, payload, dtype=A.NP_OF[dom])
    if isinstance(payload, float):
        raise NotImplementedError("float literal in an integer domain")
    return np.full(n, wrap_int(payload, dom), dtype=A.NP_OF[dom])


def _int_div(x, y):
    """Truncating division of same-dtype integer vectors with no zero in y; MIN / -1 wraps."""
    with np.errstate(all="ignore"):
        if x.dtype.kind == "u":
            return x // y
        safe = np.where(y == -1, 1, y)
        q = x // safe                                   # floor
        r = x - q * safe
        q = q + ((r != 0) & ((x < 0) != (safe < 0)))    # toward zero
        return np.where(y == -1, (0 - x).astype(x.dtype), q).astype(x.dtype)


def cast(val: Val, to: int) -> Val:
    if val.dt == to:
        return val
    src = val.v
    if to in FLOATS:
        with np.errstate(all="ignore"):
            return Val(to, src.astype(A.NP_OF[to]), val.valid.copy())
    lo, hi = int_range(to)
    out = np.zeros(len(src), dtype=A.NP_OF[to])
    fits = np.zeros(len(src), dtype=bool)
    for i, x in enumerate(src.tolist()):        # Python integers: no width to overflow
        if isinstance(x, float):
            if not math.isfinite(x):
                continue
            x = math.trunc(x)
        if lo <= x <= hi:
            out[i] = x
            fits[i] = True
    return Val(to, out, val.valid & fits)


def evaluate(expr: A.Expr, cols, idx: int, dom: Optional[int] = None) -> Val:
    """cols[c] = (dtype, values, valid) over all rows."""
    nodes = expr.nodes
    cdt = [c[0] for c in cols]
    n = len(cols[0][1]) if cols else 0
    nd = nodes[idx]
    if nd.kind == A.NODE_COLUMN:
        dt, v, valid = cols[nd.column]
        return Val(dt, v, valid)
    if nd.kind == A.NODE_SCALAR:
        dom = nd.dtype if dom is None else dom
        return Val(dom, _literal(nd, dom, n), np.ones(n, dtype=bool))
    op = nd.op
    if op == A.OP_CAST:
        return cast(evaluate(expr, cols, nd.lhs, infer(nodes, cdt, nd.lhs)), nd.dtype)
    if op in CMP:
        l, r = evaluate(expr, cols, nd.lhs, A.F64), evaluate(expr, cols, nd.rhs, A.F64)
        with np.errstate(all="ignore"):
            return Val(A.BOOL, CMP[op](l.v.astype(np.float64), r.v.astype(np.float64)), l.valid & r.valid)
    if op in (A.OP_AND, A.OP_OR):
        l, r = evaluate(expr, cols, nd.lhs), evaluate(expr, cols, nd.rhs)
        assert l.dt == A.BOOL and r.dt == A.BOOL
        return Val(A.BOOL, (l.v & r.v) if op == A.OP_AND else (l.v | r.v), l.valid & r.valid)
    if op in ARITH:
        dt = infer(nodes, cdt, nd.lhs)
        l, r = evaluate(expr, cols, nd.lhs, dt), evaluate(expr, cols, nd.rhs, dt)
        assert l.dt == dt and r.dt == dt, "arithmetic operands share one dtype"
        valid = l.valid & r.valid
        with np.errstate(all="ignore"):
            if op == A.OP_ADD:
                v = l.v + r.v
            elif op == A.OP_SUB:
                v = l.v - r.v
            elif op == A.OP_MUL:
                v = l.v * r.v
            else:
                zero = r.v == 0
                if (zero & valid).any():
                    raise ZeroDivisor()
                y = np.where(zero, np.ones(1, dtype=r.v.dtype), r.v)
                v = (l.v / y) if dt in FLOATS else _int_div(l.v, y)
                v = np.where(zero, np.zeros(1, dtype=v.dtype), v)
        assert v.dtype == np.dtype(A.NP_OF[dt])
        return Val(dt, v, valid)
    name = OP_NAME[op]
    if name in X.BINARY:
        l, r = evaluate(expr, cols, nd.lhs), evaluate(expr, cols, nd.rhs)
        assert l.dt == r.dt and l.dt in FLOATS
        hi, lo = X.exact_binary(name, l.v, r.v)
        return Val(l.dt, X.round_to(hi, lo, A.NP_OF[l.dt]), l.valid & r.valid, name, hi, lo)
    x = evaluate(expr, cols, nd.lhs)
    if name == "abs" and x.dt in SIGNED:
        with np.errstate(all="ignore"):
            return Val(x.dt, np.where(x.v < 0, (0 - x.v).astype(x.v.dtype), x.v), x.valid)
    if name in X.UNARY and x.dt in FLOATS:
        hi, lo = X.exact_unary(name, x.v)
        return Val(x.dt, X.round_to(hi, lo, A.NP_OF[x.dt]), x.valid, name, hi, lo)
    raise NotImplementedError(f"op {name} over dtype {x.dt}")


def run_store(expr, cols, value_root) -> Val:
    return evaluate(expr, cols, value_root)


def run_agg(expr, cols, value_roots, filter_root=-1):
    n = len(cols[0][1])
    keep = np.ones(n, dtype=bool)
    if filter_root >= 0:
        p = evaluate(expr, cols, filter_root)
        assert p.dt == A.BOOL
        keep = p.valid & p.v.astype(bool)
    out = []
    for root in value_roots:
        val = evaluate(expr, cols, root)
        sel = keep & val.valid
        v = val.v[sel]
        hi = val.hi[sel] if val.op else None
        lo = val.lo[sel] if val.op else None
        if val.dt in FLOATS:
            parts = v.astype(np.float64).tolist() if not val.op else hi.tolist() + lo.tolist()
            with np.errstate(all="ignore"):
                fin = v[~np.isnan(v)]
            if all(math.isfinite(t) for t in parts):
                s = math.fsum(parts)
            else:       # +inf and -inf (or a NaN) make NaN, infinities of one sign that infinity
                s = float(np.sum(np.asarray(parts, dtype=np.float64)))
            mn = (float(fin.min()) if len(fin) else float("nan")) if len(v) else 0.0
            mx = (float(fin.max()) if len(fin) else float("nan")) if len(v) else 0.0
            out.append(Agg(val.dt, len(v), s if len(v) else 0.0, mn, mx, v, val.op, hi, lo))
        else:
            ints = [int(t) for t in v.tolist()]
            out.append(Agg(val.dt, len(ints), wrap_int(sum(ints), val.dt), min(ints) if ints else 0, max(ints) if ints else 0, v))
    return out
