"""A model of the catalog of ahead-of-time specialised kernels: a restatement, in Python, of the registration lists at the
end of rdf_spec_kernel.hip.h and in rdf_spec.hip / rdf_spec_shapes.hip.

For every entry it yields the signature exactly as Prog::sig() prints it, a family label, and programs (`A.Expr` trees with
their filter root, value roots, sink and columns) that the host has to route to that entry:

  canonical  operands in the kernel's own order;
  mirrored   left and right swapped at a random non-empty subset of the nodes where the host swaps back (an arithmetic node
             whose operands differ in depth or are (column, literal): k - c, c / (subtree); a comparison written literal
             first, which the host turns into the mirrored operator);
  aliased    one program column in two column slots (entries with two or more column slots of one dtype).

Shape entries carry runtime operators: they are drawn per slot from a seed.  Literals and predicate thresholds are pairwise
distinct and columns are pairwise distinct seeded data with their own NULL fractions, so a slot bound to the wrong literal,
column or operator changes the answer.  A draw the numpy reference (tests/spec_ref.py) reports a zero divisor for is
rejected and the next seed taken (at most MAX_DRAWS per entry and variant).

The host tries the exact catalog before the shape catalog (spec_choose, rdf_capi_program.inc), so a shape entry's program whose
exact signature is registered too runs on that exact kernel: `exact_signature` restates the host's exact-signature builder,
draws that would be taken away like that are passed over while another draw reaches the entry, and `Program.expect` names
the kernel that has to run.  Entries no variant reaches are listed in UNREACHABLE.
"""
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from rust_dataframe_amd import _abi as A

import spec_ref as R

F64, I64, U64, F32, I32, U32, I16, U16, I8, U8, BOOL = A.F64, A.I64, A.U64, A.F32, A.I32, A.U32, A.I16, A.U16, A.I8, A.U8, A.BOOL
TAG = {F64: "d", I64: "l", U64: "u", F32: "f", I32: "i", U32: "j", I8: "a", U8: "h", I16: "s", U16: "t", BOOL: "b"}   # CType<>::tag
FLOATS = (F64, F32)
SIGNED = (I64, I32, I16, I8)
SINK_STORE, SINK_AGG = 0, 1      # rdfk::SINK_STORE / SINK_AGG as Prog::sig() prints them

ARITH = ("add", "subtract", "multiply", "divide")
TRIG = ("sin", "cos", "tan")
CMPS = ("gt", "ge", "eq", "ne", "lt", "le")
LOGIC = ("and", "or")
MIRRORED_CMP = {"gt": "lt", "ge": "le", "lt": "gt", "le": "ge", "eq": "eq", "ne": "ne"}
CMP_CODES = [A.OP_NAMES[c] for c in CMPS]
UNARY_MATH = ["abs", "acos", "asin", "atan", "cbrt", "ceil", "cos", "cosh", "degrees", "exp", "expm1", "floor", "log10", "log2",
              "radians", "round", "sin", "sinh", "sqrt", "tan", "tanh", "cot", "sec", "csc"]      # reg_unary_f64's 24

# literals of value expressions by literal order, thresholds of the (up to two) comparisons of a predicate
VALUE_LITERALS = {"float": (1.5, -0.25, 3.0, 0.75), "signed": (3, 7, -5, 11), "unsigned": (3, 7, 5, 11)}
THRESHOLDS = {"float": (0.05, -0.1), "signed": (37.0, -64.0), "unsigned": (480.0, 530.0), "u8": (120.0, 140.0)}
NULL_FRACTION = (0.0, 0.1, 0.0, 0.05)      # of pool column j of every dtype
CHUNK_LENS = [1031, 0, 2053, 7]            # two full tiles and a ragged tail at 1024 rows per tile, an empty chunk, one shorter than any tile
MAX_DRAWS = 20


def kind_of(dt):
    return "float" if dt in FLOATS else "signed" if dt in SIGNED else "unsigned"


# ---------------------------------------------------------------- expression nodes as the kernels spell them
@dataclass(frozen=True)
class N:
    kind: str            # col lit cast | A T C G (runtime-operator nodes) | bin un (exact nodes)
    n: int = 0           # slot of col / lit / A / T / C / G; operator code of bin / un; target dtype of cast
    dt: int = 0
    kids: Tuple["N", ...] = ()

    def sig(self) -> str:
        k = [x.sig() for x in self.kids]
        if self.kind == "col":
            return f"c{self.n}{TAG[self.dt]}"
        if self.kind == "lit":
            return f"k{self.n}{TAG[self.dt]}"
        if self.kind == "cast":
            return "{%d %s}" % (self.n, k[0])
        if self.kind in ("A", "C", "G"):
            return f"({self.kind}{self.n} {k[0]} {k[1]})"
        if self.kind == "T":
            return f"[T{self.n} {k[0]}]"
        if self.kind == "bin":
            return f"({self.n} {k[0]} {k[1]})"
        return f"[{self.n} {k[0]}]"

    def depth(self) -> int:      # levels of operators, a cast column being a leaf (ShapeSigBuilder::depth)
        if self.kind in ("col", "lit", "cast"):
            return 0
        return 1 + max(x.depth() for x in self.kids)

    def walk(self):
        yield self
        for x in self.kids:
            yield from x.walk()


def col(i, dt):
    return N("col", i, dt)


def lit(k, dt):
    return N("lit", k, dt)


def cast(to, x):
    return N("cast", to, to, (x,))


def binop(op, a, b):
    code = A.OP_NAMES[op] if isinstance(op, str) else op
    return N("bin", code, BOOL if code in CMP_CODES else a.dt, (a, b))


def unop(op, a):
    return N("un", A.OP_NAMES[op], a.dt, (a,))


@dataclass
class Entry:
    sig: str
    family: str
    pred: Optional[N]
    v0: N
    v1: Optional[N]
    sink: int
    shape: bool          # registered by the shape lists (runtime operators and / or the shape lookup)

    def roots(self):
        return [x for x in (self.pred, self.v0, self.v1) if x is not None]

    def runtime_slots(self):
        return sorted({(x.kind, x.n) for r in self.roots() for x in r.walk() if x.kind in "ATCG"}, key=lambda t: t[1])


# ---------------------------------------------------------------- Build<>: slot numbering of a shape
# a shape: "c" (Lc), "k" (Lk), ("x", FROM) (Lx<FROM>), ("A", X, Y) (Op<X, Y>), ("T", X) (Tr<X>)
def build(sh, S, C, K, dt):
    """-> (node, nS, nC, nK): operator slots in pre-order, every leaf occurrence its own column / literal slot."""
    if sh == "c":
        return col(C, dt), S, C + 1, K
    if sh == "k":
        return lit(K, dt), S, C, K + 1
    if sh[0] == "x":
        return cast(dt, col(C, sh[1])), S, C + 1, K
    if sh[0] == "A":
        x, s1, c1, k1 = build(sh[1], S + 1, C, K, dt)
        y, s2, c2, k2 = build(sh[2], s1, c1, k1, dt)
        return N("A", S, dt, (x, y)), s2, c2, k2
    x, s1, c1, k1 = build(sh[1], S + 1, C, K, dt)
    return N("T", S, dt, (x,)), s1, c1, k1


def Op(x, y):
    return ("A", x, y)


def Tr(x):
    return ("T", x)


O1cc, O1ck = Op("c", "c"), Op("c", "k")
O2ccc, O2cck, O2ckc, O2ckk = Op(O1cc, "c"), Op(O1cc, "k"), Op(O1ck, "c"), Op(O1ck, "k")
SHAPES_BASIC = [O1cc, O1ck, O2ccc, O2cck, O2ckc, O2ckk]
SHAPES_BASIC_TRIG = [Tr("c"), Tr(O1cc), Tr(O1ck)]
SHAPES_DEEP = ([Op(a, b) for a in (O2ccc, O2cck, O2ckc, O2ckk) for b in ("c", "k")]
               + [Op(a, b) for a in (O1cc, O1ck) for b in (O1cc, O1ck)]
               + [Op(a, b) for a in (O2ccc, O2cck, O2ckc, O2ckk) for b in (O1cc, O1ck)])
SHAPES_DEEP_TRIG = [Tr(O2ccc), Tr(O2cck), Tr(O2ckc), Tr(O2ckk)]


def pred_none(pdt):
    return None, 0, 0, 0


def pred1(pdt):
    return N("C", 0, BOOL, (col(0, pdt), lit(0, F64))), 1, 1, 1


def pred2(pdt):
    return N("G", 0, BOOL, (N("C", 1, BOOL, (col(0, pdt), lit(0, F64))), N("C", 2, BOOL, (col(1, pdt), lit(1, F64))))), 3, 2, 2


class Catalog:
    def __init__(self):
        self.entries: Dict[str, Entry] = {}
        self.registrations = 0

    def reg(self, family, pred, v0, v1, sink, shape):
        s = "P:" + (pred.sig() if pred else "-") + ";V:" + v0.sig() + ";" + (v1.sig() if v1 else "-") + ";S:" + str(sink)
        self.registrations += 1
        if s not in self.entries:       # (std::map: a signature registered twice is one kernel)
            self.entries[s] = Entry(s, family, pred, v0, v1, sink, shape)

    def reg_shape_list(self, family, pb, pdt, dt, sink, shapes):
        p, ns, nc, nk = pb(pdt)
        for sh in shapes:
            v, s, c, k = build(sh, ns, nc, nk, dt)
            if c <= 4 and k <= 4 and s <= 8:          # reg_shape_one
                self.reg(family, p, v, None, sink, True)

    def reg_shape_family_lists(self, family, dt, pdt, arith, trig, bare):
        if dt == pdt:
            self.reg_shape_list(family, pred_none, pdt, dt, SINK_STORE, arith)
            self.reg_shape_list(family, pred_none, pdt, dt, SINK_AGG, arith)
            if dt in FLOATS:
                self.reg_shape_list(family, pred_none, pdt, dt, SINK_STORE, trig)
                self.reg_shape_list(family, pred_none, pdt, dt, SINK_AGG, trig)
            if bare:
                self.reg_shape_list(family, pred_none, pdt, dt, SINK_AGG, ["c"])
        self.reg_shape_list(family, pred1, pdt, dt, SINK_AGG, arith)
        self.reg_shape_list(family, pred2, pdt, dt, SINK_AGG, arith)
        if dt in FLOATS:
            self.reg_shape_list(family, pred1, pdt, dt, SINK_AGG, trig)
            self.reg_shape_list(family, pred2, pdt, dt, SINK_AGG, trig)
        if bare:
            self.reg_shape_list(family, pred1, pdt, dt, SINK_AGG, ["c"])
            self.reg_shape_list(family, pred2, pdt, dt, SINK_AGG, ["c"])

    def basic(self, dt, pdt):
        family = f"basic-{TAG[dt]}{TAG[pdt]}"
        self.reg_shape_family_lists(family, dt, pdt, SHAPES_BASIC, SHAPES_BASIC_TRIG, True)
        if dt == pdt:
            self.reg(family, None, pred2(pdt)[0], None, SINK_STORE, True)     # x CMP c AND|OR y CMP d as a mask

    def deep(self, dt, pdt):
        self.reg_shape_family_lists(f"deep-{TAG[dt]}{TAG[pdt]}", dt, pdt, SHAPES_DEEP, SHAPES_DEEP_TRIG, False)

    def cast_family(self, dt):
        family = f"cast-{TAG[dt]}"
        for frm in (F64, I64, U64, F32, I32, U32, I16, U16, I8, U8):
            if frm == dt:
                continue
            self.reg_shape_list(family, pred_none, dt, dt, SINK_STORE, [Op("c", ("x", frm))])
            self.reg_shape_list(family, pred_none, dt, dt, SINK_AGG, [Op("c", ("x", frm))])
            self.reg(family, None, cast(dt, col(0, frm)), None, SINK_STORE, False)
            if dt in FLOATS:
                self.reg_shape_list(family, pred_none, dt, dt, SINK_STORE, [Tr(("x", frm))])
                self.reg_shape_list(family, pred_none, dt, dt, SINK_AGG, [Tr(("x", frm))])

    def byte_family(self, b):
        family = f"byte-{TAG[b]}"
        x, k = col(0, b), lit(0, F64)
        self.reg_shape_list(family, pred_none, b, b, SINK_AGG, ["c"])
        self.reg(family, None, cast(F64, x), None, SINK_AGG, False)
        self.reg_shape_list(family, pred1, b, b, SINK_AGG, ["c"])
        self.reg_shape_list(family, pred2, b, b, SINK_AGG, ["c"])
        self.reg_shape_list(family, pred1, b, F64, SINK_AGG, ["c"])
        self.reg_shape_list(family, pred1, b, I64, SINK_AGG, ["c"])
        self.reg(family, None, pred2(b)[0], None, SINK_STORE, True)
        for c in CMPS:
            self.reg(family, None, binop(c, x, k), None, SINK_STORE, False)
        for frm in (I64, I32, I16, F64):
            self.reg(family, None, cast(b, col(0, frm)), None, SINK_STORE, False)

    def exact(self):
        D0, D1, D2 = col(0, F64), col(1, F64), col(2, F64)
        L0, L1, L3 = col(0, I64), col(1, I64), col(3, I64)
        W0, W1 = col(0, U64), col(1, U64)
        KD0, KL0, KF0, KI0 = lit(0, F64), lit(0, I64), lit(0, F32), lit(0, I32)
        F0, F1, I0, I1, J0, J1 = col(0, F32), col(1, F32), col(0, I32), col(1, I32), col(0, U32), col(1, U32)
        for v in (D0, L0, W0, cast(F64, L0), cast(F64, W0), F0, I0, J0):        # aggregates of a plain column, avg
            self.reg("exact-agg", None, v, None, SINK_AGG, False)
        for c in CMPS:                                                           # reg_cmp_family
            fam = "exact-cmp"
            self.reg(fam, binop(c, D0, KD0), D0, None, SINK_AGG, False)
            self.reg(fam, binop(c, D0, KD0), D1, None, SINK_AGG, False)
            self.reg(fam, binop(c, D0, KD0), L1, None, SINK_AGG, False)
            self.reg(fam, binop(c, L0, KD0), L0, None, SINK_AGG, False)
            self.reg(fam, None, binop(c, D0, KD0), None, SINK_STORE, False)
            self.reg(fam, None, binop(c, L0, KD0), None, SINK_STORE, False)
            self.reg(fam, None, binop(c, D0, D1), None, SINK_STORE, False)
            self.reg(fam, None, binop(c, L0, L1), None, SINK_STORE, False)
            self.reg(fam, binop(c, F0, KD0), F0, None, SINK_AGG, False)
            self.reg(fam, binop(c, I0, KD0), I0, None, SINK_AGG, False)
            self.reg(fam, None, binop(c, F0, KD0), None, SINK_STORE, False)
            self.reg(fam, None, binop(c, I0, KD0), None, SINK_STORE, False)
        for o in ARITH:                                                          # reg_arith_family
            for a, b in ((D0, D1), (L0, L1), (W0, W1), (D0, KD0), (L0, KL0), (F0, F1), (I0, I1), (J0, J1), (F0, KF0), (I0, KI0)):
                self.reg("exact-arith", None, binop(o, a, b), None, SINK_STORE, False)
        for o in ("atan2", "hypot", "log"):
            self.reg("exact-misc", None, binop(o, D0, D1), None, SINK_STORE, False)
        for o in UNARY_MATH:                                                     # reg_unary_f64
            self.reg("exact-unary", None, unop(o, D0), None, SINK_STORE, False)
            self.reg("exact-unary", None, unop(o, binop("add", D0, KD0)), None, SINK_AGG, False)
            self.reg("exact-unary", None, unop(o, D0), None, SINK_AGG, False)
            self.reg("exact-unary", None, unop(o, F0), None, SINK_STORE, False)
        self.reg("exact-misc", None, unop("abs", L0), None, SINK_STORE, False)
        self.reg("exact-misc", None, unop("abs", I0), None, SINK_STORE, False)
        for to, frm in ((F64, L0), (I64, D0), (F64, W0), (U64, D0), (F32, I0), (I32, F0)):
            self.reg("exact-misc", None, cast(to, frm), None, SINK_STORE, False)
        fma = binop("add", binop("multiply", D0, D1), D2)
        self.reg("exact-misc", None, fma, L3, SINK_AGG, False)
        self.reg("exact-misc", None, fma, None, SINK_AGG, False)
        self.reg("exact-misc", None, fma, None, SINK_STORE, False)


def make_catalog() -> Catalog:
    c = Catalog()
    for dt, pdt in ((F64, F64), (I64, I64), (F64, I64), (I64, F64)):                         # rdf_spec.hip build_registry
        c.basic(dt, pdt)
    c.deep(F64, F64)                                                                       # rdf_spec_shapes.hip, TU 1-3
    c.deep(I64, I64)
    c.deep(F64, I64)
    c.deep(I64, F64)
    for dt, pdt in ((U64, U64), (F32, F32), (I32, I32), (U32, U32), (F32, I32), (I32, F32)):   # TU 4
        c.basic(dt, pdt)
    for dt in (F32, I32, U32, U64):                                                        # TU 5-6
        c.deep(dt, dt)
    c.basic(I16, I16)                                                                      # TU 7
    c.basic(U16, U16)
    c.deep(I16, I16)
    c.deep(U16, U16)
    c.byte_family(I8)
    c.byte_family(U8)
    for dt in (F64, I64, U64, F32, I32, U32, I16, U16):                                    # TU 8
        c.cast_family(dt)
    c.exact()
    return c


CATALOG = make_catalog()
ENTRIES: List[Entry] = list(CATALOG.entries.values())
FAMILIES = sorted({e.family for e in ENTRIES})

# Entries no program reaches through the public ABI: the exact catalog is tried first (run_program), and for these every
# program of the entry's shape — whatever its runtime operators, operand order or column reuse — has an exact signature that
# is registered as well.  test_spec_catalog.py asserts that these, and only these, never run.
_SHADOW_CMP_AGG = "every x CMP c -> aggregates program of these dtypes is one of reg_cmp_family's exact kernels (P:({op} ...))"
_SHADOW_UNARY = "sin / cos / tan of a plain column is reg_unary_f64's exact kernel ([{op} ...])"
UNREACHABLE: Dict[str, str] = {
    "P:(C0 c0d k0d);V:c1d;-;S:1": _SHADOW_CMP_AGG,       # value column = another f64 column, or (aliased) the predicate's
    "P:(C0 c0d k0d);V:c1l;-;S:1": _SHADOW_CMP_AGG,
    "P:-;V:[T0 c0d];-;S:0": _SHADOW_UNARY,
    "P:-;V:[T0 c0d];-;S:1": _SHADOW_UNARY,
    "P:-;V:[T0 c0f];-;S:0": _SHADOW_UNARY,
}


# ---------------------------------------------------------------- the columns every program draws from
_POOL: Dict[tuple, list] = {}


def element_offset(dt):
    """Every slice starts this many elements into its buffers: 16 bytes, so the specialised path is eligible whatever the
    widest element of the program, and a non-zero bit offset into the validity bitmap (2, 4, 8 or 16)."""
    return 16 // np.dtype(A.NP_OF[dt]).itemsize


def pool_column(dt, j, kind="plain"):
    """Pool column j (0..3) of a dtype as chunks of CHUNK_LENS.  plain: floats uniform(-1, 1), integers |v| <= 1000 (the type's
    range if narrower), unsigned 1..1000, never zero.  cast: a cast operand — |v| >= 1, every 97th value one the narrower
    targets cannot hold, NaN at a few rows of float columns (float -> integer makes them NULL)."""
    key = (dt, j, kind)
    if key in _POOL:
        return _POOL[key]
    rng = np.random.default_rng([2029, dt, j, 0 if kind == "plain" else 1])
    npdt = A.NP_OF[dt]
    chunks = []
    for n in CHUNK_LENS:
        if dt in FLOATS:
            if kind == "plain":
                v = rng.uniform(-1.0, 1.0, n)
                v[v == 0] = 0.5
            else:
                v = rng.uniform(1.0, 900.0, n) * rng.choice([-1.0, 1.0], n)
                v[::97] = 1e30
                v[5::131] = np.nan
        else:
            info = np.iinfo(npdt)
            lim = 900 if kind == "cast" else 1000
            lo, hi = max(int(info.min), -lim), min(int(info.max), lim)
            v = rng.integers(lo, hi, n, endpoint=True)
            v[v == 0] = 1
            if kind == "cast":
                v[::97] = {I64: 2 ** 40, U64: 2 ** 40, I32: 2 ** 30, U32: 2 ** 31 + 5, I16: 30000, U16: 60000, I8: -100, U8: 200}[dt]
        with np.errstate(all="ignore"):
            v = np.asarray(v).astype(npdt)
        nf = NULL_FRACTION[j]
        valid = rng.uniform(size=n) >= nf if nf > 0 else None
        chunks.append(A.HostArray.from_numpy(v, valid=valid, offset=element_offset(dt), dtype=dt, rng=rng))
    _POOL[key] = chunks
    return chunks


def flat_column(key):
    """(dtype, values, valid) over all rows of a pool column, for the reference."""
    fk = ("flat",) + key
    if fk not in _POOL:
        ch = pool_column(*key)
        _POOL[fk] = (key[0], np.concatenate([c.to_numpy() for c in ch]), np.concatenate([c.valid_mask() for c in ch]))
    return _POOL[fk]


# ---------------------------------------------------------------- the host's exact-signature builder, restated
def exact_signature(expr: A.Expr, filter_root, value_roots, sink, cdt) -> str:
    """SpecSigBuilder (rdf_capi.cpp): program columns numbered by first use (predicate first), every literal its own slot,
    a comparison written literal-first turned round, casts to the same type dropped."""
    nodes = expr.nodes
    cols: List[int] = []
    nlit = [0]

    def leaf(idx, dom):
        nd = nodes[idx]
        if nd.kind == A.NODE_COLUMN:
            if nd.column not in cols:
                cols.append(nd.column)
            return f"c{cols.index(nd.column)}{TAG[cdt[nd.column]]}"
        nlit[0] += 1
        return f"k{nlit[0] - 1}{TAG[dom]}"

    def node(idx, dom):
        nd = nodes[idx]
        if nd.kind != A.NODE_OP:
            return leaf(idx, dom)
        op = nd.op
        if nd.rhs >= 0:
            l, r, o = nd.lhs, nd.rhs, op
            d = F64 if op in CMP_CODES else R.infer(nodes, cdt, l)
            if op in CMP_CODES and nodes[l].kind == A.NODE_SCALAR and nodes[r].kind != A.NODE_SCALAR:
                l, r, o = r, l, A.OP_NAMES[MIRRORED_CMP[R.OP_NAME[op]]]
            a = node(l, d)
            b = node(r, d)
            return f"({o} {a} {b})"
        if op == A.OP_CAST:
            frm = R.infer(nodes, cdt, nd.lhs)
            if frm == nd.dtype:
                return node(nd.lhs, dom)
            return "{%d %s}" % (nd.dtype, node(nd.lhs, frm))
        return f"[{op} {node(nd.lhs, R.infer(nodes, cdt, nd.lhs))}]"

    s = "P:" + (node(filter_root, F64) if filter_root >= 0 else "-")
    s += ";V:" + node(value_roots[0], R.infer(nodes, cdt, value_roots[0]))
    s += ";" + (node(value_roots[1], R.infer(nodes, cdt, value_roots[1])) if len(value_roots) > 1 else "-")
    return s + ";S:" + str(sink)


# ---------------------------------------------------------------- programs
VARIANTS = ("canonical", "mirrored", "aliased")


@dataclass
class Program:
    entry: Entry
    variant: str
    seed: int
    expr: A.Expr
    filter_root: int
    value_roots: List[int]
    sink: int
    columns: List[tuple]                         # program column c = pool column (dtype, j, kind)
    ops: Dict[int, Tuple[str, str, bool]]        # runtime slot -> (A / T / C / G, operator, mirrored)
    expect: str                                  # signature of the kernel that has to run
    ref: object = None                           # the reference's result (spec_ref.Val for STORE, [spec_ref.Agg] for AGG)
    memo: dict = field(default_factory=dict)

    @property
    def out_dtype(self):
        return R.infer(self.expr.nodes, [c[0] for c in self.columns], self.value_roots[0])

    def host_columns(self):
        return [pool_column(*c) for c in self.columns]

    def flat_columns(self):
        return [flat_column(c) for c in self.columns]


def _mirrorable(x: N) -> bool:
    """The host swaps the operands of this node back into the kernel's order (ShapeSigBuilder::node)."""
    if x.kind == "C":
        return True
    if x.kind != "A":
        return False
    a, b = x.kids
    return a.depth() != b.depth() or (a.kind == "col" and b.kind == "lit")


def _column_slots(e: Entry):
    """slot -> (dtype, data kind), literal slot -> (dtype, role, dtype of the column it is compared with)."""
    cslots, lslots = {}, {}

    def visit(x: N, parent: Optional[N]):
        if x.kind == "col":
            cslots[x.n] = (x.dt, "cast" if parent is not None and parent.kind == "cast" else "plain")
        elif x.kind == "lit":
            is_thr = parent is not None and (parent.kind == "C" or (parent.kind == "bin" and parent.n in CMP_CODES))
            lslots[x.n] = (x.dt, "thr" if is_thr else "val", parent.kids[0].dt if is_thr else x.dt)
        for k in x.kids:
            visit(k, x)

    for r in e.roots():
        visit(r, None)
    return cslots, lslots


def draw(e: Entry, variant: str, attempt: int) -> Optional[Program]:
    """One seeded program of an entry, or None where the variant does not exist for it."""
    cslots, lslots = _column_slots(e)
    mirrorable = sorted({x.n for r in e.roots() for x in r.walk() if _mirrorable(x)})
    by_dt: Dict[int, List[int]] = {}
    for s in sorted(cslots):
        by_dt.setdefault(cslots[s], []).append(s)
    alias_groups = [g for g in by_dt.values() if len(g) >= 2]
    if variant != "canonical" and not e.shape:
        return None
    if variant == "mirrored" and not mirrorable:
        return None
    if variant == "aliased" and not alias_groups:
        return None
    seed = [zlib.crc32(e.sig.encode()), VARIANTS.index(variant), attempt]
    rng = np.random.default_rng(seed)
    # runtime operators, one per slot
    ops = {}
    for kind, s in e.runtime_slots():
        ops[s] = (kind, str(rng.choice({"A": ARITH, "T": TRIG, "C": CMPS, "G": LOGIC}[kind])), False)
    if variant == "mirrored":
        pick = [s for s in mirrorable if rng.uniform() < 0.5] or [int(rng.choice(mirrorable))]
        for s in pick:
            ops[s] = (ops[s][0], ops[s][1], True)
    # columns: distinct pool columns per slot (two slots share one in the aliased variant), in a shuffled program order
    pool = {}
    for (dt, kind), slots in by_dt.items():
        for s, j in zip(slots, rng.permutation(4)):
            pool[s] = (dt, int(j), kind)
    if variant == "aliased":
        g = alias_groups[int(rng.integers(len(alias_groups)))]
        a, b = sorted(rng.choice(g, 2, replace=False).tolist())
        pool[b] = pool[a]
    columns = sorted(set(pool.values()))
    columns = [columns[i] for i in rng.permutation(len(columns))]
    # literals: thresholds by comparison order, value literals by literal order
    literal, nthr, nval = {}, 0, 0
    for s in sorted(lslots):
        dt, role, cdt = lslots[s]
        if role == "thr":
            literal[s] = THRESHOLDS["u8" if cdt == U8 else kind_of(cdt)][nthr]
            nthr += 1
        else:
            literal[s] = VALUE_LITERALS[kind_of(dt)][nval]
            nval += 1
    expr = A.Expr()

    def emit(x: N) -> int:
        if x.kind == "col":
            return expr.col(columns.index(pool[x.n]))
        if x.kind == "lit":
            return expr.scalar(literal[x.n], dtype=x.dt)
        if x.kind == "cast":
            return expr.cast(emit(x.kids[0]), x.n)
        if x.kind in ("T", "un"):
            return expr.op(ops[x.n][1] if x.kind == "T" else x.n, emit(x.kids[0]))
        a, b = emit(x.kids[0]), emit(x.kids[1])
        if x.kind == "bin":
            return expr.op(x.n, a, b)
        _, name, mirrored = ops[x.n]
        return expr.op(name, b, a) if mirrored else expr.op(name, a, b)

    filter_root = emit(e.pred) if e.pred is not None else -1
    value_roots = [emit(e.v0)] + ([emit(e.v1)] if e.v1 is not None else [])
    exact = exact_signature(expr, filter_root, value_roots, e.sink, [c[0] for c in columns])
    expect = exact if (exact in CATALOG.entries or not e.shape) else e.sig
    return Program(e, variant, attempt, expr, filter_root, value_roots, e.sink, columns, ops, expect)


def reference(p: Program):
    """The numpy reference's result of a program (raises spec_ref.ZeroDivisor)."""
    if p.ref is None:
        cols = p.flat_columns()
        p.ref = R.run_store(p.expr, cols, p.value_roots[0]) if p.sink == SINK_STORE else R.run_agg(p.expr, cols, p.value_roots, p.filter_root)
    return p.ref


_PROGRAMS: Dict[Tuple[str, str], Optional[Program]] = {}


def program(e: Entry, variant: str) -> Optional[Program]:
    """The accepted draw of (entry, variant): the first seed that reaches the entry's own kernel and divides by no zero; where
    the exact catalog takes every such draw, the first that divides by no zero.  None: the variant does not exist for the
    entry.  Raises if MAX_DRAWS seeds are all rejected."""
    key = (e.sig, variant)
    if key in _PROGRAMS:
        return _PROGRAMS[key]
    taken_away = []
    found = None
    for attempt in range(MAX_DRAWS):
        p = draw(e, variant, attempt)
        if p is None:
            break
        if p.expect != e.sig:
            taken_away.append(p)
            continue
        try:
            reference(p)
        except R.ZeroDivisor:
            continue
        found = p
        break
    else:
        for p in taken_away:
            try:
                reference(p)
            except R.ZeroDivisor:
                continue
            found = p
            break
        if found is None:
            raise AssertionError(f"{e.sig} ({variant}): no draw out of {MAX_DRAWS} was accepted")
    _PROGRAMS[key] = found
    return found


def programs(family: Optional[str] = None) -> List[Program]:
    out = []
    for e in ENTRIES:
        if family is None or e.family == family:
            out += [p for p in (program(e, v) for v in VARIANTS) if p is not None]
    return out
