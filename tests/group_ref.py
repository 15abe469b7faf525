"""The executable definition of rdf_group_pipeline (include/rdf_mi355x.h, "fused grouped aggregation") in plain numpy and
Python integers, independent of the C oracle.

A column is (values, valid | None) over ALL rows (`columns_of` concatenates a chunk list).  The expression program is an
`A.Expr` node array over add / subtract / multiply, cast, the comparisons, and / or and literals, evaluated by
spec_ref.evaluate (one rounding per operation, integers wrap at the value's width, comparisons in f64, NULL where any input
is NULL).  `run` returns a `Model` in the layout of rdf_group_result, or a `Failure` carrying the status the call must fail
with.

The header's semantics:
  * a row is dropped when the predicate is false or NULL;
  * a NULL group id goes to slot `ngroups`;
  * a valid id outside [0, ngroups) at a row that passed the filter is RDF_COMPUTE_ERROR; a negative id is outside at every
    key width (a signed id is sign-extended before it is compared), an unsigned or Boolean id is taken as it is;
  * count = rows of the group minus the value's NULLs, group_rows = SQL count(*), is_some = count > 0;
  * integer and Boolean values are summed in wrapping 64-bit arithmetic after sign- or zero-extension (not re-wrapped to the
    value's width; an unsigned 64-bit sum is reported through the signed field);
  * Float32 values are widened to f64 exactly; a float sum's reference is math.fsum over the group's values in f64.

Where the header is silent the oracle decides (tests/test_group_ref.py holds this model to it):
  * the sum of a group without a valid value is 0 (0.0 for floats), and so is everything when no row passes;
  * a Boolean value (a comparison) is summed as 0 / 1 into the integer field;
  * a float group holding a NaN, or infinities of both signs, sums to NaN; infinities of one sign to that infinity;
  * argument errors come before the rows are looked at: ngroups < 1, nvalues outside [1, 8], (ngroups + 1) * nvalues > 1024
    and a group id expression that is not integer-valued are RDF_INVALID_ARGUMENT even where an id is out of range.

`check` is the comparison both the CPU and the GPU tests use: counts, rows, is_some and integer sums exactly, a float sum
within the bound that holds for EVERY order and tree of correctly rounded f64 additions (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., section 4.2),
    |got - fsum| <= gamma(n_g - 1) * sum|x_i| + spacing(|fsum|) / 2,       gamma from exact_ref at u = 2^-53,
evaluated in exact rational arithmetic.  The half spacing is the reference's own rounding; for n_g <= 1 the value itself
must come back.  The x_i are the model's own values: + - * are correctly rounded, so the bound has no slack for evaluation.
"""
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import List

import numpy as np

from rust_dataframe_amd import _abi as A

import exact_ref as X
import spec_ref as S

MASK64 = (1 << 64) - 1


@dataclass
class Failure:
    status: int
    why: str = ""


@dataclass
class Model:
    ngroups: int
    dtypes: List[int]                 # value dtypes
    sums: list                        # [v][g]: Python int (wrapped to signed 64 bits) or float (math.fsum)
    counts: list                      # [v][g]
    rows: list                        # [g]
    values: list                      # [v][g]: the group's valid values as an f64 / integer numpy vector

    def is_some(self, v, g):
        return int(self.counts[v][g] > 0)

    def as_result(self):
        """(res, rows) as Api.group_pipeline(..., with_some=True) returns them."""
        S_ = self.ngroups + 1
        return [[(self.sums[v][g], self.counts[v][g], self.is_some(v, g)) for g in range(S_)] for v in range(len(self.dtypes))], list(self.rows)


def columns_of(cols):
    """cols[c] = chunk list of HostArrays -> [(values, valid | None)] over all rows."""
    out = []
    for col in cols:
        v = np.concatenate([ch.to_numpy() for ch in col]) if col else np.zeros(0)
        valid = np.concatenate([ch.valid_mask() for ch in col]) if any(ch.validity is not None for ch in col) else None
        out.append((v, valid))
    return out


def wrap64(x: int) -> int:
    x &= MASK64
    return x - (1 << 64) if x >> 63 else x


def float_sum(vals: np.ndarray) -> float:
    """math.fsum of f64 values; a non-finite group by kind."""
    if len(vals) == 0:
        return 0.0
    if np.isnan(vals).any() or (np.isposinf(vals).any() and np.isneginf(vals).any()):
        return float("nan")
    if np.isposinf(vals).any():
        return float("inf")
    if np.isneginf(vals).any():
        return float("-inf")
    return math.fsum(vals.tolist())


def run(expr, cols, value_roots, group_root, ngroups, filter_root=-1):
    """cols[c] = (values, valid | None), numpy dtype = column dtype (bool for RDF_BOOL)."""
    nv = len(value_roots)
    if nv < 1 or nv > A.MAX_GROUP_VALUES:
        return Failure(A.RDF_INVALID_ARGUMENT, "nvalues out of range")
    if ngroups < 1 or (ngroups + 1) * nv > A.MAX_GROUP_SLOTS:
        return Failure(A.RDF_INVALID_ARGUMENT, "(ngroups + 1) * nvalues must be in [2, 1024]")
    n = len(cols[0][0]) if cols else 0
    ecols = [(A.dtype_code(v.dtype), v, np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)) for v, valid in cols]
    cdt = [c[0] for c in ecols]
    if filter_root >= 0 and S.infer(expr.nodes, cdt, filter_root) != A.BOOL:
        return Failure(A.RDF_INVALID_ARGUMENT, "predicate root must be boolean")
    gdt = S.infer(expr.nodes, cdt, group_root)
    if gdt in S.FLOATS:
        return Failure(A.RDF_INVALID_ARGUMENT, "group id expression must be integer-valued")
    keep = np.ones(n, dtype=bool)
    if filter_root >= 0:
        p = S.evaluate(expr, ecols, filter_root)
        keep = p.valid & p.v.astype(bool)
    gid = S.evaluate(expr, ecols, group_root)
    if gid.v.dtype == np.bool_:
        wide = gid.v.astype(np.int64)
        outside = wide >= ngroups
    elif gid.v.dtype.kind == "u":                             # an unsigned id is taken as it is: never negative
        wide = gid.v.astype(np.uint64)
        outside = wide >= np.uint64(ngroups)
    else:                                                     # a signed id is sign-extended: negative at every width
        wide = gid.v.astype(np.int64)
        outside = (wide < 0) | (wide >= ngroups)
    bad = keep & gid.valid & outside
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        return Failure(A.RDF_COMPUTE_ERROR, f"group id {int(gid.v[i])} outside [0, {ngroups}) at row {i}")
    slot = np.where(keep, np.where(gid.valid, np.where(outside, 0, wide).astype(np.int64), ngroups), -1).astype(np.int64)
    S_ = ngroups + 1
    rows = np.bincount(slot[keep], minlength=S_).tolist() if n else [0] * S_
    order = np.argsort(slot, kind="stable")
    bounds = np.searchsorted(slot[order], np.arange(S_ + 1))
    dtypes, sums, counts, values = [], [], [], []
    for root in value_roots:
        val = S.evaluate(expr, ecols, root)
        dtypes.append(val.dt)
        isf = val.dt in S.FLOATS
        vs, vc, vv = [], [], []
        for g in range(S_):
            idx = order[bounds[g]:bounds[g + 1]]
            idx = idx[val.valid[idx]]
            x = val.v[idx]
            vc.append(len(idx))
            if isf:
                x = x.astype(np.float64)                      # Float32 widens exactly
                vs.append(float_sum(x))
            else:
                vs.append(wrap64(sum(int(t) for t in x.tolist())))      # bool -> 0 / 1, signed sign-extends, unsigned zero-extends
            vv.append(x)
        sums.append(vs)
        counts.append(vc)
        values.append(vv)
    return Model(ngroups, dtypes, sums, counts, rows, values)


def run_chunks(expr, cols, value_roots, group_root, ngroups, filter_root=-1):
    return run(expr, columns_of(cols), value_roots, group_root, ngroups, filter_root)


# ---------------------------------------------------------------- the comparison
def float_bound(model: Model, v: int, g: int) -> Fraction:
    """gamma(n_g - 1) * sum|x_i| + spacing(|fsum|) / 2, exactly; 0 for n_g <= 1."""
    n = model.counts[v][g]
    if n <= 1:
        return Fraction(0)
    ref = model.sums[v][g]
    abs_sum = sum((Fraction(abs(t)) for t in model.values[v][g].tolist()), Fraction(0))      # exact
    return Fraction(X.gamma(n - 1)) * abs_sum + Fraction(float(np.spacing(abs(ref)))) / 2


def float_sum_ok(got: float, model: Model, v: int, g: int) -> bool:
    ref = model.sums[v][g]
    if not math.isfinite(ref):                                 # matched by kind
        return (math.isnan(got) and math.isnan(ref)) or got == ref
    if not math.isfinite(got):
        return False
    return abs(Fraction(got) - Fraction(ref)) <= float_bound(model, v, g)      # by value: the two zeros are peers


def check(got, model: Model, what="", floats_exact=False):
    """got = (res, rows) of Api.group_pipeline(..., with_some=True) (or without is_some: then it is not looked at).
    floats_exact: the case is of the exact family, every float sum must be the reference itself."""
    res, rows = got
    assert list(rows) == list(model.rows), f"{what}: count(*) per group {list(rows)} != {model.rows}"
    assert len(res) == len(model.dtypes), what
    for v, per_group in enumerate(res):
        assert len(per_group) == model.ngroups + 1, what
        for g, cell in enumerate(per_group):
            where = f"{what}: value {v} group {g}"
            assert cell[1] == model.counts[v][g], f"{where}: count {cell[1]} != {model.counts[v][g]}"
            if len(cell) > 2:
                assert cell[2] == model.is_some(v, g), f"{where}: is_some {cell[2]} with count {cell[1]}"
            ref = model.sums[v][g]
            if model.dtypes[v] in S.FLOATS:
                assert isinstance(cell[0], float), where
                if floats_exact:
                    assert cell[0] == ref or (cell[0] != cell[0] and ref != ref), f"{where}: sum {cell[0]!r} != {ref!r} (exact family)"
                else:
                    assert float_sum_ok(cell[0], model, v, g), (
                        f"{where}: sum {cell[0]!r} vs fsum {ref!r} over {model.counts[v][g]} values: "
                        f"|diff| {abs(cell[0] - ref) if math.isfinite(ref) else 'kind'} > bound {float(float_bound(model, v, g)) if math.isfinite(ref) else 0!r}")
            else:
                assert cell[0] == ref, f"{where}: sum {cell[0]} != {ref}"


def check_same(a, b, model: Model, what="", floats_exact=False):
    """Two runs of one case (host arrays, device arrays, a frame): equal in everything but general float sums."""
    (ares, arows), (bres, brows) = a, b
    assert list(arows) == list(brows), what
    for v, (ra, rb) in enumerate(zip(ares, bres)):
        for g, (ca, cb) in enumerate(zip(ra, rb)):
            assert ca[1:] == cb[1:], f"{what}: value {v} group {g}: {ca} vs {cb}"
            if floats_exact or model.dtypes[v] not in S.FLOATS:
                assert ca[0] == cb[0] or (ca[0] != ca[0] and cb[0] != cb[0]), f"{what}: value {v} group {g}: {ca} vs {cb}"


def expect_failure(fn, failure: Failure, what=""):
    try:
        fn()
    except A.RdfError as ex:
        assert ex.status == failure.status, f"{what}: status {ex.status} != {failure.status} ({failure.why})"
        return
    raise AssertionError(f"{what}: the call succeeded, the model says status {failure.status} ({failure.why})")
