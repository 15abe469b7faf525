"""The executable definition of rdf_groupby_agg (include/rdf_mi355x.h, "group-by") in plain numpy, Python integers and
math.fsum, independent of the C oracle.  It knows nothing of planner paths, tables, records or partitions: whatever path
answers a call, the result is the one the header documents.

The header's semantics:
  * 1..4 integer grouping columns; a NULL in a grouping column is a group value of its own.  A group's key is a tuple with
    None for NULL;
  * NULL values are skipped; counts[g] = non-NULL values of the group — rows of the group for COUNT, or without values;
  * out_values is Float64 for float values, UInt64 for MIN / MAX of UInt64 values, Int64 otherwise; integer sums wrap to
    64 bits after sign- or zero-extension (an unsigned sum is reported through the signed field);
  * MIN / MAX of a group without a valid value is NULL; the sum of such a group is 0 (0.0 for floats);
  * Float32 widens exactly; a float sum's reference is math.fsum, a group holding a NaN or infinities of both signs sums to
    NaN, infinities of one sign to that infinity (group_ref.float_sum);
  * float MIN / MAX follow the column aggregates' rule (rdf_min / rdf_max), as BITS: -0.0 is below
    +0.0, and NaN never wins unless every valid value of the group is NaN (then the result is a NaN: which one is open);
  * more than max_groups distinct key tuples, the NULL tuple counted, are RDF_MEMORY_ERROR; exactly max_groups succeed;
  * out_values is not specified for COUNT (ANY below); group order is unspecified.

`check_groupby` is the comparison the CPU and the GPU tests share: keys, counts, integer values, float MIN / MAX (on the
uint64 view) and the outputs' length / null_count exactly; a float sum by group_ref.float_sum_ok,
    |got - fsum| <= gamma(n_g - 1) * sum|x| + spacing(|fsum|) / 2        (exact rational arithmetic; n_g <= 1: the value itself),
the bound of ANY order and tree of correctly rounded f64 additions — nothing about it is measured.
"""
import struct

import numpy as np

from rust_dataframe_amd import _abi as A

import group_ref as GR
from group_ref import Failure  # noqa: F401  (the status a call must fail with)

ANY = object()      # a value the header leaves open
FLOATS = (A.F32, A.F64)
AGGS = ("sum", "min", "max", "count")


def bits_of(x: float) -> int:
    """The uint64 view of one f64."""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def out_dtype(agg, vdt):
    """dtype of out_values (vdt None: no values)."""
    if vdt is None or agg == "count":
        return A.I64
    if vdt in FLOATS:
        return A.F64
    return A.U64 if agg in ("min", "max") and vdt == A.U64 else A.I64


class Groups(dict):
    """The model: {key tuple: (value | None | ANY, count, the group's valid values as an f64 vector | None)}."""
    key_dtypes = ()
    value_dtype = None


class Got(dict):
    """A result: {key tuple: (value | None, count)} + what the outputs said about themselves."""
    key_dtypes = ()
    value_dtype = None          # dtype of out_values
    lengths = ()                # (every key output ..., out_values, out_counts)
    null_counts = ()            # the same order


def key_columns(keys):
    """One chunk list (a single grouping column) or a list of them -> a list of chunk lists."""
    return [keys] if isinstance(keys[0], A.HostArray) else list(keys)


def float_extreme(x: np.ndarray, agg) -> float:
    """MIN / MAX of a non-empty f64 vector as the column aggregates define it: NaN loses against every number, -0.0 < +0.0."""
    nn = x[~np.isnan(x)]
    if len(nn) == 0:
        return float("nan")
    m = float(nn.min() if agg == "min" else nn.max())
    if m == 0.0:
        zeros_neg = np.signbit(nn[nn == 0.0])
        m = (-0.0 if zeros_neg.any() else 0.0) if agg == "min" else (0.0 if (~zeros_neg).any() else -0.0)
    return m


def groupby(keys, values, agg, max_groups=None):
    """keys: one chunk list or 1..4 of them (any integer dtype, NULLs allowed); values: a chunk list or None.
    -> Groups, or Failure(RDF_MEMORY_ERROR) when max_groups is given and there are more distinct key tuples than that."""
    assert agg in AGGS
    cols = key_columns(keys)
    assert 1 <= len(cols) <= 4
    kcols = GR.columns_of(cols)
    n = len(kcols[0][0])
    sort_by, kvalid = [], []
    for v, valid in kcols:
        assert v.dtype.kind in "iu" and len(v) == n
        ok = np.ones(n, dtype=bool) if valid is None else valid
        kvalid.append(ok)
        sort_by += [np.where(ok, v, v.dtype.type(0)), ~ok]
    order = np.lexsort(sort_by)
    diff = np.zeros(n, dtype=bool)
    for s in sort_by:
        ss = s[order]
        diff[1:] |= ss[1:] != ss[:-1]
    if n:
        diff[0] = True
    starts = np.flatnonzero(diff)
    ends = np.concatenate([starts[1:], [n]]).astype(np.int64)
    out = Groups()
    out.key_dtypes = tuple(c[0].dtype for c in cols)
    counting = values is None or agg == "count"
    out.value_dtype = None if counting else values[0].dtype
    if max_groups is not None and len(starts) > max_groups:
        return Failure(A.RDF_MEMORY_ERROR, f"{len(starts)} distinct key tuples, max_groups {max_groups}")
    if not counting:
        (v, vok), = GR.columns_of([values])
        vok = np.ones(n, dtype=bool) if vok is None else vok
        isf = values[0].dtype in FLOATS
    for s, e in zip(starts.tolist(), ends.tolist()):
        first = int(order[s])
        key = tuple(int(kv[first]) if ok[first] else None for (kv, _), ok in zip(kcols, kvalid))
        if counting:
            out[key] = (ANY, e - s, None)
            continue
        rows = order[s:e]                                 # (lexsort is stable: ascending rows)
        x = v[rows][vok[rows]]
        cnt = len(x)
        if isf:
            x = x.astype(np.float64)                      # Float32 widens exactly
            val = GR.float_sum(x) if agg == "sum" else None if cnt == 0 else float_extreme(x, agg)
            out[key] = (val, cnt, x)
        else:
            ints = [int(t) for t in x.tolist()]           # signed sign-extends, unsigned zero-extends
            val = GR.wrap64(sum(ints)) if agg == "sum" else None if cnt == 0 else (min(ints) if agg == "min" else max(ints))
            out[key] = (val, cnt, None)
    return out


def groups_of(keys_out, vals_out, counts_out):
    """The three outputs of Api.groupby_agg (host arrays) -> Got; a key tuple twice is an error."""
    n = counts_out.length
    assert all(k.length == n for k in keys_out) and vals_out.length == n, f"output lengths differ: keys {[k.length for k in keys_out]}, values {vals_out.length}, counts {n}"
    cols = [k.to_pylist() for k in keys_out]
    v, c = vals_out.to_pylist(), counts_out.to_numpy().tolist()
    out = Got()
    for i in range(n):
        kt = tuple(col[i] for col in cols)
        assert kt not in out, f"group {kt} twice"
        out[kt] = (v[i], c[i])
    out.key_dtypes = tuple(k.dtype for k in keys_out)
    out.value_dtype = vals_out.dtype
    out.lengths = tuple(k.length for k in keys_out) + (vals_out.length, counts_out.length)
    out.null_counts = tuple(k.null_count for k in keys_out) + (vals_out.null_count, counts_out.null_count)
    return out


def result_of(groups: dict, key_dtypes, value_dtype, agg):
    """A Got built by hand from {key tuple: (value | None, count)}, its lengths and null counts as a correct call reports them."""
    out = Got(groups)
    out.key_dtypes, out.value_dtype = tuple(key_dtypes), value_dtype
    nk = len(key_dtypes)
    out.lengths = (len(groups),) * (nk + 2)
    vnulls = sum(1 for v, _ in groups.values() if v is None) if agg in ("min", "max") else 0
    out.null_counts = tuple(sum(1 for kt in groups if kt[k] is None) for k in range(nk)) + (vnulls, 0)
    return out


def perfect(model: Groups, agg):
    """The result a correct call could return for `model` (0 where the header leaves the value open)."""
    return result_of({k: (0 if v is ANY else v, c) for k, (v, c, _) in model.items()}, model.key_dtypes, out_dtype(agg, model.value_dtype), agg)


def _same_float(got: float, ref: float) -> bool:
    """Bit for bit; an all-NaN group answers with a NaN (the kernels' tables hold one canonical NaN, the header names none)."""
    if ref != ref:
        return got != got
    return bits_of(got) == bits_of(ref)


def check_groupby(got, model, agg, what="", max_groups=None, floats_exact=False):
    """got = groups_of(...), model = groupby(...).  floats_exact: the case is of the integer-valued family, where every
    float sum is exact in any order and must be the reference itself."""
    assert not isinstance(model, Failure), f"{what}: the call succeeded with {len(got)} groups, the model says status {model.status} ({model.why})"
    if max_groups is not None:
        assert len(got) <= max_groups, f"{what}: {len(got)} groups returned, max_groups {max_groups}"
    assert got.keys() == model.keys(), f"{what}: keys differ: {len(got)} groups vs {len(model)}; only in one: {sorted(set(got) ^ set(model), key=repr)[:8]}"
    nk = len(model.key_dtypes)
    assert tuple(got.key_dtypes) == tuple(model.key_dtypes), f"{what}: key dtypes {got.key_dtypes} != {model.key_dtypes}"
    assert got.value_dtype == out_dtype(agg, model.value_dtype), f"{what}: out_values dtype {got.value_dtype} != {out_dtype(agg, model.value_dtype)}"
    assert all(ln == len(model) for ln in got.lengths) and len(got.lengths) == nk + 2, f"{what}: output lengths {got.lengths}, {len(model)} groups"
    for k in range(nk):
        nulls = sum(1 for kt in model if kt[k] is None)
        assert got.null_counts[k] == nulls, f"{what}: null_count of key output {k}: {got.null_counts[k]} != {nulls}"
    counting = model.value_dtype is None
    if not counting:
        vnulls = sum(1 for v, _, _ in model.values() if v is None) if agg in ("min", "max") else 0
        assert got.null_counts[nk] == vnulls, f"{what}: null_count of out_values {got.null_counts[nk]} != {vnulls}"
    assert got.null_counts[nk + 1] == 0, f"{what}: null_count of out_counts {got.null_counts[nk + 1]}"
    for key, (mv, mc, x) in model.items():
        gv, gc = got[key]
        w = f"{what}: group {key}"
        assert gc == mc, f"{w}: count {gc} != {mc}"
        if mv is ANY:
            continue
        if mv is None:
            assert gv is None, f"{w}: {agg} of a group without a valid value is NULL, got {gv!r}"
        elif x is None:
            assert gv == mv and not isinstance(gv, float), f"{w}: {agg} {gv!r} != {mv!r}"
        elif agg == "sum" and not floats_exact:
            one = GR.Model(1, [A.F64], [[mv]], [[mc]], [mc], [[x]])
            assert isinstance(gv, float) and GR.float_sum_ok(gv, one, 0, 0), f"{w}: sum {gv!r} vs fsum {mv!r} over {mc} values, bound {float(GR.float_bound(one, 0, 0))!r}"
        elif agg == "sum":
            assert isinstance(gv, float) and (gv == mv or (gv != gv and mv != mv)), f"{w}: sum {gv!r} != {mv!r} (integer-valued: exact in any order)"
        else:
            assert isinstance(gv, float) and _same_float(gv, mv), f"{w}: {agg} {gv!r} ({bits_of(gv):#018x}) != {mv!r} ({bits_of(mv):#018x})"


def expect_failure(fn, failure: Failure, what=""):
    GR.expect_failure(fn, failure, what)


# ---------------------------------------------------------------- inputs both test files build their cases from
def rank_in_group(gid: np.ndarray) -> np.ndarray:
    """Row i's position among the rows of its group (0, 1, ...), gid = any integer label per row."""
    order = np.argsort(gid, kind="stable")
    s = gid[order]
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]])) if len(s) else np.zeros(0, dtype=np.int64)
    lens = np.diff(np.concatenate([start, [len(s)]]))
    out = np.empty(len(s), dtype=np.int64)
    out[order] = np.arange(len(s)) - np.repeat(start, lens)
    return out


def exact_values(rng, gid, np_dtype):
    """The integer-valued family: magnitudes 1, 3, 5, ... distinct per row within a group, random signs, |v| <= 2^20.  Every
    partial sum is an integer below 2^53: a sum is exact in any order, so a value credited to the wrong group, dropped or
    added twice always shows."""
    mag = rank_in_group(np.asarray(gid)) * 2 + 1
    assert mag.max(initial=0) <= 2 ** 20, "a group of more than 2^19 rows"
    return (mag * rng.choice(np.array([-1, 1]), len(mag))).astype(np_dtype)


def general_values(rng, n):
    """uniform(-1, 1) * 2^randint(-10, 11): held to the any-order bound."""
    return rng.uniform(-1.0, 1.0, n) * np.exp2(rng.integers(-10, 12, n))


def special_values(rng, n, np_dtype=np.float64, every=5):
    """General values with +-0.0, NaN, +-inf and denormals of the dtype scattered through them."""
    tiny = np.finfo(np_dtype).smallest_subnormal
    specials = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, tiny, -tiny, 3 * tiny], dtype=np_dtype)
    v = general_values(rng, n).astype(np_dtype)
    at = rng.uniform(size=n) < 1.0 / every
    v[at] = rng.choice(specials, int(at.sum()))
    return v


def plant_groups(v, valid, gid, g_nan, g_zeros, g_null):
    """Three groups a MIN / MAX can get wrong: one holding only NaN, one only zeros of both signs, one only NULLs."""
    valid = np.ones(len(v), dtype=bool) if valid is None else valid.copy()
    v = v.copy()
    rows = np.flatnonzero(gid == g_nan)
    v[rows], valid[rows] = np.nan, True
    rows = np.flatnonzero(gid == g_zeros)
    v[rows], valid[rows] = np.where(np.arange(len(rows)) % 2 == 0, 0.0, -0.0), True
    valid[gid == g_null] = False
    return v, valid


def ragged(data, valid, rng, cuts=None):
    """One column in ragged chunks: an empty chunk in the middle, element offsets 3, 5, 7, ... (so validity starts at odd bit
    offsets)."""
    n = len(data)
    lens = [n] if n < 4 else [n // 3, 0, n - n // 3] if cuts is None else cuts
    out, at = [], 0
    for i, ln in enumerate(lens):
        out.append(A.HostArray.from_numpy(data[at:at + ln], valid=None if valid is None else valid[at:at + ln], offset=3 + 2 * i, rng=rng))
        at += ln
    assert at == n
    return out
