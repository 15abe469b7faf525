"""The model of rdf_groupby_agg (groupby_ref.py) against the C oracle and against pandas, and the proof that its comparison
bites: a result that is wrong in exactly one of the ways a kernel goes wrong is refused."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A

import group_ref as GR
import groupby_ref as G
import hash_models as H

KEY_DTYPES = [A.I8, A.I16, A.I32, A.I64, A.U8, A.U16, A.U32, A.U64]
VALUE_DTYPES = [A.I8, A.I16, A.I32, A.I64, A.U8, A.U16, A.U32, A.U64, A.F32, A.F64]
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def _key_column(rng, dt, n, ngroups, nulls):
    info = np.iinfo(A.NP_OF[dt])
    pool = np.unique(np.concatenate([np.array([info.min, info.max], dtype=A.NP_OF[dt]), rng.integers(info.min, info.max, ngroups, dtype=A.NP_OF[dt], endpoint=True)]))
    k = rng.choice(pool, n)
    return k, (rng.uniform(size=n) >= nulls) if nulls else None


def _value_column(rng, dt, n, kind):
    npdt = A.NP_OF[dt]
    if dt in G.FLOATS:
        return G.special_values(rng, n, npdt) if kind == "special" else G.general_values(rng, n).astype(npdt)
    info = np.iinfo(npdt)
    return rng.integers(info.min, info.max, n, dtype=npdt, endpoint=True)       # the whole range: 64-bit sums wrap


@pytest.mark.parametrize("nkeys", [1, 2, 3])
@pytest.mark.parametrize("agg", G.AGGS)
def test_model_matches_oracle(ora, agg, nkeys):
    """Every key dtype and every value dtype, NULL keys and NULL values, the special floats (NaN and infinities in sums, signed
    zeros and denormals in MIN / MAX), integer values over their whole range."""
    rng = np.random.default_rng(100 * nkeys + G.AGGS.index(agg))
    n = 211
    for i, kdt in enumerate(KEY_DTYPES):
        kdts = [kdt, KEY_DTYPES[(i + 3) % 8], KEY_DTYPES[(i + 5) % 8]][:nkeys]
        for vdt in VALUE_DTYPES + [None]:
            cols = []
            for k, dt in enumerate(kdts):
                kv, valid = _key_column(rng, dt, n, (9, 3, 2)[k], (0.06, 0.1, 0.0)[k])
                cols.append(G.ragged(kv, valid, rng))
            vals = None
            if vdt is not None:
                v = _value_column(rng, vdt, n, "special")
                vals = G.ragged(v, rng.uniform(size=n) >= 0.2, rng)
            model = G.groupby(cols, vals, agg)
            got = G.groups_of(*ora.groupby_agg(cols, vals, agg, len(model)))
            G.check_groupby(got, model, agg, f"{agg} keys {kdts} values {vdt}", max_groups=len(model))


@pytest.mark.parametrize("agg", G.AGGS)
def test_model_matches_pandas(agg):
    """An independent statement of the same grouping on finite data without zeros (Python's min does not order the two zeros)."""
    from test_groupby_agg import _pandas_groups
    rng = np.random.default_rng(31)
    n = 400
    for vdt in (A.F64, A.F32, A.I64, A.U64, A.I16):
        for nkeys in (1, 2):
            cols = [G.ragged(rng.integers(lo, lo + ng, n).astype(A.NP_OF[dt]), rng.uniform(size=n) >= 0.05, rng)      # (the pandas statement passes keys through f64)
                    for dt, ng, lo in ((A.I64, 20, -2 ** 40), (A.U8, 3, 250))[:nkeys]]
            v = _value_column(rng, vdt, n, "plain")
            vals = G.ragged(v, rng.uniform(size=n) >= 0.2, rng)
            model = G.groupby(cols, vals, agg)
            exp = _pandas_groups(cols, vals, agg)
            if agg == "sum" and vdt not in G.FLOATS:
                exp = {k: (GR.wrap64(s), c) for k, (s, c) in exp.items()}
            if agg == "count":
                exp = {k: (0, c) for k, (_, c) in exp.items()}
            if vdt in G.FLOATS and agg != "count":
                exp = {k: (None if s is None else float(s), c) for k, (s, c) in exp.items()}
            got = G.result_of(exp, model.key_dtypes, G.out_dtype(agg, model.value_dtype), agg)
            G.check_groupby(got, model, agg, f"pandas {agg} values {vdt} nkeys {nkeys}")


def test_single_column_form_and_empty_input():
    """stream_ref's callers pass one chunk list: the same groups, keys as 1-tuples.  No rows: no groups."""
    rng = np.random.default_rng(2)
    k = rng.integers(0, 5, 50).astype(np.int64)
    v = rng.integers(-9, 9, 50).astype(np.int64)
    keys, vals = G.ragged(k, None, rng), G.ragged(v, None, rng)
    assert G.groupby(keys, vals, "sum") == G.groupby([keys], vals, "sum")
    assert set(G.groupby(keys, vals, "sum")) == {(int(x),) for x in np.unique(k)}
    assert len(G.groupby([[A.HostArray.from_numpy(np.zeros(0, dtype=np.int32))]], None, "count")) == 0


# ---------------------------------------------------------------- the comparison bites
def _refused(got, model, agg, **kw):
    with pytest.raises(AssertionError):
        G.check_groupby(got, model, agg, "bite", **kw)


def _case(agg, values, gid, valid=None):
    rng = np.random.default_rng(1)
    keys = [G.ragged(np.asarray(gid, dtype=np.int64), None, rng)]
    vals = G.ragged(np.asarray(values), valid, rng)
    model = G.groupby(keys, vals, agg)
    good = G.perfect(model, agg)
    G.check_groupby(good, model, agg, "the unbroken result passes")
    return model, good


def test_a_sign_of_zero_flip_in_a_min_is_refused():
    model, got = _case("min", [0.0, -0.0, 3.0, 0.0, 1.0, 0.0], [7, 7, 7, 8, 8, 8])
    assert G.bits_of(model[(7,)][0]) == 1 << 63 and G.bits_of(model[(8,)][0]) == 0
    got[(7,)] = (0.0, 3)
    _refused(got, model, "min")
    model, got = _case("max", [0.0, -0.0, -3.0, -0.0, -1.0, -0.0], [7, 7, 7, 8, 8, 8])
    assert G.bits_of(model[(7,)][0]) == 0 and G.bits_of(model[(8,)][0]) == 1 << 63
    got[(8,)] = (0.0, 3)
    _refused(got, model, "max")


def test_a_nan_reported_as_min_of_a_group_with_finite_values_is_refused():
    nan = float("nan")
    model, got = _case("min", [nan, 2.0, nan, nan, nan, 5.0], [1, 1, 1, 2, 2, 3])
    assert model[(1,)][0] == 2.0 and math.isnan(model[(2,)][0])
    got[(1,)] = (nan, 3)
    _refused(got, model, "min")
    model, got = _case("min", [nan, 2.0, nan, nan, nan, 5.0], [1, 1, 1, 2, 2, 3])
    got[(2,)] = (2.0, 2)                                  # and the other way round: an all-NaN group answers NaN
    _refused(got, model, "min")


@pytest.mark.parametrize("npdt", [np.float64, np.int64])
def test_one_value_credited_to_another_group_is_refused(npdt):
    """Counts unchanged, the integer-valued family: a value of magnitude 1 moved between two groups whose sums are of the
    order of 10^5 moves both sums by exactly 1, which an exact comparison sees and 1e-6 relative does not."""
    rng = np.random.default_rng(3)
    gid = np.repeat([4, 5], 400)
    v = np.abs(G.exact_values(rng, gid, npdt))
    model, got = _case("sum", v, gid)
    s4, s5 = got[(4,)][0], got[(5,)][0]
    assert s4 == 400 * 400 and abs(1 / s4) < 1e-5
    got[(4,)], got[(5,)] = (s4 - 1, 400), (s5 + 1, 400)
    _refused(got, model, "sum", floats_exact=npdt is np.float64)
    if npdt is np.float64:                                # the general family's bound refuses it too at these sizes
        _refused(got, model, "sum")


def test_a_sum_one_ulp_outside_the_bound_is_refused():
    rng = np.random.default_rng(4)
    v = G.general_values(rng, 300)
    model, got = _case("sum", v, np.zeros(300, dtype=np.int64))
    ref, cnt, x = model[(0,)]
    one = GR.Model(1, [A.F64], [[ref]], [[cnt]], [cnt], [[x]])
    bound = GR.float_bound(one, 0, 0)
    assert bound > 0
    edge = float(Fraction(ref) + bound)                   # rounded to nearest: step to the last double inside
    while Fraction(edge) - Fraction(ref) > bound:
        edge = math.nextafter(edge, -math.inf)
    while Fraction(math.nextafter(edge, math.inf)) - Fraction(ref) <= bound:
        edge = math.nextafter(edge, math.inf)
    got[(0,)] = (edge, cnt)
    G.check_groupby(got, model, "sum", "the last double inside the bound")
    got[(0,)] = (math.nextafter(edge, math.inf), cnt)
    _refused(got, model, "sum")
    low = float(Fraction(ref) - bound)
    while Fraction(ref) - Fraction(low) > bound:
        low = math.nextafter(low, math.inf)
    while Fraction(ref) - Fraction(math.nextafter(low, -math.inf)) <= bound:
        low = math.nextafter(low, -math.inf)
    got[(0,)] = (math.nextafter(low, -math.inf), cnt)
    _refused(got, model, "sum")
    # one value: the value itself
    model, got = _case("sum", [0.1], [0])
    got[(0,)] = (math.nextafter(0.1, 1.0), 1)
    _refused(got, model, "sum")


def test_more_groups_than_max_groups_are_refused():
    rng = np.random.default_rng(5)
    k = np.arange(10, dtype=np.int64)
    keys = [G.ragged(k, np.arange(10) != 3, rng)]         # nine keys and the NULL key: ten tuples
    model = G.groupby(keys, None, "count")
    assert len(model) == 10 and (None,) in model
    assert G.groupby(keys, None, "count", max_groups=10) == model
    fail = G.groupby(keys, None, "count", max_groups=9)
    assert isinstance(fail, G.Failure) and fail.status == A.RDF_MEMORY_ERROR
    got = G.perfect(model, "count")
    _refused(got, fail, "count")                          # max_groups + 1 groups came back where the call had to fail
    _refused(got, model, "count", max_groups=9)
    G.check_groupby(got, model, "count", "exactly max_groups", max_groups=10)


def test_wrong_lengths_null_counts_and_dtypes_are_refused():
    model, got = _case("min", [1.0, 2.0, 3.0], [1, 1, 2], valid=np.array([True, True, False]))
    assert model[(2,)][0] is None and got.null_counts == (0, 1, 0)
    for field, bad in (("lengths", (2, 3, 2)), ("null_counts", (0, 0, 0)), ("null_counts", (1, 1, 0)), ("null_counts", (0, 1, 1)), ("value_dtype", A.I64), ("key_dtypes", (A.I32,))):
        g = G.result_of(dict(got), got.key_dtypes, got.value_dtype, "min")
        setattr(g, field, bad)
        _refused(g, model, "min")


def test_the_cancellation_input_and_the_any_order_bound():
    """[1e16, 1.0 x 200, -1e16].  A plain f64 running sum loses every 1.0 and returns 0.0 against fsum = 200.0.  That IS an order
    of correctly rounded f64 additions, so the any-order bound must — and does — admit it: gamma(201) * sum|x| is about 446.
    (The window frames' bound, which this input defeats with a plain prefix, is a double-double bound; the hash GROUP BY adds
    with f64 atomics in no fixed order and cannot promise more than the any-order bound.)  What the bound does refuse on the
    same input: a sum that drops one of the two large values, and one that loses the ones twice over."""
    x = np.array([1e16] + [1.0] * 200 + [-1e16])
    model, got = _case("sum", x, np.zeros(len(x), dtype=np.int64))
    ref, cnt, xs = model[(0,)]
    assert ref == 200.0
    run = 0.0
    for t in x.tolist():
        run += t
    assert run == 0.0
    one = GR.Model(1, [A.F64], [[ref]], [[cnt]], [cnt], [[xs]])
    assert abs(Fraction(run) - Fraction(ref)) <= GR.float_bound(one, 0, 0) and 440 < float(GR.float_bound(one, 0, 0)) < 450
    got[(0,)] = (run, cnt)
    G.check_groupby(got, model, "sum", "a plain f64 running sum is one of the orders the bound covers")
    got[(0,)] = (math.fsum(x[:-1].tolist()), cnt)         # the -1e16 dropped
    _refused(got, model, "sum")
    got[(0,)] = (-300.0, cnt)                             # 500 away: beyond anything rounding can do to these 202 values
    _refused(got, model, "sum")


# ---------------------------------------------------------------- the hash model the GPU test builds its keys with
def test_g2_hash_model_constants():
    assert (H.G2_MUL * H.G2_MUL_INV) & H.M == 1
    assert H.g2_hash(H.G2_FREE_KEY) == H.M and H.g2_hash_inv(H.M) == H.G2_FREE_KEY
    rng = np.random.default_rng(6)
    for k in rng.integers(0, H.M, 200, dtype=np.uint64, endpoint=True).tolist() + [0, 1, H.M, 1 << 63]:
        assert H.g2_hash_inv(H.g2_hash(k)) == k and H.g2_hash(H.g2_hash_inv(k)) == k
    keys = H.g2_keys_in_partition(0xA7, 300, seed=1)
    assert len(set(keys)) == 300 and all(H.g2_partition(k) == 0xA7 for k in keys) and H.G2_FREE_KEY not in keys
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust_dataframe_amd", "csrc")
    kernel = open(os.path.join(csrc, "rdf_groupby.hip")).read()
    assert "g2_hash(uint64_t x) { x ^= x >> 32; x *= 0x9E3779B97F4A7C15ull; return x ^ (x >> 32); }" in kernel
    assert "z ^= z >> 32; z *= 0xF1DE83E19937733Dull; z ^= z >> 32;" in open(os.path.join(csrc, "rdf_capi_groupby.inc")).read()
    assert "constexpr int kG2PartBits = 8;" in open(os.path.join(csrc, "rdf_device.h")).read()


@pytest.mark.parametrize("with_null", [True, False])
def test_oracle_keeps_the_max_groups_promise(ora, with_null):
    """d distinct keys, the NULL key among them or not: max_groups = d succeeds, d - 1 is RDF_MEMORY_ERROR — rdf_groupby_agg and
    rdf_groupby_sum alike (the merge of partial groups keeps its slack of two)."""
    rng = np.random.default_rng(12)
    k = rng.permutation(np.repeat(np.arange(-5, 6, dtype=np.int64) * 1_000_003, 4))
    keys = G.ragged(k, (k != 0) if with_null else None, rng)
    vals = G.ragged(G.exact_values(rng, k, np.float64), None, rng)
    for agg in G.AGGS:
        model = G.groupby([keys], vals, agg)
        assert len(model) == 11 and ((None,) in model) == with_null
        G.check_groupby(G.groups_of(*ora.groupby_agg([keys], vals, agg, 11)), model, agg, f"oracle {agg}", max_groups=11, floats_exact=True)
        G.expect_failure(lambda: ora.groupby_agg([keys], vals, agg, 10), G.groupby([keys], vals, agg, 10), f"oracle {agg}")
    ok, ov, oc = ora.groupby_sum(keys, vals, 11)
    G.check_groupby(G.groups_of([ok], ov, oc), G.groupby([keys], vals, "sum"), "sum", "oracle groupby_sum", max_groups=11, floats_exact=True)
    G.expect_failure(lambda: ora.groupby_sum(keys, vals, 10), G.Failure(A.RDF_MEMORY_ERROR), "oracle groupby_sum")
