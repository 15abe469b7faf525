"""The model of the streamed batch loop (stream_ref.py) against the C oracle, on the layouts the GPU test uses (stream_cases.py):
two independent statements of every sink that must agree before the library is held to one of them.  CPU only."""
import numpy as np
import pytest

from rust_dataframe_amd import _abi as A

import group_ref as GR
import stream_cases as SC
import stream_ref as SR


@pytest.mark.parametrize("vdt", SC.NUMERIC)
def test_aggregate_model_matches_oracle(ora, vdt):
    rng = np.random.default_rng(100 + vdt)
    e, cols, values, filt = SC.agg_case(rng, vdt)
    model = SR.aggregate(e, cols, values, filt)
    assert 0 < model[0].count < sum(SC.LENS) // 2 and model[1].count > model[0].count      # the predicate and the NULLs both select
    SR.check_aggregate(ora.pipeline(e, cols, values, filt), model, f"oracle, dtype {vdt}")


def test_aggregate_model_float_data(ora):
    rng = np.random.default_rng(7)
    n = sum(SC.LENS)
    for what, v in (("markers", SC.marked_f64(rng, n)), ("uniform", rng.uniform(-1.0, 1.0, n)), ("cancelling", SC.cancelling_f64(rng, n))):
        e, cols, values, filt = SC.agg_case(rng, A.F64, v)
        model = SR.aggregate(e, cols, values, filt)
        SR.check_aggregate(ora.pipeline(e, cols, values, filt), model, what)
        if what == "markers":       # every order gives the same bits: the bound has nothing to forgive
            assert ora.pipeline(e, cols, values, filt)[0].sum == model[0].sum and model[0].sum > 2.0 ** 40
        if what == "cancelling":
            assert abs(model[0].sum) < 0.05 * float(np.abs(model[0].values).sum())      # (NULLs and the predicate break some pairs)
    # the f32 bound: half an ulp of the result for one value, and about 2^-24 sum|x| for many
    e, cols, values, filt = SC.agg_case(rng, A.F32, kind="unit")
    m = SR.aggregate(e, cols, values, filt)[0]
    assert not SR.f32_sum_is_exact(m)
    a = float(np.abs(m.values.astype(np.float64)).sum())
    assert 2.0 ** -24 * a < float(SR.f32_sum_bound(m)) < 2.0 ** -24 * a * 1.01 + float(np.spacing(np.float32(abs(m.sum))))


@pytest.mark.parametrize("dt", SC.NUMERIC)
def test_store_model_add_matches_oracle(ora, dt):
    rng = np.random.default_rng(200 + dt)
    a, b = SC.column(rng, dt, nulls=0.1, kind="extreme" if dt not in (A.F32, A.F64) else "plain"), SC.column(rng, dt, nulls=0.0, kind="plain")
    e = A.Expr()
    SR.check_store(ora.binary("add", a, b), SR.store(e, [a, b], e.op("add", e.col(0), e.col(1))), SC.LENS, f"add, dtype {dt}")


@pytest.mark.parametrize("src,dst", SC.CASTS)
def test_store_model_casts_match_oracle(ora, src, dst):
    rng = np.random.default_rng(300 + 16 * src + dst)
    a = SC.cast_case(rng, src, dst)
    model = SR.cast(a, dst)
    if (src, dst) in ((A.I64, A.U8), (A.F64, A.I32)):
        assert (model.valid != SR.columns([a])[0][2]).any(), "the cast makes NULLs of its own"
    SR.check_store(ora.cast(a, dst), model, SC.LENS, f"cast {src} -> {dst}")


def test_store_model_unary_and_mask_match_oracle(ora):
    rng = np.random.default_rng(5)
    x = SC.column(rng, A.F64, nulls=0.1)
    pos = SC.column(rng, A.F64, np.abs(rng.uniform(0.0, 100.0, sum(SC.LENS))), nulls=0.1)
    for op, col in (("abs", x), ("floor", x), ("sqrt", pos), ("sqrt", x)):       # (sqrt of a negative number: a NaN of the same bits)
        SR.check_store(ora.unary(op, col), SR.unary(op, col), SC.LENS, op)
    k = SC.column(rng, A.I32, nulls=0.1)
    e = A.Expr()
    pred = e.op("and", e.op("gt", e.col(0), e.scalar(-25.0)), e.op("le", e.col(1), e.scalar(300, A.I32)))
    SR.check_store(ora.predicate(e, pred, [x, k]), SR.mask(e, [x, k], pred), SC.LENS, "mask")


@pytest.mark.parametrize("selectivity", [0, 1, 0.5, 1 / 64])
def test_filter_model_matches_oracle(ora, selectivity):
    rng = np.random.default_rng(400)
    cols, preds = SC.filter_case(rng, selectivity)
    n = sum(SC.LENS)
    for what, (e, root) in preds.items():
        model = SR.filter_rows(e, cols, root)
        kept = sum(len(v) for v, _ in model[0])
        assert kept == (0 if selectivity == 0 else n if selectivity == 1 else kept) and (selectivity in (0, 1) or 0.8 * selectivity * n * 0.9 < kept < 1.2 * selectivity * n)
        got = ora.filter_columns(cols, ora.predicate(e, root, cols))
        SR.check_filter(got, model, cols, f"{what}, selectivity {selectivity}")


@pytest.mark.parametrize("agg", ["sum", "min", "max", "count"])
@pytest.mark.parametrize("kdt,vdt", [(A.I64, A.F64), (A.U64, A.F32), (A.I64, A.I64), (A.U64, A.I32), (A.I64, A.U64), (A.U64, None)])
def test_groupby_model_matches_oracle(ora, agg, kdt, vdt):
    rng = np.random.default_rng(500 + kdt + (vdt or 0))
    keys, vals, distinct = SC.groupby_case(rng, kdt, vdt)
    model = SR.groupby(keys, vals, agg)
    assert len(model) == distinct
    if vals is not None and agg in ("min", "max"):
        assert sum(1 for v, c, _ in model.values() if v is None and c == 0) == 1      # the group that is NULL everywhere
    got = SR.groups_of(*ora.groupby_agg([keys], vals, agg, distinct))
    SR.check_groupby(got, model, agg, f"{agg} keys {kdt} values {vdt}")


def test_grouped_model_is_group_ref(ora):
    from test_group_pipeline import q1_columns, q1_program, _cols_list
    rng = np.random.default_rng(33)
    cols = _cols_list(q1_columns(rng, [1023, 0, 1025, 700], 0.1, 3))
    e, pred, gid, vals = q1_program()
    model = SR.grouped(e, cols, vals, gid, 6, pred)
    GR.check(ora.group_pipeline(e, cols, vals, gid, 6, pred, with_some=True), model, "Q1")
