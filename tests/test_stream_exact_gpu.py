"""The streamed batch loop (rdf_capi_stream.inc) held to an independent model (stream_ref.py) at every cut and copy route.

Every case sets stream_slab_bytes itself, asserts that the call was cut into at least two slabs, and restores the option.  The
common layout (stream_cases.py) is 23 266 rows in 13 batches at 13 different offsets — pieces at every bit phase — under slabs
of 16 KiB, 64 KiB and 200 KiB (or a third of the call's input where that is smaller).  Results are compared with the model;
where the model is exact also bit for bit with the one-shot path (stream_slab_bytes = -1).  Float sums are held to the model's
bound only: the slab fold adds in another order than the one-shot path.

The page-locked routes run at 1.25 MiB slabs, where the pieces of a single Float64 column are 35 840 rows = 280 KiB, above the
256 KiB threshold of a copy of its own.  Validity bitmaps would need 2M-row pieces to pass that threshold: direct validity items
are NOT tested here (the CPU test of the planner, tests/cpp/test_stream_plan.cpp, reaches them).  rdf_stream_stats counts the
bytes of the uploads only: where outputs are written into registered memory the counters speak for the inputs, and the output
route shows in the result alone."""
import ctypes as C
import threading
from contextlib import contextmanager

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A

import group_ref as GR
import stream_cases as SC
import stream_ref as SR

pytestmark = pytest.mark.gpu


@contextmanager
def slab_option():
    """-> set(bytes); the thread's option is back at its default afterwards, whatever happened."""
    from rust_dataframe_amd import lib
    try:
        yield lambda s: lib.set_option("stream_slab_bytes", int(s))
    finally:
        lib.set_option("stream_slab_bytes", 0)


def slabs_cut():
    from rust_dataframe_amd import lib
    return lib.stream_stats()[0]


# ---------------------------------------------------------------- aggregate sink
def _agg_exact_fields(r):
    return (r.dtype, r.count, r.is_some, r.min, r.max) + (() if r.dtype in (A.F32, A.F64) else (r.sum,))


@pytest.mark.parametrize("vdt", SC.NUMERIC)
def test_streamed_aggregates_every_dtype(gpu, vdt):
    rng = np.random.default_rng(100 + vdt)
    e, cols, values, filt = SC.agg_case(rng, vdt)
    model = SR.aggregate(e, cols, values, filt)
    with slab_option() as set_slab:
        set_slab(-1)
        one = gpu.pipeline(e, cols, values, filt)
        assert slabs_cut() == 0
        SR.check_aggregate(one, model, f"one shot, dtype {vdt}")
        for slab in SC.slabs_for(cols):
            set_slab(slab)
            got = gpu.pipeline(e, cols, values, filt)
            assert slabs_cut() >= 2, (slab, slabs_cut())
            SR.check_aggregate(got, model, f"dtype {vdt}, slab {slab}")
            assert [_agg_exact_fields(g) for g in got] == [_agg_exact_fields(o) for o in one], f"dtype {vdt}, slab {slab}: streamed vs one shot"


@pytest.mark.parametrize("data", ["markers", "uniform", "cancelling", "f32 uniform"])
def test_streamed_float_sums(gpu, data):
    """Integer-valued f64 data with 2^40 markers: every order of additions gives the same bits, and a piece lost or counted twice
    moves the sum by at least 1.  Uniform and cancelling data: the any-order bound around math.fsum.  f32: see stream_ref."""
    rng = np.random.default_rng(7)
    n = sum(SC.LENS)
    if data == "f32 uniform":
        e, cols, values, filt = SC.agg_case(rng, A.F32, kind="unit")
    else:
        v = {"markers": SC.marked_f64(rng, n), "uniform": rng.uniform(-1.0, 1.0, n), "cancelling": SC.cancelling_f64(rng, n)}[data]
        e, cols, values, filt = SC.agg_case(rng, A.F64, v)
    model = SR.aggregate(e, cols, values, filt)
    with slab_option() as set_slab:
        for slab in SC.slabs_for(cols):
            set_slab(slab)
            got = gpu.pipeline(e, cols, values, filt)
            assert slabs_cut() >= 2, (slab, slabs_cut())
            print(f"{data} slab {slab}: sum {got[0].sum!r} fsum {model[0].sum!r} diff {got[0].sum - model[0].sum!r} bound {float(SR.f64_sum_bound(model[0]) if data != 'f32 uniform' else SR.f32_sum_bound(model[0]))!r}")
            SR.check_aggregate(got, model, f"{data}, slab {slab}")
            if data == "markers":
                assert got[0].sum == model[0].sum, (slab, got[0].sum, model[0].sum)


# ---------------------------------------------------------------- store sinks
def _store_case(gpu, run, model, cols, what, exact_model=True):
    """run() under every slab: at least two slabs, the model's batches, and the one-shot path's bits."""
    with slab_option() as set_slab:
        set_slab(-1)
        one = run()
        assert slabs_cut() == 0
        if exact_model:
            SR.check_store(one, model, SC.LENS, f"{what}, one shot")
        for slab in SC.slabs_for(cols):
            set_slab(slab)
            got = run()
            assert slabs_cut() >= 2, (what, slab, slabs_cut())
            if exact_model:
                SR.check_store(got, model, SC.LENS, f"{what}, slab {slab}")
            SR.check_same_chunks(got, one, f"{what}, slab {slab}: streamed vs one shot")


@pytest.mark.parametrize("dt", SC.NUMERIC)
def test_streamed_add_every_dtype(gpu, dt):
    rng = np.random.default_rng(200 + dt)
    a, b = SC.column(rng, dt, nulls=0.1, kind="extreme" if dt not in (A.F32, A.F64) else "plain"), SC.column(rng, dt, nulls=0.0, kind="plain")
    c = SC.column(rng, dt, nulls=0.0, kind="plain")
    e = A.Expr()
    root = e.op("add", e.col(0), e.col(1))
    _store_case(gpu, lambda: gpu.binary("add", a, b), SR.store(e, [a, b], root), [a, b], f"add, dtype {dt}")
    got = []
    _store_case(gpu, lambda: got.append(gpu.binary("add", c, b)) or got[-1], SR.store(e, [c, b], root), [c, b], f"add without NULLs, dtype {dt}")
    assert all(o.validity is None for outs in got for o in outs)          # outputs without a validity buffer


@pytest.mark.parametrize("src,dst", SC.CASTS)
def test_streamed_casts(gpu, src, dst):
    rng = np.random.default_rng(300 + 16 * src + dst)
    a = SC.cast_case(rng, src, dst)
    _store_case(gpu, lambda: gpu.cast(a, dst), SR.cast(a, dst), [a], f"cast {src} -> {dst}")


def test_streamed_mask_and_exact_unary(gpu):
    rng = np.random.default_rng(5)
    x = SC.column(rng, A.F64, nulls=0.1)
    pos = SC.column(rng, A.F64, np.abs(rng.uniform(0.0, 100.0, sum(SC.LENS))), nulls=0.1)
    for op, col in (("abs", x), ("floor", x), ("sqrt", pos)):
        _store_case(gpu, lambda: gpu.unary(op, col), SR.unary(op, col), [col], op)
    _store_case(gpu, lambda: gpu.unary("sin", x), None, [x], "sin", exact_model=False)       # bit-equal to the one-shot path
    k = SC.column(rng, A.I32, nulls=0.1)
    e = A.Expr()
    pred = e.op("and", e.op("gt", e.col(0), e.scalar(-25.0)), e.op("le", e.col(1), e.scalar(300, A.I32)))
    _store_case(gpu, lambda: gpu.predicate(e, pred, [x, k]), SR.mask(e, [x, k], pred), [x, k], "predicate mask over nullable inputs")


# ---------------------------------------------------------------- filter sink
@pytest.mark.parametrize("selectivity", [0, 1, 0.5, 1 / 64])
def test_streamed_filter(gpu, selectivity):
    """Columns of 1, 2, 4 and 8 bytes in one call, nullable and not (the non-nullable UInt16 column is given an output validity
    buffer, the Int64 one none), under both predicate forms.  At selectivity 1/2 and 1/64 the pieces of the long batches keep row
    counts that are no multiples of 8: the pieces behind them are appended at every bit phase."""
    rng = np.random.default_rng(400)
    cols, preds = SC.filter_case(rng, selectivity)

    def outs():
        return [[A.HostArray.empty_out(col[i].dtype, col[i].length, col[i].validity is not None or c == 1) for i in range(len(SC.LENS))] for c, col in enumerate(cols)]
    with slab_option() as set_slab:
        for what, (e, root) in preds.items():
            model = SR.filter_rows(e, cols, root)
            if selectivity not in (0, 1):
                assert any(len(v) % 8 for v, _ in model[3])
            set_slab(-1)
            one = gpu.filter_pipeline(e, root, cols, outs())
            assert slabs_cut() <= 1
            SR.check_filter(one, model, cols, f"{what}, one slab")
            for slab in SC.slabs_for(cols):
                set_slab(slab)
                got = gpu.filter_pipeline(e, root, cols, outs())
                assert slabs_cut() >= 2, (what, slab, slabs_cut())
                SR.check_filter(got, model, cols, f"{what}, selectivity {selectivity}, slab {slab}")


# ---------------------------------------------------------------- hash GROUP BY
@pytest.mark.parametrize("agg", ["sum", "min", "max", "count"])
@pytest.mark.parametrize("kdt,vdt", [(A.I64, A.F64), (A.U64, A.F32), (A.I64, A.I64), (A.U64, A.I32), (A.I64, A.U64), (A.U64, None)])
def test_streamed_groupby(gpu, agg, kdt, vdt):
    """A group whose values are NULL in every slab but the last, one that is NULL everywhere, one that appears in the last batch
    alone; max_groups equal to the distinct count, and one below it."""
    rng = np.random.default_rng(500 + kdt + (vdt or 0))
    keys, vals, distinct = SC.groupby_case(rng, kdt, vdt)
    model = SR.groupby(keys, vals, agg)
    cols = [keys] + ([vals] if vals is not None else [])
    with slab_option() as set_slab:
        set_slab(-1)
        one = SR.groups_of(*gpu.groupby_agg([keys], vals, agg, distinct))
        SR.check_groupby(one, model, agg, f"one shot {agg} keys {kdt} values {vdt}")
        for slab in SC.slabs_for(cols):
            set_slab(slab)
            got = SR.groups_of(*gpu.groupby_agg([keys], vals, agg, distinct))
            assert slabs_cut() >= 2, (slab, slabs_cut())
            SR.check_groupby(got, model, agg, f"{agg} keys {kdt} values {vdt}, slab {slab}")
            if vals is not None and agg != "count" and (vdt not in (A.F32, A.F64) or agg != "sum"):
                assert got == one, f"{agg} keys {kdt} values {vdt}, slab {slab}: streamed vs one shot"
            with pytest.raises(A.RdfError) as ei:
                gpu.groupby_agg([keys], vals, agg, distinct - 1)
            assert ei.value.status == A.RDF_MEMORY_ERROR


# ---------------------------------------------------------------- fused grouped aggregation
def test_streamed_group_pipeline(gpu):
    from test_group_pipeline import q1_program
    rng = np.random.default_rng(33)
    n = sum(SC.LENS)
    cols = [SC.column(rng, A.F64, rng.integers(1, 51, n).astype(np.float64)), SC.column(rng, A.F64, np.round(rng.uniform(900.0, 105000.0, n), 2)),
            SC.column(rng, A.F64, rng.integers(0, 11, n) / 100.0), SC.column(rng, A.F64, rng.integers(0, 9, n) / 100.0),
            SC.column(rng, A.I8, rng.integers(0, 3, n)), SC.column(rng, A.I8, rng.integers(0, 2, n)), SC.column(rng, A.I32, rng.integers(8036, 10562, n))]
    e, pred, gid, vals = q1_program()
    model = SR.grouped(e, cols, vals, gid, 6, pred)
    assert isinstance(model, GR.Model) and model.rows[6] > 0 and min(model.rows[:6]) > 0
    with slab_option() as set_slab:
        set_slab(-1)
        one = gpu.group_pipeline(e, cols, vals, gid, 6, pred, with_some=True)
        assert slabs_cut() == 0
        GR.check(one, model, "Q1 one shot")
        for slab in SC.slabs_for(cols):
            set_slab(slab)
            got = gpu.group_pipeline(e, cols, vals, gid, 6, pred, with_some=True)
            assert slabs_cut() >= 2, (slab, slabs_cut())
            GR.check(got, model, f"Q1 slab {slab}")
            GR.check_same(got, one, model, f"Q1 slab {slab}: streamed vs one shot")


# ---------------------------------------------------------------- page-locked routes
PIECE = 35_840                 # rows of a piece of ONE Float64 column at 1.25 MiB slabs: (1.25 MiB / 4 / 9 bytes) rounded down to 1024 rows
DIRECT_MIN = 256 << 10
ROUTE_SLAB = (5 << 20) // 4


def _routes(slices, piece=PIECE, es=8, pinned=True):
    """(staged, direct) bytes of the values of one column: a piece travels from the first row of the byte its bitmap starts in,
    on its own where it is page-locked and at least 256 KiB."""
    staged = direct = 0
    for start, ln in slices:
        for r0 in range(0, ln, piece):
            b = (min(piece, ln - r0) + ((start + r0) & 7)) * es
            if pinned and b >= DIRECT_MIN:
                direct += b
            else:
                staged += b
    return staged, direct


ROUTE_SHAPES = {
    "consecutive slices of 256-byte multiples (one run)": [(0, 71_680), (71_680, 35_840), (107_520, 71_680)],
    "a 40 001-row slice breaks the run": [(0, 40_001), (40_001, 71_680), (111_681, 71_680)],
    "slices at offsets 3 and 5: byte-rounded starts before the previous end": [(3, 71_680), (71_683, 35_842), (107_525, 71_680)],
    "slices with gaps between them": [(0, 71_680), (71_688, 35_840), (107_600, 71_680)],
}


@pytest.fixture(scope="module")
def pinned_column():
    """370 000 rows of integer-valued Float64 with 2^40 markers in memory from rdf_host_alloc, and a registered copy."""
    from rust_dataframe_amd import lib
    L = lib.load()
    n = 370_000
    rng = np.random.default_rng(4)
    x = SC.marked_f64(rng, n, every=4099)
    p = C.c_void_p(0)
    assert L.rdf_host_alloc(C.byref(p), n * 8) == 0
    px = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(n,))
    px[:] = x
    reg = x.copy()
    assert L.rdf_host_register(C.c_void_p(reg.ctypes.data), reg.nbytes) == 0
    yield px, reg, x
    L.rdf_host_unregister(C.c_void_p(reg.ctypes.data))
    L.rdf_host_free(p)


def _check_sum(gpu, cols, what):
    e = A.Expr()
    filt = e.op("gt", e.col(0), e.scalar(-500.0))
    values = [e.col(0)]
    got = gpu.pipeline(e, cols, values, filt)
    model = SR.aggregate(e, cols, values, filt)
    assert (got[0].count, got[0].min, got[0].max, got[0].sum) == (model[0].count, model[0].min, model[0].max, model[0].sum), (what, got[0], model[0].sum)


@pytest.mark.parametrize("shape", list(ROUTE_SHAPES))
@pytest.mark.parametrize("memory", ["rdf_host_alloc", "rdf_host_register"])
def test_page_locked_inputs(gpu, pinned_column, shape, memory):
    from rust_dataframe_amd import lib
    px, reg, _ = pinned_column
    buf = px if memory == "rdf_host_alloc" else reg
    slices = ROUTE_SHAPES[shape]
    xs = [A.HostArray(buf, None, s, ln, A.F64, 0) for s, ln in slices]
    with slab_option() as set_slab:
        set_slab(ROUTE_SLAB)
        _check_sum(gpu, [xs], shape)
        slabs, staged, direct = lib.stream_stats()
        assert slabs >= 2 and (staged, direct) == _routes(slices), (shape, slabs, staged, direct, _routes(slices))
        assert direct > 0 and (staged > 0) == ("40 001" in shape or "offsets" in shape)      # (a 4161-row tail piece; a 2-row one)


def test_page_locked_and_pageable_columns_in_one_call(gpu, pinned_column):
    """A page-locked Float64 column next to a pageable Int8 one (pieces of 32 768 rows: 256 KiB of Float64, just at the threshold)."""
    from rust_dataframe_amd import lib
    px, _, _ = pinned_column
    rng = np.random.default_rng(6)
    slices = [(0, 65_536), (65_536, 32_768), (98_304, 65_536)]
    k = rng.integers(-100, 100, 170_000).astype(np.int8)
    xs = [A.HostArray(px, None, s, ln, A.F64, 0) for s, ln in slices]
    ks = [A.HostArray(k, None, s, ln, A.I8, 0) for s, ln in slices]
    e = A.Expr()
    values, filt = [e.col(0), e.col(1)], e.op("gt", e.col(1), e.scalar(-50.0))
    with slab_option() as set_slab:
        set_slab(ROUTE_SLAB)
        got = gpu.pipeline(e, [xs, ks], values, filt)
        slabs, staged, direct = lib.stream_stats()
        model = SR.aggregate(e, [xs, ks], values, filt)
        assert [(g.count, g.min, g.max, g.sum) for g in got] == [(m.count, m.min, m.max, m.sum) for m in model]
        assert slabs >= 2 and direct == _routes(slices, 32_768)[1] == 163_840 * 8 and staged == 163_840, (slabs, staged, direct)


def test_registered_values_with_staged_validity(gpu, pinned_column):
    from rust_dataframe_amd import lib
    _, reg, _ = pinned_column
    rng = np.random.default_rng(8)
    slices = ROUTE_SHAPES["consecutive slices of 256-byte multiples (one run)"]
    valid = A.pack_bits(rng.uniform(size=len(reg)) >= 0.1)
    xs = [A.HostArray(reg, valid, s, ln, A.F64, -1) for s, ln in slices]
    with slab_option() as set_slab:
        set_slab(ROUTE_SLAB)
        _check_sum(gpu, [xs], "validity staged")
        slabs, staged, direct = lib.stream_stats()
        # (a row of Float64 and its validity bit: 1.25 MiB / 4 / 9 bytes is still 35 840 rows; every piece starts on a byte here)
        bitmap_bytes = sum((min(PIECE, ln - r0) + 7) // 8 for _, ln in slices for r0 in range(0, ln, PIECE))
        assert slabs >= 2 and direct == _routes(slices)[1] and staged == bitmap_bytes, (slabs, staged, direct, bitmap_bytes)


@pytest.mark.parametrize("shape", list(ROUTE_SHAPES))
def test_registered_outputs(gpu, pinned_column, shape):
    """abs(x) written into registered memory.  A stored Float64 row counts 17 bytes (8 in, 8 + 1 bit out): the pieces are 35 840 rows
    at 2.5 MiB slabs, and a call streams when its input passes one slab — so every shape is followed by one more slice of
    179 200 rows.  The counters speak for the inputs (see the module docstring); the outputs are compared value by value, and the
    memory around every output slice must be untouched."""
    from rust_dataframe_amd import lib
    L = lib.load()
    px, _, x = pinned_column
    slices = ROUTE_SHAPES[shape] + [(sum(ROUTE_SHAPES[shape][-1]), 179_200)]
    y = np.full(len(x) + 16, -7.0)
    assert L.rdf_host_register(C.c_void_p(y.ctypes.data), y.nbytes) == 0
    try:
        xs = [A.HostArray(px, None, s, ln, A.F64, 0) for s, ln in slices]
        outs = [A.HostArray(y[s:s + ln], None, 0, ln, A.F64, 0) for s, ln in slices]
        with slab_option() as set_slab:
            set_slab(2 * ROUTE_SLAB)
            got = gpu.unary("abs", xs, outs)
            slabs, staged, direct = lib.stream_stats()
            assert slabs >= 2 and (staged, direct) == _routes(slices), (shape, slabs, staged, direct)
        expect = np.full(len(y), -7.0)
        for s, ln in slices:
            expect[s:s + ln] = np.abs(x[s:s + ln])
        assert np.array_equal(y, expect), np.flatnonzero(y != expect)[:8]
        assert [(o.length, o.null_count) for o in got] == [(ln, 0) for _, ln in slices]
    finally:
        L.rdf_host_unregister(C.c_void_p(y.ctypes.data))


# ---------------------------------------------------------------- thread buffers
def _small_agg(rng, ncols, lens):
    cols = [SC.column(rng, A.F64, SC.marked_f64(rng, sum(lens)), nulls=0.1, lens=lens, offsets=[(3 * i + c) % 10 for i in range(len(lens))], all_null=-1) for c in range(ncols)]
    e = A.Expr()
    values = [e.col(c) for c in range(min(ncols, 4))]
    filt = e.op("gt", e.col(ncols - 1), e.scalar(-400.0))
    return e, cols, values, filt


def _run_exact(api, case, slab, what):
    from rust_dataframe_amd import lib
    e, cols, values, filt = case
    lib.set_option("stream_slab_bytes", slab)
    try:
        got = api.pipeline(e, cols, values, filt)
        assert lib.stream_stats()[0] >= 2, what
    finally:
        lib.set_option("stream_slab_bytes", 0)
    model = SR.aggregate(e, cols, values, filt)
    assert [(g.count, g.min, g.max, g.sum) for g in got] == [(m.count, m.min, m.max, m.sum) for m in model], what


def test_thread_buffers_are_regrown_and_reused(gpu):
    """A small plan after a large one, then a larger one: the slab and staging buffers the thread keeps are reused and regrown."""
    rng = np.random.default_rng(11)
    _run_exact(gpu, _small_agg(rng, 3, [5000, 1023, 9000]), 64 << 10, "3 columns at 64 KiB")
    _run_exact(gpu, _small_agg(rng, 1, [2049, 7, 3000]), 8 << 10, "1 column at 8 KiB")
    _run_exact(gpu, _small_agg(rng, 5, [6000, 1025, 12_000]), 256 << 10, "5 columns at 256 KiB")


def test_two_threads_stream_at_once(gpu):
    rng = np.random.default_rng(12)
    cases = [(_small_agg(rng, 2, [6000, 1023, 9000]), 32 << 10), (_small_agg(rng, 3, [1025, 8000, 63, 7000]), 48 << 10)]
    errors = {}

    def work(i):
        try:
            for rep in range(3):
                _run_exact(gpu, cases[i][0], cases[i][1], f"thread {i} call {rep}")
        except BaseException as ex:   # noqa: BLE001
            errors[i] = ex
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---------------------------------------------------------------- errors mid-stream
def test_zero_divisor_in_the_third_slab(gpu):
    """Error values: RDF_DIVIDE_BY_ZERO from the slab that meets the zero, and the thread's next streamed call is exact.
    Two Int32 columns at 32 KiB slabs are cut into 1024-row pieces (4 KiB + 256 a column).  The store sink counts 5 more bytes
    a row for its output: two pieces a slab, the third slab is rows 4096-6143.  The filter sink: three pieces a slab, the third
    slab is rows 6144-9215."""
    rng = np.random.default_rng(13)
    lens = [4096] * 6
    num = SC.column(rng, A.I32, nulls=0.0, lens=lens, offsets=[0, 3, 5, 1, 7, 2], all_null=-1)
    den = SC.column(rng, A.I32, np.where(rng.integers(0, 2, sum(lens)) == 0, -3, 7), nulls=0.0, lens=lens, offsets=[1, 0, 2, 6, 4, 3], all_null=-1)
    e = A.Expr()
    quot = e.op("divide", e.col(0), e.col(1))
    pred = e.op("gt", quot, e.scalar(0.0))
    model = SR.store(e, [num, den], quot)
    kept = SR.filter_rows(e, [num, den], pred)
    sinks = {"store": (lambda: SR.check_store(gpu.binary("divide", num, den), model, lens, "store sink"), 4096 + 77),
             "filter": (lambda: SR.check_filter(gpu.filter_pipeline(e, pred, [num, den]), kept, [num, den], "filter sink"), 6144 + 77)}
    with slab_option() as set_slab:
        set_slab(32 << 10)
        for what, (run_and_check, row) in sinks.items():
            run_and_check()
            assert slabs_cut() >= 4, what
            cell = den[row // 4096].values[den[row // 4096].offset + row % 4096:][:1]
            saved = int(cell[0])
            cell[0] = 0
            try:
                with pytest.raises(A.RdfError) as ei:
                    run_and_check()
                assert ei.value.status == A.RDF_DIVIDE_BY_ZERO, (what, ei.value)
            finally:
                cell[0] = saved
            run_and_check()                                 # the thread's stream buffers are intact
            assert slabs_cut() >= 4, what
