"""rdf_group_pipeline (the fused GroupAggregate sink, TPC-H Q1's shape) held to tests/group_ref.py — a model in numpy and Python
integers that does not depend on the oracle — on every path behind the call: the 11 catalog kernels of rdf_gspec.hip by name,
the rows around every unit of gspec_kernel, its persistent loop with the next-tile prefetch and the rotated / swizzled walks,
the sparse LDS path, ids out of range at every key width, the interpreter's LDS table at all six replica counts and at the
slot limit, and the template through the run-time compiler at G2 / G4 / G8.

Counts, rows, is_some and integer sums are compared exactly.  Inputs of the exact family (tests/group_cases.py) have every
product and partial sum exactly representable, so their float sums must come back bit for bit on every engine in every order;
general float sums are held to the bound that holds for any order of correctly rounded additions (group_ref.check).  Each case
runs from host arrays and from device arrays (and through a pinned frame where it says so); the runs must agree with the model
and, in everything but general float sums, with each other.  tests/test_group_ref.py draws the same inputs without a GPU and
asserts what the cases rely on."""
from contextlib import contextmanager

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A

import group_cases as GC
import group_ref as GR

pytestmark = pytest.mark.gpu

RESET = {"gspec_blocks_per_cu": 0, "spec_tile_rot": -1, "spec_xcd_swz": -1, "jit": 0}


def to_device(cols):
    """The same chunks in device memory (values and bitmaps keep their element / bit offsets)."""
    import torch
    dev = []
    for col in cols:
        dcol = []
        for ch in col:
            vt = torch.from_numpy(np.frombuffer(ch.values.tobytes() + b"\0" * 64, dtype=np.uint8).copy()).cuda()
            bt = None
            if ch.validity is not None:
                bt = torch.from_numpy(np.frombuffer(ch.validity.tobytes() + b"\0" * 64, dtype=np.uint8).copy()).cuda()
            dcol.append(A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, ch.offset, ch.length, ch.dtype, -1, keep=(vt, bt)))
        dev.append(dcol)
    torch.cuda.synchronize()
    return dev


@contextmanager
def options(opts):
    from rust_dataframe_amd import lib
    try:
        for k, v in opts.items():
            lib.set_option(k, v)
        yield
    finally:
        for k, v in RESET.items():
            lib.set_option(k, v)


def assert_kernel(c, mode, what):
    from rust_dataframe_amd import lib
    ran = lib.last_kernel()
    if mode == "interp" or c.kernel == GC.INTERP:
        assert ran.startswith(GC.INTERP), f"{what}: {ran}"
    elif c.kernel is not None:
        assert ran == f"gspec_kernel<{c.kernel}>" + (" [compiled at run time]" if c.jit else ""), f"{what}: {ran}"
    return ran


def run_case(gpu, request, c, model=None):
    """-> the kernel names that ran.  The model's answer, or the status it fails with, from host arrays, device arrays and
    (c.frame) a pinned frame."""
    mode = request.node.callspec.params["gpu"]
    model = c.model() if model is None else model
    ran, results = set(), []
    with options({**c.options, **({"jit": 2} if c.jit else {})}):
        dev = to_device(c.cols)
        for how in ("host", "device") + (("frame",) if c.frame else ()):
            what = f"{c.name} [{how}]"
            frame = A.PinnedFrame(gpu, dev) if how == "frame" else None
            cols = c.cols if how == "host" else dev if how == "device" else frame
            try:
                def call():
                    return gpu.group_pipeline(c.expr, cols, c.vals, c.gid, c.ngroups, c.pred, with_some=True)
                if isinstance(model, GR.Failure):
                    GR.expect_failure(call, model, what)
                    if model.status == A.RDF_INVALID_ARGUMENT:
                        continue
                else:
                    got = call()
                    GR.check(got, model, what, floats_exact=c.exact)
                    results.append((what, got))
                if c.rows():
                    ran.add(assert_kernel(c, mode, what))
            finally:
                if frame is not None:
                    frame.release()
    for what, got in results[1:]:
        GR.check_same(results[0][1], got, model, f"{results[0][0]} against {what}", floats_exact=c.exact)
    return ran


def _ids(pairs):
    return [n for n, _ in pairs]


# ---------------------------------------------------------------- every catalog kernel by name
def test_every_catalog_kernel_by_name(gpu, request):
    """The 11 registrations of rdf_gspec.hip (GC.CATALOG restates them): Q1 at G6 and at G8 (ngroups 7 and 8: a fourth flag
    code), the key family at G8 with ngroups 7, 8 and 1, over one ragged layout with 10 % NULLs in keys and values."""
    seen = set()
    for _, build in GC.catalog_cases():
        seen |= run_case(gpu, request, build())
    if request.node.callspec.params["gpu"] == "spec":
        assert len(GC.CATALOG) == 11 and seen == {f"gspec_kernel<{s}>" for s in GC.CATALOG}, sorted(seen)
    else:
        assert seen == {GC.INTERP}


# ---------------------------------------------------------------- rows around every unit of the kernel
@pytest.mark.parametrize("n", GC.UNIT_ROWS)
def test_rows_around_every_unit(gpu, request, n):
    cases = dict(GC.unit_cases())
    for name in (f"q1-{n}", f"key2-{n}"):
        run_case(gpu, request, cases[name]())


LAYOUT = GC.layout_cases()


@pytest.mark.parametrize("name,build", LAYOUT, ids=_ids(LAYOUT))
def test_chunks_and_offsets(gpu, request, name, build):
    """A tail tile before a full one with an empty chunk between (also through a frame); even start offsets keep the 2-row
    vector loads and start the validity windows on both sides of a 64-bit word; the odd offset falls back to the interpreter."""
    run_case(gpu, request, build())


# ---------------------------------------------------------------- the persistent loop
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


LONG = [name for name, _ in GC.long_cases(256)]


@pytest.mark.parametrize("name", LONG)
def test_persistent_loop(gpu, request, name):
    """One block a CU and (3 CUs + 1) * 1024 + 300 rows: every block walks three or four tiles, so the next-tile prefetch, the
    full -> tail and tail -> full transitions between chunks and the rotated / swizzled walks all run.  Exact family: every sum,
    count and row count bit for bit."""
    c = dict(GC.long_cases(_cus()))[name]()
    assert min(GC.tiles_per_block([ch.length for ch in c.cols[0]], _cus())) >= 3
    run_case(gpu, request, c)


# ---------------------------------------------------------------- the sparse path
SPARSE = GC.sparse_cases()


@pytest.mark.parametrize("name,build", SPARSE, ids=_ids(SPARSE))
def test_sparse_path(gpu, request, name, build):
    c = build()
    model = c.model()
    if name == "null-group":
        assert model.rows[3] > 0 and model.counts[0][3] == 0 and model.sums[0][3] == 0.0
    if name == "null-column":
        assert sum(model.counts[1]) == 0 and sum(model.rows) == c.rows()
    if name == "none-pass":
        assert sum(model.rows) == 0
    run_case(gpu, request, c, model)


# ---------------------------------------------------------------- ids out of range
def _bad_ids(key_dt, ng):
    return ([ng] if ng <= np.iinfo(A.NP_OF[key_dt]).max else []) + ([-1] if key_dt in (A.I8, A.I16, A.I32, A.I64) else [])


@pytest.mark.parametrize("key_dt", GC.RANGE_KEYS, ids=[GC.TAG[k] for k in GC.RANGE_KEYS])
def test_ids_out_of_range(gpu, request, key_dt):
    """One id equal to ngroups and one negative id, at the first row, at the last row of a tail tile and at a row whose value
    is NULL: RDF_COMPUTE_ERROR, and the model's answer once a predicate drops the row.  With 300 groups a zero-extended -1 of
    an I8 / I16 key would be a legal id."""
    for ng in (5, 300) if key_dt in (A.I8, A.I16) else (5,):
        for where in GC.RANGE_POSITIONS:
            for bad in _bad_ids(key_dt, ng):
                failing = GC.range_case(key_dt, where, bad, ng)
                assert isinstance(failing.model(), GR.Failure)
                run_case(gpu, request, failing)
                run_case(gpu, request, GC.range_case(key_dt, where, bad, ng, dropped=True))


@pytest.mark.parametrize("key_dt", GC.RANGE_KEYS, ids=[GC.TAG[k] for k in GC.RANGE_KEYS])
def test_ids_out_of_range_in_a_third_tile(gpu, request, key_dt):
    for bad in _bad_ids(key_dt, 5):
        run_case(gpu, request, GC.range_case(key_dt, None, bad, 5, cus=_cus()))
        run_case(gpu, request, GC.range_case(key_dt, None, bad, 5, cus=_cus(), dropped=True))


def test_q1_id_out_of_range(gpu, request):
    """The computed Q1 id: a fourth flag code with ngroups 6 fails on the G6 kernel, and passes once the ship date drops the row."""
    for row in GC.Q1_RANGE_ROWS:
        failing = GC.q1_range_case(row)
        assert isinstance(failing.model(), GR.Failure)
        run_case(gpu, request, failing)
        run_case(gpu, request, GC.q1_range_case(row, dropped=True))


# ---------------------------------------------------------------- the interpreter's table
TABLE = GC.table_cases()


@pytest.mark.parametrize("name,build", TABLE, ids=_ids(TABLE))
def test_interpreter_table(gpu, request, name, build):
    """Replica counts 32, 16, 8, 4, 2 and 1 (both sides of every halving; test_group_ref.py asserts which) and the slot limit,
    every group populated: general-family f64 sums within the any-order bound, wrapping i64 sums exactly."""
    run_case(gpu, request, build())


@pytest.mark.parametrize("ng,nv", [(1024, 1), (128, 8), (512, 2)])
def test_one_past_the_slot_limit(gpu, request, ng, nv):
    c = GC.key_case("one past the slot limit", 950, A.I32, (A.F64,), [100], 8)
    c.ngroups, c.vals, c.kernel = ng, c.vals * nv, None
    model = c.model()
    assert isinstance(model, GR.Failure) and model.status == A.RDF_INVALID_ARGUMENT
    run_case(gpu, request, c, model)


# ---------------------------------------------------------------- the template through the run-time compiler
JIT = GC.jit_cases()


@pytest.mark.parametrize("name,build", JIT, ids=_ids(JIT))
def test_template_compiled_at_run_time(gpu, request, name, build):
    """G2, G4 and G8 over 1-, 2-, 4- and 8-byte columns, none of them in the catalog.  The BOOL key asserts the interpreter: the
    host declines a Boolean column for the template (its values are a bitmap, not elements the 2-row vector loads can read)."""
    run_case(gpu, request, build())


# ---------------------------------------------------------------- value classes
VALUE = GC.value_cases()


@pytest.mark.parametrize("name,build", VALUE, ids=_ids(VALUE))
def test_value_classes(gpu, request, name, build):
    """Every integer width at its extremes (sums wrap in 64 bits, not at the value's width), a comparison summed as 0 / 1,
    F32 widened exactly, NaN and infinities by kind."""
    run_case(gpu, request, build())
