"""tests/group_ref.py (the model of rdf_group_pipeline) held to the C oracle and to numpy_q1, and every input of
tests/test_group_pipeline_gpu.py drawn here, without a GPU, to assert what its cases rely on: an exact-family case really is
exact, a threshold case really has the replica count it names, the long case really gives every block three tiles."""
import numpy as np
import pytest

from rust_dataframe_amd import _abi as A

import group_cases as GC
import group_ref as GR
import spec_ref as S
from test_group_pipeline import _cols_list, numpy_q1, q1_columns, q1_program

CU_COUNTS = (256, 304)


# ---------------------------------------------------------------- the model against the oracle
def _small_programs():
    """A dozen small programs and layouts: (name, builder of a Case)."""
    def pick(gen, name):
        return dict(GC.GENERATORS[gen]())[name]
    out = [("q1 exact, NULLs, chunked", pick("layout", "q1-chunked")),
           ("q1 general family", pick("layout", "q1-general-chunked")),
           ("q1 at an odd offset", pick("layout", "q1-off13")),
           ("q1 with a fourth flag code", pick("catalog", "q1-G8-ng7")),
           ("i8 key, two f64 values", pick("layout", "key2-chunked")),
           ("i64 key, i64 extremes, one group", pick("catalog", "keyl-l-ng1")),
           ("a group of NULL values", pick("sparse", "null-group")),
           ("a column of NULL values", pick("sparse", "null-column")),
           ("no row passes", pick("sparse", "none-pass")),
           ("a NULL predicate", pick("sparse", "null-predicate")),
           ("BOOL key", pick("jit", "bool-G2")),
           ("u16 cast to i64", pick("jit", "u8-u16-G4")),
           ("computed i16 key, f32 value", pick("jit", "i16-computed-G8")),
           ("eight values", pick("jit", "q1-wide-G8")),
           ("u64 extremes", pick("value", "int-u")),
           ("i8 extremes", pick("value", "int-a")),
           ("a comparison as a value", pick("value", "compare")),
           ("NaN and infinities", pick("value", "nonfinite")),
           ("the slot limit, 8 values", pick("table", "limit-ng127-nv8")),
           ("an id out of range", lambda: GC.range_case(A.I16, "tail-end", -1)),
           ("an id out of range behind the filter", lambda: GC.range_case(A.I16, "tail-end", -1, dropped=True)),
           ("u8 id equal to ngroups", lambda: GC.range_case(A.U8, "null-value", 5)),
           ("i8 id -1 with 300 groups", lambda: GC.range_case(A.I8, "first", -1, ngroups=300))]
    return out


SMALL = _small_programs()


@pytest.mark.parametrize("name,build", SMALL, ids=[n for n, _ in SMALL])
def test_model_matches_oracle(ora, name, build):
    """Counts, rows, is_some and integer sums exactly; float sums by the any-order bound (the oracle adds in f64)."""
    c = build()
    model = GR.run_chunks(c.expr, c.cols, c.vals, c.gid, c.ngroups, c.pred)

    def call():
        return ora.group_pipeline(c.expr, c.cols, c.vals, c.gid, c.ngroups, c.pred, with_some=True)
    if isinstance(model, GR.Failure):
        GR.expect_failure(call, model, name)
        return
    GR.check(call(), model, name, floats_exact=c.exact)
    GR.check(model.as_result(), model, name, floats_exact=True)        # the comparison accepts its own reference
    if c.q1_groups is not None:                                          # ... and the integer restatement is the model, bit for bit
        GR.check(GC.q1_exact_model(c.cols, c.q1_groups).as_result(), model, name + " (integer arithmetic)", floats_exact=True)


def test_model_argument_errors_match_oracle(ora):
    c = GC.key_case("arguments", 1, A.I32, (A.F64,), [10], 4)
    e = c.expr
    f = e.cast(c.gid, A.F64)
    for what, vals, gid, ng in [("float id", c.vals, f, 4), ("no groups", c.vals, c.gid, 0), ("past the slot limit", c.vals, c.gid, 1024),
                                ("past the slot limit, 8 values", c.vals * 8, c.gid, 128), ("nine values", c.vals * 9, c.gid, 4),
                                ("past the limit with an id out of range", c.vals * 2, c.gid, 512)]:
        model = GR.run_chunks(e, c.cols, vals, gid, ng)
        assert isinstance(model, GR.Failure) and model.status == A.RDF_INVALID_ARGUMENT, what
        GR.expect_failure(lambda: ora.group_pipeline(e, c.cols, vals, gid, ng), model, what)


def test_q1_restatement_matches_numpy_q1():
    rng = np.random.default_rng(71)
    cols = q1_columns(rng, [1024, 1024, 576])
    e, pred, gid, vals = q1_program()
    model = GR.run_chunks(e, _cols_list(cols), vals, gid, 6, pred)
    GR.check(numpy_q1(cols), model, "numpy_q1 (pairwise sums) against the model")


def test_the_bound_bites():
    """A lost row, an f32 accumulation and a count off by one are outside the comparison; the reference itself is inside."""
    c = dict(GC.layout_cases())["q1-general-chunked"]()
    model = c.model()
    res, rows = model.as_result()
    g = int(np.argmax(model.counts[1][:6]))
    x = model.values[1][g]

    def with_sum(s, dcount=0):
        r = [list(v) for v in res]
        r[1][g] = (s, res[1][g][1] + dcount, res[1][g][2])
        return r, rows
    GR.check(with_sum(float(np.sum(x))), model, "numpy's pairwise sum")
    GR.check(with_sum(float(np.cumsum(x)[-1])), model, "a sequential sum")
    biggest = float(x[np.argmax(np.abs(x))])
    for what, bad in [("a lost row", (res[1][g][0] - biggest, 0)), ("f32 accumulation", (float(np.sum(x.astype(np.float32), dtype=np.float32)), 0)),
                      ("a count", (res[1][g][0], 1))]:
        with pytest.raises(AssertionError):
            GR.check(with_sum(*bad), model, what)
    one = GR.Model(1, [A.F64], [[1.5, 0.0]], [[1, 0]], [1, 0], [[np.array([1.5]), np.zeros(0)]])
    GR.check(([[(1.5, 1, 1), (0.0, 0, 0)]], [1, 0]), one, "one value")
    GR.check(([[(1.5, 1, 1), (-0.0, 0, 0)]], [1, 0]), one, "the two zeros are peers")
    with pytest.raises(AssertionError):
        GR.check(([[(float(np.nextafter(1.5, 2.0)), 1, 1), (0.0, 0, 0)]], [1, 0]), one, "one value comes back itself")


# ---------------------------------------------------------------- what the GPU cases rely on
def _assert_exact_family(model, what):
    """Every float value a multiple of 2^-14 and sum |x| 2^14 < 2^53: each partial sum in any order is exactly representable."""
    for v, dt in enumerate(model.dtypes):
        if dt not in S.FLOATS:
            continue
        for g in range(model.ngroups + 1):
            x = model.values[v][g]
            if x is None or len(x) == 0:
                continue
            scaled = np.ldexp(x, 14)
            assert np.array_equal(scaled, np.trunc(scaled)), f"{what}: value {v} group {g} is not in 2^-14 steps"
            assert int(np.abs(scaled).astype(np.int64).sum()) < 2 ** 53, f"{what}: value {v} group {g} can leave the exact range"


def _check_drawn(c):
    model = GR.run_chunks(c.expr, c.cols, c.vals, c.gid, c.ngroups, c.pred)
    assert isinstance(model, GR.Model), c.name
    if c.exact:
        _assert_exact_family(model, c.name)
    if c.q1_groups is not None:        # the integer restatement asserts its own preconditions (numerators, partial sums below 2^53)
        GR.check(GC.q1_exact_model(c.cols, c.q1_groups).as_result(), model, c.name, floats_exact=True)
    if c.replicas is not None:
        ntmp = 0       # a column, or a column + a literal: neither operand is a subtree, so no TMP slot is spilled
        assert GC.group_replicas(GC.group_words(c.ngroups, len(c.vals)), ntmp) == c.replicas, c.name
        assert min(model.rows[:c.ngroups]) > 0, f"{c.name}: every group populated"
    return model


ALL_SMALL_CASES = [(f"{g}-{name}", build) for g, gen in GC.GENERATORS.items() for name, build in gen()]


@pytest.mark.parametrize("name,build", ALL_SMALL_CASES, ids=[n for n, _ in ALL_SMALL_CASES])
def test_every_gpu_case_is_what_it_says(name, build):
    _check_drawn(build())


def test_catalog_table_and_replica_table():
    assert len(GC.CATALOG) == 11 and len(set(GC.CATALOG)) == 11
    named = {c.kernel for _, b in GC.catalog_cases() for c in [b()]}
    assert named == set(GC.CATALOG), "the catalog sweep names every registered kernel"
    assert sorted({r for _, _, r in GC.REPLICA_CASES}) == [1, 2, 4, 8, 16, 32]
    for ng, nv, reps in GC.REPLICA_CASES:
        assert GC.group_replicas(GC.group_words(ng, nv)) == reps
        assert (ng + 1) * nv <= A.MAX_GROUP_SLOTS
    for ng, nv in GC.SLOT_LIMIT_CASES:
        assert (ng + 1) * nv == A.MAX_GROUP_SLOTS and GC.group_replicas(GC.group_words(ng, nv)) == 1
    skewed = dict(GC.table_cases())["limit-ng511-nv2"]().model()
    assert skewed.rows[7] > 0.8 * GC.TABLE_ROWS, "most rows in one group"


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_long_cases_give_every_block_three_tiles(cus):
    n = GC.long_rows(cus)
    for lens in ([n], GC.long_key_lens(cus)):
        assert sum(lens) == n and min(lens) > 0
        per_block = GC.tiles_per_block(lens, cus)              # gspec_blocks_per_cu = 1: the grid is the CU count
        assert len(per_block) == cus and min(per_block) >= 3 and max(per_block) <= 4, (lens, min(per_block), max(per_block))
    assert n % GC.TILE == 300 and GC.tiles_of([n]) == 3 * cus + 2                  # the last tile is partial
    first = GC.long_key_lens(cus)[0]
    assert (first - 1) // GC.TILE == cus + 7 and first % GC.TILE == 500            # chunk 0 ends inside tile cus + 7: block 7's second
    for block, row in ((9, 513), (9, 514), (5, 77)):
        r = GC.third_tile_row(cus, block, row)
        assert r < n and r // GC.TILE == 2 * cus + block                           # tile 2 cus + block: block `block`'s third
    for name, build in GC.long_cases(cus):
        c = build()
        assert c.options.get("gspec_blocks_per_cu") == 1 and c.exact
        model = _check_drawn(c)
        if name == "q1-planted":
            dense = dict(GC.long_cases(cus))["q1-dense"]().model()
            assert model.rows[6] == 1 and dense.rows[6] == 0                        # exactly one NULL id ...
            nulls = [sum(model.rows) - sum(cnt) for cnt in model.counts]
            assert nulls == [0, 1, 1, 1, 0]                                         # ... and one NULL price, on rows that pass


@pytest.mark.parametrize("key_dt", GC.RANGE_KEYS, ids=[GC.TAG[k] for k in GC.RANGE_KEYS])
def test_range_cases_fail_and_pass_as_they_say(key_dt):
    for ng in (5, 300) if key_dt in (A.I8, A.I16) else (5,):
        for where in GC.RANGE_POSITIONS:
            for bad in ([ng] if ng <= np.iinfo(A.NP_OF[key_dt]).max else []) + ([-1] if key_dt in S.SIGNED else []):
                m = GC.range_case(key_dt, where, bad, ng).model()
                assert isinstance(m, GR.Failure) and m.status == A.RDF_COMPUTE_ERROR, (key_dt, where, bad)
                m = GC.range_case(key_dt, where, bad, ng, dropped=True).model()
                assert isinstance(m, GR.Model) and sum(m.rows) == sum(GC.RANGE_LENS) - 1
    assert GC.RANGE_POSITIONS["tail-end"] == sum(GC.RANGE_LENS) - 1 and GC.RANGE_LENS[-1] % GC.TILE


def test_q1_range_cases_fail_and_pass_as_they_say():
    for row in GC.Q1_RANGE_ROWS:
        m = GC.q1_range_case(row).model()
        assert isinstance(m, GR.Failure) and m.status == A.RDF_COMPUTE_ERROR
        c = GC.q1_range_case(row, dropped=True)
        _check_drawn(c)
        assert sum(c.model().rows) > 0
