"""rdf_moments / rdf_comoments on the MI355X, held to the exact reference of tests/moments_ref.py: the count exactly, every
statistic inside its bound (B = gamma(2n) + 16u, see that module).  Every case runs over host and over device memory,
twice each, and the four states are identical bytes.  Shapes are the smallest at which each part of the kernel can go wrong:
around one lane row (64), one wave tile (512) and one block tile (2048), and 200 003 rows in seven unequal chunks behind
odd offsets, which makes several blocks write states and bitmap windows start inside a byte.

Each case prints its largest error in units of its bound (`pytest -s`); DESIGN.md 13 quotes the largest of them."""
import functools
import math

import numpy as np
import pytest

import moments_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

WAVE_TILE, TILE = 512, 2048
COUNTS = [0, 1, 2, 63, 64, 65, WAVE_TILE - 1, WAVE_TILE, WAVE_TILE + 1, TILE - 1, TILE, TILE + 1]
BIG = 200_003
CUTS = [1, 2049, 40_000, 40_511, 100_000, 163_840]            # seven chunks of unequal length, one of a single row
OFFSETS = [0, 1, 3, 7, 9, 13, 64]
INPUTS = R.ILL + R.BENIGN + R.HARD + ["constant"]


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


# ---------------------------------------------------------------- inputs
def to_device(x):
    vt = torch.from_numpy(np.ascontiguousarray(x.values)).cuda()
    bt = torch.from_numpy(np.ascontiguousarray(x.validity)).cuda() if x.validity is not None else None
    return A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, x.offset, x.length, x.dtype, x.null_count, keep=(vt, bt))


def split(x, valid=None, cuts=(), offsets=None, dtype=None):
    bounds = [0] + [c for c in cuts if c < len(x)] + [len(x)]
    return [A.HostArray.from_numpy(x[a:b], None if valid is None else valid[a:b], offset=offsets[i] if offsets else 0, dtype=dtype)
            for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))]


def counted(chunks, mask=None):
    """The values that count, `as f64`, in row order."""
    parts = []
    for i, ch in enumerate(chunks):
        keep = ch.valid_mask()
        if mask is not None:
            keep = keep & mask[i].valid_mask() & mask[i].to_numpy()
        parts.append(ch.to_numpy()[keep].astype(np.float64))
    return np.concatenate(parts) if parts else np.zeros(0)


@functools.lru_cache(maxsize=None)
def named(name, n, as_int=False):
    x = R.make_input(name, n)
    return np.round(x).astype(np.int64) if as_int else x


def four_ways(call, chunk_lists):
    """call(*lists) over host memory and over device memory, twice each: identical bytes; -> the state."""
    dev = [None if c is None else [to_device(a) for a in c] for c in chunk_lists]
    states = [call(*chunk_lists), call(*dev), call(*chunk_lists), call(*dev)]
    assert all(bytes(s) == bytes(states[0]) for s in states[1:]), [bytes(s).hex() for s in states]
    return states[0]


def check_moments(api, chunks, mask=None, what=""):
    st = four_ways(lambda c, m: api.moments(c, m), [chunks, mask])
    ref = R.MomentsRef(counted(chunks, mask))
    assert st.count == ref.n, what
    if ref.n == 0:
        assert bytes(st) == bytes(48), what
    worst = R.error_in_bounds({s: api.moments_stat(st, s) for s in R.STATS}, ref, R.STATS)
    print(f"MOMENTS_ERR {what} n={ref.n} worst={max(worst.values()):.3g} of its bound ({max(worst, key=worst.get)})")
    assert max(worst.values()) <= 1.0, (what, worst)
    return st, ref


def ratio(err, bound):
    return 0.0 if err == 0 else (float(err) / bound if bound > 0 else math.inf)


def check_comoments(api, x, y, mask=None, what=""):
    st = four_ways(lambda a, b, m: api.comoments(a, b, m), [x, y, mask])
    keep = [a.valid_mask() & b.valid_mask() for a, b in zip(x, y)]
    if mask is not None:
        keep = [k & m.valid_mask() & m.to_numpy() for k, m in zip(keep, mask)]
    keep = np.concatenate([np.zeros(0, dtype=bool)] + keep)
    xv = np.concatenate([np.zeros(0)] + [a.to_numpy().astype(np.float64) for a in x])[keep]
    yv = np.concatenate([np.zeros(0)] + [a.to_numpy().astype(np.float64) for a in y])[keep]
    ref = R.ComomentsRef(xv, yv)
    assert st.count == ref.n, what
    if ref.n == 0:
        assert bytes(st) == bytes(64), what
    worst = R.error_in_bounds({s: api.comoments_stat(st, s) for s in R.COSTATS}, ref, R.COSTATS)
    if ref.n:   # the per-column sums and means of the pair state are the single-column ones
        worst["m2x"] = ratio(abs(R.Fraction(st.m2x) - ref.x.m2), ref.x.bound("var_pop") * ref.n)
        worst["m2y"] = ratio(abs(R.Fraction(st.m2y) - ref.y.m2), ref.y.bound("var_pop") * ref.n)
        worst["mean_x"] = ratio(abs(R.Fraction(st.mean_x) + R.Fraction(st.mean_x_lo) - ref.x.mean), ref.x.bound("mean"))
        worst["mean_y"] = ratio(abs(R.Fraction(st.mean_y) + R.Fraction(st.mean_y_lo) - ref.y.mean), ref.y.bound("mean"))
    print(f"MOMENTS_ERR co {what} n={ref.n} worst={max(worst.values()):.3g} of its bound ({max(worst, key=worst.get)})")
    assert max(worst.values()) <= 1.0, (what, worst)
    return st, ref


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("as_int", [False, True], ids=["f64", "i64"])
@pytest.mark.parametrize("n", COUNTS)
def test_counted_rows_around_the_tile_sizes(api, n, as_int):
    """n rows that all count, and n counted rows scattered among NULL ones."""
    x = named("two_pow_52" if as_int else "offset_1e9", 3 * TILE + 7, as_int)
    check_moments(api, split(x[:n], offsets=[5]), what=f"plain {n}")
    rng = np.random.default_rng(n)
    rows = n + n // 2 + 3
    valid = np.zeros(rows, dtype=bool)
    valid[rng.choice(rows, n, replace=False)] = True
    check_moments(api, split(x[:rows], valid, cuts=[rows // 3], offsets=[3, 9]), what=f"{n} counted of {rows}")


@pytest.mark.parametrize("name", INPUTS)
def test_seven_unequal_chunks(api, name):
    x = named(name, BIG)
    st, ref = check_moments(api, split(x, cuts=CUTS, offsets=OFFSETS), what=f"{name} 7 chunks")
    if name == "constant":
        assert (st.m2, st.m3, st.m4, st.mean, st.mean_lo) == (0.0, 0.0, 0.0, 0.1, 0.0)
        assert api.moments_stat(st, "var_samp") == 0.0 and api.moments_stat(st, "skewness") is None and api.moments_stat(st, "kurtosis") is None


@pytest.mark.parametrize("name", ["two_pow_52", "offset_1e15", "outlier_first", "offset_1e9"])
def test_seven_unequal_chunks_int64(api, name):
    x = named(name, BIG, True)
    check_moments(api, split(x, cuts=CUTS, offsets=OFFSETS), what=f"{name} as Int64, 7 chunks")


@pytest.mark.parametrize("as_int", [False, True], ids=["f64", "i64"])
def test_nulls_masks_and_dead_chunks(api, as_int):
    x = named("offset_1e9", BIG, as_int)
    rng = np.random.default_rng(11)
    valid = rng.uniform(size=BIG) >= 0.1                                     # 10 % NULLs
    check_moments(api, split(x, valid, cuts=CUTS, offsets=OFFSETS), what="10% NULLs")
    dead = valid.copy()
    dead[2049:40_000] = False                                               # all-NULL chunks among live ones
    dead[100_000:163_840] = False
    check_moments(api, split(x, dead, cuts=CUTS, offsets=OFFSETS), what="all-NULL chunks")
    bits, mvalid = rng.uniform(size=BIG) < 0.4, rng.uniform(size=BIG) >= 0.2  # a mask with NULLs of its own, behind other offsets
    mask = split(bits, mvalid, cuts=CUTS, offsets=OFFSETS[::-1], dtype=A.BOOL)
    check_moments(api, split(x, valid, cuts=CUTS, offsets=OFFSETS), mask, what="masked, NULLs in column and mask")
    check_moments(api, split(x, cuts=CUTS, offsets=OFFSETS), split(bits, cuts=CUTS, offsets=OFFSETS, dtype=A.BOOL), what="masked, no NULLs")
    nothing = split(np.zeros(BIG, dtype=bool), mvalid, cuts=CUTS, offsets=OFFSETS, dtype=A.BOOL)
    st, _ = check_moments(api, split(x, valid, cuts=CUTS, offsets=OFFSETS), nothing, what="a mask that keeps nothing")
    assert all(api.moments_stat(st, s) is None for s in R.STATS)


# ---------------------------------------------------------------- dtypes
@pytest.mark.parametrize("dt", [A.I8, A.I16, A.I32, A.I64, A.U8, A.U16, A.U32, A.U64, A.F32, A.F64])
def test_every_numeric_dtype(api, dt):
    rng = np.random.default_rng(dt)
    n = 2 * TILE + 300
    npdt = A.NP_OF[dt]
    if dt in (A.F32, A.F64):
        x = (1e4 + rng.standard_normal(n)).astype(npdt)
    else:
        info = np.iinfo(npdt)
        x = rng.integers(info.min, info.max, n, dtype=npdt, endpoint=True)     # Int64 / UInt64: values far beyond 2^53, held to the converted values
        x[:2] = info.min, info.max
    valid = rng.uniform(size=n) >= 0.1
    check_moments(api, split(x, valid, cuts=[700, TILE + 1], offsets=[1, 3, 7]), what=f"dtype {dt}")
    check_moments(api, split(x, cuts=[700], offsets=[13, 0]), what=f"dtype {dt}, no NULLs")


# ---------------------------------------------------------------- pairs
@pytest.mark.parametrize("name", R.ILL + ["lognormal", "two_clusters"])
def test_comoments_of_a_noisy_line(api, name):
    n = 50_001
    x = named(name, n)
    y = 3.0 * x + R.make_input("normal", n, seed=5)
    rng = np.random.default_rng(3)
    vx, vy = rng.uniform(size=n) >= 0.1, rng.uniform(size=n) >= 0.15             # NULLs in different rows of x and y
    cuts, offs = [1, 2049, 30_000], [0, 3, 9, 64]
    check_comoments(api, split(x, cuts=cuts, offsets=offs), split(y, cuts=cuts, offsets=offs[::-1]), what=f"{name} y = 3x + noise")
    check_comoments(api, split(x, vx, cuts=cuts, offsets=offs), split(y, vy, cuts=cuts, offsets=offs[::-1]), what=f"{name} NULLs in both")
    bits, mvalid = rng.uniform(size=n) < 0.5, rng.uniform(size=n) >= 0.1
    check_comoments(api, split(x, vx, cuts=cuts, offsets=offs), split(y, cuts=cuts, offsets=offs),
                    split(bits, mvalid, cuts=cuts, offsets=[7, 1, 0, 13], dtype=A.BOOL), what=f"{name} masked")


@pytest.mark.parametrize("n", [0, 1, 2, 65, WAVE_TILE + 1, TILE + 1])
def test_comoments_small_shapes_and_self_correlation(api, n):
    x = named("offset_1e9", TILE + 1)[:n]
    st, ref = check_comoments(api, split(x, offsets=[3]), split(x, offsets=[64]), what=f"corr(x, x) {n}")
    if n >= 2:
        corr = api.comoments_stat(st, "corr")
        assert abs(corr - 1.0) <= R.gamma(2 * n) + 16 * R.U
        assert st.m2x == st.m2y == st.cxy
    else:
        assert api.comoments_stat(st, "corr") is None


def test_comoments_mixed_dtypes(api):
    rng = np.random.default_rng(8)
    n = TILE + 777
    x = rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32)
    y = 0.5 * x.astype(np.float64) + 1e6 * rng.standard_normal(n)
    valid = rng.uniform(size=n) >= 0.1
    check_comoments(api, split(x, valid, cuts=[600], offsets=[5, 1]), split(y, cuts=[600], offsets=[0, 9]), what="Int32 x Float64")
    check_comoments(api, split(y, cuts=[600], offsets=[0, 9]), split(x, valid, cuts=[600], offsets=[5, 1]), what="Float64 x Int32")
    u8 = rng.integers(0, 255, n, dtype=np.int64).astype(np.uint8)
    i16 = (u8.astype(np.int64) * 100 - rng.integers(0, 1000, n)).astype(np.int16)
    check_comoments(api, split(u8, cuts=[600], offsets=[5, 1]), split(i16, valid, cuts=[600], offsets=[3, 2]), what="UInt8 x Int16")


# ---------------------------------------------------------------- properties
@pytest.mark.parametrize("name", ["offset_1e9", "two_pow_52", "lognormal"])
def test_the_halves_merge_to_the_whole(api, name):
    x = named(name, BIG)
    whole, ref = check_moments(api, split(x, cuts=CUTS, offsets=OFFSETS), what=f"{name} whole")
    a = api.moments(split(x[:77_777], cuts=CUTS, offsets=OFFSETS))
    b = api.moments(split(x[77_777:], cuts=CUTS, offsets=OFFSETS))
    assert a.count + b.count == BIG
    api.moments_merge(a, b)
    assert a.count == whole.count == BIG
    worst = R.error_in_bounds({s: api.moments_stat(a, s) for s in R.STATS}, ref, R.STATS)
    print(f"MOMENTS_ERR {name} merged halves worst={max(worst.values()):.3g} of its bound")
    assert max(worst.values()) <= 1.0, worst
    y = 3.0 * x + R.make_input("normal", BIG, seed=5)
    cw, cref = check_comoments(api, split(x, cuts=CUTS, offsets=OFFSETS), split(y, cuts=CUTS, offsets=OFFSETS), what=f"{name} pair whole")
    ca = api.comoments(split(x[:77_777]), split(y[:77_777]))
    api.moments_merge(ca, api.comoments(split(x[77_777:]), split(y[77_777:])))
    assert ca.count == BIG
    assert max(R.error_in_bounds({s: api.comoments_stat(ca, s) for s in R.COSTATS}, cref, R.COSTATS).values()) <= 1.0


@pytest.mark.parametrize("as_int", [False, True], ids=["f64", "i64"])
def test_a_mask_is_the_filtered_column(api, as_int):
    """rdf_moments with a mask against rdf_moments of rdf_filter's output with the same mask: both inside the bounds of one
    exact reference; the count is rdf_count's answer on the filtered column."""
    x = named("offset_1e15", 60_001, as_int)
    rng = np.random.default_rng(21)
    valid = rng.uniform(size=len(x)) >= 0.1
    bits, mvalid = rng.uniform(size=len(x)) < 0.3, rng.uniform(size=len(x)) >= 0.1
    col = split(x, valid, cuts=[1, 2049, 30_000], offsets=[0, 3, 9, 64])
    mask = split(bits, mvalid, cuts=[1, 2049, 30_000], offsets=[13, 1, 0, 7], dtype=A.BOOL)
    masked, ref = check_moments(api, col, mask, what="masked")
    filtered = api.filter(col, mask)
    st = api.moments(filtered)
    assert st.count == masked.count == api.count(filtered) == ref.n
    assert max(R.error_in_bounds({s: api.moments_stat(st, s) for s in R.STATS}, ref, R.STATS).values()) <= 1.0


# ---------------------------------------------------------------- non-finite values
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", [0, 700, 5000])
def test_a_non_finite_value_makes_every_statistic_nan(api, bad, where):
    x = named("normal", 3 * TILE).copy()
    x[where] = bad
    valid = np.ones(len(x), dtype=bool)
    valid[where + 1] = False
    chunks = split(x, valid, cuts=[900], offsets=[3, 1])
    st = four_ways(lambda c: api.moments(c), [chunks])
    assert st.count == len(x) - 1
    got = {s: api.moments_stat(st, s) for s in R.STATS}
    assert all(v is not None and math.isnan(v) for v in got.values()), got
    co = four_ways(lambda a, b: api.comoments(a, b), [chunks, split(named("uniform", 3 * TILE), cuts=[900], offsets=[0, 5])])
    assert co.count == len(x) - 1
    assert all(math.isnan(api.comoments_stat(co, s)) for s in R.COSTATS)
    # the same value under a NULL slot or outside the mask is not seen
    valid[where], valid[where + 1] = False, True
    st = api.moments(split(x, valid, cuts=[900], offsets=[3, 1]))
    assert st.count == len(x) - 1 and all(math.isfinite(api.moments_stat(st, s)) for s in R.STATS)
    bits = np.ones(len(x), dtype=bool)
    bits[where] = False
    st = api.moments(split(x, cuts=[900], offsets=[3, 1]), split(bits, cuts=[900], offsets=[6, 2], dtype=A.BOOL))
    assert st.count == len(x) - 1 and all(math.isfinite(api.moments_stat(st, s)) for s in R.STATS)
