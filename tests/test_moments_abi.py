"""rdf_moments / rdf_comoments at the C-ABI boundary, without a GPU: the six symbols are exported, the struct and enum
mirrors match the header, every refusal the header lists is a value returned before any device work, zero chunks is the
zero state, and with no device a valid call fails loudly with RDF_DEVICE_ERROR.  The merge and stat functions never touch
the device and are tested in full here: states built by tests/moments_ref.py's restatement of the kernel's tile step are
merged by the library — left fold and tree fold — and held to the exact reference's bounds."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import moments_ref as R
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = A.RDF_INVALID_ARGUMENT
NAMES = ["rdf_moments", "rdf_comoments", "rdf_moments_merge", "rdf_comoments_merge", "rdf_moments_stat", "rdf_comoments_stat"]
TILE = 256


@pytest.fixture(scope="module")
def so():
    s = lib.load()
    for n in NAMES:
        getattr(s, n).restype = C.c_int
    return s


@pytest.fixture(scope="module")
def api():
    return lib.api()


def test_the_symbols_are_exported():
    s = lib.load()
    for n in NAMES:
        assert hasattr(s, n) and n in lib.EXPORTS


def test_the_struct_and_enum_mirrors_match_the_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "rdf_mi355x.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
  S(rdf_moments_state); O(rdf_moments_state, count); O(rdf_moments_state, mean); O(rdf_moments_state, mean_lo); O(rdf_moments_state, m2);
  O(rdf_moments_state, m3); O(rdf_moments_state, m4);
  S(rdf_comoments_state); O(rdf_comoments_state, count); O(rdf_comoments_state, mean_x); O(rdf_comoments_state, mean_x_lo);
  O(rdf_comoments_state, mean_y); O(rdf_comoments_state, mean_y_lo); O(rdf_comoments_state, m2x); O(rdf_comoments_state, m2y); O(rdf_comoments_state, cxy);
  printf("enum %d %d %d %d %d %d %d %d %d %d\n", RDF_STAT_MEAN, RDF_STAT_VAR_POP, RDF_STAT_VAR_SAMP, RDF_STAT_STDDEV_POP, RDF_STAT_STDDEV_SAMP,
         RDF_STAT_SKEWNESS, RDF_STAT_KURTOSIS, RDF_COSTAT_COVAR_POP, RDF_COSTAT_COVAR_SAMP, RDF_COSTAT_CORR);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        lines = subprocess.check_output([exe], text=True).splitlines()
    out = dict(line.rsplit(" ", 1) for line in lines if not line.startswith("enum"))
    for cls in (A.rdf_moments_state, A.rdf_comoments_state):
        assert int(out[cls.__name__]) == C.sizeof(cls), cls.__name__
        fields = [k for k in out if k.startswith(cls.__name__ + ".")]
        assert len(fields) == len(cls._fields_)
        for key in fields:
            assert getattr(cls, key.split(".")[1]).offset == int(out[key]), key
    assert C.sizeof(A.rdf_moments_state) == 48 and C.sizeof(A.rdf_comoments_state) == 64
    assert lines[-1] == "enum " + " ".join(str(A.STATS[s]) for s in R.STATS) + " " + " ".join(str(A.COSTATS[s]) for s in R.COSTATS)


def arr(*cols):
    return [(A.rdf_array * len(c))(*[x.c_struct() for x in c]) for c in cols]


def test_argument_errors_come_back_before_the_device(so):
    x = [A.HostArray.from_numpy(np.arange(5.0)), A.HostArray.from_numpy(np.arange(3.0))]
    y = [A.HostArray.from_numpy(np.arange(5, dtype=np.int32)), A.HostArray.from_numpy(np.arange(3, dtype=np.int32))]
    m = [A.HostArray.from_numpy(np.ones(5, dtype=bool)), A.HostArray.from_numpy(np.ones(3, dtype=bool))]
    cx, cy, cm = arr(x, y, m)
    st, co = A.rdf_moments_state(), A.rdf_comoments_state()
    n = C.c_int64(2)
    st.count = 77

    def says(text):
        assert text in so.rdf_last_error().decode(), so.rdf_last_error()

    # a NULL out, a missing chunk list, a negative chunk count
    assert so.rdf_moments(cx, None, n, None) == BAD
    assert so.rdf_comoments(cx, cy, None, n, None) == BAD
    assert so.rdf_moments(None, None, n, C.byref(st)) == BAD
    assert so.rdf_comoments(cx, None, None, n, C.byref(co)) == BAD
    assert so.rdf_moments(cx, None, C.c_int64(-1), C.byref(st)) == BAD
    # a non-numeric dtype (the value column may not be Boolean), chunks of two dtypes
    assert so.rdf_moments(cm, None, n, C.byref(st)) == BAD
    says("numeric")
    assert so.rdf_comoments(cx, cm, None, n, C.byref(co)) == BAD
    mixed, = arr([x[0], y[1]])
    assert so.rdf_moments(mixed, None, n, C.byref(st)) == BAD
    # a mask that is not RDF_BOOL
    assert so.rdf_moments(cx, cy, n, C.byref(st)) == BAD
    says("Boolean")
    assert so.rdf_comoments(cx, cy, cx, n, C.byref(co)) == BAD
    # chunk lengths that differ: y against x, the mask against x
    swapped, mswapped = arr([y[1], y[0]], [m[1], m[0]])
    assert so.rdf_comoments(cx, swapped, None, n, C.byref(co)) == BAD
    says("lengths differ")
    assert so.rdf_moments(cx, mswapped, n, C.byref(st)) == BAD
    says("lengths differ")
    assert so.rdf_comoments(cx, cy, mswapped, n, C.byref(co)) == BAD
    # two memory spaces in one call
    dev, = arr(m)
    dev[0].mem = dev[1].mem = A.MEM_DEVICE
    assert so.rdf_moments(cx, dev, n, C.byref(st)) == BAD
    assert st.count == 77                                    # nothing was written by any refused call
    # unknown statistics, NULL pointers of the host-only calls
    out, some = C.c_double(0), C.c_int32(0)
    for bad in (-1, 7, 100):
        assert so.rdf_moments_stat(C.byref(st), C.c_int32(bad), C.byref(out), C.byref(some)) == BAD
    for bad in (-1, 3, 100):
        assert so.rdf_comoments_stat(C.byref(co), C.c_int32(bad), C.byref(out), C.byref(some)) == BAD
    assert so.rdf_moments_stat(None, C.c_int32(0), C.byref(out), C.byref(some)) == BAD
    assert so.rdf_moments_stat(C.byref(st), C.c_int32(0), None, C.byref(some)) == BAD
    assert so.rdf_comoments_stat(C.byref(co), C.c_int32(0), C.byref(out), None) == BAD
    assert so.rdf_moments_merge(None, C.byref(st)) == BAD and so.rdf_moments_merge(C.byref(st), None) == BAD
    assert so.rdf_comoments_merge(None, C.byref(co)) == BAD and so.rdf_comoments_merge(C.byref(co), None) == BAD


def test_zero_chunks_and_zero_rows_are_the_zero_state(so, api):
    st = A.rdf_moments_state(5, 1.0, 2.0, 3.0, 4.0, 5.0)
    assert so.rdf_moments(None, None, C.c_int64(0), C.byref(st)) == A.RDF_OK
    assert bytes(st) == bytes(48)
    co = A.rdf_comoments_state(5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0)
    assert so.rdf_comoments(None, None, None, C.c_int64(0), C.byref(co)) == A.RDF_OK
    assert bytes(co) == bytes(64)
    empty = [A.HostArray.from_numpy(np.zeros(0)), A.HostArray.from_numpy(np.zeros(0))]
    assert bytes(api.moments(empty)) == bytes(48)
    assert bytes(api.comoments(empty, empty)) == bytes(64)
    assert all(api.moments_stat(api.moments(empty), s) is None for s in R.STATS)


@pytest.mark.skipif(lib.device_count() > 0, reason="a GPU is visible")
def test_no_gpu_means_device_error_for_valid_calls(api):
    x = [A.HostArray.from_numpy(np.array([1.0, 2.0, 4.0]), valid=[1, 0, 1])]
    y = [A.HostArray.from_numpy(np.array([3, 2, 1], dtype=np.int32))]
    m = [A.HostArray.from_numpy(np.array([1, 1, 0], dtype=bool), valid=[1, 1, 1])]
    for call in (lambda: api.moments(x), lambda: api.moments(y, m), lambda: api.comoments(x, y), lambda: api.comoments(x, y, m)):
        with pytest.raises(A.RdfError) as ei:
            call()
        assert ei.value.status == A.RDF_DEVICE_ERROR
        assert "no CPU fallback" in ei.value.message


# ---------------------------------------------------------------- merge and stat: fully functional without a device
def tile_states(x):
    return [A.rdf_moments_state(*R.tile_state(x[i:i + TILE])) for i in range(0, len(x), TILE)]


def cotile_states(x, y):
    return [A.rdf_comoments_state(*R.cotile_state(x[i:i + TILE], y[i:i + TILE])) for i in range(0, len(x), TILE)]


def left_fold(api, states, zero):
    acc = zero()
    for s in states:
        api.moments_merge(acc, s)
    return acc


def tree_fold(api, states, zero):
    level = [type(s).from_buffer_copy(s) for s in states] or [zero()]
    while len(level) > 1:
        nxt = [api.moments_merge(level[i], level[i + 1]) if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
        level = nxt
    return level[0]


def stats_of(api, st):
    return {s: api.moments_stat(st, s) for s in R.STATS}


def costats_of(api, st):
    return {s: api.comoments_stat(st, s) for s in R.COSTATS}


@pytest.mark.parametrize("fold", [left_fold, tree_fold])
@pytest.mark.parametrize("name", R.ILL + R.BENIGN + R.HARD)
def test_merged_tile_states_meet_the_bounds(api, name, fold):
    x = R.make_input(name, 20000)
    ref = R.MomentsRef(x)
    st = fold(api, tile_states(x), A.rdf_moments_state)
    assert st.count == len(x)
    worst = R.error_in_bounds(stats_of(api, st), ref, R.STATS)
    print(name, fold.__name__, {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("fold", [left_fold, tree_fold])
@pytest.mark.parametrize("name", R.ILL + R.BENIGN + R.HARD)
def test_merged_pair_states_meet_the_bounds(api, name, fold):
    x = R.make_input(name, 20000)
    y = 3.0 * x + R.make_input("normal", 20000, seed=3) * (1.0 if name not in ("two_clusters", "outlier_first") else 1e3)
    ref = R.ComomentsRef(x, y)
    st = fold(api, cotile_states(x, y), A.rdf_comoments_state)
    assert st.count == len(x)
    worst = R.error_in_bounds(costats_of(api, st), ref, R.COSTATS)
    # the per-column sums of the pair state are the single-column ones
    worst["m2x"] = abs(float(R.Fraction(st.m2x) - ref.x.m2)) / (ref.x.bound("var_pop") * len(x))
    worst["m2y"] = abs(float(R.Fraction(st.m2y) - ref.y.m2)) / (ref.y.bound("var_pop") * len(x))
    print(name, fold.__name__, {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def test_a_split_column_merges_to_the_whole(api):
    """Shards: the states of the two halves of a column, each folded from its tiles, merge to a state within the bounds of the
    whole column; the count is exact."""
    for name in R.ILL + ["lognormal", "two_clusters"]:
        x = R.make_input(name, 12345)
        a = left_fold(api, tile_states(x[:7000]), A.rdf_moments_state)
        b = tree_fold(api, tile_states(x[7000:]), A.rdf_moments_state)
        assert (a.count, b.count) == (7000, 5345)
        api.moments_merge(a, b)
        assert a.count == 12345
        worst = R.error_in_bounds(stats_of(api, a), R.MomentsRef(x), R.STATS)
        assert max(worst.values()) <= 1.0, (name, worst)


def test_merging_with_the_zero_state_is_the_identity(api):
    x = R.make_input("offset_1e9", 700)
    st = left_fold(api, tile_states(x), A.rdf_moments_state)
    before = bytes(st)
    api.moments_merge(st, A.rdf_moments_state())
    assert bytes(st) == before
    z = A.rdf_moments_state()
    api.moments_merge(z, st)
    assert bytes(z) == before
    y = R.make_input("uniform", 700)
    co = left_fold(api, cotile_states(x, y), A.rdf_comoments_state)
    before = bytes(co)
    api.moments_merge(co, A.rdf_comoments_state())
    assert bytes(co) == before
    z = A.rdf_comoments_state()
    api.moments_merge(z, co)
    assert bytes(z) == before
    z = A.rdf_moments_state()
    api.moments_merge(z, A.rdf_moments_state())
    assert bytes(z) == bytes(48)


def test_a_constant_column_has_variance_zero_exactly(api):
    x = R.make_input("constant", 5000)
    st = left_fold(api, tile_states(x), A.rdf_moments_state)
    assert (st.count, st.mean, st.mean_lo, st.m2, st.m3, st.m4) == (5000, 0.1, 0.0, 0.0, 0.0, 0.0)
    got = stats_of(api, st)
    assert got["var_pop"] == 0.0 and got["var_samp"] == 0.0 and got["stddev_samp"] == 0.0
    assert got["skewness"] is None and got["kurtosis"] is None and got["mean"] == 0.1


def test_every_rule_for_an_absent_statistic(api):
    zero = A.rdf_moments_state()
    assert all(api.moments_stat(zero, s) is None for s in R.STATS)
    one = A.rdf_moments_state(*R.tile_state([2.5]))
    assert api.moments_stat(one, "mean") == 2.5 and api.moments_stat(one, "var_pop") == 0.0 and api.moments_stat(one, "stddev_pop") == 0.0
    assert all(api.moments_stat(one, s) is None for s in ("var_samp", "stddev_samp", "skewness", "kurtosis"))
    two = A.rdf_moments_state(*R.tile_state([1.0, 3.0]))
    assert api.moments_stat(two, "var_samp") == 2.0 and api.moments_stat(two, "var_pop") == 1.0
    assert api.moments_stat(two, "skewness") == 0.0 and api.moments_stat(two, "kurtosis") == -2.0
    same = A.rdf_moments_state(*R.tile_state([4.0, 4.0, 4.0]))
    assert api.moments_stat(same, "var_samp") == 0.0 and api.moments_stat(same, "skewness") is None and api.moments_stat(same, "kurtosis") is None
    czero = A.rdf_comoments_state()
    assert all(api.comoments_stat(czero, s) is None for s in R.COSTATS)
    cone = A.rdf_comoments_state(*R.cotile_state([1.0], [2.0]))
    assert api.comoments_stat(cone, "covar_pop") == 0.0 and api.comoments_stat(cone, "covar_samp") is None and api.comoments_stat(cone, "corr") is None
    flat_x = A.rdf_comoments_state(*R.cotile_state([1.0, 1.0, 1.0], [1.0, 2.0, 4.0]))
    flat_y = A.rdf_comoments_state(*R.cotile_state([1.0, 2.0, 4.0], [5.0, 5.0, 5.0]))
    for st in (flat_x, flat_y):
        assert api.comoments_stat(st, "corr") is None and api.comoments_stat(st, "covar_pop") == 0.0 and api.comoments_stat(st, "covar_samp") == 0.0
    line = A.rdf_comoments_state(*R.cotile_state([1.0, 2.0, 3.0], [2.0, 4.0, 6.0]))
    assert api.comoments_stat(line, "corr") == 1.0 and api.comoments_stat(line, "covar_samp") == 2.0


def test_a_non_finite_state_gives_nan_statistics(api):
    """What the kernel leaves behind when a valid value is NaN or infinite: NaN sums and the right count; every statistic is
    NaN and present, and merging keeps it so."""
    with np.errstate(invalid="ignore"):
        bad = A.rdf_moments_state(*R.tile_state([1.0, np.inf, 2.0]))
        nan = A.rdf_moments_state(*R.tile_state([1.0, np.nan, 2.0]))
    good = A.rdf_moments_state(*R.tile_state([1.0, 5.0, 2.0]))
    for st in (bad, nan):
        assert st.count == 3
        assert all(math.isnan(api.moments_stat(st, s)) for s in R.STATS)
        acc = A.rdf_moments_state.from_buffer_copy(good)
        api.moments_merge(acc, st)
        assert acc.count == 6 and all(math.isnan(api.moments_stat(acc, s)) for s in R.STATS)
