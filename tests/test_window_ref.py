"""tests/window_ref.py — the CPU restatement the GPU tests hold rdf_window to — checked on its own: the worked example of the
header, pandas on randomised inputs (without NULL / NaN order keys: pandas ranks those as NA, a different convention), and
the committed fixture tests/golden/window_v1.npz against what its generator makes today."""
import importlib.util
import os

import numpy as np
import pytest

import window_ref
from window_ref import window_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "window_v1.npz")


def golden_module():
    spec = importlib.util.spec_from_file_location("make_window_golden", os.path.join(ROOT, "tests", "golden", "make_window_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def same(got, exp):
    if isinstance(exp, tuple):
        return np.array_equal(got[1], exp[1]) and np.array_equal(got[0][exp[1]], np.asarray(exp[0])[exp[1]])
    if np.asarray(exp).dtype == np.float64:
        return np.array_equal(np.asarray(got).view(np.uint64), np.asarray(exp).view(np.uint64))
    return np.array_equal(got, exp)


def test_the_worked_example():
    p = np.array([1, 1, 1, 2, 2, 1], dtype=np.int64)
    o = np.array([10, 20, 10, 5, 0, 20], dtype=np.int64)
    ov = np.array([1, 1, 1, 1, 0, 1], dtype=bool)
    rn, rk, dr, pr, cd, nt, lag, lead = ref([(p, None)], [(o, ov, False)],
                                            ["row_number", "rank", "dense_rank", "percent_rank", "cume_dist", ("ntile", 3), ("lag", 1), ("lead", 1)])
    assert rn.tolist() == [1, 3, 2, 1, 2, 4]
    assert rk.tolist() == [1, 3, 1, 1, 2, 3]
    assert dr.tolist() == [1, 2, 1, 1, 2, 2]
    assert pr.tolist() == [0.0, 2 / 3, 0.0, 0.0, 1.0, 2 / 3]
    assert cd.tolist() == [0.5, 1.0, 0.5, 0.5, 1.0, 1.0]
    assert nt.tolist() == [1, 2, 1, 1, 2, 3]
    assert window_ref.gather(list(range(6)), *lag) == [None, 2, 0, None, 3, 1]
    assert window_ref.gather(list(range(6)), *lead) == [2, 5, 1, 4, None, None]


def test_float_keys_are_canonical_and_nulls_are_peers():
    x = np.array([0.0, -0.0, np.nan, np.inf, -np.nan, 1.0, 0.0], dtype=np.float64)
    x[4] = np.array([0xFFF8000000000123], dtype=np.uint64).view(np.float64)[0]
    rn, rk = ref([], [(x, None, False)], ["row_number", "rank"])
    assert rn.tolist() == [1, 2, 6, 5, 7, 4, 3]                  # zeros in row order, NaNs after +inf in row order
    assert rk.tolist() == [1, 1, 6, 5, 6, 4, 1]
    rn, rk = ref([], [(x, None, True)], ["row_number", "rank"])
    assert rn.tolist() == [5, 6, 1, 3, 2, 4, 7]
    valid = np.array([1, 0, 1, 0, 1, 1, 0], dtype=bool)
    rn, rk, dr = ref([], [(np.arange(7) % 2, valid, True)], ["row_number", "rank", "dense_rank"])
    assert rn.tolist() == [2, 5, 3, 6, 4, 1, 7] and rk.tolist() == [2, 5, 2, 5, 2, 1, 5] and dr.tolist() == [2, 3, 2, 3, 2, 1, 3]
    one = ref([(x, None)], [], ["dense_rank", "cume_dist"])       # no order keys: every row of a partition is a peer
    assert one[0].tolist() == [1] * 7 and one[1].tolist() == [1.0] * 7
    assert window_ref.total_order_argsort(x).tolist() == [4, 1, 0, 6, 5, 3, 2]


def test_ntile_formula_and_offsets():
    for n in (1, 2, 7, 10, 64):
        for b in (1, 2, 3, n, n + 1, 1000):
            t = ref([], [], [("ntile", b)], nrows=n)[0]
            sizes = np.bincount(t)[1:]
            q, r = divmod(n, b)
            assert sizes.tolist() == ([q + 1] * r + [q] * (b - r) if b <= n else [1] * n), (n, b)
            assert (np.diff(t) >= 0).all()
    idx, ok = ref([], [], [("lag", 0)], nrows=5)[0]
    assert idx.tolist() == [0, 1, 2, 3, 4] and ok.all()
    idx, ok = ref([], [], [("lead", 7)], nrows=5)[0]
    assert not ok.any()
    assert [a.shape for a in ref([], [], ["rank", "cume_dist"], nrows=0)] == [(0,), (0,)]


def test_text_keys_compare_as_unsigned_bytes():
    rows = [b"b", b"a\0", None, b"a", b"", b"\xff", b"a", None]
    rn, rk = ref([], [(rows, None, False)], ["row_number", "rank"])
    assert rn.tolist() == [5, 4, 7, 2, 1, 6, 3, 8] and rk.tolist() == [5, 4, 7, 2, 1, 6, 2, 7]


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_against_pandas(seed):
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(seed)
    n = int(rng.integers(200, 3000))
    p1 = rng.integers(0, 6, n)
    p2 = rng.integers(0, 3, n)
    o1 = np.round(rng.normal(size=n) * 2, 0) + 0.0
    o2 = rng.integers(0, 4, n)
    desc = bool(seed % 2)
    df = pd.DataFrame({"p1": p1, "p2": p2, "o1": o1, "o2": o2, "row": np.arange(n)})
    off = int(rng.integers(1, 4))
    rn, rk, dr, pr, cd, lag, lead = ref([(p1, None), (p2, None)], [(o1, None, desc), (o2, None, False)],
                                        ["row_number", "rank", "dense_rank", "percent_rank", "cume_dist", ("lag", off), ("lead", off)])
    # pandas ranks one column: fold (o1, o2) into one code that orders the same way
    code = np.where(desc, -o1, o1) * 10 + o2
    df["code"] = code
    g = df.groupby(["p1", "p2"])["code"]
    assert np.array_equal(rn, g.rank(method="first").to_numpy().astype(np.int64))
    assert np.array_equal(rk, g.rank(method="min").to_numpy().astype(np.int64))
    assert np.array_equal(dr, g.rank(method="dense").to_numpy().astype(np.int64))
    size = g.transform("size").to_numpy()
    assert np.array_equal(cd, g.rank(method="max").to_numpy() / size)
    exp_pr = np.where(size == 1, 0.0, (g.rank(method="min").to_numpy() - 1) / np.maximum(size - 1, 1))
    assert np.array_equal(pr, exp_pr)
    s = df.sort_values(["p1", "p2", "code"], kind="stable")
    for (idx, ok), shift in ((lag, off), (lead, -off)):
        exp = s.groupby(["p1", "p2"])["row"].shift(shift).reindex(df.index).to_numpy()
        assert np.array_equal(ok, ~np.isnan(exp))
        assert np.array_equal(idx[ok].astype(np.int64), exp[ok].astype(np.int64))


def test_the_committed_fixture_is_what_the_generator_makes():
    m = golden_module()
    fresh = m.to_arrays(m.build_cases())
    z = np.load(GOLDEN)
    assert sorted(z.files) == sorted(fresh.keys())
    for k in z.files:
        a, b = z[k], np.asarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "mixed_batches.arrow"))


def test_the_fixture_loads_back_into_the_reference():
    m = golden_module()
    for name, case in m.load(GOLDEN).items():
        got = m.expected(case)
        for c, (g, e) in enumerate(zip(got, case["expected"])):
            assert same(g, e), (name, case["calls"][c])
