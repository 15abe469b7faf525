"""Inputs of tests/test_sort_routes_gpu.py: columns built so that the planner of rdf_sort_to_indices (os_column_passes,
csrc/rdf_sort_plan.h, csrc/rdf_sort_map.h) takes a known route.  Plain numpy, no library.

Integer keys are (bucket << R) | low with the rows of every bucket counted out exactly; Float64 columns plant their specials
on or off the rows the planner's sample reads, so the plan does not depend on the draw."""
import numpy as np

LADDER = [0, 1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096]
NBUCKETS = 4096


# ---------------------------------------------------------------- integer keys

def bucket_sizes(rng, ladder, n=None, filler=12):
    """rows per bucket: the ladder's sizes on scattered buckets (never the two end buckets), `filler` rows in every other
    one, then single rows added to / taken from filler buckets until the sum is n."""
    sizes = np.full(NBUCKETS, filler, dtype=np.int64)
    at = 1 + rng.permutation(NBUCKETS - 2)[:len(ladder)]
    sizes[at] = ladder
    free = np.setdiff1d(np.arange(NBUCKETS), at)
    if n is not None:
        d = n - int(sizes.sum())
        assert abs(d) <= (filler - 2) * len(free), "no room to reach n"
        step = 1 if d > 0 else -1
        for _ in range(abs(d) // len(free)):
            sizes[free] += step
        sizes[free[:abs(d) % len(free)]] += step
        assert int(sizes.sum()) == n
    return sizes


def bucket_keys(rng, sizes, R):
    """uint64 keys, shuffled: bucket b holds exactly sizes[b] rows; `low` takes a handful of values (ties in every bucket);
    bucket 0 holds low = 0 and the last bucket low = 2^R - 1, so max - min has exactly R + 12 bits in both directions and
    (key - min) >> R, as well as (max - key) >> R, is the bucket."""
    assert sizes[0] >= 1 and sizes[-1] >= 1 and len(sizes) == NBUCKETS and 1 <= R <= 52
    top = (1 << R) - 1
    lows = np.array(sorted({0, 1, top, top - 1, 1 << (R - 1), (1 << (R - 1)) - 1, int(rng.integers(0, top + 1))}), dtype=np.uint64)
    b = np.repeat(np.arange(NBUCKETS, dtype=np.uint64), sizes)
    low = lows[rng.integers(0, len(lows), len(b))]
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    low[first[0]] = 0
    low[first[-1]] = top
    keys = (b << np.uint64(R)) | low
    return keys[rng.permutation(len(keys))]


def as_dtype(keys, npdt, sig):
    """the uint64 keys (below 2^sig) as values of `npdt`: signed types straddle zero (at 64 / 32 bits: the whole range),
    unsigned ones sit at the top of their range, above the signed maximum."""
    npdt = np.dtype(npdt)
    bits = 8 * npdt.itemsize
    assert sig <= bits
    if npdt.kind == "i":
        shifted = keys - np.uint64(1 << (sig - 1))                  # wraps below zero
        return shifted.view(np.int64).astype(npdt)
    lift = np.uint64((1 << bits) - (1 << sig)) if sig < bits else np.uint64(0)
    return (keys + lift).astype(npdt)


def with_nulls(rng, values, fraction):
    """-> (values, valid) with `fraction` EXTRA rows that are NULL (arbitrary values under them), shuffled in: the rows that
    are not NULL are exactly `values`, so counted-out buckets stay counted out."""
    if not fraction:
        return values, None
    k = max(1, int(len(values) * fraction))
    junk = values[rng.integers(0, len(values), k)]
    allv = np.concatenate([values, junk])
    valid = np.concatenate([np.ones(len(values), bool), np.zeros(k, bool)])
    p = rng.permutation(len(allv))
    return allv[p], valid[p]


# ---------------------------------------------------------------- Float64: what the sample sees

def sampled_rows(n, nsamp=8192):
    """the rows os_sample_kernel reads of a column in its original order: row i * stride + (h_i mod stride), stride = n // nsamp,
    h_i = i * 0x9E3779B97F4A7C15 mod 2^64, h_i ^= h_i >> 29."""
    assert n >= nsamp
    stride = np.uint64(n // nsamp)
    i = np.arange(nsamp, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = i * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    pos = i * stride + h % stride
    return np.minimum(pos, np.uint64(n - 1)).astype(np.int64)


def plant(rng, values, specials, count, on_sample):
    """writes `count` specials (cycled) on rows the sample reads (on_sample) or on rows it does not; -> the rows."""
    n = len(values)
    s = sampled_rows(n)
    pool = np.unique(s) if on_sample else np.setdiff1d(np.arange(n), s)
    at = rng.choice(pool, size=count, replace=False)
    values[at] = np.resize(np.asarray(specials, dtype=np.float64), count)
    return at


NEG_NAN = np.array([0xFFF8000000000000], dtype=np.uint64).view(np.float64)[0]
ORDER_SPECIALS = [np.inf, -np.inf, np.nan, NEG_NAN, 1e300, -1e300, 0.0, -0.0, 5e-324, -5e-324]


def null_mask_off_sample(rng, n, fraction):
    """valid mask with `fraction` NULL rows, none of them a sampled row: the sample's view of the column stays as built."""
    valid = np.ones(n, bool)
    pool = np.setdiff1d(np.arange(n), sampled_rows(n))
    valid[rng.choice(pool, size=int(n * fraction), replace=False)] = False
    return valid


def f64_case(name, seed=0):
    """-> (values, n): the Float64 columns of the issue, by name."""
    rng = np.random.default_rng(9000 + seed)
    if name == "uniform":
        return rng.uniform(size=70_001)
    if name == "normal":
        return rng.normal(size=70_001) * 1e3 + 7.0
    if name == "lognormal":
        return rng.lognormal(size=70_001)
    if name in ("outliers_unseen", "outliers_seen"):
        v = rng.normal(size=70_001) * 3.0 + 100.0
        plant(rng, v, ORDER_SPECIALS, 40, on_sample=False)
        if name == "outliers_seen":
            plant(rng, v, [1e300, -1e300], 2, on_sample=True)
        return v
    if name == "spike":
        v = rng.uniform(size=70_001)
        v[rng.uniform(size=len(v)) < 0.10] = 0.25
        return v
    if name == "exp6":
        # whether the plan is refused hangs on the largest value the sample meets (a draw's own maximum, ~12^6, leaves the
        # concentration estimate within 10 % of the limit either way): 1e9 on a sampled row (31.6^6, a value of the
        # distribution) stretches the sample's range so that every level of the zoom finds all of it in one sub-bin
        v = rng.exponential(size=200_000) ** 6
        plant(rng, v, [1e9], 1, on_sample=True)
        return v
    if name == "nonfinite_6pct":
        v = rng.uniform(size=200_000)
        at = rng.uniform(size=len(v)) < 0.06
        v[at] = np.resize(np.array([np.inf, -np.inf, np.nan, NEG_NAN]), int(at.sum()))
        return v
    if name == "nonfinite_unseen":
        v = rng.uniform(size=70_001)
        plant(rng, v, [np.inf, -np.inf, np.nan, NEG_NAN], int(0.015 * len(v)), on_sample=False)
        return v
    raise KeyError(name)
