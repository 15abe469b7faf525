"""The executable definition of rdf_groupby_percentile (include/rdf_mi355x.h, "percentiles and median per group") in plain
Python / numpy.

A column is (values, valid): `values` a numpy array (numeric) or a sequence of bytes objects (Utf8; None = NULL), `valid` a
bool array or None.  The rows go into a dict of key tuple -> row list (group_sorted_ref.group_rows_of: the key of a row is
the tuple of its columns' dense codes, floats canonical, NULL the largest code), so iterating the dict in sorted key order IS
the header's group order.  Inside a group the non-NULL rows are ordered by the value column's code — its rank among the
distinct values, NaN after +inf, -0.0 and +0.0 one value — so "peers" are rows of equal code.  Nothing here is derived from the
library: no sort of (key, value) pairs, no permutation, no scan.

The arithmetic mirrors rdf_percentile.h expression by expression — Python floats are IEEE doubles and every operation below
rounds once — so CONT results are comparable bit for bit:
    pos = float(m - 1) * p;  lo = floor(pos);  hi = ceil(pos);  wlo = hi - pos;  whi = pos - lo
    lo == hi or peers:  d(v_lo)            else:  (wlo * d(v_lo)) + (whi * d(v_hi))
    DISC: k = max(0, ceil(p * float(m)) - 1), answered by the smallest row index among the peers of the k-th value
"""
import math
import struct

import numpy as np

from group_sorted_ref import _valid_of, group_rows_of
from window_ref import key_codes

NAN_BITS = 0x7FF8000000000000
DTYPES = ("i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64", "f32", "f64")
DTYPE_CODE = {name: i for i, name in enumerate(DTYPES)}      # rdf_dtype
NP = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32,
      "u64": np.uint64, "f32": np.float32, "f64": np.float64}


def bits_of(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def p_ok(p: float) -> bool:
    return 0.0 <= p <= 1.0


def rank(m: int, p: float):
    """-> (lo, hi, wlo, whi) for m >= 1 values."""
    pos = float(m - 1) * p
    lo, hi = math.floor(pos), math.ceil(pos)
    wlo, whi = float(hi) - pos, pos - float(lo)
    hi = min(hi, m - 1)
    lo = min(lo, hi)
    return lo, hi, wlo, whi


def disc_index(m: int, p: float) -> int:
    return min(m - 1, max(0, math.ceil(p * float(m)) - 1))


def d_of(v) -> float:
    """d(v) of one numpy scalar or Python number: Float32 widened, integers to nearest even, -0.0 -> +0.0, one NaN."""
    if isinstance(v, (np.floating, float)):
        x = float(v)
        if x != x:
            return from_bits(NAN_BITS)
        return 0.0 if x == 0.0 else x
    return float(int(v))          # Python rounds an int to the nearest double, ties to even


def interpolate(rk, dlo: float, dhi: float, peers: bool) -> int:
    """-> the bits of the result."""
    lo, hi, wlo, whi = rk
    if lo == hi or peers:
        v = dlo
    else:
        a = wlo * dlo
        b = whi * dhi
        v = a + b
    return NAN_BITS if v != v else bits_of(v)


def normalise_calls(calls):
    out = []
    for c in calls:
        if c == "median":
            out.append(("cont", 0.5))
        else:
            out.append((c[0], float(c[1])))
    return out


def percentile_ref(keys, value, calls):
    """calls: [("cont", p) | ("disc", p) | "median"].  -> (group_rows uint32, [(values, valid) per call], counts int64):
    values are uint64 BITS of the Float64 result for "cont" and uint32 row indices for "disc"; 0 under a NULL."""
    calls = normalise_calls(calls)
    cols = list(keys) + ([value] if value is not None else [])
    n = len(cols[0][0]) if cols else 0
    groups = group_rows_of(keys, n) if n else []
    G = len(groups)
    group_rows = np.array([rows[0] for _, rows in groups], dtype=np.uint32).reshape(G)
    counts = np.zeros(G, dtype=np.int64)
    outs = [(np.zeros(G, dtype=np.uint64 if kind == "cont" else np.uint32), np.zeros(G, dtype=bool)) for kind, _ in calls]
    if value is None:
        return group_rows, outs, counts
    numeric = isinstance(value[0], np.ndarray)
    ok = _valid_of(value)
    codes = key_codes(value[0], value[1] if len(value) > 1 else None)
    for g, (_, rows) in enumerate(groups):
        live = sorted((int(codes[i]), i) for i in rows if ok[i])       # by value, then by row: the first of equal codes is the smallest row
        m = counts[g] = len(live)
        if m == 0:
            continue
        for (kind, p), (vals, valid) in zip(calls, outs):
            if not p_ok(p):
                raise ValueError("p outside [0, 1]")
            valid[g] = True
            if kind == "cont":
                if not numeric:
                    raise ValueError("a continuous percentile of a Utf8 column")
                rk = rank(m, p)
                (clo, ilo), (chi, ihi) = live[rk[0]], live[rk[1]]
                vals[g] = interpolate(rk, d_of(value[0][ilo]), d_of(value[0][ihi]), clo == chi)
            elif kind == "disc":
                code = live[disc_index(m, p)][0]
                vals[g] = min(i for c, i in live if c == code)
            else:
                raise ValueError(kind)
    return group_rows, outs, counts


# ---------------------------------------------------------------- the select route's decisions: keys and the planner step
def key_bits(name: str) -> int:
    return np.dtype(NP[name]).itemsize * 8


def key_of(name: str, v) -> int:
    """The ordered unsigned image of a value at its own width: integers counted from the type's minimum; floats by their bits,
    negatives reversed below the positives, -0.0 as +0.0, every NaN the one quiet NaN above +inf."""
    if not name.startswith("f"):
        return int(v) - int(np.iinfo(NP[name]).min)
    w = key_bits(name)
    x = float(v)
    if x != x:
        bits = 0x7FC00000 if w == 32 else NAN_BITS
    else:
        if x == 0.0:
            x = 0.0
        bits = struct.unpack("<I", struct.pack("<f", x))[0] if w == 32 else bits_of(x)
    top = 1 << (w - 1)
    return ((1 << w) - 1 - bits) if bits & top else (bits | top)


def unkey_raw(name: str, key: int) -> int:
    """The raw bits of the value a key stands for (of peers: their canonical member)."""
    if not name.startswith("f"):
        return _raw(name, key + int(np.iinfo(NP[name]).min))
    w = key_bits(name)
    top = 1 << (w - 1)
    return (key - top) if key & top else ((1 << w) - 1 - key)


def order_of(name: str, a, b) -> int:
    """-1 / 0 / 1: a before, a peer of, or after b in the sort's order — by the values, not by their keys."""
    if name.startswith("f"):
        fa, fb = float(a), float(b)
        na, nb = fa != fa, fb != fb
        if na or nb:
            return 0 if na and nb else (1 if na else -1)
        return (fa > fb) - (fa < fb)            # -0.0 == +0.0
    return (int(a) > int(b)) - (int(a) < int(b))


def plan_bucket(hist, residual: int):
    """-> (bucket, residual inside it) of the 0-based rank `residual` among the candidates `hist` counts by digit; a rank
    beyond them ends in the last bucket at rank 0."""
    r = residual
    for b, h in enumerate(hist):
        if r < h:
            return b, r
        r -= h
    return len(hist) - 1, 0


# ---------------------------------------------------------------- the table tests/cpp/test_percentile_host.cpp reads
def _raw(name: str, v) -> int:
    return int(np.array([v], dtype=NP[name]).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(NP[name]).itemsize])[0])


def edge_values(name: str):
    t = NP[name]
    if name.startswith("f"):
        fi = np.finfo(t)
        vals = [0.0, -0.0, 1.0, -1.0, 1.5, fi.max, fi.min, fi.tiny, -fi.tiny, fi.smallest_subnormal, np.inf, -np.inf, np.nan, 0.1, -2.5e-7]
        out = [t(v) for v in vals]
        nan_bits = [0x7FC00001, 0xFFC00000, 0x7F800001] if name == "f32" else [0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001]
        out += [np.array([b], dtype=np.uint32 if name == "f32" else np.uint64).view(t)[0] for b in nan_bits]     # other NaN payloads and signs
        return out
    ii = np.iinfo(t)
    vals = {ii.min, ii.min + 1, -1, 0, 1, 2, ii.max - 1, ii.max}
    if ii.bits == 64:     # beyond 2^53: the conversion rounds, ties to even
        for k in (53, 54, 60, 62):
            for dlt in (-3, -2, -1, 0, 1, 2, 3, 5):
                vals.add((1 << k) + dlt)
                vals.add(-((1 << k) + dlt))
        vals.update({ii.max - 511, ii.max - 512, ii.max - 513, ii.max - 1023, ii.max - 1024, ii.max - 1025})
    return [t(v) for v in sorted(vals) if ii.min <= v <= ii.max]


P_EDGES = (0.0, 1.0, 0.5, 1e-300, float(np.nextafter(1.0, 0.0)), 0.25, 0.75, 0.95, 0.99, 1.0 / 3.0, 0.1, float(np.nextafter(0.5, 0.0)), float(np.nextafter(0.5, 1.0)))
M_EDGES = (1, 2, 3, 4, 5, 7, 8, 100, 101, 255, 256, 257, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1)


def write_host_table(path: str, seed: int = 20250) -> dict:
    """One line per case, every double as its 16 hex digits:
         D <dtype code> <raw hex> <d bits>                         d(v)
         R <m> <p> <lo> <hi> <wlo> <whi>                           the rank rule
         K <m> <p> <k>                                             the DISC index
         I <m> <p> <dlo> <dhi> <peers> <result>                    the interpolation
         P <p> <ok>                                                the p test
         Q <dtype code> <raw hex> <key hex> <unkey raw hex>        the ordered key of a value and the way back
         O <dtype code> <raw a hex> <raw b hex> <-1 | 0 | 1>       the order of two values, which their keys must show
         B <nbuckets> <residual> <bucket> <new residual> <counts>  the planner step on one digit histogram
       -> the number of lines of each letter."""
    rng = np.random.default_rng(seed)
    count = {"D": 0, "R": 0, "K": 0, "I": 0, "P": 0, "Q": 0, "O": 0, "B": 0}
    h = lambda x: f"{bits_of(float(x)):016x}"
    with open(path, "w") as f:
        for name in DTYPES:
            vals = edge_values(name)
            if name.startswith("f"):
                w = np.uint32 if name == "f32" else np.uint64
                vals += list(rng.integers(0, np.iinfo(w).max, size=2000, dtype=w, endpoint=True).view(NP[name]))
            else:
                ii = np.iinfo(NP[name])
                vals += list(rng.integers(ii.min, ii.max, size=2000, dtype=NP[name], endpoint=True))
            for v in vals:
                f.write(f"D {DTYPE_CODE[name]} {_raw(name, v):x} {h(d_of(v))}\n")
                count["D"] += 1
        ms = list(M_EDGES) + [int(x) for x in rng.integers(1, 1 << 32, size=300)] + [int(x) for x in rng.integers(1, 64, size=100)]
        ps = list(P_EDGES) + [float(x) for x in rng.uniform(size=40)] + [k / 8.0 for k in range(9)]
        for m in ms:
            for p in ps:
                lo, hi, wlo, whi = rank(m, p)
                f.write(f"R {m} {h(p)} {lo} {hi} {h(wlo)} {h(whi)}\n")
                f.write(f"K {m} {h(p)} {disc_index(m, p)}\n")
                count["R"] += 1
                count["K"] += 1
        dvals = [d_of(v) for v in edge_values("f64")] + [d_of(v) for v in edge_values("i64")[::7]] + [float(x) for x in rng.normal(size=60) * 1e3]
        for m in (1, 2, 3, 10, 101, (1 << 32) - 1):
            for p in ps[:24]:
                rk = rank(m, p)
                for _ in range(40):
                    dlo, dhi = dvals[int(rng.integers(len(dvals)))], dvals[int(rng.integers(len(dvals)))]
                    peers = bool(rng.integers(2)) and (dlo == dhi or (dlo != dlo and dhi != dhi))
                    f.write(f"I {m} {h(p)} {h(dlo)} {h(dhi)} {int(peers)} {interpolate(rk, dlo, dhi, peers):016x}\n")
                    count["I"] += 1
        for p in list(P_EDGES) + [-0.0, -1e-300, float(np.nextafter(1.0, 2.0)), 2.0, -1.0, math.inf, -math.inf, math.nan]:
            f.write(f"P {h(p)} {int(p_ok(p))}\n")
            count["P"] += 1
        for name in DTYPES:
            vals = edge_values(name)
            if name.startswith("f"):
                w = np.uint32 if name == "f32" else np.uint64
                vals += list(rng.integers(0, np.iinfo(w).max, size=300, dtype=w, endpoint=True).view(NP[name]))
            else:
                ii = np.iinfo(NP[name])
                vals += list(rng.integers(ii.min, ii.max, size=300, dtype=NP[name], endpoint=True))
            for v in vals:                      # the key, and the round trip through it
                k = key_of(name, v)
                assert 0 <= k < (1 << key_bits(name)) and key_of(name, np.array([unkey_raw(name, k)], dtype=f"u{key_bits(name) // 8}").view(NP[name])[0]) == k
                f.write(f"Q {DTYPE_CODE[name]} {_raw(name, v):x} {k:x} {unkey_raw(name, k):x}\n")
                count["Q"] += 1
            edges = edge_values(name)
            pairs = [(a, b) for a in edges for b in edges] + [(vals[int(i)], vals[int(j)]) for i, j in rng.integers(0, len(vals), size=(400, 2))]
            for a, b in pairs:                  # key order is value order; -0.0 / +0.0 and the NaNs collapse
                f.write(f"O {DTYPE_CODE[name]} {_raw(name, a):x} {_raw(name, b):x} {order_of(name, a, b)}\n")
                count["O"] += 1
        nb = 256
        hists = []
        for at in (0, 1, 100, nb - 1):          # all mass in one bucket
            h = [0] * nb
            h[at] = 50_000_000
            hists.append((h, [0, 1, 24_999_999, 25_000_000, 49_999_999]))
        h = [0] * nb                             # ranks that straddle a bucket edge
        h[3], h[4], h[200] = 10, 7, 5
        hists.append((h, [0, 9, 10, 11, 16, 17, 21]))
        h = [0] * nb                             # 16 ranks in 16 buckets, empty buckets in between
        for i in range(16):
            h[i * 16 + 5] = 1000 + i
        starts = [sum(h[:i * 16 + 5]) for i in range(16)]
        hists.append((h, [st + (i * 61) % (1000 + i) for i, st in enumerate(starts)]))
        hists.append(([(1 << 32) - 1] * nb, [0, (1 << 32) - 2, (1 << 32) - 1, 255 * ((1 << 32) - 1), 256 * ((1 << 32) - 1) - 1]))   # counters at their limit
        for _ in range(40):
            h = [int(x) for x in rng.integers(0, 1000, nb) * (rng.random(nb) < 0.3)]
            tot = sum(h)
            hists.append((h, [int(x) for x in rng.integers(0, max(tot, 1), 16)] if tot else []))
        for h, ranks in hists:
            tot = sum(h)
            for r in list(ranks) + [tot, tot + 1, tot + (1 << 40)]:      # ... and the ranks beyond the candidates: the clamp
                b, nr = plan_bucket(h, r)
                if r < tot:
                    assert h[b] > nr and sum(h[:b]) + nr == r
                f.write(f"B {nb} {r} {b} {nr} {' '.join(str(x) for x in h)}\n")
                count["B"] += 1
    return count
