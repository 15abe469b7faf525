"""The model of rdf_groupby_moments (include/rdf_mi355x.h, "moments per group"): which groups there are and in which order
(group_sorted_ref's rules), and per group the EXACT moments of the counted values in row order with the bounds a result is
held to — moments_ref's MomentsRef / ComomentsRef, B = gamma(2n) + 16u with n the GROUP's count.

Two things beside it:
  - a fast exact path for integer-valued columns with |x| < 2^9 (the multi-level cases of the GPU tests): a group's values
    are counted per distinct value (pairs: per distinct pair) with int64 numpy, and the moments follow from at most 1023
    (1023^2) weighted Python integers as `Fraction`s — the same numbers MomentsRef gets, without a Python integer per row;
  - `restated_states`: the kernel's algorithm in numpy and Python floats — fixed tiles of T sorted positions, one tile step
    (moments_ref.tile_state) per piece, interior pieces final, a tile's first and last piece carried to the next level, the
    levels merged with `merge` / `comerge` in item order.  The CPU tests hold it to the bounds.  With seq=True every sum of a
    piece is taken in item order, which is what the serial emulation in rdf_group_moments_plan.h does: `write_host_table`
    writes cases for the compiled host test (tests/cpp/test_group_moments_host.cpp), which must reproduce them bit for bit.
"""
import math
import struct
from fractions import Fraction

import numpy as np

import moments_ref as M
from group_sorted_ref import group_rows_of

T = 256          # RDF_GROUP_MOMENTS_TILE (the ABI test pins the header and the Python mirror to it)
STATS, COSTATS = M.STATS, M.COSTATS


# ---------------------------------------------------------------- exact moments per group
class SmallIntMomentsRef(M.MomentsRef):
    """MomentsRef of an integer-valued vector with |x| < 2^9, from the counts of its distinct values."""

    def __init__(self, x):
        xi = np.asarray(x).astype(np.int64)
        self.n = n = len(xi)
        if n == 0:
            return
        vals, cnt = np.unique(xi, return_counts=True)
        k, w = [int(v) for v in vals], [int(c) for c in cnt]
        s1, s2, s3, s4 = (sum(c * v ** p for v, c in zip(k, w)) for p in (1, 2, 3, 4))
        self.mean = Fraction(s1, n)
        self.sum_abs = Fraction(sum(c * abs(v) for v, c in zip(k, w)))
        self.m2 = s2 - Fraction(s1 * s1, n)
        self.m3 = s3 - Fraction(3 * s2 * s1, n) + Fraction(2 * s1 ** 3, n * n)
        self.m4 = s4 - Fraction(4 * s3 * s1, n) + Fraction(6 * s2 * s1 * s1, n * n) - Fraction(3 * s1 ** 4, n ** 3)
        self.abs3 = Fraction(sum(c * abs(v * n - s1) ** 3 for v, c in zip(k, w)), n ** 3)


class SmallIntComomentsRef(M.ComomentsRef):
    def __init__(self, x, y):
        xi, yi = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
        self.n = n = len(xi)
        self.x, self.y = SmallIntMomentsRef(xi), SmallIntMomentsRef(yi)
        if n == 0:
            return
        pairs, cnt = np.unique((xi + 512) * 1024 + (yi + 512), return_counts=True)
        px = [int(p) // 1024 - 512 for p in pairs]
        py = [int(p) % 1024 - 512 for p in pairs]
        w = [int(c) for c in cnt]
        sx, sy = sum(c * a for a, c in zip(px, w)), sum(c * b for b, c in zip(py, w))
        self.cxy = sum(c * a * b for a, b, c in zip(px, py, w)) - Fraction(sx * sy, n)
        self.abs_xy = Fraction(sum(c * abs((a * n - sx) * (b * n - sy)) for a, b, c in zip(px, py, w)), n * n)


def small_ints(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.isfinite(x).all() and (np.abs(x) < 512).all() and (x == np.rint(x)).all())


def moments_ref_of(x):
    return SmallIntMomentsRef(x) if len(x) > 64 and small_ints(x) else M.MomentsRef(x)


def comoments_ref_of(x, y):
    return SmallIntComomentsRef(x, y) if len(x) > 64 and small_ints(x) and small_ints(y) else M.ComomentsRef(x, y)


def as_f64(values):
    """A numeric column `as f64`, the conversion rdf_moments makes (integers beyond 2^53 round to nearest even)."""
    return np.asarray(values).astype(np.float64)


def group_moments_ref(keys, x, y=None):
    """keys: [(values, valid | None) | (list of bytes | None,)], x / y: (numpy values, valid | None).
    -> (group_rows uint32, counts int64, [values of the counted rows per group as f64: x | (x, y)], [row lists])."""
    n = len(x[0])
    groups = group_rows_of(keys, n) if n else []
    ok = np.ones(n, dtype=bool) if len(x) < 2 or x[1] is None else np.asarray(x[1], dtype=bool).copy()
    if y is not None and len(y) > 1 and y[1] is not None:
        ok &= np.asarray(y[1], dtype=bool)
    xv = as_f64(x[0])
    yv = as_f64(y[0]) if y is not None else None
    rows_of = [np.array(rows, dtype=np.int64) for _, rows in groups]
    counted = [r[ok[r]] for r in rows_of]
    vals = [xv[r] if y is None else (xv[r], yv[r]) for r in counted]
    return (np.array([r[0] for r in rows_of], dtype=np.uint32).reshape(len(groups)),
            np.array([len(r) for r in counted], dtype=np.int64).reshape(len(groups)), vals, rows_of)


# ---------------------------------------------------------------- the merge and the statistics, restated (rdf_moments_math.h)
def merge(a, b):
    """Chan / Pebay on (count, mean, mean_lo, m2, m3, m4), the roundings of mo_merge."""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    na, nb = float(a[0]), float(b[0])
    inv = 1.0 / (na + nb)
    fa, fb = na * inv, nb * inv
    d = (b[1] - a[1]) + (b[2] - a[2])
    d2, w = d * d, na * fb
    m4 = (a[5] + b[5]) + ((d2 * d2) * (w * ((fa * fa - fa * fb) + fb * fb)) + (6.0 * d2) * (fa * fa * b[3] + fb * fb * a[3]) +
                          (4.0 * d) * (fa * b[4] - fb * a[4]))
    m3 = (a[4] + b[4]) + ((d2 * d) * (w * (fa - fb)) + (3.0 * d) * (fa * b[3] - fb * a[3]))
    m2 = (a[3] + b[3]) + d2 * w
    mean, lo = M.mean_add(a[1], a[2], d * fb)
    return (a[0] + b[0], float(mean), float(lo), m2, m3, m4)


def comerge(a, b):
    """(count, mean_x, mean_x_lo, mean_y, mean_y_lo, m2x, m2y, cxy), the roundings of mo_comerge."""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    na, nb = float(a[0]), float(b[0])
    inv = 1.0 / (na + nb)
    fb = nb * inv
    w = na * fb
    dx = (b[1] - a[1]) + (b[2] - a[2])
    dy = (b[3] - a[3]) + (b[4] - a[4])
    mx, mxl = M.mean_add(a[1], a[2], dx * fb)
    my, myl = M.mean_add(a[3], a[4], dy * fb)
    return (a[0] + b[0], float(mx), float(mxl), float(my), float(myl), (a[5] + b[5]) + (dx * dx) * w, (a[6] + b[6]) + (dy * dy) * w,
            (a[7] + b[7]) + (dx * dy) * w)


def _sqrt(v):
    return math.sqrt(v) if v >= 0 else math.nan


def stats_of(state):
    """name -> float | None off a moments state: mo_stat."""
    n, mean, lo, m2, m3, m4 = state
    out = dict.fromkeys(STATS)
    if n <= 0:
        return out
    nd = float(n)
    with np.errstate(all="ignore"):
        out["mean"] = mean + lo
        out["var_pop"] = m2 / nd
        out["stddev_pop"] = _sqrt(m2 / nd)
        if n >= 2:
            out["var_samp"] = m2 / (nd - 1.0)
            out["stddev_samp"] = _sqrt(m2 / (nd - 1.0))
        if m2 != 0.0:
            out["skewness"] = float(np.float64(_sqrt(nd) * m3) / np.float64(m2 * _sqrt(m2)))
            out["kurtosis"] = float(np.float64(nd * m4) / np.float64(m2 * m2)) - 3.0
    return out


def costats_of(state):
    n, _, _, _, _, m2x, m2y, cxy = state
    out = dict.fromkeys(COSTATS)
    if n <= 0:
        return out
    nd = float(n)
    out["covar_pop"] = cxy / nd
    if n >= 2:
        out["covar_samp"] = cxy / (nd - 1.0)
    if m2x != 0.0 and m2y != 0.0:
        out["corr"] = float(np.float64(cxy) / np.float64(_sqrt(m2x * m2y)))
    return out


# ---------------------------------------------------------------- the algorithm, restated
def levels_of(n, tile=T):
    """The item counts of every level: n, 2 ceil(n / T), ... down to the level that fits one tile."""
    out = [n]
    while out[-1] > tile:
        out.append(2 * ((out[-1] + tile - 1) // tile))
    return out


def _fold_level(items, merge_fn, empty, final, tile, last_level):
    """items: [(seg, state)] with ascending seg.  One level: per tile the states of every segment merged in item order;
    a segment that neither is the tile's first nor its last is final, the first and the last go to the next level (a tile
    of one segment hands on the empty state as its second).  -> the next level's items."""
    nxt = []
    for base in range(0, len(items), tile):
        part = items[base:base + tile]
        segs, states = [], []
        for seg, st in part:
            if segs and segs[-1] == seg:
                states[-1] = merge_fn(states[-1], st)
            else:
                segs.append(seg)
                states.append(st)
        for j, (seg, st) in enumerate(zip(segs, states)):
            if not last_level and j == 0:
                nxt.append((seg, st))
            elif not last_level and j == len(segs) - 1:
                nxt.append((seg, st))
            else:
                final[seg] = st
        if not last_level and len(segs) == 1:
            nxt.append((segs[0], empty))
    return nxt


def tile_state_seq(x):
    """moments_ref.tile_state with every sum taken in item order (numpy's cumsum adds one element after the other)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if n == 0:
        return (0, 0.0, 0.0, 0.0, 0.0, 0.0)
    c = x[0] if (x == x[0]).all() else np.cumsum(x)[-1] / np.float64(n)
    d = x - c
    d2 = d * d
    with np.errstate(all="ignore"):
        s1, s2, s3, s4 = (np.cumsum(v)[-1] for v in (d, d2, d2 * d, d2 * d2))
        nd = np.float64(n)
        e = s1 / nd
        e2 = e * e
        mean, lo = M.mean_add(np.float64(c), np.float64(0.0), e)
        m2 = s2 - nd * e2
        m3 = (s3 - (3.0 * e) * s2) + (2.0 * nd) * (e2 * e)
        m4 = ((s4 - (4.0 * e) * s3) + (6.0 * e2) * s2) - (3.0 * nd) * (e2 * e2)
    return (n, float(mean), float(lo), float(m2), float(m3), float(m4))


def restated_states(seg, ok, x, y=None, tile=T, seq=False):
    """seg[j]: the group of sorted position j (0, 1, 2 ... ascending), ok[j]: the row counts, x[j] (and y[j]): its value as
    f64.  -> {group: state} the way the kernels form it (seq=True: a piece's sums in item order, one column only)."""
    seg, ok = np.asarray(seg), np.asarray(ok, dtype=bool)
    n = len(seg)
    pair = y is not None
    empty = (0,) + (0.0,) * (7 if pair else 5)
    merge_fn = comerge if pair else merge
    final = {}
    sizes = levels_of(n, tile)
    # level 0: a tile step per piece
    items = []
    cut = np.flatnonzero(np.diff(seg)) + 1
    for base in range(0, n, tile):
        end = min(base + tile, n)
        bounds = [base] + [int(c) for c in cut[(cut > base) & (cut < end)]] + [end]
        for a, b in zip(bounds[:-1], bounds[1:]):
            sel = ok[a:b]
            st = M.cotile_state(x[a:b][sel], y[a:b][sel]) if pair else (tile_state_seq if seq else M.tile_state)(x[a:b][sel])
            items.append((int(seg[a]), st))
    # (level 0's pieces are the items of a fold over one tile's worth of pieces each: reuse the emission rule)
    nxt, at = [], 0
    for base in range(0, n, tile):
        end = min(base + tile, n)
        k = int(seg[end - 1]) - int(seg[base]) + 1
        nxt += _fold_level(items[at:at + k], merge_fn, empty, final, k, len(sizes) == 1)
        at += k
    items = nxt
    for lv in range(1, len(sizes)):
        assert len(items) == sizes[lv], (len(items), sizes)
        items = _fold_level(items, merge_fn, empty, final, tile, lv == len(sizes) - 1)
    assert not items
    return final


def errors_in_bounds(got_stats, ref, names):
    """max over `names` of |got - exact| / bound for one group (moments_ref.error_in_bounds), and the worst name."""
    e = M.error_in_bounds(got_stats, ref, names)
    worst = max(e, key=e.get)
    return e[worst], worst


# ---------------------------------------------------------------- the case table of the compiled host test
def _hex(v):
    return "%x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _state_text(st):
    return " ".join([str(int(st[0]))] + [_hex(v) for v in st[1:]])


def write_host_table(path):
    """-> {line kind: rows written}.  L: the level plan; S / Q: every statistic of states of every kind (empty, one row,
    constant, ill-conditioned, NaN); M: merges; F: whole folds — group sizes around the wave and the tile, rows that do not
    count, a constant group, a group without a counted row, boundaries around a tile, three levels."""
    written = dict.fromkeys("LSQMF", 0)
    rng = np.random.default_rng(77)
    with open(path, "w") as f:
        for n in (1, 2, T - 1, T, T + 1, 2 * T, T * T // 2, T * T // 2 + 1, 2 * T * T + 77, 50_000_000, 2**32 - 1):
            lv = levels_of(n)
            f.write("L %d %d %s\n" % (n, len(lv), " ".join(map(str, lv))))
            written["L"] += 1
        states = [(0, 0.0, 0.0, 0.0, 0.0, 0.0), (3, 0.1, 0.0, 0.0, 0.0, 0.0), (2, math.nan, math.nan, math.nan, math.nan, math.nan),
                  (5, 1.0, 0.0, math.inf, 1.0, 1.0)]
        costates = [(0,) + (0.0,) * 7, (1, 1.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0), (4, 0.0, 0.0, 0.0, 0.0, 0.0, 3.0, 0.0), (4, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0),
                    (3, 0.0, 0.0, 0.0, 0.0, math.nan, 1.0, math.nan)]
        for name in M.ILL + M.BENIGN + M.HARD:
            for n in (1, 2, 3, 100):
                x = M.make_input(name, n)
                states.append(M.tile_state(x))
                costates.append(M.cotile_state(x, 3.0 * x + M.make_input("normal", n, seed=1)))
        for st in states:
            got = stats_of(st)
            for k, name in enumerate(STATS):
                f.write("S %s %d %d %s\n" % (_state_text(st), k, got[name] is not None, _hex(got[name] or 0.0)))
                written["S"] += 1
        for st in costates:
            with np.errstate(all="ignore"):
                got = costats_of(st)
            for k, name in enumerate(COSTATS):
                f.write("Q %d %s %s %s %d %d %s\n" % (st[0], _hex(st[5]), _hex(st[6]), _hex(st[7]), k, got[name] is not None, _hex(got[name] or 0.0)))
                written["Q"] += 1
        for a in states[:2] + states[4:]:                            # (not the NaN and infinity states: which of two NaNs an add keeps is the compiler's choice)
            for b in states[:2] + states[4::5]:
                with np.errstate(all="ignore"):
                    f.write("M %s %s %s\n" % (_state_text(a), _state_text(b), _state_text(merge(a, b))))
                written["M"] += 1
        sizes = [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]
        cases = []
        for name in M.ILL + ["normal", "two_clusters"]:
            for order in (sizes, sizes[::-1]):
                seg = np.repeat(np.arange(len(order)), order)
                x = M.make_input(name, len(seg))
                ok = rng.random(len(seg)) >= 0.1
                ok[seg == 1] = name != "normal"                      # one group without a counted row
                x[seg == 4] = 0.1                                    # a constant group
                cases.append((seg, ok, x))
        for start in (T - 1, T, T + 1):
            seg = np.repeat(np.arange(4), [start, 2 * T, 1, 3])
            cases.append((seg, np.ones(len(seg), dtype=bool), M.make_input("offset_1e15", len(seg), seed=start)))
        n = 2 * T * T + 77
        for seg in (np.zeros(n, dtype=np.int64), np.repeat(np.arange(6), [40 * T, 1, 100 * T + 3, 1, 1, n - 140 * T - 6])):
            cases.append((seg, rng.random(n) >= 0.1, rng.integers(-511, 512, n).astype(np.float64)))
        for seg, ok, x in cases:
            states = restated_states(seg, ok, x, seq=True)
            groups = int(seg[-1]) + 1
            f.write("F %d %d\n" % (len(seg), groups))
            f.write("\n".join("%d %d %s" % (s_, o_, _hex(v_)) for s_, o_, v_ in zip(seg.tolist(), ok.tolist(), x.tolist())))
            f.write("\n" + "\n".join(_state_text(states[g]) for g in range(groups)) + "\n")
            written["F"] += 1
    return written
