"""Exact references for the float accuracy tests: transcendentals, ulp distances and exact sums.

An exact value is carried as a double-double (hi, lo): hi = the value rounded to f64, lo = the rest rounded to f64.  That
holds the 64-bit significand of x86 extended precision (np.longdouble) without loss, and an mpmath value at 200 bits to
about 106 bits, far below the quarter-ulp resolution the bounds need.  Where np.longdouble has fewer than 63 fraction bits
(not x86-64) the values come from mpmath one point at a time: callers sample their argument sets down (`SAMPLE_LIMIT`).

A device result is judged by `ulp_error`: |got - exact| in units of the last place of the EXACT value's binade in the
result's format (f64: 53 bits, f32: 24 bits; below the normal range the subnormal spacing).  Sign and NaN-ness must match
exactly, and an infinity is accepted only where the exact value rounds past the largest finite number.
"""
import math

import numpy as np

HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63
SAMPLE_LIMIT = None if HAVE_LONGDOUBLE else 4000   # points per call on the mpmath path

_FMT = {np.dtype(np.float64): (53, -1074, float(np.finfo(np.float64).max)),
        np.dtype(np.float32): (24, -149, float(np.finfo(np.float32).max))}

UNARY = ["abs", "acos", "asin", "atan", "cbrt", "ceil", "cos", "cosh", "degrees", "exp", "expm1", "floor", "log10", "log2",
         "radians", "round", "sin", "sinh", "sqrt", "tan", "tanh", "cot", "sec", "csc"]
BINARY = ["atan2", "hypot", "log"]


# ---------------------------------------------------------------- reference values
_ODD_AT_ZERO = ("sin", "tan", "asin", "atan", "sinh", "tanh", "cbrt", "expm1", "degrees", "radians", "sqrt")


def _ld_pi():
    return np.longdouble(4) * np.arctan(np.longdouble(1))


def _ld_round(x):          # half away from zero (f64::round)
    t = np.trunc(x)
    return np.where(np.abs(x - t) >= 0.5, t + np.sign(x), t)     # (t itself where nothing is added: -0.0 stays -0.0)


def _ld_unary(op, x):
    pi = _ld_pi()
    f = {"abs": np.abs, "acos": np.arccos, "asin": np.arcsin, "atan": np.arctan, "cbrt": np.cbrt, "ceil": np.ceil,
         "cos": np.cos, "cosh": np.cosh, "exp": np.exp, "expm1": np.expm1, "floor": np.floor, "log10": np.log10,
         "log2": np.log2, "sin": np.sin, "sinh": np.sinh, "sqrt": np.sqrt, "tan": np.tan, "tanh": np.tanh,
         "degrees": lambda v: v * (np.longdouble(180) / pi), "radians": lambda v: v * (pi / np.longdouble(180)),
         "round": _ld_round, "cot": lambda v: np.cos(v) / np.sin(v), "sec": lambda v: 1 / np.cos(v),
         "csc": lambda v: 1 / np.sin(v)}[op]
    r = f(x)
    if op in _ODD_AT_ZERO:     # f(+-0) = +-0 (C99 F.9; np.expm1 on long double loses the sign)
        r = np.where(x == 0, x, r)
    return r


def _ld_binary(op, x, y):
    if op == "atan2":
        return np.arctan2(x, y)
    if op == "hypot":
        return np.hypot(x, y)
    return np.log(x) / np.log(y)      # log(self, base) = self.ln() / base.ln()


def _mp_one(op, x, y=None):
    import mpmath as mp
    fx = float(x)
    if op in ("abs", "ceil", "floor"):            # exact in binary floating point
        return {"abs": abs, "ceil": np.ceil, "floor": np.floor}[op](np.float64(fx))
    if op == "round":
        return float(_ld_round(np.float64(fx)))
    if not math.isfinite(fx) or (y is not None and not math.isfinite(float(y))):
        # infinities and NaNs: the IEEE result of the operation, taken from the platform's f64 functions
        with np.errstate(all="ignore"):
            v = _ld_binary(op, np.float64(fx), np.float64(y)) if y is not None else _ld_unary(op, np.float64(fx))
        return mp.mpf(float(v)) if not math.isnan(v) else mp.mpf("nan")
    a = mp.mpf(fx)
    with mp.workprec(200):
        try:
            if y is not None:
                b = mp.mpf(float(y))
                v = mp.atan2(a, b) if op == "atan2" else mp.hypot(a, b) if op == "hypot" else mp.log(a) / mp.log(b)
            else:
                f = {"acos": mp.acos, "asin": mp.asin, "atan": mp.atan, "cbrt": mp.cbrt, "cos": mp.cos, "cosh": mp.cosh,
                     "exp": mp.exp, "expm1": mp.expm1, "log10": mp.log10, "log2": lambda t: mp.log(t, 2), "sin": mp.sin,
                     "sinh": mp.sinh, "sqrt": mp.sqrt, "tan": mp.tan, "tanh": mp.tanh,
                     "degrees": lambda t: t * 180 / mp.pi, "radians": lambda t: t * mp.pi / 180,
                     "cot": lambda t: mp.cos(t) / mp.sin(t), "sec": lambda t: 1 / mp.cos(t), "csc": lambda t: 1 / mp.sin(t)}[op]
                if op == "cbrt" and a < 0:
                    v = -mp.cbrt(-a)
                elif op in ("cot", "csc") and a == 0:
                    v = mp.mpf("-inf") if math.copysign(1.0, fx) < 0 else mp.mpf("inf")
                else:
                    v = f(a)
        except (ValueError, ZeroDivisionError):
            return mp.mpf("nan")
        if isinstance(v, mp.mpc):
            return mp.mpf("nan") if v.imag != 0 else v.real
        if v == 0:      # keep the sign of an exact zero: sin(-0) = -0, tan(-0) = -0, ...
            return -0.0 if op in _ODD_AT_ZERO and math.copysign(1.0, fx) < 0 else 0.0
        return v


def _split_mp(vals):
    import mpmath as mp
    hi, lo = np.empty(len(vals)), np.empty(len(vals))
    with mp.workprec(200):
        for i, v in enumerate(vals):
            if isinstance(v, float) or not isinstance(v, mp.mpf):
                hi[i], lo[i] = float(v), 0.0
                continue
            if mp.isnan(v) or mp.isinf(v):
                hi[i], lo[i] = float(v), 0.0
                continue
            h = float(v)      # (mpf -> float rounds to nearest)
            hi[i] = h
            lo[i] = float(v - mp.mpf(h)) if math.isfinite(h) else 0.0
    return hi, lo


def _split_ld(v):
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float64)
        lo = np.where(np.isfinite(hi), (v - hi.astype(np.longdouble)).astype(np.float64), 0.0)
    return hi, lo


def exact_unary(op, x, use_mpmath=False):
    """(hi, lo) of op(x) for every element of the f64 / f32 vector x, exact to far below an ulp of the result's format."""
    x = np.asarray(x)
    if HAVE_LONGDOUBLE and not use_mpmath:
        with np.errstate(all="ignore"):
            return _split_ld(_ld_unary(op, x.astype(np.longdouble)))
    return _split_mp([_mp_one(op, v) for v in x])


def exact_binary(op, x, y, use_mpmath=False):
    x, y = np.asarray(x), np.asarray(y)
    if HAVE_LONGDOUBLE and not use_mpmath:
        with np.errstate(all="ignore"):
            return _split_ld(_ld_binary(op, x.astype(np.longdouble), y.astype(np.longdouble)))
    return _split_mp([_mp_one(op, a, b) for a, b in zip(x, y)])


def sample(rng, n, limit=SAMPLE_LIMIT):
    """Indices to check: all of them with exact long double, an even sample of `limit` on the mpmath path."""
    if limit is None or n <= limit:
        return np.arange(n)
    return np.sort(rng.choice(n, limit, replace=False))


def round_to(hi, lo, dtype):
    """The exact value hi + lo rounded ONCE to `dtype` (f32: hi alone can sit exactly half-way between two floats while lo
    decides the side; rounding hi would then round twice)."""
    hi, lo = np.asarray(hi, dtype=np.float64), np.asarray(lo, dtype=np.float64)
    if np.dtype(dtype) == np.float64:
        return hi.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        f = hi.astype(np.float32)
        fd = f.astype(np.float64)
        up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
        f = np.where((hi > fd) & (hi == (fd + up.astype(np.float64)) / 2) & (lo > 0), up, f)
        f = np.where((hi < fd) & (hi == (fd + dn.astype(np.float64)) / 2) & (lo < 0), dn, f)
    return f.astype(np.float32)


# ---------------------------------------------------------------- ulp distance
def ulp_of(hi, lo, dtype):
    """The spacing of `dtype` in the binade of the exact value hi + lo (the subnormal spacing below the normal range)."""
    p, emin, _ = _FMT[np.dtype(dtype)]
    hi = np.asarray(hi, dtype=np.float64)
    m, e = np.frexp(hi)                       # |hi| = |m| 2^e, |m| in [0.5, 1)
    e = e.astype(np.int64) - 1                # binade exponent of hi
    # hi a power of two rounded UP from just below it: the exact value lives one binade lower
    e = e - ((np.abs(m) == 0.5) & (lo != 0) & (np.sign(lo) != np.sign(hi)))
    e = np.where(hi == 0, emin + p - 1, e)
    return np.ldexp(1.0, np.maximum(e - (p - 1), emin))


def ulp_error(got, hi, lo, dtype):
    """|got - exact| in ulps of the exact value (see the module docstring); inf where sign, NaN-ness or overflow disagree."""
    got = np.asarray(got).astype(np.float64)
    hi, lo = np.asarray(hi, dtype=np.float64), np.asarray(lo, dtype=np.float64)
    _, _, fmax = _FMT[np.dtype(dtype)]
    ulp = ulp_of(hi, lo, dtype)
    with np.errstate(all="ignore"):
        err = np.abs((got - hi) - lo) / ulp
        en, gn = np.isnan(hi), np.isnan(got)
        err = np.where(en & gn, 0.0, err)
        err = np.where(en != gn, np.inf, err)
        # an infinity: right only where the exact value rounds past the largest finite number (or is infinite itself)
        overflows = np.abs(hi) + np.abs(lo) >= fmax + ulp_of(np.full_like(hi, fmax), 0 * hi, dtype) / 2
        gi = np.isinf(got)
        err = np.where(gi, np.where(overflows & (np.sign(got) == np.sign(hi)), 0.0, np.inf), err)
        err = np.where(~gi & ~gn & overflows & ~en, np.inf, err)
        # the sign, zeros included
        err = np.where(~en & ~gn & (np.signbit(got) != np.signbit(hi)), np.inf, err)
    return err


# ---------------------------------------------------------------- sums
def fsum_valid(chunks):
    """The correctly rounded sum of every valid value of a chunk list (math.fsum), and sum |x| and n over the same rows."""
    vals = [ch.to_numpy()[ch.valid_mask()].astype(np.float64) for ch in chunks]
    allv = np.concatenate(vals) if vals else np.zeros(0)
    return math.fsum(allv.tolist()), math.fsum(np.abs(allv).tolist()), len(allv)


def gamma(n, u=2.0 ** -53):
    """gamma_n = n u / (1 - n u): |computed - exact| <= gamma_(n-1) sum|x| for ANY order of n - 1 f64 additions."""
    return n * u / (1 - n * u)
