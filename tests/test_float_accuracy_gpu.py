"""Float kernels against EXACT references (tests/exact_ref.py), not against the oracle at 1e-6.

Transcendentals: the library's own sin / cos / tan (rdf_common.hip.h: Cody-Waite reduction + minimax polynomials, a per-row
form and an R-rows-per-lane form) and the device-libm ops, measured in ulps of the exact value at the arguments where such
code goes wrong (next to every multiple of pi/2 in the reduction's range, the hand-over points to libm, the tiny-argument
threshold, subnormals, specials), through every kernel form that runs them, each form confirmed by the kernel's name; the
forms must agree bit for bit.  Reductions: sums within the bound that holds for ANY summation order, integer-valued sums
bit-exact in every layout (a dropped or duplicated row changes them), the f32 sum's fold in f64, min / max bitwise.

Every check prints the measured maximum ulp per (op, dtype, form) (`pytest -s`).
"""
import math

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A

import exact_ref as X
from ulp_bounds import BOUND, DEFAULT_ULP, bound  # noqa: F401  (the bound table: max |error| in ulps of the exact value, shared with test_spec_catalog.py)

pytestmark = pytest.mark.gpu

F64, F32 = A.F64, A.F32
NP = {F64: np.float64, F32: np.float32}
UINT = {F64: np.uint64, F32: np.uint32}

TRIG = ["sin", "cos", "tan", "cot", "sec", "csc"]


@pytest.fixture(scope="module")
def dev():
    """The library with the kernel-selection switches under the test's own control (every form is chosen explicitly)."""
    from rust_dataframe_amd import lib
    api = lib.api()
    if lib.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    yield api, lib
    lib.set_option("spec", 1)
    lib.set_option("fast_filter", 1)
    lib.set_option("jit", 1)
    lib.set_option("interp_lean", 1)


# ---------------------------------------------------------------- layouts
def ragged(x, dt, rng, null_frac=0.02, offset=None):
    """x cut into chunks whose lengths are not multiples of any tile (and one empty chunk), sliced at a non-zero `offset` that
    keeps the 16-byte alignment the specialised kernels need (an unaligned slice is the interpreter's), with NULLs."""
    offset = 16 // np.dtype(NP[dt]).itemsize if offset is None else offset
    pattern = [100_003, 64 * 8 * 7 + 13, 777, 0, 65_537, 4097]
    chunks, i, j = [], 0, 0
    while i < len(x):
        n = min(pattern[j % len(pattern)], len(x) - i)
        j += 1
        valid = rng.uniform(size=n) >= null_frac if null_frac else None
        chunks.append(A.HostArray.from_numpy(x[i:i + n].astype(NP[dt]), valid=valid, offset=offset, dtype=dt, rng=rng))
        i += n
    return chunks


def same_layout(chunks, value):
    """A column of the constant `value` with the chunk lengths of `chunks` (no NULLs)."""
    return [A.HostArray.from_numpy(np.full(c.length, value, dtype=NP[c.dtype]), dtype=c.dtype) for c in chunks]


def flat(chunks):
    """(values, valid mask) over all chunks."""
    if not chunks:
        return np.zeros(0), np.zeros(0, dtype=bool)
    return np.concatenate([c.to_numpy() for c in chunks]), np.concatenate([c.valid_mask() for c in chunks])


# ---------------------------------------------------------------- kernel forms
STORE_FORMS = ["unary", "interp", "trig_rt", "jit"]


def _opts(lib, spec, jit):
    lib.set_option("spec", spec)
    lib.set_option("jit", jit)
    lib.set_option("interp_lean", 1)


def run_store(api, lib, form, op, xs):
    """op over the chunks xs through one kernel form -> (output chunks, kernel that ran).  Every form computes op(x) exactly:
    x - (+0.0) and v + (-0.0) are x and v, bit for bit, -0.0 and NaN included."""
    dt = xs[0].dtype
    if form == "unary":                # rdf_unary on the catalog's Un<op, col> store kernel (R rows per lane)
        _opts(lib, 1, 0)
        out = api.unary(op, xs)
        return out, lib.last_kernel()
    if form == "interp":               # the general evaluator: per-row functions
        _opts(lib, 0, 0)
        out = api.unary(op, xs)
        return out, lib.last_kernel()
    e = A.Expr()
    x, y, z = e.col(0), e.col(1), e.col(2)
    cols = [xs, same_layout(xs, 0.0), same_layout(xs, -0.0)]
    if form == "trig_rt":              # op(x - y): the shape kernels' runtime-op TrigRT node
        _opts(lib, 1, 0)
        v = e.op(op, e.op("subtract", x, y))
    else:                              # op(x - y) + z: outside the catalogs, compiled at run time
        _opts(lib, 1, 2)
        v = e.op("add", e.op(op, e.op("subtract", x, y)), z)
    outs = [[A.HostArray.empty_out(dt, c.length, True) for c in xs]]
    api.pipeline(e, cols, [v], -1, A.SINK_STORE, outs)
    return outs[0], lib.last_kernel()


def expect_kernel(form, kernel):
    if form == "unary":
        return kernel.startswith("spec_kernel<") and not kernel.endswith("[compiled at run time]")
    if form == "interp":
        return kernel.startswith("eval_kernel<STORE")
    if form == "trig_rt":
        return kernel.startswith("spec_kernel<") and "[T" in kernel
    if form == "jit":
        return kernel.startswith("spec_kernel<") and kernel.endswith("[compiled at run time]")
    if form in ("sum", "sum_rt"):
        return kernel.startswith("spec_kernel<") and (form == "sum" or "[T" in kernel)
    raise AssertionError(form)


def run_sum(api, lib, form, op, xs):
    """sum(op(x)) (form "sum") or sum(op(x - y)) (form "sum_rt", TrigRT) -> AggResult, kernel."""
    e = A.Expr()
    x, y = e.col(0), e.col(1)
    _opts(lib, 1, 2)
    v = e.op(op, x) if form == "sum" else e.op(op, e.op("subtract", x, y))
    r = api.pipeline(e, [xs, same_layout(xs, 0.0)], [v], -1)[0]
    return r, lib.last_kernel()


class Report:
    """Measured maxima per (op, dtype, form); failures collected so one run shows every number."""

    def __init__(self, title):
        self.title, self.rows, self.fail = title, {}, []

    def ulps(self, op, dt, form, err, args):
        m = float(err.max()) if len(err) else 0.0
        key = (op, "f64" if dt == F64 else "f32", form)
        self.rows[key] = max(self.rows.get(key, 0.0), m)
        if m > bound(op, dt):
            i = int(np.argmax(err))
            self.fail.append(f"{op} {key[1]} {form}: {m:.3f} ulp > {bound(op, dt)} at x = {args[i]!r}")

    def check(self, ok, msg):
        if not ok:
            self.fail.append(msg)

    def finish(self):
        print(f"\n[{self.title}] max ulp per (op, dtype, form):")
        for (op, d, f), m in sorted(self.rows.items()):
            print(f"  {op:7s} {d} {f:8s} {m:8.3f}   (bound {bound(op, F64 if d == 'f64' else F32)})")
        assert not self.fail, "\n".join(self.fail[:40])


def check_all_forms(api, lib, op, x, dt, rep, rng, forms=None, sums=True):
    """x through every form: ulps of the first form against the exact value, the others bit-identical to it, the sums
    against the exact sum of the first form's values."""
    forms = forms or (STORE_FORMS if op in ("sin", "cos", "tan") else ["unary", "interp", "jit"])
    xs = ragged(x, dt, rng)
    xv, valid = flat(xs)
    first = None
    for form in forms:
        out, kern = run_store(api, lib, form, op, xs)
        rep.check(expect_kernel(form, kern), f"{op} {form}: ran on {kern}")
        gv, gm = flat(out)
        rep.check(np.array_equal(gm, valid), f"{op} {form}: validity differs from the input's")
        gv = gv[valid]
        if first is None:
            first = gv
            idx = X.sample(rng, len(gv))
            h, l = X.exact_unary(op, xv[valid][idx])
            rep.ulps(op, dt, form, X.ulp_error(gv[idx], h, l, NP[dt]), xv[valid][idx])
        else:
            same = gv.view(UINT[dt]) == first.view(UINT[dt])
            if same.all():          # the same bits: the same errors
                rep.rows[(op, "f64" if dt == F64 else "f32", form)] = rep.rows[(op, "f64" if dt == F64 else "f32", forms[0])]
            else:
                i = int(np.argmin(same))
                rep.check(False, f"{op} {form}: {int((~same).sum())} results differ from {forms[0]}'s, first at x = {xv[valid][i]!r}: "
                                 f"{gv[i]!r} vs {first[i]!r}")
    if not sums or dt != F64:
        return
    fin = np.isfinite(first)
    ys = ragged(xv[valid][fin], dt, rng)
    _, yvalid = flat(ys)
    vals = first[fin][yvalid]
    s_exact, mag = math.fsum(vals.tolist()), math.fsum(np.abs(vals).tolist())
    for form in (["sum", "sum_rt"] if op in ("sin", "cos", "tan") else ["sum"]):
        r, kern = run_sum(api, lib, form, op, ys)
        rep.check(expect_kernel(form, kern), f"{op} {form}: ran on {kern}")
        rep.check(r.count == len(vals), f"{op} {form}: count {r.count} != {len(vals)}")
        rep.check(abs(r.sum - s_exact) <= X.gamma(len(vals) - 1) * mag, f"{op} {form}: sum {r.sum!r} vs exact {s_exact!r}")
        if len(vals):
            rep.check(r.min == vals.min() and r.max == vals.max(), f"{op} {form}: min/max {r.min!r}/{r.max!r} vs {vals.min()!r}/{vals.max()!r}")


# ---------------------------------------------------------------- argument sets
def _steps(c, k, dt):
    """The values k ulps away from each c (k may be negative; c > 0)."""
    bits = c.astype(NP[dt]).view(UINT[dt]).astype(np.int64) + k
    return bits.astype(UINT[dt]).view(NP[dt])


def f64_trig_args(rng):
    pi2 = X._ld_pi() / 2
    k = np.arange(1, 63_662, dtype=np.int64)
    c = (k.astype(np.longdouble) * pi2).astype(np.float64)       # the double nearest k pi / 2
    near = np.concatenate([_steps(c, s, F64) for s in range(-3, 4)])
    near = np.concatenate([near, -near])
    edges = []
    for p in (1.0e5, 2.0 ** -26):
        edges += [_steps(np.array([p]), s, F64) for s in range(-3, 4)]
    edges = np.concatenate(edges)
    edges = np.concatenate([edges, -edges])
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -1e-310, 1e-320, np.inf, -np.inf, np.nan,
                        -75885.045330917957, 63600.224891491329, 46639.304862655372])   # the worst of a host restatement
    logu = np.exp2(rng.uniform(-30, np.log2(1e300), 200_000)) * rng.choice([-1.0, 1.0], 200_000)
    return np.concatenate([near, edges, special, logu])


def f32_trig_args(rng):
    """Everything except the dense sweep next to k pi / 2 (test_f32_sin_cos_next_to_every_multiple_of_half_pi)."""
    edges = []
    for p in (1.0e9, 2.0 ** -13):
        edges += [_steps(np.array([p], dtype=np.float32), s, F32) for s in range(-8, 9)]
    edges = np.concatenate(edges)
    edges = np.concatenate([edges, -edges])
    finite = np.arange(0, 0x7F800000, 1999, dtype=np.uint32).view(np.float32)     # a stride over all finite f32
    finite = np.concatenate([finite, -finite])
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, np.inf, -np.inf, np.nan], dtype=np.float32)
    return np.concatenate([edges, finite, special]).astype(np.float32)


# ---------------------------------------------------------------- (a) + (b) + (d): the library's own trig
@pytest.mark.parametrize("op", TRIG)
def test_f64_trig_ulps_and_identical_forms(dev, op):
    api, lib = dev
    rng = np.random.default_rng(2026)
    rep = Report(f"f64 {op}")
    check_all_forms(api, lib, op, f64_trig_args(rng), F64, rep, rng)
    rep.finish()


@pytest.mark.parametrize("op", TRIG)
def test_f32_trig_ulps_and_identical_forms(dev, op):
    api, lib = dev
    rng = np.random.default_rng(2027)
    rep = Report(f"f32 {op}")
    check_all_forms(api, lib, op, f32_trig_args(rng), F32, rep, rng, sums=False)
    rep.finish()


def test_f32_sin_cos_next_to_every_multiple_of_half_pi(dev):
    """Every f32 within 4 ulps of k pi / 2 for 0 < k <= 4e6 (every 7th k also negated), in batches."""
    api, lib = dev
    rng = np.random.default_rng(2028)
    rep = Report("f32 sin / cos next to k pi / 2")
    pi2 = X._ld_pi() / 2
    K, step = 4_000_000, 500_000
    for k0 in range(1, K + 1, step):
        k = np.arange(k0, min(k0 + step, K + 1), dtype=np.int64)
        c = (k.astype(np.longdouble) * pi2).astype(np.float32)
        x = np.concatenate([_steps(c, s, F32) for s in range(-4, 5)])
        x = np.concatenate([x, -x[::7]])
        for op in ("sin", "cos"):
            check_all_forms(api, lib, op, x, F32, rep, rng, forms=["unary", "interp", "trig_rt", "jit"], sums=False)
    rep.finish()


# ---------------------------------------------------------------- (c): one big argument per wave changes nothing
@pytest.mark.parametrize("dt", [F64, F32])
def test_wave_wide_libm_fallback_changes_no_bits(dev, dt):
    """The R-rows form tests all of a wave's rows at once and sends the WHOLE wave down the per-row path when one lane holds
    |x| >= 1e5 (f64) / 1e9 (f32).  One such argument planted in every 256 rows (every 64 x R group for R = 4 and 8) must not
    change a single bit of the other rows' results."""
    api, lib = dev
    rng = np.random.default_rng(99)
    n = 256 * 2000
    x = rng.uniform(-2e4, 2e4, n) * np.exp2(rng.integers(-30, 1, n))
    x[::97] = rng.uniform(-1, 1, len(x[::97])) * 2.0 ** -27          # the tiny-argument path as well
    planted = x.copy()
    j = np.arange(n // 256)
    pos = 256 * j + (j * 41) % 256
    planted[pos] = (3.0e5 if dt == F64 else 3.0e9) * np.where(j % 2, 1, -1)
    keep = np.ones(n, dtype=bool)
    keep[pos] = False
    rep = Report(f"wave-wide fallback {'f64' if dt == F64 else 'f32'}")
    for op in TRIG:
        for form in ["unary", "interp", "trig_rt", "jit"] if op in ("sin", "cos", "tan") else ["unary", "interp", "jit"]:
            got = []
            for v in (x, planted):
                out, kern = run_store(api, lib, form, op, [A.HostArray.from_numpy(v.astype(NP[dt]), dtype=dt)])
                rep.check(expect_kernel(form, kern), f"{op} {form}: ran on {kern}")
                got.append(out[0].to_numpy()[keep].view(UINT[dt]))
            diff = got[0] != got[1]
            rep.check(not diff.any(), f"{op} {form}: {int(diff.sum())} rows changed when a wave-mate took the libm path")
    rep.finish()


# ---------------------------------------------------------------- device-libm ops
def _domain(op, rng, n):
    if op in ("acos", "asin"):
        v = rng.uniform(-1, 1, n)
    elif op in ("log10", "log2", "sqrt"):
        v = np.exp2(rng.uniform(-1000, 1000, n))
    elif op in ("exp", "expm1", "cosh", "sinh"):
        v = rng.uniform(-750, 750, n)
        v[: n // 2] = rng.uniform(-2, 2, n // 2) * np.exp2(rng.integers(-40, 1, n // 2))
    elif op == "tanh":
        v = rng.uniform(-20, 20, n) * np.exp2(rng.integers(-40, 1, n))
    else:
        v = rng.uniform(-1e3, 1e3, n) * np.exp2(rng.integers(-60, 60, n))
    return v


@pytest.mark.parametrize("dt", [F64, F32])
def test_device_libm_unary_ops_ulps(dev, dt):
    api, lib = dev
    rng = np.random.default_rng(5)
    rep = Report(f"device-libm unary {'f64' if dt == F64 else 'f32'}")
    specials = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.5, -2.5, np.inf, -np.inf, np.nan, 5e-324, 1e-310])
    for op in [o for o in A.UNARY_OPS if o not in TRIG]:
        x = np.concatenate([_domain(op, rng, 60_000), specials])
        with np.errstate(all="ignore"):
            x = x.astype(NP[dt])
        check_all_forms(api, lib, op, x, dt, rep, rng, forms=["unary", "interp"], sums=False)
    rep.finish()


@pytest.mark.parametrize("dt", [F64, F32])
def test_device_libm_binary_ops_ulps(dev, dt):
    api, lib = dev
    rng = np.random.default_rng(6)
    rep = Report(f"device-libm binary {'f64' if dt == F64 else 'f32'}")
    n = 60_000
    for op in ["atan2", "hypot", "log"]:
        a = np.exp2(rng.uniform(-60, 60, n)) * (rng.choice([-1, 1], n) if op != "log" else 1)
        b = np.exp2(rng.uniform(-60, 60, n)) * (rng.choice([-1, 1], n) if op != "log" else 1)
        b[:100] = 1.0 + rng.uniform(-1e-3, 1e-3, 100)          # log: a base next to 1
        a, b = a.astype(NP[dt]), b.astype(NP[dt])
        results = []
        for form, spec in (("spec", 1), ("interp", 0)):
            _opts(lib, spec, 0)
            xs, ys = ragged(a, dt, np.random.default_rng(1)), ragged(b, dt, np.random.default_rng(1))
            out = api.binary(op, xs, ys)
            # (the catalog holds the binary math ops for f64 only: f32 is the interpreter's in both runs)
            rep.check(expect_kernel("unary" if spec and dt == F64 else "interp", lib.last_kernel()), f"{op} {form}: ran on {lib.last_kernel()}")
            gv, gm = flat(out)
            av, am = flat(xs)
            bv, _ = flat(ys)
            results.append(gv[gm])
        h, l = X.exact_binary(op, av[am], bv[am])
        rep.ulps(op, dt, "spec", X.ulp_error(results[0], h, l, NP[dt]), av[am])
        rep.check(np.array_equal(results[0].view(UINT[dt]), results[1].view(UINT[dt])), f"{op}: spec and interp differ")
    rep.finish()


# ---------------------------------------------------------------- reductions
AGG_LAYOUTS = [  # test_aggregates' layouts, reader batches, chunks straddling 2^16 and 2^20 rows
    ([5], 0.0, 0), ([1000], 0.0, 0), ([1024, 1024, 576], 0.0, 0), ([4097], 0.1, 0), ([700, 0, 3000], 0.1, 13),
    ([2500], -1.0, 5), ([50_000, 70_001], 0.05, 3), ([1024] * 50 + [576], 0.0, 0), ([1024] * 50 + [576], 0.05, 7),
    ([2 ** 16 - 1, 2 ** 16 + 3, 2 ** 20 + 5, 2 ** 16], 0.02, 1), ([2 ** 20 - 3, 7, 2 ** 20 + 1], 0.0, 0),
]


def _chunks(values, lens, nf, off, rng, dt=F64):
    out, i = [], 0
    for n in lens:
        valid = None if nf == 0 else (np.zeros(n, dtype=bool) if nf < 0 else rng.uniform(size=n) >= nf)
        out.append(A.HostArray.from_numpy(values[i:i + n].astype(NP[dt]), valid=valid, offset=off, dtype=dt, rng=rng))
        i += n
    return out


def _agg_paths(gpu, lib, request, cols, filt_threshold=None):
    """sum of column 0 through the fused pipeline: as the fixture param selects, plus the lean / general interpreter."""
    e = A.Expr()
    c = e.col(0)
    filt = e.op("gt", c, e.scalar(float(filt_threshold))) if filt_threshold is not None else -1
    res = {}
    spec_on = request.node.callspec.params["gpu"] == "spec"
    if spec_on:
        res["pipeline"] = (gpu.pipeline(e, cols, [c], filt)[0], lib.last_kernel())
    else:
        for lean in (1, 0):
            lib.set_option("interp_lean", lean)
            res["lean" if lean else "general"] = (gpu.pipeline(e, cols, [c], filt)[0], lib.last_kernel())
        lib.set_option("interp_lean", 1)
    return res


def test_integer_valued_f64_sums_are_bit_exact(gpu, request):
    """x[i] = i + 1 (with 2^k tile markers on a few rows): every partial sum is an integer below 2^53, so every summation
    order gives the exact sum — a dropped or duplicated row cannot hide.  rdf_sum / avg / min / max and the fused pipeline
    (with and without a filter) in the spec / lean interpreter / general interpreter paths."""
    from rust_dataframe_amd import lib
    rng = np.random.default_rng(31)
    spec_on = request.node.callspec.params["gpu"] == "spec"
    for lens, nf, off in AGG_LAYOUTS:
        n = sum(lens)
        x = np.arange(1, n + 1, dtype=np.float64)
        x[::4099] += 2.0 ** 40                  # markers: a missing one is off by 2^40
        cols = _chunks(x, lens, nf, off, rng)
        xv, m = flat(cols)
        v = xv[m]
        what = f"lens={lens[:4]}{'...' if len(lens) > 4 else ''} nf={nf} off={off}"
        exact = math.fsum(v.tolist())
        assert exact < 2.0 ** 53
        got = gpu.sum(cols)
        assert (got is None and len(v) == 0) or got == exact, f"rdf_sum {what}: {got!r} vs {exact!r}"
        if len(v):
            assert gpu.avg(cols) == exact / len(v), f"avg {what}"
            assert gpu.min(cols) == v.min() and gpu.max(cols) == v.max(), f"min/max {what}"
        t = float(n // 3) + 0.5
        for thr, sel in ((None, v), (t, v[v > t])):
            for path, (r, kern) in _agg_paths(gpu, lib, request, [cols], thr).items():
                if not spec_on:     # (spec on: the shape's kernel, or the interpreter for an unaligned slice)
                    assert kern == ("eval_kernel<AGG, lean>" if path == "lean" else "eval_kernel<AGG>"), f"{path}: {kern}"
                assert r.count == len(sel), f"{path} thr={thr} {what}: count"
                if len(sel):
                    assert r.sum == math.fsum(sel.tolist()), f"{path} thr={thr} {what}: {r.sum!r} vs {math.fsum(sel.tolist())!r}"
                    assert r.min == sel.min() and r.max == sel.max(), f"{path} thr={thr} {what}: min/max"


def test_f64_sum_within_the_any_order_bound(gpu, ora, request):
    """|got - fsum| <= gamma_(n-1) sum|x|: true for every summation order (it cannot flake), and 10^8 x tighter than a sum
    accumulated in f32 would meet.  Cancelling data too, where the relative error of the result is large."""
    from rust_dataframe_amd import lib
    rng = np.random.default_rng(32)
    for lens, nf, off in AGG_LAYOUTS:
        n = sum(lens)
        for kind in ("uniform", "cancelling"):
            x = rng.uniform(-1, 1, n) * (np.exp2(rng.integers(-20, 21, n)) if kind == "cancelling" else 1.0)
            cols = _chunks(x, lens, nf, off, rng)
            s, mag, cnt = X.fsum_valid(cols)
            what = f"{kind} lens={lens[:4]} nf={nf}"
            if cnt == 0:
                assert gpu.sum(cols) == ora.sum(cols)
                continue
            tol = X.gamma(cnt - 1) * mag
            g = gpu.sum(cols)
            assert abs(g - s) <= tol, f"rdf_sum {what}: {g!r} vs {s!r} (bound {tol:.3g})"
            a = gpu.avg(cols)
            assert abs(a - s / cnt) <= tol / cnt + 0.5 * np.spacing(abs(s / cnt)) + 2.0 ** -1074, f"avg {what}: {a!r} vs {s / cnt!r}"
            for thr in (None, 0.5):
                sel_s = s if thr is None else math.fsum([float(t) for c in cols for t in c.to_numpy()[c.valid_mask() & (c.to_numpy() > thr)]])
                sel_m = mag if thr is None else math.fsum([abs(float(t)) for c in cols for t in c.to_numpy()[c.valid_mask() & (c.to_numpy() > thr)]])
                for path, (r, _) in _agg_paths(gpu, lib, request, [cols], thr).items():
                    assert abs(r.sum - sel_s) <= X.gamma(max(r.count - 1, 0)) * sel_m, f"{path} thr={thr} {what}: {r.sum!r} vs {sel_s!r}"


def test_f32_sum_folds_in_f64_and_rounds_once(gpu):
    """DESIGN: the f32 sum folds in f64 and rounds once -> |got - fsum| <= half an f32 ulp + n 2^-53 sum|x|."""
    rng = np.random.default_rng(33)
    for lens, nf, off in AGG_LAYOUTS:
        n = sum(lens)
        for kind in ("plain", "cancelling"):
            x = rng.uniform(-100, 100, n) * (np.exp2(rng.integers(-12, 13, n)) if kind == "cancelling" else 1.0)
            cols = _chunks(x, lens, nf, off, rng, F32)
            s, mag, cnt = X.fsum_valid(cols)
            if cnt == 0:
                continue
            g = gpu.sum(cols)
            half = 0.5 * X.ulp_of(np.array([s]), np.zeros(1), np.float32)[0]
            assert abs(g - s) <= half + cnt * 2.0 ** -53 * mag, f"{kind} lens={lens[:4]} nf={nf}: {g!r} vs {s!r}"
            a = gpu.avg(cols)
            assert abs(a - s / cnt) <= (cnt * 2.0 ** -53 * mag) / cnt + np.spacing(abs(s / cnt)), f"avg {kind} lens={lens[:4]}"


def _group_sums(gpu, keys, vals, ngroups):
    k, s, c = gpu.groupby_sum(keys, vals, ngroups + 8)
    km = k.valid_mask()
    return {(int(kk) if ok else None): (float(ss), int(cc)) for kk, ok, ss, cc in zip(k.to_numpy(), km, s.to_numpy(), c.to_numpy())}


@pytest.mark.parametrize("val_dt", [F64, F32])
@pytest.mark.parametrize("ngroups,n", [(50, 40_000), (5_000, 300_000), (300_000, 1_200_000)])
def test_groupby_sums_within_the_any_order_bound(gpu, val_dt, ngroups, n):
    """Per group: |got - fsum| <= gamma_(n_g - 1) sum_g|x| (the group sum is returned in f64 for both value types), and
    integer-valued groups bit-exact; the small-table, the LDS-table and the partitioned high-cardinality paths."""
    rng = np.random.default_rng(ngroups)
    lens = [n // 3, 0, n - n // 3]
    kv = rng.integers(0, ngroups, n)
    for kind in ("random", "integers"):
        x = rng.uniform(-1, 1, n) * np.exp2(rng.integers(-10, 11, n)) if kind == "random" else (np.arange(n) % 1000).astype(np.float64)
        keys = [A.HostArray.from_numpy(kv[i:i + ln], valid=rng.uniform(size=ln) >= 0.01, offset=5, rng=rng)
                for i, ln in zip(np.cumsum([0] + lens[:-1]), lens)]
        vals = _chunks(x, lens, 0.02, 2, rng, val_dt)
        got = _group_sums(gpu, keys, vals, ngroups)
        kk = np.concatenate([np.where(k.valid_mask(), k.to_numpy(), -1) for k in keys])
        vv, vm = flat(vals)
        groups = {}
        for key, val, ok in zip(kk.tolist(), vv.astype(np.float64).tolist(), vm.tolist()):
            g = groups.setdefault(None if key == -1 else key, [[], 0])
            g[1] += 1
            if ok:
                g[0].append(val)
        assert set(got) == set(groups), f"{kind}: group keys differ"
        bad = []
        for key, (vs, cnt) in groups.items():
            gs, gc = got[key]
            s, mag = math.fsum(vs), math.fsum(abs(t) for t in vs)
            tol = 0.0 if kind == "integers" else X.gamma(max(len(vs) - 1, 0)) * mag
            if abs(gs - s) > tol:
                bad.append((key, gs, s, tol))
        assert not bad, f"{kind} {len(bad)} groups off, e.g. {bad[:3]}"


def test_min_max_bitwise_signed_zeros_and_nans(gpu, ora):
    """min / max compared as bits: -0.0 is below +0.0 whatever the order the rows meet in, NaN never wins unless every
    value is NaN."""
    rng = np.random.default_rng(34)
    for dt in (F64, F32):
        for n in (7, 1000, 4097, 70_001):
            for arr in ("zeros", "zeros_nan", "mixed"):
                v = np.where(rng.uniform(size=n) < 0.5, -0.0, 0.0)
                if arr == "zeros_nan":
                    v[rng.uniform(size=n) < 0.3] = np.nan
                if arr == "mixed":
                    v[rng.uniform(size=n) < 0.1] = np.nan
                    v[n // 2] = 3.5
                    v[n // 3] = -1.25
                v[0], v[-1] = (0.0, -0.0) if n % 2 else (-0.0, 0.0)
                cols = _chunks(v, [n // 2, n - n // 2], 0.0, 3, rng, dt)
                fin = v[~np.isnan(v)]
                exp_min = fin.min() if arr == "mixed" else -0.0
                exp_max = fin.max() if arr == "mixed" else 0.0
                for what, got, exp in (("min", gpu.min(cols), exp_min), ("max", gpu.max(cols), exp_max)):
                    g = np.array([got], dtype=NP[dt]).view(UINT[dt])[0]
                    e = np.array([exp], dtype=NP[dt]).view(UINT[dt])[0]
                    assert g == e, f"{what} dt={dt} n={n} {arr}: {got!r} vs {exp!r}"
    a = [A.HostArray.from_numpy(np.array([np.nan, np.nan]))]
    assert np.isnan(gpu.min(a)) and np.isnan(gpu.max(a))


def test_headline_filter_sum_at_two_million_rows(gpu, request):
    """filter(x > 0.5) -> sum, 2e6 rows in reader batches: integer-valued (bit-exact) and uniform (any-order bound)."""
    from rust_dataframe_amd import lib
    rng = np.random.default_rng(35)
    n = 2_000_000
    lens = [1024] * (n // 1024) + [n % 1024]
    for kind in ("integers", "uniform"):
        x = (np.arange(n) % 3) * 0.5 if kind == "integers" else rng.uniform(size=n)     # 0, 0.5, 1.0: exact in any order
        cols = _chunks(x, lens, 0.1, 3, rng)
        xv, m = flat(cols)
        sel = xv[m & (xv > 0.5)]
        s, mag = math.fsum(sel.tolist()), math.fsum(np.abs(sel).tolist())
        for path, (r, _) in _agg_paths(gpu, lib, request, [cols], 0.5).items():
            assert r.count == len(sel), f"{kind} {path}"
            if kind == "integers":
                assert r.sum == s, f"{kind} {path}: {r.sum!r} vs {s!r}"
            else:
                assert abs(r.sum - s) <= X.gamma(len(sel) - 1) * mag, f"{kind} {path}: {r.sum!r} vs {s!r}"
