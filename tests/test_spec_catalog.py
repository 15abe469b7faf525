"""Every kernel of the specialised catalog (rdf_spec_catalog_size() of them) against a numpy reference, by name.

tests/spec_catalog.py restates the registration lists and builds, for every entry, programs the host has to route to it
(canonical / mirrored / aliased, seeded runtime operators); tests/spec_ref.py evaluates them in numpy, independently of the
C oracle.  The CPU tests hold the model to the library's catalog size, the draws to their conditions and the reference to the
oracle.  The GPU tests run every program over one ragged, sliced, NULL-carrying layout in device memory and assert WHICH
kernel ran (`spec_kernel<signature>`, not just "a specialised kernel"), exact validity / counts / integers / stored float
arithmetic, the ulp bounds of tests/ulp_bounds.py for math functions and the any-order bound for float sums; the entries whose
kernel never ran must be exactly spec_catalog.UNREACHABLE.
"""
import math
import time

import numpy as np
import pytest

from rust_dataframe_amd import _abi as A

import exact_ref as X
import spec_catalog as M
import spec_ref as R
from ulp_bounds import bound

NP = A.NP_OF
UINT = {A.F64: np.uint64, A.F32: np.uint32}


# ---------------------------------------------------------------- comparisons (the oracle and the device are held to the same ones)
def what_of(p):
    return f"{p.entry.sig} [{p.variant}, seed {p.seed}, ops {sorted(p.ops.items())}, columns {p.columns}]"


def check_store(chunks, ref, fails, what):
    """Output chunks against the reference: validity bitmap and null count exact, integers / masks / float + - * / bit-exact,
    math functions within their ulp bound of the exact value."""
    lens = [c.length for c in chunks]
    if lens != M.CHUNK_LENS:
        fails.append(f"{what}: chunk lengths {lens}")
        return
    i = 0
    for k, c in enumerate(chunks):
        n = c.length
        valid = ref.valid[i:i + n]
        if c.dtype != ref.dt:
            fails.append(f"{what}: dtype {c.dtype} != {ref.dt}")
        if not np.array_equal(c.valid_mask(), valid):
            fails.append(f"{what}: chunk {k}: validity bitmap differs at {int((c.valid_mask() != valid).sum())} rows")
        elif c.null_count != int(n - valid.sum()):
            fails.append(f"{what}: chunk {k}: null count {c.null_count} != {int(n - valid.sum())}")
        else:
            got, exp = c.to_numpy()[valid], ref.v[i:i + n][valid]
            if ref.op:
                err = X.ulp_error(got, ref.hi[i:i + n][valid], ref.lo[i:i + n][valid], NP[ref.dt])
                if len(err) and err.max() > bound(ref.op, ref.dt):
                    fails.append(f"{what}: chunk {k}: {ref.op} is {err.max():.3f} ulp off (bound {bound(ref.op, ref.dt)})")
            else:
                if ref.dt in UINT:
                    got, exp = got.view(UINT[ref.dt]), exp.view(UINT[ref.dt])
                if not np.array_equal(got, exp):
                    j = int(np.argmax(got != exp))
                    fails.append(f"{what}: chunk {k}: {int((got != exp).sum())} values differ, first at valid row {j}: {got[j]!r} vs {exp[j]!r}")
        i += n


def _same_nonfinite(got, exp):
    return (math.isnan(exp) and math.isnan(got)) or got == exp


def check_agg(got, refs, fails, what, f32_fold=False):
    """rdf_agg_result against the reference.  count exact; integer sum / min / max exact; float min / max equal by value (a math
    function's: inside the interval its ulp bound leaves); float sums |got - fsum(v)| <= gamma(count - 1) sum|v| — true for any
    summation order — plus sum(bound_ulps ulp(v_i)) where v is a math function's; an f32 sum is that f64 fold rounded once to
    f32, so it lies between the two ends of the interval rounded to f32.  f32_fold: the oracle folds f32 sums in f32 as
    the reference does (DESIGN.md lists the divergence), so its f32 sums get the same any-order bound at f32's unit roundoff."""
    if len(got) != len(refs):
        fails.append(f"{what}: {len(got)} results")
        return
    for v, (g, r) in enumerate(zip(got, refs)):
        w = f"{what} value {v}"
        if (g.count, g.is_some, g.dtype) != (r.count, r.count > 0, r.dt):
            fails.append(f"{w}: count / is_some / dtype {(g.count, g.is_some, g.dtype)} != {(r.count, r.count > 0, r.dt)}")
            continue
        if r.dt not in R.FLOATS:
            if (g.sum, g.min, g.max) != (r.sum, r.min, r.max):
                fails.append(f"{w}: sum / min / max {(g.sum, g.min, g.max)} != {(r.sum, r.min, r.max)}")
            continue
        if r.count == 0:
            if g.sum != 0.0:
                fails.append(f"{w}: sum of no rows {g.sum!r}")
            continue
        npdt = NP[r.dt]
        b = bound(r.op, r.dt) if r.op else 0.0
        exact = r.hi if r.op else r.values.astype(np.float64)            # the exact values' leading part
        with np.errstate(all="ignore"):
            slack = b * X.ulp_of(r.hi, r.lo, npdt) if r.op else np.zeros(len(exact))
            num = ~np.isnan(exact)
            if num.any():
                lo_end, hi_end = exact[num] - slack[num], exact[num] + slack[num]
                if r.op and b > 0:
                    ok = lo_end.min() <= g.min <= hi_end.min() and lo_end.max() <= g.max <= hi_end.max()
                else:
                    ok = g.min == r.min and g.max == r.max
            else:
                ok = math.isnan(g.min) and math.isnan(g.max)
        if not ok:
            fails.append(f"{w}: min / max {g.min!r} / {g.max!r} vs {r.min!r} / {r.max!r}")
        if not math.isfinite(r.sum) or not np.isfinite(exact).all():
            if not _same_nonfinite(g.sum, r.sum):
                fails.append(f"{w}: sum {g.sum!r} vs the non-finite {r.sum!r}")
            continue
        mag = math.fsum((np.abs(exact) + slack).tolist())
        tol = X.gamma(r.count - 1, 2.0 ** -24 if f32_fold and r.dt == A.F32 else 2.0 ** -53) * mag + math.fsum(slack.tolist())
        if r.dt == A.F32 and not f32_fold:
            with np.errstate(over="ignore"):
                ok = float(np.float32(r.sum - tol)) <= g.sum <= float(np.float32(r.sum + tol))
        else:
            ok = abs(g.sum - r.sum) <= tol
        if not ok:
            fails.append(f"{w}: sum {g.sum!r} vs {r.sum!r}: off by {abs(g.sum - r.sum):.3g}, bound {tol:.3g}")


# ---------------------------------------------------------------- CPU: the model, the draws, the reference
def test_model_holds_exactly_the_catalog():
    from rust_dataframe_amd import lib
    assert len(M.CATALOG.entries) == lib.spec_catalog_size()
    assert len({e.sig for e in M.ENTRIES}) == len(M.ENTRIES)
    assert M.CATALOG.registrations > len(M.ENTRIES)          # a few signatures are registered twice (the casts, the bare columns)
    assert all(e.shape for e in M.ENTRIES if e.runtime_slots())     # runtime operators come from the shape lists only


def test_every_entry_has_an_accepted_draw_for_every_variant_it_has():
    """program() raises where MAX_DRAWS seeds were all rejected.  Every entry has its canonical program; a shape entry has the
    mirrored one when some node of it can be written the other way round and the aliased one when two column slots share a
    dtype; an exact entry's program spells exactly the registered signature."""
    for e in M.ENTRIES:
        got = {v: M.program(e, v) for v in M.VARIANTS}
        assert got["canonical"] is not None, e.sig
        if not e.shape:
            assert got["canonical"].expect == e.sig and got["mirrored"] is None and got["aliased"] is None, e.sig
            continue
        cols = [x for r in e.roots() for x in r.walk() if x.kind == "col"]
        two_of_a_kind = len(cols) != len({x.dt for x in cols})
        assert (got["aliased"] is not None) == two_of_a_kind, e.sig
        assert (got["mirrored"] is not None) == any(M._mirrorable(x) for r in e.roots() for x in r.walk()), e.sig
        for p in got.values():
            if p is not None and p.variant == "aliased":
                assert len(p.columns) == len(cols) - 1, e.sig
            if p is not None and p.variant == "mirrored":
                assert any(m for _, _, m in p.ops.values()), e.sig


def test_every_operator_occurs_at_every_slot_it_can_occupy():
    """Over the accepted draws of the whole catalog: the four arithmetic operators at every arithmetic slot index, sin / cos / tan
    at every trig slot, the six comparisons at every comparison slot, and / or at the logic slot; and, with the operands the
    other way round (the swap bit / the mirrored comparison), subtract and divide and every comparison."""
    want = {"A": set(M.ARITH), "T": set(M.TRIG), "C": set(M.CMPS), "G": set(M.LOGIC)}
    seen, seen_mirrored, can_mirror = {}, {}, set()
    for e in M.ENTRIES:
        can_mirror |= {(x.kind, x.n) for r in e.roots() for x in r.walk() if x.kind in "AC" and M._mirrorable(x)}
    for p in M.programs():
        for s, (kind, name, mirrored) in p.ops.items():
            seen.setdefault((kind, s), set()).add(name)
            if mirrored:
                seen_mirrored.setdefault((kind, s), set()).add(name)
    assert set(seen) == {slot for e in M.ENTRIES for slot in e.runtime_slots()} and {k for k, _ in seen} == set(want)
    for key, names in sorted(seen.items()):
        assert names == want[key[0]], f"slot {key}: only {sorted(names)}"
    for key in sorted(can_mirror):
        assert seen_mirrored.get(key, set()) >= (want["C"] if key[0] == "C" else {"subtract", "divide"}), f"slot {key} mirrored: only {sorted(seen_mirrored.get(key, ()))}"


def test_unreachable_is_what_the_exact_catalog_takes_away():
    """The routing rule the model states (the exact signature, if registered, wins) leaves exactly UNREACHABLE without a program;
    the GPU sweep asserts the same of the kernels that really ran."""
    reached = {p.expect for p in M.programs()}
    assert {e.sig for e in M.ENTRIES if e.sig not in reached} == set(M.UNREACHABLE)
    assert all(p.expect in M.CATALOG.entries for p in M.programs())


@pytest.mark.parametrize("family", M.FAMILIES)
def test_numpy_reference_agrees_with_the_oracle(ora, family):
    fails = []
    for p in M.programs(family):
        ref = M.reference(p)
        cols = p.host_columns()
        try:
            if p.sink == M.SINK_STORE:
                outs = [[A.HostArray.empty_out(p.out_dtype, n, True) for n in M.CHUNK_LENS]]
                ora.pipeline(p.expr, cols, p.value_roots, -1, A.SINK_STORE, outs)
                check_store(outs[0], ref, fails, what_of(p))
            else:
                check_agg(ora.pipeline(p.expr, cols, p.value_roots, p.filter_root), ref, fails, what_of(p), f32_fold=True)
        except A.RdfError as ex:
            fails.append(f"{what_of(p)}: the oracle raised {ex}")
    assert not fails, f"{len(fails)} disagreements:\n" + "\n".join(fails[:20])


# ---------------------------------------------------------------- GPU: every program, by kernel name
_DEVICE_COLUMNS = {}
_OUT_BUFFERS = {}
_SWEPT = {}          # (family, mode) -> failures
_RAN = {"spec": set(), "interp": set()}


def _device_column(key):
    """A pool column's chunks in device memory, values and bitmaps behind the same element / bit offsets; uploaded once."""
    if key not in _DEVICE_COLUMNS:
        import torch
        out = []
        for ch in M.pool_column(*key):
            vt = torch.from_numpy(np.frombuffer(ch.values.tobytes() + b"\0" * 64, dtype=np.uint8).copy()).cuda()
            bt = torch.from_numpy(np.frombuffer(ch.validity.tobytes() + b"\0" * 64, dtype=np.uint8).copy()).cuda() if ch.validity is not None else None
            out.append(A.DeviceArray(vt.data_ptr(), bt.data_ptr() if bt is not None else None, ch.offset, ch.length, ch.dtype, ch.null_count, keep=(vt, bt)))
        torch.cuda.synchronize()
        _DEVICE_COLUMNS[key] = out
    return _DEVICE_COLUMNS[key]


def _out_buffer(dt):
    """One device buffer for the output chunks of a dtype (values 256-byte aligned, bitmaps whole words + one), reused."""
    if dt not in _OUT_BUFFERS:
        import torch
        offs, total = [], 0
        for n in M.CHUNK_LENS:
            vbytes = ((n + 63) // 64) * 8 + 8 if dt == A.BOOL else n * np.dtype(NP[dt]).itemsize
            bbytes = ((n + 63) // 64) * 8 + 8
            ov = total
            ob = ov + (vbytes + 255) // 256 * 256 + 256
            total = ob + (bbytes + 255) // 256 * 256 + 256
            offs.append((ov, vbytes, ob, bbytes))
        _OUT_BUFFERS[dt] = (torch.empty(total, dtype=torch.uint8, device="cuda"), offs)
    return _OUT_BUFFERS[dt]


def _run_store(api, p):
    import torch
    dt = p.out_dtype
    buf, offs = _out_buffer(dt)
    buf.fill_(0xA5)          # a row the kernel does not write shows
    torch.cuda.synchronize()
    base = buf.data_ptr()
    outs = [[A.DeviceArray(base + ov, base + ob, 0, n, dt, 0) for n, (ov, _, ob, _) in zip(M.CHUNK_LENS, offs)]]
    api.pipeline(p.expr, [_device_column(c) for c in p.columns], p.value_roots, -1, A.SINK_STORE, outs)
    host = buf.cpu().numpy()
    chunks = []
    for o, (ov, vbytes, ob, bbytes) in zip(outs[0], offs):
        vals = host[ov:ov + vbytes].copy()
        chunks.append(A.HostArray(vals if dt == A.BOOL else vals.view(NP[dt]), host[ob:ob + bbytes].copy(), 0, o.length, dt, o.null_count))
    return chunks


def _sweep(api, lib, family, mode):
    if (family, mode) in _SWEPT:
        return _SWEPT[(family, mode)]
    fails = []
    for p in M.programs(family):
        ref = M.reference(p)
        w = what_of(p)
        try:
            if p.sink == M.SINK_STORE:
                chunks = _run_store(api, p)
                kernel = lib.last_kernel()
                check_store(chunks, ref, fails, w)
            else:
                got = api.pipeline(p.expr, [_device_column(c) for c in p.columns], p.value_roots, p.filter_root)
                kernel = lib.last_kernel()
                check_agg(got, ref, fails, w)
        except A.RdfError as ex:
            fails.append(f"{w}: {ex}")
            continue
        _RAN[mode].add(kernel)
        if mode == "spec" and kernel != "spec_kernel<" + p.expect + ">":
            fails.append(f"{w}: ran on {kernel}, not on spec_kernel<{p.expect}>")
        if mode == "interp" and not kernel.startswith("eval_kernel<"):
            fails.append(f"{w}: ran on {kernel} with the specialised kernels switched off")
    _SWEPT[(family, mode)] = fails
    return fails


@pytest.mark.gpu
@pytest.mark.parametrize("family", M.FAMILIES)
def test_every_program_of_the_family_runs_its_own_kernel_and_matches_numpy(gpu, request, family):
    from rust_dataframe_amd import lib
    mode = request.node.callspec.params["gpu"]
    t0 = time.perf_counter()
    fails = _sweep(gpu, lib, family, mode)
    print(f"\n[{family} / {mode}] {len(M.programs(family))} programs in {time.perf_counter() - t0:.2f} s")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:20])


@pytest.mark.gpu
def test_the_entries_that_never_run_are_exactly_the_unreachable_list(gpu, request):
    """spec mode: a catalog entry's kernel ran (under its own name, for every variant: the family cases assert that) or the entry
    is in UNREACHABLE with its reason — nothing else, and nothing listed there ran.  interp mode: no specialised kernel ran."""
    from rust_dataframe_amd import lib
    mode = request.node.callspec.params["gpu"]
    for family in M.FAMILIES:       # (already swept when the whole file runs; swept here when this test is selected alone)
        _sweep(gpu, lib, family, mode)
    if mode == "interp":
        assert all(k.startswith("eval_kernel<") for k in _RAN["interp"]), sorted(_RAN["interp"])[:5]
        return
    never = {e.sig for e in M.ENTRIES if "spec_kernel<" + e.sig + ">" not in _RAN["spec"]}
    assert never == set(M.UNREACHABLE), f"never ran but not listed: {sorted(never - set(M.UNREACHABLE))[:10]}; listed but ran: {sorted(set(M.UNREACHABLE) - never)}"
