"""The twelve rdf_list_* entry points on the MI355X against tests/list_ref.py, on the case table of tests/list_cases.py (which
says, case by case, which edge of rdf_list.hip it is built around).  Every comparison is for equality of bytes: values as
uint8 views, value_offsets, validity bits, null_count and length — only a max / min over nothing but NaNs may be any NaN.

Every case of find / extreme / remove / set that can take both kernel forms runs in both on the same rows (unreferenced child
elements behind the last row push values.length / rows across 48), and every call asserts rdf_last_kernel: a case that no
longer reaches the kernel it was built for fails.  The sort cases sit on both sides of total / rows = 24; both sides report
one kernel name, so there the case's own shape is asserted instead, and the radix fallback by its name.

Device memory: outputs are allocated exactly as the header says (bitmaps in whole 64-bit words) between guard bytes."""
import numpy as np
import pytest

import list_cases as LC
from rust_dataframe_amd import _abi as A
from rust_dataframe_amd import lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GUARD = 64


@pytest.fixture(scope="module")
def api():
    a = lib.api()
    if lib.device_count() < 1:
        pytest.fail("no GPU visible")
    lib.set_device(0)
    return a


class Dev:
    """Device-resident inputs and outputs for list_cases.run."""

    def __init__(self):
        self.outs = {}

    @staticmethod
    def _tensor(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).cuda()

    def put(self, lst):
        vt = self._tensor(lst.values.values)
        cv = self._tensor(lst.values.validity) if lst.values.validity is not None else None
        ot = self._tensor(lst.offsets)
        lv = self._tensor(lst.validity) if lst.validity is not None else None
        values = A.DeviceArray(vt.data_ptr(), cv.data_ptr() if cv is not None else None, lst.values.offset, lst.values.length,
                               lst.values.dtype, lst.values.null_count, keep=(vt, cv))
        return A.DeviceList(ot.data_ptr(), lst.length, values, lv.data_ptr() if lv is not None else None, lst.offset, keep=(ot, lv))

    def out(self, dtype, capacity, with_validity):
        words = (capacity + 63) // 64 * 8
        vbytes = words if dtype == A.BOOL else max(capacity, 1) * np.dtype(A.NP_OF[dtype]).itemsize
        vt = torch.full((GUARD + vbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        bt = torch.full((GUARD + words + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") if with_validity else None
        d = A.DeviceArray(vt.data_ptr() + GUARD, bt.data_ptr() + GUARD if bt is not None else None, 0, capacity, dtype, 0, keep=(vt, bt))
        self.outs[id(d)] = (vbytes, words)
        return d

    def fetch(self, d):
        vbytes, words = self.outs.pop(id(d))
        vt, bt = d.keep
        torch.cuda.synchronize()
        parts = []
        for t, nbytes in ((vt, vbytes), (bt, words)):
            if t is None:
                parts.append(None)
                continue
            h = t.cpu().numpy()
            assert (h[:GUARD] == 0xA5).all() and (h[GUARD + nbytes:] == 0xA5).all(), "bytes outside the output buffer were written"
            parts.append(h[GUARD:GUARD + nbytes].copy())
        values = parts[0] if d.dtype == A.BOOL else parts[0].view(A.NP_OF[d.dtype])
        return A.HostArray(values, parts[1], 0, d.length, d.dtype, d.null_count)


@pytest.mark.parametrize("name,dtname", LC.cases_of("reduce", "set"))
def test_both_forms(api, name, dtname):
    forms = LC.built(name, dtname).forms()
    assert forms == LC.CASES[name]["forms"]
    for form in forms:
        LC.check_case(api, name, dtname, form, last_kernel=lib.last_kernel)


@pytest.mark.parametrize("name,dtname", LC.cases_of("sort"))
def test_sort(api, name, dtname):
    assert LC.built(name, dtname).sort_form() == LC.CASES[name]["sort_form"]
    LC.check_case(api, name, dtname, last_kernel=lib.last_kernel)


@pytest.mark.parametrize("dtname", list(LC.DTYPES))
@pytest.mark.parametrize("name", LC.LAYOUT_CASES)
def test_behind_offsets(api, name, dtname):
    """A row offset of 3, a child values.offset of 5 and a child validity buffer full of zeros, which must be ignored."""
    LC.check_case(api, name, dtname, layout="offsets", last_kernel=lib.last_kernel)


@pytest.mark.parametrize("dtname", list(LC.DTYPES))
def test_row_offsets_and_zero_rows(api, dtname):
    for ro in (1, 7, 67):
        for form in ("lane", "wave"):
            LC.check_case(api, "rows129", dtname, form, row_offset=ro, last_kernel=lib.last_kernel)
    for with_validity in (False, True):
        for layout in ("plain", "offsets"):
            LC.check_zero_rows(api, dtname, with_validity, layout)
            LC.check_zero_rows(api, dtname, with_validity, layout, dev=Dev())


@pytest.mark.parametrize("dtname", list(LC.DTYPES))
@pytest.mark.parametrize("name", LC.LAYOUT_CASES)
def test_device_memory(api, name, dtname):
    """DeviceList inputs and RDF_MEM_DEVICE outputs: the model's result again, in the very bytes of the host call."""
    for layout in ("plain", "offsets"):
        host = LC.check_case(api, name, dtname, layout=layout, last_kernel=lib.last_kernel)
        dev = LC.check_case(api, name, dtname, layout=layout, last_kernel=lib.last_kernel, dev=Dev())
        assert host.keys() == dev.keys()
        for call, h in host.items():
            for k, v in h.items():
                if isinstance(v, np.ndarray):
                    assert np.array_equal(np.ascontiguousarray(v).view(np.uint8), np.ascontiguousarray(dev[call][k]).view(np.uint8)), (name, dtname, call[0], k)
                else:
                    assert v == dev[call][k], (name, dtname, call[0], k)


def test_repeat_past_int32_offsets(api):
    """array_repeat of 3-element rows 2^30 times: the count pass alone finds 3 * 2^30 > 2^31 - 1 elements a row ->
    RDF_COMPUTE_ERROR, and neither output is touched."""
    b = LC.Built(LC.LL([3, 3, 0, 3], None).fill(np.random.default_rng(1), np.arange(1, 9, dtype=np.int32)))
    la, _ = LC.materialise(b, A.I32, "lane")
    oo, ov = A.HostArray.empty_out(A.I32, 5, False), A.HostArray.empty_out(A.I32, 16, False)
    oo.values[:], ov.values[:] = -7, -7
    with pytest.raises(A.RdfError) as ei:
        api.list_set("repeat", la, count=1 << 30, outs=(oo, ov))
    assert ei.value.status == A.RDF_COMPUTE_ERROR
    assert (oo.values == -7).all() and (ov.values == -7).all()


@pytest.mark.parametrize("dtname", ["i8", "i32", "f64"])
def test_values_capacity_one_short(api, dtname):
    """rdf_list_sort and the set functions with room for one element less than the result -> RDF_MEMORY_ERROR."""
    code = LC.DTYPES[dtname]
    b = LC.built("sort_lane", dtname)
    la, _ = LC.materialise(b, code, None)
    need = LC.model(b, "sort")["length"]
    with pytest.raises(A.RdfError) as ei:
        api.list_sort(la, out=A.HostArray.empty_out(code, need - 1, False))
    assert ei.value.status == A.RDF_MEMORY_ERROR
    assert api.list_sort(la, out=A.HostArray.empty_out(code, need, False)).length == need
    b = LC.built("set_rows", dtname)
    for form in ("lane", "wave"):
        la, lb = LC.materialise(b, code, form)
        for op in LC.SET_OPS:
            need = LC.model(b, op, None, 3)["length"]
            other = lb if op in ("except", "intersect", "union") else None
            with pytest.raises(A.RdfError) as ei:
                api.list_set(op, la, other, count=3, outs=(A.HostArray.empty_out(A.I32, la.length + 1, False), A.HostArray.empty_out(code, need - 1, False)))
            assert ei.value.status == A.RDF_MEMORY_ERROR, op
            oo, ov = api.list_set(op, la, other, count=3, outs=(A.HostArray.empty_out(A.I32, la.length + 1, False), A.HostArray.empty_out(code, need, False)))
            assert ov.length == need, op
