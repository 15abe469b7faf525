"""tests/list_ref.py (the model of the twelve List entry points) and the CPU oracle pinned to each other on the whole case
table of tests/list_cases.py, for all ten child dtypes and bit for bit, before any GPU is involved; and the model held to the
reference's known answers that tests/test_list_functions.py lists.  Where the two disagreed the header's contract decided:
the oracle's max / min now order -0.0 below +0.0 like the sort does (it used to return whichever zero came first)."""
import numpy as np
import pytest

import list_cases as LC
import list_ref as R
import test_list_functions as T
from rust_dataframe_amd import _abi as A


class ModelApi:
    """tests/list_ref.py behind the call layer of the product and the oracle (host lists in, host arrays out)."""

    @staticmethod
    def _parts(lst):
        off = lst.offsets[lst.offset:lst.offset + lst.length + 1].astype(np.int64)
        valid = A.unpack_bits(lst.validity, lst.offset, lst.length) if lst.validity is not None else None
        return off, valid, lst.values.to_numpy()

    @staticmethod
    def _pair(off, vals):
        return A.HostArray.from_numpy(off.astype(np.int32)), A.HostArray(vals if len(vals) else np.zeros(1, vals.dtype), None, 0, len(vals), A.dtype_code(vals.dtype), 0)

    def list_contains(self, lst, value):
        has, ok, _ = R.find(*self._parts(lst), value)
        return A.HostArray.from_numpy(has, ok)

    def list_position(self, lst, value):
        return A.HostArray.from_numpy(R.find(*self._parts(lst), value)[2])

    def list_extreme(self, lst, want_max):
        v, ok, _ = R.extreme(*self._parts(lst), want_max)
        return A.HostArray.from_numpy(v, ok)

    def list_remove(self, lst, value):
        return self._pair(*R.remove(*self._parts(lst), value))

    def list_sort(self, lst):
        v = R.sort(*self._parts(lst))
        return A.HostArray(v if len(v) else np.zeros(1, v.dtype), None, 0, len(v), A.dtype_code(v.dtype), 0)

    def list_set(self, op, lst, other=None, count=0):
        ob, _, cb = self._parts(other) if other is not None else (None, None, None)
        return self._pair(*R.set_op(op, *self._parts(lst), ob, cb, count))


def test_model_reference_known_answers():
    T.check_reference_answers(ModelApi())


def test_model_set_known_answers():
    T.check_set_known_answers(ModelApi())


@pytest.mark.parametrize("name,dtname", LC.cases_of("reduce", "set", "sort"))
def test_oracle_against_model(ora, name, dtname):
    for form in LC.built(name, dtname).forms() if LC.CASES[name]["group"] != "sort" else (None,):
        LC.check_case(ora, name, dtname, form)


@pytest.mark.parametrize("dtname", list(LC.DTYPES))
@pytest.mark.parametrize("name", LC.LAYOUT_CASES)
def test_oracle_against_model_behind_offsets(ora, name, dtname):
    LC.check_case(ora, name, dtname, layout="offsets")


@pytest.mark.parametrize("dtname", list(LC.DTYPES))
def test_oracle_against_model_row_offsets_and_zero_rows(ora, dtname):
    for ro in (1, 7, 67):
        LC.check_case(ora, "rows129", dtname, row_offset=ro)
    for with_validity in (False, True):
        LC.check_zero_rows(ora, dtname, with_validity)
        LC.check_zero_rows(ora, dtname, with_validity, layout="offsets")


@pytest.mark.parametrize("dtype", [A.F32, A.F64])
def test_oracle_set_functions_against_model_floats(ora, dtype):
    """The float half of test_oracle_set_functions_against_python: the same random rows (NaNs among them), the model in
    place of the Python lists, bit for bit."""
    rng = np.random.default_rng(77)
    model = ModelApi()
    a_rows, b_rows = T.random_lists(rng, dtype, 300, 9, 0.1), T.random_lists(rng, dtype, 300, 7, 0.1)
    la, lb = A.HostList.from_lists(a_rows, dtype, row_offset=2), A.HostList.from_lists(b_rows, dtype)
    for op in LC.SET_OPS:
        other = lb if op in ("except", "intersect", "union") else None
        (go, gv), (wo, wv) = ora.list_set(op, la, other, count=3), model.list_set(op, la, other, count=3)
        assert np.array_equal(go.to_numpy(), wo.to_numpy()) and gv.length == wv.length, f"{op} dtype={dtype}"
        assert np.array_equal(gv.to_numpy().view(np.uint8), wv.to_numpy().view(np.uint8)), f"{op} dtype={dtype}"
