"""The ulp bounds the float kernels are held to: max |error| in ulps of the exact value (tests/exact_ref.py), per (op, dtype).
Shared by test_float_accuracy_gpu.py (which measures them at the hard arguments) and test_spec_catalog.py."""
from rust_dataframe_amd import _abi as A

F64, F32 = A.F64, A.F32

DEFAULT_ULP = 4.0
BOUND = {
    ("sin", F64): 2.5, ("cos", F64): 2.5, ("tan", F64): 4.0,
    ("csc", F64): 3.5, ("sec", F64): 3.5, ("cot", F64): 5.0,          # 1 / base: the base's bound + 1
    ("sin", F32): 2.0, ("cos", F32): 2.0,
    ("csc", F32): 3.0, ("sec", F32): 3.0, ("cot", F32): DEFAULT_ULP + 1,   # f32 tan is the device libm's tanf
    # IEEE-exact operations
    ("abs", F64): 0.0, ("ceil", F64): 0.0, ("floor", F64): 0.0, ("round", F64): 0.0, ("sqrt", F64): 0.5,
    ("abs", F32): 0.0, ("ceil", F32): 0.0, ("floor", F32): 0.0, ("round", F32): 0.0, ("sqrt", F32): 0.5,
    # measured 4.115: log(x, base) = logf(x) / logf(base), two rounded logs and a rounded quotient in f32
    ("log", F32): 4.25,
}


def bound(op, dt):
    return BOUND.get((op, dt), DEFAULT_ULP)
