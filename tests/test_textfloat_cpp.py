"""Builds and runs tests/cpp/test_textfloat.cpp: Float32 / Float64 to and from text in the C++ mirror (include/rdf_frame.hpp) —
ScalarFunctions::cast between Utf8 and the float types, Column::cast_text, Column::utf8_parse_float / utf8_format_float, held to
literals taken from the model.  Same recipe as tests/test_textconv_cpp.py."""
import os
import subprocess
import tempfile

import pytest

import textfloat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust_dataframe_amd")


def build(name):
    out = os.path.join(tempfile.gettempdir(), f"rdf_{name}_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", out, "-L", PKG, "-lrdf_mi355x",
                           f"-Wl,-rpath,{PKG}"])
    return out


def test_textfloat_mirror_builds_and_its_literals_are_the_models():
    assert os.path.exists(build("test_textfloat"))
    assert R.parse(b"123.456", False) == 0x405edd2f1a9fbe77 and R.parse(b"123.456", True) == 0x42f6e979
    assert R.parse(b"2.50", False) == 0x4004000000000000 and R.parse(b"1e-3", False) == 0x3f50624dd2f1a9fc and R.parse(b"1e-3", True) == 0x3a83126f
    assert R.parse(b"9007199254740993.0000000000000000000000000000001", False) == 0x4340000000000001
    assert R.fmt(1, False) == b"4.9E-324" and R.fmt(1, True) == b"1.4E-45" and R.fmt(0x3fd3333333333334, False) == b"0.30000000000000004"


@pytest.mark.gpu
def test_textfloat_mirror_cpp():
    exe = build("test_textfloat")
    p = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 failed" in p.stdout
