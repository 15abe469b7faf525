"""Builds and runs tests/cpp/test_group_moments.cpp: Evaluate::group_moments / group_comoments and the GroupAggregate step's
Variance / StdDev / Skewness / Kurtosis arms in the C++ mirror (include/rdf_frame.hpp), on the device, against values worked
out in the test.  Same recipe as tests/test_group_sorted_cpp.py."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust_dataframe_amd")


def build(name):
    out = os.path.join(tempfile.gettempdir(), f"rdf_{name}_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", out, "-L", PKG, "-lrdf_mi355x",
                           f"-Wl,-rpath,{PKG}"])
    return out


def test_group_moments_mirror_builds():
    assert os.path.exists(build("test_group_moments"))


@pytest.mark.gpu
def test_group_moments_mirror_cpp():
    exe = build("test_group_moments")
    p = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 failed" in p.stdout
