"""Builds and runs tests/cpp/test_window_range.cpp: WindowSpec::range_by and DataFrame::with_window_agg over RANGE frames with
value offsets in the C++ mirror (include/rdf_frame.hpp), on the device — sums, counts, averages, first value and one-sided max /
min over the committed CSV with Float64 `lat` and an Int64 row number as order keys, answers from tests/window_range_ref.py;
range_by on a text order column throws.  Same recipe as tests/test_window_agg_cpp.py."""
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


def test_window_range_mirror_builds():
    assert os.path.exists(build("test_window_range"))


@pytest.mark.gpu
def test_window_range_mirror_cpp():
    exe = build("test_window_range")
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "uk_cities_with_headers.csv")], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 failed" in p.stdout
