"""Builds and runs tests/cpp/test_sort_plan.cpp: the top-bits decision of a numeric sort column (csrc/rdf_sort_plan.h, the
function os_column_passes calls) as a stand-alone host program — no library, no GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sort_plan_cpp():
    out = os.path.join(tempfile.gettempdir(), f"rdf_test_sort_plan_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_sort_plan.cpp"), "-o", out])
    try:
        p = subprocess.run([out], cwd=ROOT, capture_output=True, text=True, timeout=120)
    finally:
        os.remove(out)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 failed" in p.stdout
