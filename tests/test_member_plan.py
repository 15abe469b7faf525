"""Builds and runs tests/cpp/test_member_plan.cpp: table size and route of rdf_member_mask / rdf_first_occurrence
(csrc/rdf_member_plan.h) as a stand-alone host program — no library, no GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_member_plan_cpp():
    out = os.path.join(tempfile.gettempdir(), f"rdf_test_member_plan_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_member_plan.cpp"), "-o", out])
    try:
        p = subprocess.run([out], cwd=ROOT, capture_output=True, text=True, timeout=120)
    finally:
        os.remove(out)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 failed" in p.stdout
