"""Builds tests/cpp/test_datetime_host.cpp — rust_dataframe_amd/csrc/rdf_datetime.h under plain g++, no HIP and no GPU — and
runs it over the table of tests/golden/datetime_cases.npz (written by tests/datetime_ref.py, handed over as text): the
calendar arithmetic of the kernels round trips on three whole eras, on both ends of Int32 and on a walk across all of it,
and gives the table's fields, truncations and shifts."""
import os
import subprocess
import tempfile

import datetime_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_calendar_header_on_the_host():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_datetime_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_datetime_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    R.write_table_text(cases)
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 failed" in p.stdout
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
