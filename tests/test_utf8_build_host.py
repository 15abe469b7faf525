"""Builds tests/cpp/test_utf8_build_host.cpp — rust_dataframe_amd/csrc/rdf_utf8_build.h under plain g++ with
-fsanitize=address,undefined, no HIP, no GPU, no Python in the process — and runs it over the table tests/utf8_build_ref.py
writes: 10^5 random rows per op, Spark's examples, long rows, broken UTF-8.  Every output byte is produced through the pad
plan, the piece function, the reverse map and the substring_index span the kernels call."""
import os
import re
import subprocess
import tempfile

import utf8_build_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_build_header_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_utf8_build_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_utf8_build_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    assert R.write_host_table(cases) >= 500_000
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert " 0 failed" in p.stdout
    counts = [int(x) for x in re.search(r"pad (\d+), repeat (\d+), reverse (\d+), substring_index (\d+), concat (\d+) rows", p.stdout).groups()]
    assert all(c >= 100_000 for c in counts), counts
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
    os.remove(cases)
    os.remove(exe)
