"""Builds tests/cpp/test_utf8_pattern_host.cpp — rust_dataframe_amd/csrc/rdf_utf8_pattern.h under plain g++ with
-fsanitize=address,undefined, no HIP, no GPU, no Python in the process — and runs it over the table tests/utf8_pred_ref.py
writes: 10^5 random (pattern, row) pairs, the edge-case lists, patterns of 32 / 33 segments and of 1024 / 1025 bytes, the bad
escapes, comparisons, counts and locate.  The functions it checks are the ones the kernels run on their lane-per-row path."""
import os
import subprocess
import tempfile

import utf8_pred_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_pattern_header_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_utf8_pattern_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_utf8_pattern_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    assert R.write_host_table(cases) >= 100_000
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert " 0 failed" in p.stdout
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
    os.remove(cases)
    os.remove(exe)
