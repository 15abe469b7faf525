"""Builds tests/cpp/test_utf8_rewrite_host.cpp — rust_dataframe_amd/csrc/rdf_utf8_rewrite.h under plain g++ with
-fsanitize=address,undefined, no HIP, no GPU, no Python in the process — and runs it over the table tests/utf8_rewrite_ref.py
writes: 10^5 random rows per op, long rows, self-overlapping needles, needles longer than a wave's window, broken UTF-8.
Every output byte is produced through the scanner, the window selection, the translate table and the emit functions the
kernels call, in the lane's form and in the wave's."""
import os
import re
import subprocess
import tempfile

import utf8_rewrite_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rewrite_header_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_utf8_rewrite_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_utf8_rewrite_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    assert R.write_host_table(cases) >= 400_000
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert " 0 failed" in p.stdout
    counts = [int(x) for x in re.search(r"replace (\d+), translate (\d+), initcap (\d+), split (\d+) rows", p.stdout).groups()]
    assert all(c >= 100_000 for c in counts), counts
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
    os.remove(cases)
    os.remove(exe)
