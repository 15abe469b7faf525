"""Builds tests/cpp/test_textconv_host.cpp — rust_dataframe_amd/csrc/rdf_textconv.h under plain g++ with
-fsanitize=address,undefined, no HIP, no GPU, no Python in the process, nothing preloaded — and runs it over the table
tests/textconv_ref.py writes: at least 10^5 rows per kind and direction, every grammar branch, the long rows, every pattern.
Every text is parsed out of an exactly sized heap block and every row is written into one."""
import os
import re
import subprocess
import tempfile

import textconv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_textconv_header_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_textconv_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_textconv_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    written = R.write_case_table(cases)
    assert all(n >= 100_000 for n in written.values()) and len(written) == 8, written
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert " 0 failed" in p.stdout
    m = re.search(r"parse: bool (\d+), int (\d+), date (\d+), timestamp (\d+) rows; format: bool (\d+), int (\d+), date (\d+), timestamp (\d+) rows", p.stdout)
    counts = [int(x) for x in m.groups()]
    assert counts == [written[(d, k)] for d in "PF" for k in range(4)], (counts, written)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
    os.remove(cases)
    os.remove(exe)
