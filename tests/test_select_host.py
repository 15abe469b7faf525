"""Builds tests/cpp/test_select_host.cpp — rust_dataframe_amd/csrc/rdf_select.h under plain g++ with
-fsanitize=address,undefined, no HIP, no GPU, no Python in the process — and runs it over the table tests/select_ref.py
writes: per dtype at least 10^4 random rows of 1..8 parts with random NULLs through coalesce, greatest and least, as many
through case_when of 1..8 branches, every ordered pair and triple of the dtype's edge values (the extremes, +-0, +-inf,
NaNs of different payloads), and nanvl for the two float types."""
import os
import re
import subprocess
import tempfile

import select_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_select_header_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_select_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_select_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    assert R.write_host_table(cases) >= 10 * 20_000
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert " 0 failed" in p.stdout
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r" (\w+) (\d+)", p.stdout.split("rows:")[1].splitlines()[0])}
    for name in R.DTYPES:
        assert counts[f"X_{name}"] >= 10_000 and counts[f"W_{name}"] >= 10_000, counts
    for name in R.FLOATS:
        assert counts[f"N_{name}"] >= 10_000, counts
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
    os.remove(cases)
    os.remove(exe)
