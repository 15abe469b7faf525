"""Builds tests/cpp/test_window_range_host.cpp — rust_dataframe_amd/csrc/rdf_window_range.h under plain g++ with
-fsanitize=address,undefined, no HIP, no GPU, no Python in the process — and runs it over the table tests/window_range_ref.py
writes: every (start / end, PRECEDING / FOLLOWING) search of every ordinary row of partitions that hold INT64_MIN, INT64_MAX and
INT32_MIN keys with offsets 1, 2^62 and 2^63 - 1, +-inf, +-0.0, subnormal and 0.1 / 0.2 / 0.3 keys with offsets down to one
subnormal and up to the largest double, NaN prefixes and NULL suffixes, both directions, and random partitions with peers.
The expected positions come from the model's direct predicate; a signed overflow in the bound arithmetic shows up here."""
import os
import subprocess
import tempfile

import window_range_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_window_range_header_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_window_range_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_window_range_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    written = R.write_host_table(cases)
    assert written >= 5000
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert " 0 failed" in p.stdout
    assert f"rows: {written}\n" in p.stdout
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
    os.remove(cases)
    os.remove(exe)
