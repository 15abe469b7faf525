"""Builds tests/cpp/test_percentile_host.cpp — rust_dataframe_amd/csrc/rdf_percentile.h under plain g++ with
-fsanitize=address,undefined, no HIP, no GPU, no Python in the process — and runs it over the table tests/percentile_ref.py
writes: d(v) of every dtype at its extremes (Int64 / UInt64 beyond 2^53, the NaNs of other payloads, +-0) and at 2000
random bit patterns each, the rank rule and the DISC index at m = 1, 2, 3 .. 2^32 - 1 and p = 0, 1, 0.5, 1e-300, the largest
double below 1 and random p, the interpolation over pairs of edge values, the test of p, and the select route's decisions:
the ordered key of every dtype's edge and random values with the way back, the order of every pair of edge values (key order is
value order; -0.0 / +0.0 and the NaNs collapse), and the planner step on histograms with all mass in one bucket, ranks that
straddle a bucket edge, 16 ranks in 16 buckets, counters at their limit and ranks beyond the candidates."""
import os
import re
import subprocess
import tempfile

import percentile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_percentile_header_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_percentile_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_percentile_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    written = R.write_host_table(cases)
    assert written["D"] >= 10 * 2000 and written["R"] >= 20_000 and written["K"] == written["R"] and written["I"] >= 5000 and written["P"] >= 20
    assert written["Q"] >= 10 * 300 and written["O"] >= 10 * 400 and written["B"] >= 300
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert " 0 failed" in p.stdout
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r" (\w) (\d+)", p.stdout.split("rows:")[1].splitlines()[0])}
    assert counts == written, (counts, written)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
    os.remove(cases)
    os.remove(exe)
