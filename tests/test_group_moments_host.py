"""Builds tests/cpp/test_group_moments_host.cpp — rust_dataframe_amd/csrc/rdf_group_moments_plan.h and rdf_moments_math.h
under plain g++ with -fsanitize=address,undefined -ffp-contract=off, no HIP, no GPU, no Python in the process — and runs it
over the table tests/group_moments_ref.py writes: the level plan at the row counts where a level is added, every statistic of
empty, one-row, constant, ill-conditioned and NaN states, merges, and whole folds (group sizes around the wave and the tile,
rows that do not count, a constant group, a group without a counted row, boundaries around a tile, three levels), each
reproduced bit for bit by the serial emulation."""
import os
import re
import subprocess
import tempfile

import group_moments_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_group_moments_headers_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_group_moments_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_group_moments_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    written = R.write_host_table(cases)
    assert written["L"] >= 10 and written["S"] >= 7 * 40 and written["Q"] >= 3 * 40 and written["M"] >= 100 and written["F"] >= 15
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
