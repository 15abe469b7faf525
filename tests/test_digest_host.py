"""Builds tests/cpp/test_digest_host.cpp — rust_dataframe_amd/csrc/rdf_digest.h under plain g++ with
-fsanitize=address,undefined, no HIP, no GPU, no Python in the process — and runs it over the table tests/digest_ref.py
writes: every length 0..300 and 10^4 random rows per function, the row [nullptr, nullptr), rows of 4 KiB + 1, every dtype of
the fixed-width forms.  Every row sits in a heap block of exactly its length."""
import os
import re
import subprocess
import tempfile

import digest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_digest_header_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_digest_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_digest_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    assert R.write_host_table(cases) >= 9 * 10_300
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert " 0 failed" in p.stdout
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r" (\w+) (\d+)", p.stdout.split("rows:")[1].splitlines()[0])}
    assert set(R.FUNCTIONS) <= set(counts), counts
    assert all(counts[fn] >= 10_000 for fn in R.FUNCTIONS), counts
    assert counts["int"] >= 2 * len(R.DTYPES) * 200, counts
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
    os.remove(cases)
    os.remove(exe)
