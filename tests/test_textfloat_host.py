"""Builds tests/cpp/test_textfloat_host.cpp — rust_dataframe_amd/csrc/rdf_textfloat.h under plain g++ with
-fsanitize=address,undefined, no HIP, no GPU, no Python in the process, nothing preloaded — and runs it over the table
tests/textfloat_ref.py writes: at least 10^5 rows per direction and dtype, every hard case and long row.  Every text is parsed
out of an exactly sized heap block, by the default routing and by the exact path alone; every row is written into one."""
import os
import re
import subprocess
import tempfile

import textfloat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_textfloat_header_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_textfloat_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_textfloat_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    written = R.write_case_table(cases)
    assert all(n >= 100_000 for n in written.values()) and len(written) == 4, written
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert " 0 failed" in p.stdout
    m = re.search(r"parse: f64 (\d+), f32 (\d+) rows; format: f64 (\d+), f32 (\d+) rows", p.stdout)
    counts = [int(x) for x in m.groups()]
    assert counts == [written[(d, f32)] for d in "PF" for f32 in (False, True)], (counts, written)
    # the share of undecided rows per family is printed (DESIGN §30 records it); the hard cases do reach the exact path
    und = {(m.group(1), m.group(2)): int(m.group(3)) for m in re.finditer(r"undecided (f\d\d) (\w+): (\d+) of", p.stdout)}
    assert len(und) == 12 and und[("f64", "hard")] >= 40 and und[("f32", "hard")] >= 10, und
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
    os.remove(cases)
    os.remove(exe)
