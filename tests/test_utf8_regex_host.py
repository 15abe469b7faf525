"""Builds tests/cpp/test_utf8_regex_host.cpp — rust_dataframe_amd/csrc/rdf_utf8_regex.h, compiler and stepping, under plain
g++ with -fsanitize=address,undefined, no HIP, no GPU, no Python in the process — and runs it over the table
tests/utf8_regex_ref.py writes: the hand-written patterns and over 2 000 generated ones, over 10^5 (pattern, row) pairs with
broken UTF-8 among the rows, every refused construct with its position, and the patterns that must hit a cap or be right:
the hand-written blow-ups and the six generated patterns the model lists by name.  Every other pattern must compile."""
import os
import re
import subprocess
import tempfile

import utf8_regex_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_regex_header_on_the_host_under_sanitizers():
    exe = os.path.join(tempfile.gettempdir(), f"rdf_test_utf8_regex_host_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "test_utf8_regex_host.cpp"), "-o", exe])
    cases = exe + "_cases.txt"
    npat, npairs = R.write_host_table(cases)
    assert npat >= 2000 and npairs >= 100_000
    p = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert " 0 failed" in p.stdout
    pats, pairs, refused, capped = [int(x) for x in re.search(r"(\d+) patterns, (\d+) pairs, (\d+) refusals, (\d+) capped", p.stdout).groups()]
    assert pats + capped == npat and pats >= 2000 and capped <= len(R.CAP_OR_RIGHT) + len(R.GENERATED_PAST_A_CAP) and pairs >= 100_000 and refused == len(R.HAND_REFUSED)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    assert subprocess.run([exe], capture_output=True).returncode == 2          # it takes exactly one argument
    os.remove(cases)
    os.remove(exe)
