"""Builds and runs the C++ host-side mirror's tests (tests/cpp/*.cpp over include/rdf_frame.hpp).

test_plan: plan builders (src/operation/scalar.rs) — CPU only.
test_frame: the reference's #[test]s for the hot path restated in C++ and run on the device, plus the fused
            batch loop against the unfused oracle — GPU."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rust_dataframe_amd")
ORA = os.path.join(ROOT, "oracle")


def build(name, with_oracle):
    out = os.path.join(tempfile.gettempdir(), f"rdf_{name}_{os.getpid()}")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", ORA,
           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", out, "-L", PKG, "-lrdf_mi355x", f"-Wl,-rpath,{PKG}"]
    if with_oracle:
        if not os.path.exists(os.path.join(ORA, "librdf_oracle.so")):
            subprocess.check_call(["make", "-C", ORA, "-s"])
        cmd += ["-L", ORA, "-lrdf_oracle", f"-Wl,-rpath,{ORA}"]
    subprocess.check_call(cmd)
    return out


def run(exe, *args):
    p = subprocess.run([exe, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(p.stdout[-4000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-4000:]
    assert " 0 failed" in p.stdout


def test_plan_builders_cpp():
    run(build("test_plan", False))


def test_jit_signatures_cpp():
    """rdf_jit.cpp's host logic (signature -> template argument, refusals, code-object symbol lookup) — built with hipcc because the
    file includes the HIP runtime's headers; nothing in it touches a device."""
    out = os.path.join(tempfile.gettempdir(), f"rdf_test_jit_sig_{os.getpid()}")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "rust_dataframe_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_jit_sig.cpp"), "-o", out, "-ldl"])
    run(out)


def test_stage_copy_cpp():
    """packed_copy (csrc/rdf_stage_copy.h): host chunks into / out of the staging buffer, cut by bytes over threads — every staged byte
    exactly once, nothing else touched, for a handful of huge pieces, thousands of tiny batches, empty and unstaged items."""
    out = os.path.join(tempfile.gettempdir(), f"rdf_test_stage_copy_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_stage_copy.cpp"), "-o", out])
    run(out)


def test_stream_plan_cpp():
    """The host logic of the streamed batch loop (csrc/rdf_stream_plan.h: the planner, DownLayout, bits_append) on the CPU: over a
    few thousand seeded layouts the upload is emulated and every view read back — every row of every batch exactly once, in order,
    with its value and validity bit; items disjoint, staged in front and direct behind on 256-byte boundaries; merged runs only over
    contiguous memory; plan.max_* bound every slab.  bits_append against a per-bit loop at every phase pair."""
    out = os.path.join(tempfile.gettempdir(), f"rdf_test_stream_plan_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_stream_plan.cpp"), "-o", out])
    run(out)


SANITIZE = "-fsanitize=address,undefined"


def _sanitizer_links():
    """Can a trivial program be linked with the sanitizers' runtimes at all?"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        return subprocess.run(["g++", SANITIZE, src, "-o", os.path.join(d, "t")], capture_output=True).returncode == 0


@pytest.mark.parametrize("name", ["test_stream_plan", "test_stage_copy"])
def test_stream_host_code_under_sanitizers_cpp(name):
    """The same stand-alone programs (their own main, no library, nothing loaded into Python) built with AddressSanitizer and
    UndefinedBehaviorSanitizer: a byte read past a column's buffer, a copy past a staging buffer or a shift out of range ends the
    program."""
    if not _sanitizer_links():
        pytest.skip("g++ cannot link a program with " + SANITIZE)
    out = os.path.join(tempfile.gettempdir(), f"rdf_{name}_san_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", SANITIZE, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", out])
    run(out)


def test_sort_bucket_map_cpp():
    """The bucket map of Float64 sort keys (csrc/rdf_sort_map.h: the function the kernels run, under the planner the host runs) on
    the CPU: monotone over sorted columns of every shape and across every seam, inside its buckets, the fullest bucket inside the
    LDS finish; columns no map can split are refused by the plan."""
    out = os.path.join(tempfile.gettempdir(), f"rdf_test_sort_map_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_sort_map.cpp"), "-o", out])
    run(out)


def test_join_place_cpp():
    """The scan that lays out the equi-join's table of distinct build keys (csrc/rdf_join_place.h, the code the kernels run) on the CPU:
    run summaries combine associatively, tiles cut any way place every key where sequential linear probing would, a probe walking from a
    key's home slot meets no empty slot before the key."""
    out = os.path.join(tempfile.gettempdir(), f"rdf_test_join_place_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_join_place.cpp"), "-o", out])
    run(out)


def test_program_plan_cpp():
    """The launch policy of the program path (csrc/rdf_program_plan.h, the code run_program's phases call) on the CPU: blocks per CU,
    grid and tile walk of the specialised kernels for every kind of program and every pinned option, the grouped kernel's grid cap,
    the LDS copies of the interpreted grouped sink, the tile prefix and its 128-bit reciprocal — against figures written out from
    the rules."""
    out = os.path.join(tempfile.gettempdir(), f"rdf_test_program_plan_{os.getpid()}")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_program_plan.cpp"), "-o", out])
    run(out)


@pytest.mark.gpu
def test_frame_mirror_cpp():
    run(build("test_frame", True), os.path.join(ROOT, "tests", "golden", "uk_cities_with_headers.csv"),
        os.path.join(ROOT, "tests", "golden", "mixed_batches.arrow"))
