"""The LDS layout of the general system solve (bundletrack_amd/csrc/btba_solve_layout.hpp), which the kernel carves its pointers out of and
the host sizes the launch with: a header without HIP, checked on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bundletrack_amd", "csrc", "btba_solve_layout.hpp")


def test_layout_header_needs_no_hip():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", HEADER])


def test_layout_sizes_and_alignment_under_sanitizers(tmp_path):
    """tests/cpp/solve_layout_host.cpp built with AddressSanitizer and UBSan: for every window of 2 ... 85 frames and 0, 1, P and 2 P dense
    pairs the struct's rest_floats is the closed form the host used to write out, every region read with 16-byte accesses is 16-byte
    aligned, and every region starts exactly where the one before it ends, for the matrix in LDS and in the global scratch."""
    exe = str(tmp_path / "solve_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           os.path.join(ROOT, "tests", "cpp", "solve_layout_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert run.stdout.strip() == f"checked {84 * 4 * 2} layouts", run.stdout
