"""The work split and scratch layout of the objective report (bundletrack_amd/csrc/btba_objective_layout.hpp), which the kernels index their
partial records with and the host sizes the scratch and the launches with: a header without HIP, checked on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bundletrack_amd", "csrc", "btba_objective_layout.hpp")


def test_layout_header_needs_no_hip():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", HEADER])


def test_tiles_chunks_and_scratch_under_sanitizers(tmp_path):
    """tests/cpp/objective_host.cpp built with AddressSanitizer and UBSan: tiles and chunks visit every pixel and entry once and nothing past the
    end (cache sizes 117 and 1500, segments of 0 and 1 entries among them), the scratch regions are disjoint, aligned and inside the stated size,
    every partial record has bytes of its own."""
    exe = str(tmp_path / "objective_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           os.path.join(ROOT, "tests", "cpp", "objective_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert run.stdout.strip() == "checked 192 layouts", run.stdout
