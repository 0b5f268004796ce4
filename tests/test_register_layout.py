"""Point blocks, partial records and scratch layout of frame-to-model registration (bundletrack_amd/csrc/btba_register_layout.hpp), which the
kernels index the scratch with and the host sizes it with: a header without HIP, checked on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bundletrack_amd", "csrc", "btba_register_layout.hpp")


def test_layout_header_needs_no_hip():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", HEADER])


def test_blocks_records_and_scratch_under_sanitizers(tmp_path):
    """tests/cpp/register_host.cpp built with AddressSanitizer and UBSan: items' record ranges disjoint and in order, every point in exactly one
    (block, thread, slot) of the accumulate kernel's walk, regions disjoint, aligned and inside the stated size, empty items own nothing, the caps
    on points per item and records per call hold."""
    exe = str(tmp_path / "register_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           os.path.join(ROOT, "tests", "cpp", "register_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert run.stdout.strip() == "checked 12 layouts", run.stdout
