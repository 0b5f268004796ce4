"""The LDS layout of the covariance kernel (bundletrack_amd/csrc/btba_marginals_layout.hpp), which the kernel carves its pointers out of and
the host sizes the launch with: a header without HIP, checked on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bundletrack_amd", "csrc", "btba_marginals_layout.hpp")


def test_layout_header_needs_no_hip():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", HEADER])


def test_layout_regions_alignment_and_budget_under_sanitizers(tmp_path):
    """tests/cpp/marginals_host.cpp built with AddressSanitizer and UBSan: for every window of 2 ... 31 frames the regions follow each other
    without overlap on 8-byte boundaries, the total is what the host asks for and at most 160 KB, the packed triangle gives every entry a
    slot of its own, and the row starts of 32 neighbouring lanes fall into 32 different bank pairs."""
    exe = str(tmp_path / "marginals_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           os.path.join(ROOT, "tests", "cpp", "marginals_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert run.stdout.strip() == "checked 30 layouts", run.stdout
