"""Voxel offsets, compaction blocks and scratch layout of keyframe fusion (bundletrack_amd/csrc/btba_fusion_layout.hpp), which the kernels index
their planes with and the host sizes the scratch with: a header without HIP, checked on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bundletrack_amd", "csrc", "btba_fusion_layout.hpp")


def test_layout_header_needs_no_hip():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", HEADER])


def test_offsets_cap_and_scratch_under_sanitizers(tmp_path):
    """tests/cpp/fusion_host.cpp built with AddressSanitizer and UBSan: instances' voxel and block ranges disjoint and in order, planes disjoint,
    aligned and inside the stated size, empty instances own nothing, the cap holds per box and per call, sides near 2^31 do not wrap."""
    exe = str(tmp_path / "fusion_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           os.path.join(ROOT, "tests", "cpp", "fusion_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert run.stdout.strip() == "checked 15 layouts", run.stdout
