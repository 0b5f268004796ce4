"""The LDS layout of a dense sweep item on the compact cache (bundletrack_amd/csrc/btba_sweep_layout.hpp), which the kernels carve their
pointers out of and the host sizes the launches with: a header without HIP, checked on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bundletrack_amd", "csrc", "btba_sweep_layout.hpp")


def test_layout_header_needs_no_hip():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", HEADER])


def test_layout_sizes_order_alignment_and_band_limit_under_sanitizers(tmp_path):
    """tests/cpp/sweep_layout_host.cpp built with AddressSanitizer and UBSan: for every cache with width and height multiples of 8 and
    width + height <= 1024, at 1, 2, 3 and 7 tiles and for the three kinds of item, `total` is the closed form the host used to write out,
    the regions follow one another without overlap or gap, colA, rowB and hull are 16-byte aligned, and a band of more than
    kMaxBandBlocks blocks is reported as "no block walk" and sized as row strips."""
    exe = str(tmp_path / "sweep_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           os.path.join(ROOT, "tests", "cpp", "sweep_layout_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    caches = sum(128 - k for k in range(1, 128))          # width 8 k, height 8 j, k + j <= 128
    assert run.stdout.strip() == f"checked {caches * 4 * 3} layouts", run.stdout
