"""Pool records and the select kernel's LDS layout of the device keyframe memory (bundletrack_amd/csrc/btba_keyframes_layout.hpp) and its
distance functions (btba_keyframes_point.hpp): headers without HIP, checked on the CPU under the host sanitizers."""
import os
import subprocess

import numpy as np

import keyframes_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bundletrack_amd", "csrc")
SANITIZE = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"]


def test_headers_need_no_hip():
    for h in ("btba_keyframes_layout.hpp", "btba_keyframes_point.hpp"):
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, h)])


def test_pool_and_lds_layout_under_sanitizers(tmp_path):
    """tests/cpp/keyframes_host.cpp built with AddressSanitizer and UBSan: regions disjoint, aligned and inside the stated size, the LDS limit
    holds, sizes outside the limits are refused."""
    exe = str(tmp_path / "keyframes_host")
    subprocess.check_call(SANITIZE + [os.path.join(ROOT, "tests", "cpp", "keyframes_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    assert run.stdout.strip() == "checked 16 layouts", run.stdout


def test_header_functions_give_the_restatements_bits(tmp_path):
    """tests/cpp/keyframes_point.cpp under the same sanitizers: keyframes_acosf, keyframes_degrees and keyframes_tmp of the host compiler on a
    fixed argument list, bit for bit the numpy restatement's."""
    exe = str(tmp_path / "keyframes_point")
    subprocess.check_call(SANITIZE + [os.path.join(ROOT, "tests", "cpp", "keyframes_point.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    rows = [l.split() for l in run.stdout.splitlines()]
    a = np.array([[int(w, 16) for w in r[1:]] for r in rows if r[0] == "a"], np.uint32)
    t = np.array([[int(w, 16) for w in r[1:]] for r in rows if r[0] == "t"], np.uint32)
    assert len(a) == 4 + 5 * 64 + 2049 + 4096 and len(t) == 512
    arg = a[:, 0].copy().view(np.float32)
    d = G.acosf(arg)
    assert np.array_equal(d.view(np.uint32), a[:, 1]), np.nonzero(d.view(np.uint32) != a[:, 1])[0][:10]
    assert np.array_equal(G.degrees(d).view(np.uint32), a[:, 2])
    A, B = t[:, :16].copy().view(np.float32), t[:, 16:32].copy().view(np.float32)
    assert np.array_equal(G.tmp(A, B).view(np.uint32), t[:, 32])
    assert d[0] == 0.0 and d[1] == np.float32(np.pi) and d[2] == d[3] == np.float32(np.pi / 2)
