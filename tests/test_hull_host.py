"""The dead-block test of the dense block walk (bundletrack_amd/csrc/btba_hull.hpp: a header without HIP that the kernel includes), compiled for
the host and held to fp64 references by tests/cpp/hull_host.cpp: random relative poses (rotations up to 0.6 rad, translations up to 0.3 m), random
intrinsics near the project's, caches of 16 x 16, 24 x 16 and 160 x 120, block depth ranges including empty, degenerate and full-range ones.

Observed (the program's seed is fixed): 19000 blocks, 12359 live, 6641 dead (3836 of them with a non-empty depth range), 2209536 pixel-depth
samples of dead blocks projected in fp64 with 0 inside the target image; 0 blocks with an fp64 form within 1e-4 of zero (the bar: below 0.1 % of
the blocks) and 0 verdicts that differ from the four-corner evaluation in fp64."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bundletrack_amd", "csrc", "btba_hull.hpp")
SOURCE = os.path.join(ROOT, "tests", "cpp", "hull_host.cpp")


def test_hull_header_needs_no_hip():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", HEADER])


def test_hull_verdicts_against_fp64_under_sanitizers(tmp_path):
    """Check 1: no pixel of a dead block, at both ends of its depth range and 7 depths inside, lies in the target image (fp64 per-pixel projection):
    zero violations.  Check 2: the separable verdict equals the four-corner verdict of the forms in fp64 wherever no fp64 form lies within 1e-4 of
    zero, and fewer than 0.1 % of the blocks are such exceptions.  Check 3: a corner at or behind the camera plane keeps the block, a NaN anywhere in
    the pose keeps it, and without ranges every block is live.  Built with AddressSanitizer and UBSan."""
    exe = str(tmp_path / "hull_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           SOURCE, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and run.stderr == "", run.stdout + run.stderr
    m = re.search(r"blocks (\d+) live (\d+) dead (\d+) \(non-empty range: (\d+)\) pixel-depth samples (\d+) violations (\d+) exceptions (\d+) mismatches (\d+)", run.stdout)
    assert m, run.stdout
    blocks, live, dead, dead_nonempty, samples, violations, exceptions, mismatches = map(int, m.groups())
    assert blocks >= 10000 and live + dead == blocks and samples == dead_nonempty * 64 * 9
    assert 20 * dead_nonempty >= blocks and 20 * live >= blocks          # both verdicts are exercised
    assert violations == 0
    assert mismatches == 0
    assert 1000 * exceptions < blocks
    assert "check 3: behind 6/6 plane 6/6 side 0/6 nan 78/78 no-ranges 6/6" in run.stdout
    assert run.stdout.strip().endswith("ok")
