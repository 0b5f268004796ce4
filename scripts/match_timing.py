"""Timing of btba_match_pairs (descriptor kNN + gate) at three sizes, one JSON line.  GPU box only.
    python scripts/match_timing.py              hipEvent time per call, and the same cases under rocprofv3 --kernel-trace --stats
                                                (each case in a fresh child process), next to the bounds below
    python scripts/match_timing.py --no-rocprof hipEvent times only
Cases: the tracker call (new frame against 14 others, 500 keypoints, D 256, mutual), a window rebuild (all 105 pairs of 15 frames),
a batch of 32 windows x 105 pairs (the windows share one scene's data).  Bounds printed next to each time:
  mfma_bound_us : 2 nA nB D flop per pair and direction at the fp32 MFMA peak of an MI355X (157.3 TFLOP/s)
  cpu_numpy_ms  : brute force in numpy on the same data (BLAS d2 + argpartition top-k, both directions), the stand-in for the
                  reference's NO_OPENCV_CUDA path; the batch case is timed on one window and scaled by 32."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

N_KPTS, D, PEAK = 500, 256, 157.3e12


def scene():
    from bundletrack_amd import synthetic as S
    pb = S.make_problem(15, 10, seed=5, background=False)
    kp = S.make_keypoints(pb, 1200, 100, D=D, seed=5)
    rng = np.random.default_rng(5)
    kpts, desc = [], []
    for k in range(15):
        keep = rng.permutation(len(kp.kpts[k]))[:N_KPTS]
        kpts.append(kp.kpts[k][keep]); desc.append(kp.desc[k][keep])
    return pb, kpts, desc


def cases():
    win = [(a, b) for a in range(15) for b in range(a)]
    return {"tracker": (1, [(14, b) for b in range(14)]), "window": (1, win),
            "batch": (32, [(15 * w + a, 15 * w + b) for w in range(32) for a, b in win])}


def frames_on_gpu(pb, kpts, desc, n_windows):
    import torch
    from bundletrack_amd.bundler import FrameRef
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    base = [dict(kpts_gpu=t(kpts[k]), desc_gpu=t(desc[k]), depth_gpu=t(pb.depth[k]), normal_gpu=t(pb.normals[k])) for k in range(15)]
    return [FrameRef(id=1000 * w + k, pose_in_model=pb.poses_gt[k].astype(np.float32), **base[k]) for w in range(n_windows) for k in range(15)]


def event_ms(name, reps):
    import torch
    from bundletrack_amd.matching import match_pairs
    from bundletrack_amd.optimizer import Workspace
    pb, kpts, desc = scene()
    n_windows, pairs = cases()[name]
    frames = frames_on_gpu(pb, kpts, desc, n_windows)
    ws = Workspace()
    for _ in range(3):
        res = match_pairs(ws, frames, pairs, K=pb.K, H=pb.H, W=pb.W)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record()
        match_pairs(ws, frames, pairs, K=pb.K, H=pb.H, W=pb.W)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), int(res.n_out.sum()), pb, kpts, desc


def cpu_numpy_ms(kpts, desc, pairs, k=5):
    t0 = time.perf_counter()
    for a, b in pairs:
        A, B = desc[a % 15].astype(np.float32), desc[b % 15].astype(np.float32)
        d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)
        for M in (d2, d2.T):
            idx = np.argpartition(M, k, axis=1)[:, :k]
            np.take_along_axis(M, idx, 1).argsort(1)
    return (time.perf_counter() - t0) * 1e3


def rocprof_us(name, reps):
    """Kernel time per call of the k_match_* kernels, from rocprofv3 --kernel-trace --stats of a fresh child process."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "match", "--", sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(reps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise RuntimeError(f"no kernel stats from rocprofv3 in {sorted(glob.glob(os.path.join(d, '**'), recursive=True))}")
        total_ns = calls = 0
        per = {}
        for row in csv.DictReader(open(stats[0])):
            if "k_match" in row["Name"]:
                ns = float(row["TotalDurationNs"])
                total_ns += ns
                calls = max(calls, int(row["Calls"]))
                per[row["Name"].split("(")[0].split("::")[-1]] = round(ns / int(row["Calls"]) / 1e3, 2)
        return total_ns / max(calls, 1) / 1e3, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:                                   # under rocprofv3: warm-up + reps calls of one case, no output
        event_ms(a.child, a.reps)
        return
    out = {"what": "btba_match_pairs", "n_kpts": N_KPTS, "D": D, "cases": {}}
    for name, (n_windows, pairs) in cases().items():
        ms, n_matches, pb, kpts, desc = event_ms(name, a.reps)
        flop = 2 * 2 * N_KPTS * N_KPTS * D * len(pairs)          # both directions
        one = cases()["window"][1] if name == "batch" else pairs
        cpu = cpu_numpy_ms(kpts, desc, one) * (32 if name == "batch" else 1)
        row = {"pairs": len(pairs), "event_us": round(ms * 1e3, 1), "mfma_bound_us": round(flop / PEAK * 1e6, 1),
               "mfma_bound_one_direction_us": round(flop / 2 / PEAK * 1e6, 1), "cpu_numpy_ms": round(cpu, 2), "matches": n_matches}
        if not a.no_rocprof:
            us, per = rocprof_us(name, a.reps)
            row["rocprof_kernel_us"], row["rocprof_per_kernel_us"] = round(us, 1), per
        out["cases"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
