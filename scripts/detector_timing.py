"""Timing of the detector front end (btba_detector_inputs, btba_detector_keypoints_to_image) at 1 and 32 frames of 480 x 640,
out_size 400, one JSON line.  GPU box only.
    python scripts/detector_timing.py              hipEvent time per call, and the same cases under rocprofv3 --kernel-trace --stats
                                                   (each case in a fresh child process, one at a time, each under its own timeout)
    python scripts/detector_timing.py --no-rocprof hipEvent times only
Frames: synthetic colour (synthetic.make_color) with the object's ROI (about 105 x 150 pixels: the crop is upscaled), both
outputs written; keypoints: 2000 per frame.  Bounds printed next to each time:
  bytes          : what the kernel must move: S * S * (3 + 4) output bytes per frame plus the crop's colour pixels (4 bytes each)
                   read once, or 16 bytes per keypoint
  hbm_bound_us   : bytes at 6.3 TB/s (the MI355X's achievable HBM rate; 8 TB/s is the spec)
  host_ms        : the host stand-in: the numpy restatement (tests/detector_ref.py) of the crop, resize and grey image plus the
                   upload of both results, or the numpy back-mapping plus the keypoint upload -- what a caller without these
                   kernels does after copying the masked colour image down."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

H, W, SIZE, HBM, NK = 480, 640, 400, 6.3e12, 2000
CASES = {"inputs_1": ("inputs", 1), "inputs_32": ("inputs", 32), "kpts_1": ("kpts", 1), "kpts_32": ("kpts", 32)}


def scene(n):
    from bundletrack_amd import synthetic as S
    pb = S.make_problem(min(n, 8), 10, seed=6, background=True)
    colors, rois = [], []
    for k in range(n):
        T = pb.poses_gt[k % pb.n_frames]
        colors.append(S.make_color(T, pb.K, H, W, seed=k))
        ys, xs = np.nonzero(S.make_mask(T, pb.K, H, W, seed=k))
        rois.append((float(xs.min()), float(xs.max()), float(ys.min()), float(ys.max())))
    return colors, rois


def setup(kind, n):
    import torch
    from bundletrack_amd.bundler import FrameRef
    colors, rois = scene(n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    frames = [FrameRef(id=k, pose_in_model=np.eye(4, dtype=np.float32), color_gpu=t(c), roi=r) for k, (c, r) in enumerate(zip(colors, rois))]
    rng = np.random.default_rng(0)
    kpts = [t(rng.uniform(0, SIZE, (NK, 2)).astype(np.float32)) for _ in range(n)]
    return colors, rois, frames, kpts


def event_us(name, reps):
    import torch
    from bundletrack_amd.detection import keypoints_to_image, prepare_detector_inputs
    from bundletrack_amd.optimizer import Workspace
    kind, n = CASES[name]
    colors, rois, frames, kpts = setup(kind, n)
    ws = Workspace()
    outs = [torch.empty_like(k) for k in kpts]
    call = (lambda: prepare_detector_inputs(ws, frames)) if kind == "inputs" else (lambda: keypoints_to_image(ws, frames, kpts, out=outs))
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    ws.close()
    return float(np.median(times)), colors, rois


def host_ms(kind, colors, rois):
    import torch
    import detector_ref as R
    t0 = time.perf_counter()
    for c, r in zip(colors, rois):
        if kind == "inputs":
            bgr, gray = R.inputs(c, r, SIZE)
            torch.from_numpy(bgr).cuda()
            torch.from_numpy(gray).cuda()
        else:
            k = np.random.default_rng(0).uniform(0, SIZE, (NK, 2)).astype(np.float32)
            torch.from_numpy(R.keypoints_to_image(k, r)).cuda()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rocprof_us(name, reps):
    """Kernel time per call of the k_detect_* kernels, from rocprofv3 --kernel-trace --stats of a fresh child process."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "detect", "--",
               sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(reps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise RuntimeError(f"no kernel stats from rocprofv3 in {sorted(glob.glob(os.path.join(d, '**'), recursive=True))}")
        total_ns = calls = 0
        for row in csv.DictReader(open(stats[0])):
            if "k_detect" in row["Name"]:
                total_ns += float(row["TotalDurationNs"])
                calls = max(calls, int(row["Calls"]))
        return total_ns / max(calls, 1) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:                                   # under rocprofv3: warm-up + reps calls of one case, no output
        event_us(a.child, a.reps)
        return
    out = {"what": "btba_detector_inputs / btba_detector_keypoints_to_image", "H": H, "W": W, "out_size": SIZE, "keypoints": NK, "cases": {}}
    for name, (kind, n) in CASES.items():
        us, colors, rois = event_us(name, a.reps)
        if kind == "inputs":
            crop = sum(int(r[1] - r[0]) * int(r[3] - r[2]) for r in rois)
            nbytes = n * SIZE * SIZE * 7 + crop * 4
        else:
            nbytes = n * NK * 16
        row = {"frames": n, "event_us": round(us, 1), "bytes": nbytes, "hbm_bound_us": round(nbytes / HBM * 1e6, 2),
               "host_ms": round(host_ms(kind, colors, rois), 2)}
        if not a.no_rocprof:
            row["rocprof_kernel_us"] = round(rocprof_us(name, a.reps), 2)
        out["cases"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
