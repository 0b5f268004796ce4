"""Timing of btba_apply_masks (foreground-mask segmentation), both paths at 1 and 32 frames of 480 x 640, one JSON line.  GPU box only.
    python scripts/mask_timing.py              hipEvent time per call, and the same cases under rocprofv3 --kernel-trace --stats
                                               (each case in a fresh child process), next to the bounds below
    python scripts/mask_timing.py --no-rocprof hipEvent times only
Frames: synthetic object silhouettes (synthetic.make_mask, about 4 % of the image, with 3 spurious blobs) on background-rendered
depth / normals, colour present.  The maps are not restored between calls: after the first call they are already zero outside the
mask, which changes no work (the kernels store those zeros again and never read depth, normals or colour).  Bounds printed next to each time:
  apply_bytes          : what k_mask_apply must move: the mask byte read and the mask_out byte written for every pixel, plus
                         depth 4 + normal 16 + colour 4 bytes stored for every pixel off the final mask
  hbm_bound_us         : apply_bytes at 6.3 TB/s (the MI355X's achievable HBM rate; 8 TB/s is the spec)
  cpu_numpy_ms         : the same function on the host -- scipy.ndimage.label, numpy hull fill, binary_dilation, numpy
                         invalidation, ROI -- plus the three host -> device uploads of the maps the reference does afterwards
                         (updateColorGPU, updateDepthGPU, updateNormalGPU), the stand-in for its OpenCV path."""
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

H, W, HBM = 480, 640, 6.3e12
CASES = {"plain_1": (False, 1), "plain_32": (False, 32), "hull_1": (True, 1), "hull_32": (True, 32)}


def scene(n):
    from bundletrack_amd import synthetic as S
    pb = S.make_problem(min(n, 8), 10, seed=6, background=True)
    masks = [S.make_mask(pb.poses_gt[k % pb.n_frames], pb.K, H, W, seed=k, n_blobs=3) for k in range(n)]
    return pb, masks


def frames_on_gpu(pb, masks):
    import torch
    from bundletrack_amd.bundler import FrameRef
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(0)
    return [FrameRef(id=k, pose_in_model=np.eye(4, dtype=np.float32), depth_gpu=t(pb.depth[k % pb.n_frames]), normal_gpu=t(pb.normals[k % pb.n_frames]),
                     color_gpu=t(rng.integers(0, 256, (H, W, 4), dtype=np.uint8)), mask_gpu=t(m)) for k, m in enumerate(masks)]


def event_us(name, reps):
    import torch
    from bundletrack_amd.optimizer import Workspace
    from bundletrack_amd.segmentation import apply_masks
    hull, n = CASES[name]
    pb, masks = scene(n)
    frames = frames_on_gpu(pb, masks)
    ws = Workspace()
    for _ in range(3):
        apply_masks(ws, frames, largest_component_hull=hull)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record()
        apply_masks(ws, frames, largest_component_hull=hull)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    off = sum(int((f.fg_mask_gpu == 0).sum()) for f in frames)
    return float(np.median(times)), off, masks


def cpu_ms(masks, hull, maps):
    """The host restatement with scipy / numpy, and the three uploads."""
    import torch
    from scipy import ndimage
    t0 = time.perf_counter()
    for m, (dep, nrm, col) in zip(masks, maps):
        fg = m != 0
        if hull:
            lab, n = ndimage.label(fg, structure=np.ones((3, 3), int))
            if n:
                cnt = np.bincount(lab.ravel())[1:]
                ys, xs = np.nonzero(lab == 1 + int(np.argmax(cnt)))
                from scipy.spatial import ConvexHull
                qh = ConvexHull(np.stack([xs, ys], 1).astype(float))
                gy, gx = np.mgrid[0:H, 0:W]
                fg = (qh.equations[:, :2] @ np.stack([gx.ravel(), gy.ravel()]) + qh.equations[:, 2:] <= 0).all(0).reshape(H, W)
            else:
                fg[:] = False
        M = ndimage.binary_dilation(fg, structure=np.ones((5, 5), bool), border_value=0)
        dep, nrm, col = dep.copy(), nrm.copy(), col.copy()
        dep[~M] = 0; nrm[~M] = 0; col[~M] = 0
        ys, xs = np.nonzero(M)
        _ = (xs.min(), xs.max(), ys.min(), ys.max()) if xs.size else None
        for a in (col, dep, nrm):
            torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rocprof_us(name, reps):
    """Kernel time per call of the k_mask_* kernels, from rocprofv3 --kernel-trace --stats of a fresh child process."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "mask", "--", sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(reps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise RuntimeError(f"no kernel stats from rocprofv3 in {sorted(glob.glob(os.path.join(d, '**'), recursive=True))}")
        total_ns = calls = 0
        per = {}
        for row in csv.DictReader(open(stats[0])):
            if "k_mask" in row["Name"]:
                ns = float(row["TotalDurationNs"])
                total_ns += ns
                calls = max(calls, int(row["Calls"]))
                per[row["Name"].split("(")[0].split("::")[-1].split("<")[0] + ("<hull>" if "<true>" in row["Name"] else "")] = round(ns / int(row["Calls"]) / 1e3, 2)
        return total_ns / max(calls, 1) / 1e3, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:                                   # under rocprofv3: warm-up + reps calls of one case, no output
        event_us(a.child, a.reps)
        return
    out = {"what": "btba_apply_masks", "H": H, "W": W, "dilate": 5, "cases": {}}
    for name, (hull, n) in CASES.items():
        us, off, masks = event_us(name, a.reps)
        nbytes = n * H * W * 2 + off * 24
        pb, _ = scene(1)
        maps = [(pb.depth[0], pb.normals[0], np.zeros((H, W, 4), np.uint8))] * n
        row = {"frames": n, "event_us": round(us, 1), "apply_bytes": nbytes, "hbm_bound_us": round(nbytes / HBM * 1e6, 2),
               "off_mask_fraction": round(off / (n * H * W), 4), "cpu_numpy_ms": round(cpu_ms(masks, hull, maps), 2)}
        if not a.no_rocprof:
            kus, per = rocprof_us(name, a.reps)
            row["rocprof_kernel_us"], row["rocprof_per_kernel_us"] = round(kus, 1), per
        out["cases"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
