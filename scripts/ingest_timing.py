#!/usr/bin/env python3
"""Times btba_ingest_frames against the per-frame calls it replaces, on the GPU, and writes profiles/ingest_timing.json.

For 32 frames and for 1 frame of 480 x 640 (millimetre codes + BGR):
  (a) batched   one ingest_frames call: 2 launches per 32 frames
  (b) per_frame the loop a caller writes today, same process and library: torch decode in double, torch colour pack,
                process_depth and depth_to_normals per frame (2 n launches of this library plus the torch kernels)
(b) is measured twice, before and after (a); the distance between its two medians is its own run-to-run spread.  Each figure is
the median of hipEvent times over --repeats calls after --warmup calls.  The fused-normals variant was not built, so it is not
timed.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_timing.json"))
    args = ap.parse_args()
    import torch
    from bundletrack_amd import synthetic as S
    from bundletrack_amd.ingest import ingest_frames
    from bundletrack_amd.optimizer import Workspace, depth_to_normals, process_depth
    if not torch.cuda.is_available():
        sys.exit("ingest_timing.py needs a GPU")
    H, W, K = 480, 640, np.asarray(S.NOCS_K, np.float32)
    ws = Workspace()
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rng = np.random.default_rng(0)

    def frame(k):
        d, _ = S.render(S.orbit_pose(0.05 * k), S.NOCS_K, xs, ys, True)
        d = d + rng.normal(scale=0.0008, size=d.shape).astype(np.float32)
        codes = np.clip(np.rint(d.astype(np.float64) * 1000.0), 0, 65535).astype(np.uint16)
        return torch.from_numpy(codes).cuda(), torch.from_numpy(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).cuda()

    class F:
        depth_gpu = normal_gpu = color_gpu = None

    def batched(codes, bgr):
        fs = [F() for _ in codes]
        ingest_frames(ws, fs, codes, bgr, K)
        return fs

    def per_frame(codes, bgr):
        fs = []
        for c, b in zip(codes, bgr):
            f = F()
            d = (c.to(torch.float32).to(torch.float64) * 0.001).to(torch.float32)
            d = torch.where(d.to(torch.float64) < 0.1, torch.zeros_like(d), d)
            f.color_gpu = torch.cat([b, torch.zeros((H, W, 1), dtype=torch.uint8, device=b.device)], dim=2)
            f.depth_gpu = process_depth(ws, d)
            f.normal_gpu = depth_to_normals(ws, f.depth_gpu, K)
            fs.append(f)
        return fs

    def median_ms(fn, codes, bgr):
        for _ in range(args.warmup):
            fn(codes, bgr)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(codes, bgr)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return float(np.median(times)), float(np.percentile(times, 10)), float(np.percentile(times, 90))

    result = {"device": torch.cuda.get_device_name(0), "H": H, "W": W, "repeats": args.repeats, "warmup": args.warmup,
              "timer": "hipEvent pairs around each call, median (p10, p90) in ms", "fused_normals_variant": "not built, not timed", "cases": []}
    for n in (32, 1):
        data = [frame(k) for k in range(n)]
        codes, bgr = [c for c, _ in data], [b for _, b in data]
        a, b = batched(codes, bgr), per_frame(codes, bgr)
        torch.cuda.synchronize()
        same = all(torch.equal(x.depth_gpu, y.depth_gpu) and torch.equal(x.normal_gpu, y.normal_gpu) and torch.equal(x.color_gpu, y.color_gpu) for x, y in zip(a, b))
        b1 = median_ms(per_frame, codes, bgr)
        a1 = median_ms(batched, codes, bgr)
        b2 = median_ms(per_frame, codes, bgr)
        spread = abs(b1[0] - b2[0])
        b_med = 0.5 * (b1[0] + b2[0])
        case = {"n_frames": n, "outputs_identical": bool(same),
                "batched_ms": a1[0], "batched_p10_p90_ms": a1[1:], "batched_us_per_frame": 1000.0 * a1[0] / n,
                "batched_launches": 2 * ((n + 31) // 32),
                "per_frame_ms_run1": b1[0], "per_frame_ms_run2": b2[0], "per_frame_p10_p90_ms_run1": b1[1:], "per_frame_p10_p90_ms_run2": b2[1:],
                "per_frame_spread_ms": spread, "per_frame_library_launches": 2 * n,
                "batched_not_slower_than_per_frame_within_its_spread": bool(a1[0] <= b_med + spread)}
        print(json.dumps(case))
        result["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
