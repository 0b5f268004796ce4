"""Timing of btba_corres_chain (hipEvents around the call, median of --reps after --warmup):
  1. a 1-pair neighbour chain,
  2. a 14-pair chain (one K = 15 window's new pairs: the new frame against 14 earlier frames; keypoints per frame are printed),
  3. the host round-trip sequence the chain replaces for the same 14 pairs: btba_match_pairs with a download, the map-point
     stages restated on the host (tests/corres_ref.py), btba_ransac_pairs_ex per pair.
Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/corres_timing.py`.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from bundletrack_amd import _lib, synthetic as S
    from bundletrack_amd.bundler import FrameRef
    from bundletrack_amd.correspondence import MapPointMemory, find_corres_chain
    from bundletrack_amd.matching import match_pairs
    from bundletrack_amd.optimizer import Workspace
    from bundletrack_amd.ransac import ransac_packed
    from corres_ref import CorresRef, model_points

    pb = S.make_problem(15, 10, seed=11, background=False, rot_step_deg=(2.0, 3.0))
    kp = S.make_keypoints(pb, 1400, 60, D=256, seed=11)          # ~690 keypoints per frame (the visible landmarks + 60 distractors)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    frames = [FrameRef(id=k, pose_in_model=np.asarray(pb.poses_gt[k], np.float32), kpts_gpu=t(kp.kpts[k]), desc_gpu=t(kp.desc[k]),
                       depth_gpu=t(pb.depth[k]), normal_gpu=t(pb.normals[k])) for k in range(15)]
    ws = Workspace()
    prm = _lib.match_params()

    K, H, W = pb.K, pb.H, pb.W

    def gpu_history():
        """A memory that has processed every earlier pair of the window (frames 0..13, in tracker order)."""
        mem = MapPointMemory(ws)
        slots = [mem.register_frame(f.kpts_gpu) for f in frames]
        status = np.zeros(15, np.int32)
        for a in range(1, 14):
            find_corres_chain(ws, mem, frames, [(a, b) for b in range(a - 1, -1, -1)], slots, status, prm, K=K, H=H, W=W)
        return mem, slots, status

    def host_step(R, status, pairs):
        """The round trip the chain replaces: NN with a download, then per pair propagation / RANSAC / update on the host."""
        nn = match_pairs(ws, frames, pairs, prm, K=K, H=H, W=W, device_resident=False, want_points=False).per_pair
        pts = {}
        for (a, b), recs in zip(pairs, nn):
            for r in recs:
                pts.setdefault((a, R.key_index(a, R.uv(a, r["idx_a"]))), r["ptA_cam"])
                pts.setdefault((b, R.key_index(b, R.uv(b, r["idx_b"]))), r["ptB_cam"])
        for (a, b), recs in zip(pairs, nn):
            def rs(m, a=a, b=b):
                pa, pbm = model_points(m, frames[a].pose_in_model, frames[b].pose_in_model)
                return ransac_packed(ws, pa, pbm, np.array([len(m)], np.int32))[0]["inlier_ids"]
            R.find_corres(a, b, abs(a - b) == 1, recs, status, rs, lambda f, i: pts.get((f, i), np.zeros(3, np.float32)))

    def host_history():
        R, status = CorresRef(), {}
        for k in range(15):
            R.register(k, kp.kpts[k])
        for a in range(1, 14):
            host_step(R, status, [(a, b) for b in range(a - 1, -1, -1)])
        return R, status

    def event_ms(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1), (time.perf_counter() - w0) * 1e3

    out = {"kpts_per_frame": float(np.mean([k.shape[0] for k in kp.kpts])), "reps": args.reps}
    one, window = [(14, 13)], [(14, b) for b in range(13, -1, -1)]
    for name, pairs in (("chain_1pair_neighbour", one), ("chain_14pairs", window)):
        ms = []
        for r in range(args.warmup + args.reps):
            mem, slots, status = gpu_history()          # the chain changes the memory: every rep starts from the same history, untimed
            t_ev, t_wall = event_ms(lambda: find_corres_chain(ws, mem, frames, pairs, slots, status.copy(), prm, K=K, H=H, W=W))
            mem.close()
            if r >= args.warmup:
                ms.append((t_ev, t_wall))
        ms = np.array(ms)
        out[name] = {"event_ms_median": round(float(np.median(ms[:, 0])), 4), "wall_ms_median": round(float(np.median(ms[:, 1])), 4)}
    import copy
    R0, st0 = host_history()
    ms = []
    for r in range(args.warmup + min(args.reps, 5)):
        R, st = copy.deepcopy(R0), dict(st0)
        t_ev, t_wall = event_ms(lambda: host_step(R, st, window))
        if r >= args.warmup:
            ms.append((t_ev, t_wall))
    ms = np.array(ms)
    out["host_roundtrip_14pairs"] = {"event_ms_median": round(float(np.median(ms[:, 0])), 4), "wall_ms_median": round(float(np.median(ms[:, 1])), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
