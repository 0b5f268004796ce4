"""Time of keyframe fusion -> profiles/fusion_timing.json: 15 keyframes of 480 x 640 masked to the object (~5 % valid), leaf 5 mm, for 1 instance and
for 32 (each instance its own copy of the maps).  Medians of 30 device-event times after 5 warm-up calls on the workspace stream, same run, same GPU:
  bounds          btba_fuse_bounds (the data-derived box)
  fuse_frames     btba_fuse_frames with that box: clear, accumulate, compaction (normals and colour fused)
  fuse_positions  the same without the normal and colour planes
  torch           the same voxel means with torch ops on the same GPU (transform, floor, torch.unique with inverse, index_add_): the familiar yardstick
--kernel-stats FILE merges the per-kernel averages of a `rocprofv3 --kernel-trace --stats` run of `--no-torch --profile-run` (taken in a run of its own)
into the JSON: k_fuse_bounds, k_fuse_accumulate and the three compaction kernels separately.  GPU box only.
    python scripts/fusion_timing.py [--out profiles/fusion_timing.json]"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

N_KF, LEAF, WARMUP, REPS = 15, 0.005, 5, 30


def merge_kernel_stats(out, path):
    res = json.load(open(out))
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        if "k_fuse" in name:
            short = name.split("k_fuse")[1].split("(")[0]
            rows["k_fuse" + short] = dict(calls=int(r["Calls"]), average_us=round(float(r["AverageNs"]) / 1e3, 2), min_us=round(float(r["MinNs"]) / 1e3, 2),
                                          max_us=round(float(r["MaxNs"]) / 1e3, 2))
    res["kernel_stats_rocprofv3_profile_run"] = rows
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_timing.json"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--profile-run", action="store_true", help="5 calls of bounds and fuse_frames per case and nothing else: the run a kernel trace is taken of")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.out, args.kernel_stats)
    import torch
    from bundletrack_amd import synthetic as S
    from bundletrack_amd._lib import check, fuse_params, lib
    from bundletrack_amd.fusion import Segment, _segment_array, fuse_bounds, fuse_frames
    from bundletrack_amd.optimizer import Workspace
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")

    def median_ms(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        return round(float(np.median(times)), 4), round(float(np.min(times)), 4), round(float(np.max(times)), 4)

    seq = S.SyntheticSequence(n_frames=N_KF, seed=S.config_seed(3), step_deg=(20.0, 24.0), background=False)
    rng = np.random.default_rng(0)
    host = []
    for k in range(N_KF):
        depth, normals = seq.render(k)[:2]
        col = np.zeros((seq.H, seq.W, 4), np.uint8)
        col[..., :3] = rng.integers(0, 256, size=(seq.H, seq.W, 3), dtype=np.uint8)
        host.append((depth, normals, col))
    valid = float(np.mean([(d >= 0.1).mean() for d, _, _ in host]))
    ws = Workspace()
    res = dict(workload=dict(keyframes=N_KF, H=seq.H, W=seq.W, valid_fraction=round(valid, 4), leaf=LEAF, warmup=WARMUP, reps=REPS,
                             device=torch.cuda.get_device_name(0)), cases={})
    for B in (1, 32):
        segs = []
        for b in range(B):
            for k, (d, n, c) in enumerate(host):
                segs.append(Segment(b, seq.poses_gt[k].astype(np.float32), depth=torch.from_numpy(d).to(dev), normal=torch.from_numpy(n).to(dev),
                                    colour=torch.from_numpy(c).to(dev)))
        box = fuse_bounds(ws, segs, B, seq.K, leaf=LEAF).cpu().numpy()
        cloud = fuse_frames(ws, segs, B, seq.K, leaf=LEAF, box=box)
        cap = cloud.xyz.shape[1]
        n_out = cloud.counts()
        # the timed calls go straight to the C ABI on a prebuilt segment array: the Python layer's per-segment marshalling (~30 us each) is host time,
        # not what is measured here
        arr, H, W, _, keep_alive = _segment_array(segs, B)
        Kf = np.ascontiguousarray(seq.K, np.float32).reshape(9)
        prm = fuse_params(leaf=LEAF)
        box_dev = torch.empty((B, 6), dtype=torch.int32, device=dev)
        ptr = lambda x: None if x is None else x.data_ptr()

        def bounds():
            check(lib().btba_fuse_bounds(ws.handle, C.byref(prm), B, len(segs), C.cast(arr, C.c_void_p), H, W, Kf.ctypes.data, box_dev.data_ptr()), "btba_fuse_bounds")

        def fuse(full=True):
            check(lib().btba_fuse_frames(ws.handle, C.byref(prm), B, len(segs), C.cast(arr, C.c_void_p), H, W, Kf.ctypes.data, box.ctypes.data, cap, ptr(cloud.xyz),
                                         ptr(cloud.normal) if full else None, ptr(cloud.colour) if full else None, ptr(cloud.count), ptr(cloud.lin),
                                         ptr(cloud.n_out), ptr(cloud.n_outside), ptr(cloud.status)), "btba_fuse_frames")

        if args.profile_run:
            for _ in range(5):
                bounds()
                fuse()
            torch.cuda.synchronize()
            continue
        case = dict(instances=B, segments=len(segs), box_instance0=box[0].tolist(), voxels_total=int(np.prod(box[:, 3:].astype(np.int64), axis=1).sum()),
                    n_out_instance0=int(n_out[0]), points_instance0=int(cloud.count[0, :n_out[0]].sum().item()), ms_median_min_max={})
        t = case["ms_median_min_max"]
        t["bounds"] = median_ms(bounds)
        t["fuse_frames"] = median_ms(fuse)
        t["fuse_positions"] = median_ms(lambda: fuse(False))
        assert np.array_equal(box_dev.cpu().numpy(), box) and np.array_equal(cloud.counts(), n_out)
        if not args.no_torch:
            # the same voxel means with torch ops: the camera-space points are made once outside the timed region (the xyz maps a tracker may keep)
            Kd = torch.from_numpy(np.asarray(seq.K, np.float32)).to(dev)
            v, u = torch.meshgrid(torch.arange(seq.H, device=dev, dtype=torch.float32), torch.arange(seq.W, device=dev, dtype=torch.float32), indexing="ij")
            depth = torch.stack([s.depth for s in segs])
            cam = torch.stack([(u - Kd[0, 2]) / Kd[0, 0] * depth, (v - Kd[1, 2]) / Kd[1, 1] * depth, depth], -1).reshape(len(segs), -1, 3)
            nrm = torch.stack([s.normal for s in segs]).reshape(len(segs), -1, 4)[..., :3]
            col = torch.stack([s.colour for s in segs]).reshape(len(segs), -1, 4)[..., :3].float()
            T = torch.from_numpy(np.stack([np.asarray(s.pose, np.float32) for s in segs])).to(dev)
            inst = torch.tensor([s.instance for s in segs], device=dev)[:, None].expand(-1, cam.shape[1])
            segidx = torch.arange(len(segs), device=dev)[:, None].expand(-1, cam.shape[1])
            keep = (depth.reshape(len(segs), -1) >= 0.1) & (nrm != 0).any(-1)
            mn = torch.from_numpy(box[:, :3].astype(np.int64)).to(dev)
            dims = torch.from_numpy(box[:, 3:].astype(np.int64)).to(dev)

            def torch_fuse():
                sid = segidx[keep]                       # valid pixels first, as a caller would: 95 % of the maps are masked out
                Rm, b = T[sid, :3, :3], inst[keep]
                p = (Rm * cam[keep][:, None, :]).sum(-1) + T[sid, :3, 3]
                n = (Rm * nrm[keep][:, None, :]).sum(-1)
                i = torch.floor(p / LEAF).long() - mn[b]
                key = b * (1 << 40) + i[:, 0] + dims[b, 0] * (i[:, 1] + dims[b, 1] * i[:, 2])
                uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
                acc = torch.zeros((uniq.shape[0], 9), device=dev)
                acc.index_add_(0, inv, torch.cat([p, n, col[keep]], 1))
                return acc / cnt[:, None], cnt

            means, cnt = torch_fuse()
            torch.cuda.synchronize()
            case["torch_voxels"] = int(means.shape[0])
            case["voxels_all_instances"] = int(n_out.sum())
            t["torch"] = median_ms(torch_fuse)
        res["cases"][f"instances_{B}"] = case
        del segs
    if args.profile_run:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
