"""Time of frame-to-model registration -> profiles/register_timing.json: one 480 x 640 frame masked to the object (~5 % valid) per instance against
the fusion timing's model (15 keyframes, leaf 5 mm, normalised normals), from 3 degrees / 5 mm off its pose, 10 Gauss-Newton iterations (the
convergence thresholds off, so that all 10 run) plus the evaluation pass, for 1 instance and for 32 (each instance its own copy of the model
and the frame).  Medians of 30 device-event times after 5 warm-up calls on the workspace stream, same run, same GPU:
  index            btba_register_index (once per cloud)
  register_frames  btba_register_frames, 10 iterations
  pose_check       btba_register_frames with n_iters = 0: one accumulation pass
  associate        btba_register_associate: one association pass
  torch            the same 10 iterations with torch ops on the same GPU (valid pixels compacted once outside the timed region; 27-cell lookup
                   through the same cell index, gates, fp64 normal equations, torch.linalg.solve, the update): the familiar yardstick
--kernel-stats FILE merges the per-kernel averages of a `rocprofv3 --kernel-trace --stats` run of `--no-torch --profile-run` (taken in a run of
its own) into the JSON.  No time was fixed beforehand: the JSON records what was measured.  GPU box only.
    python scripts/register_timing.py [--out profiles/register_timing.json]"""
import argparse
import csv
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

N_KF, LEAF, WARMUP, REPS, N_ITERS, FRAME = 15, 0.005, 5, 30, 10, 7


def merge_kernel_stats(out, path):
    res = json.load(open(out))
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        if "k_register" in name:
            short = name.split("k_register")[1].split("(")[0]
            rows["k_register" + short] = dict(calls=int(r["Calls"]), average_us=round(float(r["AverageNs"]) / 1e3, 2), min_us=round(float(r["MinNs"]) / 1e3, 2),
                                              max_us=round(float(r["MaxNs"]) / 1e3, 2))
    res["kernel_stats_rocprofv3_profile_run"] = rows
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_timing.json"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--profile-run", action="store_true", help="5 calls of register_frames per case and nothing else: the run a kernel trace is taken of")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.out, args.kernel_stats)
    import torch
    from bundletrack_amd import synthetic as S
    from bundletrack_amd._lib import REGISTER_RESULT_DTYPE, check, lib, register_params
    from bundletrack_amd.fusion import Segment, _segment_array, fuse_frames
    from bundletrack_amd.optimizer import Workspace
    from bundletrack_amd.registration import build_index
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
    host = [seq.render(k)[:2] for k in range(N_KF)]
    rng = np.random.default_rng(1)
    w, u = rng.normal(size=3), rng.normal(size=3)
    start = (S.se3_exp(w / np.linalg.norm(w) * np.deg2rad(3.0), u / np.linalg.norm(u) * 0.005) @ seq.poses_gt[FRAME]).astype(np.float32)
    ws = Workspace()
    res = dict(workload=dict(keyframes=N_KF, H=seq.H, W=seq.W, valid_fraction=round(float((host[FRAME][0] >= 0.1).mean()), 4), leaf=LEAF, n_iters=N_ITERS,
                             start="3 deg / 5 mm", warmup=WARMUP, reps=REPS, device=torch.cuda.get_device_name(0)), cases={})
    for B in (1, 32):
        kf = [Segment(b, seq.poses_gt[k].astype(np.float32), depth=torch.from_numpy(d).to(dev), normal=torch.from_numpy(n).to(dev))
              for b in range(B) for k, (d, n) in enumerate(host)]
        cloud = fuse_frames(ws, kf, B, seq.K, leaf=LEAF, normalize_normals=True, want_colour=False)
        index = build_index(ws, cloud)
        cap, n_out = cloud.xyz.shape[1], cloud.counts()
        items = [Segment(b, start, depth=torch.from_numpy(host[FRAME][0]).to(dev), normal=torch.from_numpy(host[FRAME][1]).to(dev)) for b in range(B)]
        # the timed calls go straight to the C ABI on a prebuilt segment array: the Python layer's marshalling is host time, not what is measured here
        arr, H, W, _, keep_alive = _segment_array(items, B)
        Kf = np.ascontiguousarray(seq.K, np.float32).reshape(9)
        box = np.ascontiguousarray(cloud.box, np.int32)
        pose_out = torch.empty((B, 12), dtype=torch.float32, device=dev)
        result = torch.empty((B, REGISTER_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        match = [torch.empty((H * W,), dtype=torch.int32, device=dev) for _ in range(B)]
        table = (C.c_void_p * B)(*[m.data_ptr() for m in match])

        def head(prm):
            return (ws.handle, C.byref(prm), B, B, C.cast(arr, C.c_void_p), H, W, Kf.ctypes.data, box.ctypes.data, cap, cloud.xyz.data_ptr(), cloud.normal.data_ptr(),
                    index.cell_index.data_ptr())

        p_run = register_params(leaf=LEAF, n_iters=N_ITERS, eps_rot=0.0, eps_trans=0.0)
        p_check = register_params(leaf=LEAF, n_iters=0)
        run = lambda: check(lib().btba_register_frames(*head(p_run), pose_out.data_ptr(), result.data_ptr(), None), "btba_register_frames")
        pose_check = lambda: check(lib().btba_register_frames(*head(p_check), pose_out.data_ptr(), result.data_ptr(), None), "btba_register_frames")
        assoc = lambda: check(lib().btba_register_associate(*head(p_check), C.cast(table, C.c_void_p)), "btba_register_associate")
        reindex = lambda: check(lib().btba_register_index(ws.handle, B, box.ctypes.data, cap, cloud.lin.data_ptr(), cloud.n_out.data_ptr(),
                                                          index.cell_index.data_ptr()), "btba_register_index")
        if args.profile_run:
            for _ in range(5):
                run()
            torch.cuda.synchronize()
            continue
        case = dict(instances=B, box_instance0=box[0].tolist(), cells_total=int(index.voxel_offsets[-1]), model_records_instance0=int(n_out[0]), ms_median_min_max={})
        t = case["ms_median_min_max"]
        t["index"] = median_ms(reindex)
        t["register_frames"] = median_ms(run)
        r = result.cpu().numpy().reshape(-1).view(REGISTER_RESULT_DTYPE)
        T = np.tile(np.eye(4), (B, 1, 1))
        T[:, :3] = pose_out.cpu().numpy().reshape(B, 3, 4)
        D = T[0] @ np.linalg.inv(seq.poses_gt[FRAME])
        case.update(status=int(r["status"][0]), iters_done=int(r["iters_done"][0]), n_valid=int(r["n_valid"][0]), n_matched=int(r["n_matched"][0]),
                    rms_mm=round(float(np.sqrt(r["cost"][0] / max(r["n_matched"][0], 1))) * 1e3, 4),
                    end_mrad=round(float(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1))) * 1e3, 3),
                    end_mm=round(float(np.linalg.norm(T[0, :3, 3] - seq.poses_gt[FRAME][:3, 3])) * 1e3, 3))
        t["pose_check"] = median_ms(pose_check)
        t["associate"] = median_ms(assoc)
        print(json.dumps(case), flush=True)
        if not args.no_torch:
            Kd = torch.from_numpy(np.asarray(seq.K, np.float32)).to(dev)
            v, uu = torch.meshgrid(torch.arange(seq.H, device=dev, dtype=torch.float32), torch.arange(seq.W, device=dev, dtype=torch.float32), indexing="ij")
            depth = torch.stack([s.depth for s in items])
            nmap = torch.stack([s.normal for s in items]).reshape(B, -1, 4)[..., :3]
            cam = torch.stack([(uu - Kd[0, 2]) / Kd[0, 0] * depth, (v - Kd[1, 2]) / Kd[1, 1] * depth, depth], -1).reshape(B, -1, 3)
            keep = (depth.reshape(B, -1) >= 0.1) & (nmap != 0).any(-1)
            inst = torch.arange(B, device=dev)[:, None].expand(-1, cam.shape[1])[keep]
            pc, pn = cam[keep], nmap[keep]                                           # compacted once, outside the timed region
            mn = torch.from_numpy(box[:, :3].astype(np.int64)).to(dev)[inst]
            dims = torch.from_numpy(box[:, 3:].astype(np.int64)).to(dev)[inst]
            voff = torch.from_numpy(index.voxel_offsets[:-1]).to(dev)[inst]
            offs = torch.tensor([(ox, oy, oz) for oz in (-1, 0, 1) for oy in (-1, 0, 1) for ox in (-1, 0, 1)], device=dev)
            mxyz, mnrm, cells = cloud.xyz[..., :3], cloud.normal[..., :3], index.cell_index.long()
            T0 = torch.from_numpy(np.tile(np.asarray(start, np.float64), (B, 1, 1))).to(dev)
            delta = 0.005

            def torch_register():
                Tc = T0.clone()
                for _ in range(N_ITERS):
                    Tf = Tc.float()[inst]
                    q = (Tf[:, :3, :3] * pc[:, None, :]).sum(-1) + Tf[:, :3, 3]
                    nq = (Tf[:, :3, :3] * pn[:, None, :]).sum(-1)
                    j = (torch.floor(q / LEAF).long() - mn)[:, None, :] + offs[None]
                    ok = ((j >= 0) & (j < dims[:, None, :])).all(-1)
                    lin = torch.where(ok, voff[:, None] + j[..., 0] + dims[:, None, 0] * (j[..., 1] + dims[:, None, 1] * j[..., 2]), torch.zeros_like(j[..., 0]))
                    k = torch.where(ok, cells[lin], torch.full_like(lin, -1))
                    m = mxyz[inst[:, None], k.clamp(min=0)]
                    d2 = torch.where(k >= 0, ((q[:, None, :] - m) ** 2).sum(-1), torch.full_like(q[:, :1], float("inf")))
                    best = d2.argmin(1, keepdim=True)
                    kb = k.gather(1, best)[:, 0]
                    hit = kb >= 0
                    mb, nb = mxyz[inst, kb.clamp(min=0)], mnrm[inst, kb.clamp(min=0)]
                    d = q - mb
                    on = hit & (d2.gather(1, best)[:, 0] <= 0.02 ** 2) & ((nq * nb).sum(-1) >= 0.70710678)
                    r = (nb * d).sum(-1).double()
                    a = torch.cat([torch.cross(q, nb, dim=-1), nb], -1).double()
                    wgt = torch.where(r.abs() <= delta, torch.ones_like(r), delta / r.abs()) * on
                    # every instance has the same frame, so the same number of points in instance order: a batched matrix product sums them.  (An
                    # index_add_ of fp64 terms onto 36 addresses per instance serialises on those addresses and is slower by orders of magnitude.)
                    ab, wb = a.reshape(B, -1, 6), wgt.reshape(B, -1, 1)
                    Hm = (ab * wb).transpose(1, 2) @ ab
                    g = ((ab * wb).transpose(1, 2) @ r.reshape(B, -1, 1))[:, :, 0]
                    xi = torch.linalg.solve(Hm, -g)
                    om, tr = xi[:, :3], xi[:, 3:]
                    th = om.norm(dim=1).clamp(min=1e-12)[:, None, None]
                    Kx = torch.zeros((B, 3, 3), dtype=torch.float64, device=dev)
                    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -om[:, 2], om[:, 1], om[:, 2], -om[:, 0], -om[:, 1], om[:, 0]
                    eye, K2 = torch.eye(3, dtype=torch.float64, device=dev), Kx @ Kx
                    Rm = eye + torch.sin(th) / th * Kx + (1 - torch.cos(th)) / th ** 2 * K2
                    Vm = eye + (1 - torch.cos(th)) / th ** 2 * Kx + (th - torch.sin(th)) / th ** 3 * K2
                    E = torch.eye(4, dtype=torch.float64, device=dev).repeat(B, 1, 1)
                    E[:, :3, :3], E[:, :3, 3] = Rm, (Vm @ tr[:, :, None])[:, :, 0]
                    Tc = (E @ Tc).float().double()
                return Tc

            assert (keep.sum(1) == keep[0].sum()).all()
            print("torch comparison ...", flush=True)
            Tt = torch_register()
            torch.cuda.synchronize()
            case["torch_pose_max_abs_diff"] = float((Tt[:, :3].cpu().numpy() - T[:, :3]).__abs__().max())
            t["torch"] = median_ms(torch_register)
        res["cases"][f"instances_{B}"] = case
        del kf, items
    if args.profile_run:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
