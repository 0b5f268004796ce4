"""Time of the two pose-covariance calls at c3 x 32 (K = 15 frames, 2 000 matches per pair, 32 instances) -> profiles/covariance_timing.json.
Medians of 30 device-event times after 5 warm-up calls, each in the same run on the same GPU:
  linearize_zn        btba_linearize_batch_zn_aux (one traced solve iterate on a copy of the poses + the gather)
  traced_iterate      one traced solve iterate alone (solve_zn, n_gn_iters = 1, trace on): what the linearisation is made of
  pose_covariances    btba_pose_covariances, blocks only and with the full matrix
  torch_linalg_inv    torch.linalg.inv on the same matrices widened to fp64: the familiar yardstick
GPU box only.
    python scripts/covariance_timing.py [--out profiles/covariance_timing.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bundletrack_amd import synthetic as S
from bundletrack_amd.covariance import pose_covariances
from bundletrack_amd.optimizer import BatchSolver, Workspace

K, M, B, WARMUP, REPS = 15, 2000, 32, 5, 30


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "covariance_timing.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    pbs = [S.make_problem(K, M, S.config_seed(5, i), background=True, full_res=False) for i in range(B)]      # bench.py's c3 instances
    ws = Workspace()
    bs = BatchSolver(ws)
    corr, offs, mx = bs.pack_correspondences([pb.corr for pb in pbs], K)
    zn = torch.from_numpy(np.stack([S.compact_cache(pb) for pb in pbs])).to(dev)
    corr_d = torch.from_numpy(corr.view(np.uint8).reshape(B, -1, 32)).to(dev)
    offs_d = torch.from_numpy(offs.astype(np.int32)).to(dev)
    poses0 = torch.from_numpy(np.stack([pb.poses_init for pb in pbs]).astype(np.float32)).to(dev)
    pb0 = pbs[0]
    aux = bs.cache_aux(zn)

    poses = poses0.clone()
    bs.solve_zn(zn, pb0.H, pb0.W, pb0.K, corr_d, offs_d, mx, poses, aux=aux)          # the poses a tracker would ask about: the solve's result
    ws.sync()
    info = bs.linearize_zn(zn, pb0.H, pb0.W, pb0.K, corr_d, offs_d, mx, poses, aux=aux)
    ws.sync()
    out = pose_covariances(ws, info, full=True)
    ws.sync()
    H64 = info.double()
    status = out.status.cpu().numpy()
    kappa = [float(np.linalg.cond(h)) for h in H64.cpu().numpy()]
    inv = torch.linalg.inv(H64)
    diff = float((out.full - inv).abs().max())

    one = BatchSolver(ws, n_gn_iters=1)
    scratch = poses.clone()

    def traced():
        scratch.copy_(poses)
        one.solve_zn(zn, pb0.H, pb0.W, pb0.K, corr_d, offs_d, mx, scratch, aux=aux, trace=True)

    res = dict(
        workload=dict(config="c3", K=K, corr_per_pair=M, instances=B, na=6 * (K - 1), warmup=WARMUP, reps=REPS, device=torch.cuda.get_device_name(0)),
        ms_median_min_max=dict(
            linearize_zn=median_ms(lambda: bs.linearize_zn(zn, pb0.H, pb0.W, pb0.K, corr_d, offs_d, mx, poses, aux=aux)),
            traced_iterate=median_ms(traced),
            pose_covariances_blocks=median_ms(lambda: pose_covariances(ws, info)),
            pose_covariances_full=median_ms(lambda: pose_covariances(ws, info, full=True)),
            torch_linalg_inv_fp64=median_ms(lambda: torch.linalg.inv(H64)),
        ),
        status_nonzero=int((status != 0).sum()), kappa2_info_min_max=[min(kappa), max(kappa)],
        pivot_ratio_min_max=[float(out.pivot_ratio.min()), float(out.pivot_ratio.max())],
        max_abs_diff_to_torch_inv=diff,
    )
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
