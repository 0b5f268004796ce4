"""Time of the objective report at c3 x 32 (K = 15 frames, 2 000 matches per pair, 160 x 120 caches, 32 instances) -> profiles/objective_timing.json.
Medians of 30 device-event times after 5 warm-up calls, each in the same run on the same GPU:
  objective_zn        btba_objective_batch_zn_aux, both terms (k_prepare, the dense and the sparse sweep, the fold), outputs left on the device
  objective_sparse    the same with weight_dense_depth = 0: the sparse term alone
  linearize_zn        btba_linearize_batch_zn_aux: one traced solve iterate over the same pixels and entries, the call the report sits beside
  torch_sparse        the sparse sums (sum ||r||^2, sum rho, outlier count per instance) with torch ops on the same GPU: the familiar yardstick
GPU box only.
    python scripts/objective_timing.py [--out profiles/objective_timing.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bundletrack_amd import synthetic as S
from bundletrack_amd.objective import residual_variance
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "objective_timing.json"))
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
    args_ = (zn, pb0.H, pb0.W, pb0.K, corr_d, offs_d, mx)

    before = bs.objective_zn(*args_, poses0)
    poses = poses0.clone()
    bs.solve_zn(*args_, poses)
    after = bs.objective_zn(*args_, poses)
    sparse_only = BatchSolver(ws, weight_dense_depth=0.0)

    # the sparse sums with torch ops: gather each entry's two matrices, transform, subtract; squares and rho in fp64
    words = corr_d.view(torch.int32).reshape(B, -1, 8)
    fi, fj = words[..., 0].long(), words[..., 1].long()
    valid = words[..., 0] != -1
    pos = corr_d.view(torch.float32).reshape(B, -1, 8)
    fi_c, fj_c = fi.clamp(0, K - 1), fj.clamp(0, K - 1)
    delta = float(np.float32(bs.params.robust_delta))

    def torch_sparse():
        bi = torch.arange(B, device=dev)[:, None]
        Ti, Tj = poses[bi, fi_c], poses[bi, fj_c]
        wi = (Ti[..., :3, :3] * pos[..., None, 2:5]).sum(-1) + Ti[..., :3, 3]      # (elementwise: a batched 3 x 3 matmul over 6.7 M entries measured 187 ms)
        wj = (Tj[..., :3, :3] * pos[..., None, 5:8]).sum(-1) + Tj[..., :3, 3]
        e = torch.where(valid, ((wi - wj).double() ** 2).sum(-1), torch.zeros((), dtype=torch.float64, device=dev))
        out = e > delta * delta
        rho = torch.where(out, 2 * delta * e.sqrt() - delta * delta, e)
        return e.sum(1), rho.sum(1), (out & valid).sum(1)

    t_sq, t_rho, t_out = torch_sparse()
    torch.cuda.synchronize()
    res = dict(
        workload=dict(config="c3", K=K, corr_per_pair=M, instances=B, cache="160x120", warmup=WARMUP, reps=REPS, device=torch.cuda.get_device_name(0)),
        ms_median_min_max=dict(
            objective_zn=median_ms(lambda: bs.objective_zn(*args_, poses, device=True)),
            objective_sparse=median_ms(lambda: sparse_only.objective_zn(*args_, poses, device=True)),
            linearize_zn=median_ms(lambda: bs.linearize_zn(*args_, poses)),
            torch_sparse=median_ms(torch_sparse),
        ),
        objective_before_after_instance0=[float(before[0]["objective"][0]), float(after[0]["objective"][0])],
        outliers_before_after_instance0=[int(before[1]["n_outlier"][0].sum() + before[2]["n_outlier"][0].sum()), int(after[1]["n_outlier"][0].sum() + after[2]["n_outlier"][0].sum())],
        residual_variance_after_min_max=[float(residual_variance(after[0], K).min()), float(residual_variance(after[0], K).max())],
        # (torch evaluates at the given matrices, the report at Exp(Log(.)) of them: equal to fp32 round-off, not bit for bit)
        sparse_rho_rel_diff_to_torch_max=float(np.abs(after[0]["sparse_rho"] - t_rho.cpu().numpy()).max() / np.abs(after[0]["sparse_rho"]).max()),
        sparse_outliers_minus_torch_min_max=[int((after[1]["n_outlier"].sum(1) - t_out.cpu().numpy()).min()), int((after[1]["n_outlier"].sum(1) - t_out.cpu().numpy()).max())],
    )
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
