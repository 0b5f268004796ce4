"""Timing of btba_pose_errors (ADD / ADD-S) at four sizes, one JSON line.  GPU box only.
    python scripts/eval_timing.py              hipEvent time per call, and the same cases under rocprofv3 --kernel-trace --stats
                                               (each case in a fresh child process), next to the bounds below
    python scripts/eval_timing.py --no-rocprof hipEvent times only
Cases: one frame of 2620 points (the tracker's per-frame case), a sequence of 1000 frames, a dataset of 10 000 frames, one frame
of a dense 100 000-point model.  Per case:
  pairs_per_s     : evaluations x N^2 (query, candidate) pairs over the rocprofv3 kernel time (hipEvent time without rocprofv3)
  valu_bound_us   : the pairs at the VALU issue bound: VALU instructions per pair counted in k_eval_nn's inner loop of the
                    -save-temps ISA (v_pk_* count once), 256 CUs x 4 SIMDs x 64 lanes / 4 cycles per wave instruction at 2.4 GHz
                    (MI355X_MICROARCH: v_fma_f32 4 cycles; v_pk_fma_f32 at the 157.3 TFLOP/s vector peak is the same issue rate)
  valu_frac       : valu_bound_us / kernel time of k_eval_nn
  ckdtree_ms      : scipy cKDTree(workers=16) build + query on the same points (ADD-S only), the reference's method."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

CASES = {"frame_2620": (1, 2620), "sequence_1000x2620": (1000, 2620), "dataset_10000x2620": (10000, 2620), "dense_1x100000": (1, 100000)}
LANE_ISSUE_PER_S = 256 * 4 * 64 * 2.4e9 / 4


def inputs(name):
    from bundletrack_amd import synthetic as S
    from eval_ref import scene_poses
    n_evals, n = CASES[name]
    pred, gt = scene_poses(min(n_evals, 97), 7)
    idx = np.arange(n_evals) % pred.shape[0]
    return S.model_points(n, 7), pred[idx], gt[idx]


def event_ms(name, reps):
    import torch
    from bundletrack_amd.evaluation import pose_errors
    from bundletrack_amd.optimizer import Workspace
    model, pred, gt = inputs(name)
    ws = Workspace()
    m, p, g = torch.from_numpy(model).cuda(), torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    for _ in range(3):
        pose_errors(ws, m, p, g)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record()
        pose_errors(ws, m, p, g)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    ws.close()
    return float(np.median(times))


def ckdtree_ms(name):
    from scipy.spatial import cKDTree
    model, pred, gt = inputs(name)
    n_evals = pred.shape[0]
    k = min(n_evals, 20)                                         # timed on up to 20 evaluations, scaled
    t0 = time.perf_counter()
    for e in range(k):
        c = model.astype(np.float64) @ pred[e, :3, :3].T.astype(np.float64) + pred[e, :3, 3]
        q = model.astype(np.float64) @ gt[e, :3, :3].T.astype(np.float64) + gt[e, :3, 3]
        cKDTree(c).query(q, k=1, workers=16)
    return (time.perf_counter() - t0) * 1e3 * n_evals / k


def valu_per_pair():
    """VALU instructions per (query, candidate) pair in k_eval_nn's inner loop, from the -save-temps ISA of btba_api_eval.hip."""
    from bundletrack_amd import _lib
    with tempfile.TemporaryDirectory() as d:
        _lib.build(force=True, out=os.path.join(d, "lib.so"), extra_flags=["-save-temps"])
        isa = open(glob.glob(os.path.join(d, "build", "lib", "btba_api_eval-*gfx950*.s"))[0]).read()
    body = isa[isa.index("_ZN4btba9k_eval_nn"):]
    body = body[:body.index("s_endpgm")]
    blocks = re.split(r"\n\.LBB\d+_\d+:", body)
    loop = max(blocks, key=lambda b: b.count("v_pk_fma_f32"))
    ops = [ln.split()[0] for ln in loop.split("\n") if ln.strip() and not ln.strip().startswith((";", "."))]
    valu = sum(1 for o in ops if o.startswith("v_"))
    pairs = sum(1 for o in ops if o == "v_pk_fma_f32")           # two v_pk_fma_f32 per d2 of two queries: one per pair
    return valu / pairs, {o: ops.count(o) for o in sorted(set(ops))}


def rocprof_us(name, reps):
    """Kernel time per call (k_eval_nn, k_eval_reduce), from rocprofv3 --kernel-trace --stats of a fresh child process."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "eval", "--", sys.executable, os.path.abspath(__file__),
               "--child", name, "--reps", str(reps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise RuntimeError("no kernel stats from rocprofv3")
        per = {}
        for row in csv.DictReader(open(stats[0])):
            if "k_eval" in row["Name"]:
                per[row["Name"].split("(")[0].split("::")[-1]] = float(row["TotalDurationNs"]) / (reps + 3) / 1e3
        return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:                                   # under rocprofv3: warm-up + reps calls of one case, no output
        event_ms(a.child, a.reps)
        return
    vpp, mix = valu_per_pair()
    out = {"what": "btba_pose_errors", "valu_per_pair": round(vpp, 3), "inner_loop": mix, "cases": {}}
    for name, (n_evals, n) in CASES.items():
        ms = event_ms(name, a.reps)
        pairs = n_evals * n * n
        bound_us = pairs * vpp / LANE_ISSUE_PER_S * 1e6
        row = {"evals": n_evals, "points": n, "event_us": round(ms * 1e3, 1), "valu_bound_us": round(bound_us, 1),
               "pairs_per_s_event": float(f"{pairs / (ms * 1e-3):.4g}"), "ckdtree_ms": round(ckdtree_ms(name), 1)}
        if not a.no_rocprof:
            per = rocprof_us(name, a.reps)
            nn = sum(v for k, v in per.items() if "k_eval_nn" in k)
            row["rocprof_kernel_us"] = {k: round(v, 1) for k, v in per.items()}
            row["pairs_per_s_kernel"] = float(f"{pairs / (sum(per.values()) * 1e-6):.4g}")
            row["valu_frac"] = round(bound_us / nn, 3) if nn else None
        out["cases"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
