#!/usr/bin/env python3
"""Times btba_vos_propagate against the reference's method on the same GPU, and writes profiles/vos_timing.json.

At the tracker's shape -- a 60 x 80 grid, 256 channels, nine references, two classes -- for 1 and for 8 videos:
  (a) fused   one btba_vos_propagate call (two launches per four videos; no similarity matrix, no weight tables)
  (b) torch   lib/predict.py's formulas restated in torch on the same device: mm, softmax over all keys, the two [HW, HW] weight tables
              (built once, outside the timed region, as run_video.py builds them), mm with the labels; video after video
(b) is measured before and after (a); the distance between its two medians is its own run-to-run spread.  Each figure is the median
of device-event times over --repeats calls after --warmup calls.  Bytes: (a) the workspace scratch the call needs (computed from the
shapes as the library does) plus its outputs; (b) torch's peak allocation during one call above what was allocated before it, plus
the two tables.  The product is 2 * C * HW * n_ref * HW FLOP per video (106 GFLOP); its time at the fp32 matrix peak of 157.3 TFLOP/s
is the floor the result is stated against.  Before anything is timed both results for the first video are held against the same formulas in fp64 on the device
(max |x - x64| / max_c |x64[:, q]|).  Needs a GPU: no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MATRIX = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vos_timing.json"))
    args = ap.parse_args()
    import torch
    from bundletrack_amd import vos
    from bundletrack_amd.optimizer import Workspace
    if not torch.cuda.is_available():
        sys.exit("vos_timing.py needs a GPU")
    Hd, Wd, Cn, d, n_ref, n_dense = 60, 80, 256, 2, 9, 4
    HW = Hd * Wd
    ws = Workspace()
    gen = torch.Generator(device="cuda").manual_seed(0)

    def video():
        base = torch.randn((Cn, HW), generator=gen, device="cuda")
        feats = (base[None] + 0.5 * torch.randn((n_ref + 1, Cn, HW), generator=gen, device="cuda")) * (0.33 * Cn ** -0.25 * 3.0)
        cls = torch.randint(0, d, (n_ref, HW), generator=gen, device="cuda")
        labels = torch.nn.functional.one_hot(cls, d).permute(0, 2, 1).float().contiguous()
        return feats[:n_ref].contiguous(), labels, feats[n_ref].contiguous()

    def tables():
        i = torch.arange(HW, device="cuda")
        yx = torch.stack((i // Wd, i % Wd), -1)
        d2 = (yx - yx.unsqueeze(1)).float().pow(2).sum(-1)
        return (-d2 / 8.0 ** 2).exp(), (-d2 / 21.0 ** 2).exp()

    def torch_predict(refs, labels, tgt, w_dense, w_sparse):
        sim = refs.permute(0, 2, 1).reshape(-1, Cn).mm(tgt)
        sim = sim.softmax(dim=0).view(n_ref, HW, HW)
        sim[:-n_dense] *= w_sparse
        sim[-n_dense:] *= w_dense
        return labels.permute(1, 0, 2).reshape(d, -1).mm(sim.view(-1, HW))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts)), float(np.min(ts))

    w_dense, w_sparse = tables()
    result = {"shape": dict(Hd=Hd, Wd=Wd, C=Cn, d=d, n_ref=n_ref, n_dense=n_dense), "repeats": args.repeats, "warmup": args.warmup,
              "gflop_per_video": 2.0 * Cn * HW * n_ref * HW / 1e9, "floor_ms_per_video_at_fp32_matrix_peak": 2.0 * Cn * HW * n_ref * HW / PEAK_FP32_MATRIX * 1e3,
              "runs": []}
    for n in (1, 8):
        vids = [video() for _ in range(n)]
        refs = [[r for r in v[0]] for v in vids]
        labs = [[l for l in v[1]] for v in vids]
        tgts = [v[2] for v in vids]
        pred = [torch.empty((d, Hd, Wd), device="cuda") for _ in range(n)]
        hot = [torch.empty((d, Hd, Wd), device="cuda") for _ in range(n)]

        def fused():
            vos.propagate(ws, refs, labs, tgts, [n_dense] * n, Hd, Wd, None, pred_out=pred, onehot_out=hot)

        def by_torch():
            return [torch_predict(v[0], v[1], v[2], w_dense, w_sparse) for v in vids]

        fused()
        want = by_torch()
        torch.cuda.synchronize()
        v0 = [t.double() for t in vids[0]]
        p64 = torch_predict(v0[0], v0[1], v0[2], w_dense.double(), w_sparse.double())      # the first video in fp64: which of the two is closer
        col = p64.abs().amax(0, keepdim=True)
        err_fused, err_torch = (float(((x.reshape(d, -1).double() - p64).abs() / col).max()) for x in (pred[0], want[0]))
        del want, v0, p64, col
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        by_torch()
        torch.cuda.synchronize()
        torch_bytes = torch.cuda.max_memory_allocated() - before + 2 * HW * HW * 4
        t1 = timed(by_torch)
        f = timed(fused)
        t2 = timed(by_torch)
        run = {"videos": n, "fused_ms_median": f[0], "fused_ms_min": f[1], "torch_ms_median_before": t1[0], "torch_ms_median_after": t2[0],
               "torch_ms_min": min(t1[1], t2[1]), "fused_bytes": 16 * (2 + d) * HW * 4 * n + 2 * d * HW * 4 * n, "torch_bytes": int(torch_bytes),
               "fused_tflops": result["gflop_per_video"] * n / f[0], "fused_share_of_fp32_matrix_peak": result["gflop_per_video"] * n / f[0] * 1e9 / PEAK_FP32_MATRIX * 1e3,
               "fused_max_rel_err_vs_fp64": err_fused, "torch_max_rel_err_vs_fp64": err_torch}
        print(json.dumps(run))
        result["runs"].append(run)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
