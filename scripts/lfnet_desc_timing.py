#!/usr/bin/env python3
"""Times the descriptor net (btba_lfnet_descriptors) and writes profiles/lfnet_desc_timing.json.

At the release shape -- 32 x 32 patches, 64 / 3 / 512 / 256, relu, l2norm, seeded weights -- for 500 patches x 1 frame and x 32 frames:
  descriptors   one btba_lfnet_descriptors call (no host wait), per call and per frame
  share         of the 157.3 TFLOP/s fp32 peak, from 23.6 MFLOP per patch
  torch         the same net with the same weights as torch ops on the same GPU (what a caller does today): F.pad (0, 1, 0, 1) +
                conv2d stride 2, the folded batch norm, relu, the (h, w, c) flatten, two matmuls, normalize.  If torch's convolution
                cannot run there the JSON says so.
Each figure is the median of device-event times over --repeats calls after --warmup calls; the torch form is measured before and
after the library, and the distance between its two medians is its own run-to-run spread.  Needs a GPU: no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLOP_PER_PATCH = 23.6e6
PEAK_FP32 = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lfnet_desc_timing.json"))
    args = ap.parse_args()
    import torch
    import lfnet_desc_ref as R
    from bundletrack_amd import lfnet_desc
    from bundletrack_amd.optimizer import Workspace
    if not torch.cuda.is_available():
        sys.exit("lfnet_desc_timing.py needs a GPU")
    F = torch.nn.functional
    cfg = R.config()
    weights = R.model_weights(R.make_model(7, cfg))
    ws = Workspace()
    net = lfnet_desc.LfnetDescriptor(ws, weights)
    gen = torch.Generator(device="cuda").manual_seed(0)

    layers = []
    for layer, bn in R.layer_scopes(cfg["depth"]):
        w = weights[f"SimpleDesc/{layer}/weights"]
        scale, shift = R.fold(weights, R.SCOPE, bn, w.shape[-1], cfg["bn_eps"], weights.get(f"{R.SCOPE}/{layer}/biases"))
        wt = torch.from_numpy(w).cuda()
        layers.append((wt.permute(3, 2, 0, 1).contiguous() if w.ndim == 4 else wt, torch.from_numpy(scale.astype(np.float32)).cuda(),
                       torch.from_numpy(shift.astype(np.float32)).cuda()))

    def by_torch(patches):
        x = patches.reshape(-1, 1, 32, 32)
        for w, sc, sh in layers[:cfg["depth"]]:
            x = torch.relu(F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2) * sc[None, :, None, None] + sh[None, :, None, None])
        x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
        x = torch.relu(x @ layers[-2][0] * layers[-2][1] + layers[-2][2])
        x = x @ layers[-1][0] * layers[-1][1] + layers[-1][2]
        return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))

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

    result = {"shape": dict(cfg, patches_per_frame=500), "flop_per_patch": FLOP_PER_PATCH, "peak_fp32_flops": PEAK_FP32,
              "repeats": args.repeats, "warmup": args.warmup, "runs": []}
    for n in (1, 32):
        patches = torch.rand((n, 500, 32, 32), generator=gen, device="cuda")
        run = {"frames": n, "patches": n * 500}
        try:
            torch_ok = True
            want = by_torch(patches)
            torch.cuda.synchronize()
            t1 = timed(lambda: by_torch(patches))
        except RuntimeError as e:
            torch_ok = False
            run["torch"] = f"torch's convolution could not run here: {str(e).splitlines()[0]}"
        got = net.describe(patches)
        torch.cuda.synchronize()
        lib = timed(lambda: net.describe(patches))
        run.update({"descriptors_ms_median": lib[0], "descriptors_ms_min": lib[1], "ms_per_frame": lib[0] / n,
                    "share_of_fp32_peak": n * 500 * FLOP_PER_PATCH / (lib[0] * 1e-3) / PEAK_FP32})
        if torch_ok:
            t2 = timed(lambda: by_torch(patches))
            run.update({"torch_ms_median_before": t1[0], "torch_ms_median_after": t2[0], "torch_ms_min": min(t1[1], t2[1]),
                        "torch_ms_per_frame": min(t1[0], t2[0]) / n, "torch_max_abs_diff": float((want.reshape(got.shape) - got).abs().max())})
        print(json.dumps(run))
        result["runs"].append(run)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
