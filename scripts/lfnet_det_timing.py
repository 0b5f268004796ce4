#!/usr/bin/env python3
"""Times the detector net (btba_lfnet_scores) and writes profiles/lfnet_det_timing.json.

At the release shape -- 16 channels, 5 x 5 windows, 3 blocks, 5 scales sqrt(2) .. 1 / sqrt(2), leaky relu, seeded weights -- on
400 x 400 photos, 1 and 32 frames:
  scores        one btba_lfnet_scores call (no host wait) into preallocated maps, per call and per frame
  share         of the 157.3 TFLOP/s fp32 peak, from 13.4 GFLOP per frame
  torch         the same net with the same weights as torch ops on the same GPU (what a caller does today): conv2d with padding
                k / 2, the folded norms, leaky relu, TF1's resize as a gather of the four taps (interpolate is not TF1's rule), the
                score and orientation convolutions, the normalisation.  If torch's convolution cannot run there the JSON says so.
Each figure is the median of device-event times over --repeats calls after --warmup calls; the torch form is measured before and
after the library, and the distance between its two medians is its own run-to-run spread.  Needs a GPU: no CPU fallback."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FLOP_PER_FRAME = 13.4e9
PEAK_FP32 = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lfnet_det_timing.json"))
    args = ap.parse_args()
    import torch
    import lfnet_det_ref as R
    from lfnet_ref import resize_taps
    from bundletrack_amd import _lib, lfnet_det
    from bundletrack_amd.optimizer import Workspace
    if not torch.cuda.is_available():
        sys.exit("lfnet_det_timing.py needs a GPU")
    F = torch.nn.functional
    cfg = R.config()
    weights = R.model_weights(R.make_model(7, cfg))
    ws = Workspace()
    net = lfnet_det.LfnetScoreNet(ws, weights)
    H = W = args.size
    k, Cn, alpha = cfg["ksize"], cfg["channels"], cfg["leaky_alpha"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    conv_w = lambda name: dev(weights[f"ConvOnlyResNet/{name}/weights"]).permute(3, 2, 0, 1).contiguous()
    bias = lambda name: weights.get(f"ConvOnlyResNet/{name}/biases")
    pair = lambda name, n, b=None: tuple(dev(v)[None, :, None, None] for v in R.N.fold(weights, R.SCOPE, name, n, cfg["bn_eps"], b))
    init = (conv_w("init_conv"), pair("none", Cn, bias("init_conv")))
    blocks = []
    for i in range(1, cfg["blocks"] + 1):
        b = f"block-{i}"
        blocks.append((pair(f"{b}/pre-bn", Cn), conv_w(f"{b}/conv1"), pair(f"{b}/mid-bn", Cn, bias(f"{b}/conv1")), conv_w(f"{b}/conv2"),
                       pair("none", Cn, bias(f"{b}/conv2"))))
    fin = pair("fin-bn", Cn)
    heads = []
    for j, (h, w) in enumerate(R.map_sizes(cfg, H, W)):
        taps = None
        if (h, w) != (H, W):
            ya, yb, fy = resize_taps(H, h, np.float32)
            xa, xb, fx = resize_taps(W, w, np.float32)
            taps = (torch.from_numpy(ya).cuda(), torch.from_numpy(yb).cuda(), dev(fy)[None, None, :, None], torch.from_numpy(xa).cuda(),
                    torch.from_numpy(xb).cuda(), dev(fx)[None, None, None, :])
        heads.append((taps, conv_w(f"score_conv_{j}"), pair("none", 1, bias(f"score_conv_{j}"))))
    ori = (conv_w("ori_conv"), pair("none", 2, bias("ori_conv")))
    act = lambda x: F.leaky_relu(x, alpha)
    affine = lambda x, p: x * p[0] + p[1]

    def by_torch(photo):
        x = affine(F.conv2d(photo[:, None], init[0], padding=k // 2), init[1])
        for pre, w1, mid, w2, out in blocks:
            t = act(affine(F.conv2d(act(affine(x, pre)), w1, padding=k // 2), mid))
            x = affine(F.conv2d(t, w2, padding=k // 2), out) + x
        f = act(affine(x, fin))
        maps = []
        for taps, w, p in heads:
            r = f
            if taps is not None:
                ya, yb, fy, xa, xb, fx = taps
                top, bot = f[:, :, ya], f[:, :, yb]
                top = top[..., xa] + (top[..., xb] - top[..., xa]) * fx
                bot = bot[..., xa] + (bot[..., xb] - bot[..., xa]) * fx
                r = top + (bot - top) * fy
            maps.append(affine(F.conv2d(r, w, padding=k // 2), p)[:, 0])
        o = affine(F.conv2d(f, ori[0], padding=k // 2), ori[1])
        o = o * torch.rsqrt(torch.clamp((o * o).sum(1, keepdim=True), min=1e-12))
        return maps, o.permute(0, 2, 3, 1)

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

    shape = {key: cfg[key] for key in ("channels", "ksize", "blocks", "num_scales", "scale_factors", "activation", "leaky_alpha", "bn_eps")}
    result = {"shape": dict(shape, H=H, W=W), "flop_per_frame": FLOP_PER_FRAME, "peak_fp32_flops": PEAK_FP32, "repeats": args.repeats,
              "warmup": args.warmup, "runs": []}
    gen = torch.Generator(device="cuda").manual_seed(0)
    L = _lib.lib()
    for n in (1, 32):
        photo = torch.rand((n, H, W), generator=gen, device="cuda")
        run = {"frames": n}
        try:
            torch_ok = True
            want_maps, want_ori = by_torch(photo)
            torch.cuda.synchronize()
            t1 = timed(lambda: by_torch(photo))
        except RuntimeError as e:
            torch_ok = False
            run["torch"] = f"torch's convolution could not run here: {str(e).splitlines()[0]}"
        maps, o = net.scores(photo)                          # the call itself, without the allocations, is what is timed
        table = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
        call = lambda: _lib.check(L.btba_lfnet_scores(ws.handle, net.handle, n, H, W, photo.data_ptr(), C.cast(table, C.c_void_p), o.data_ptr()),
                                  "btba_lfnet_scores")
        torch.cuda.synchronize()
        lib = timed(call)
        run.update({"scores_ms_median": lib[0], "scores_ms_min": lib[1], "ms_per_frame": lib[0] / n,
                    "share_of_fp32_peak": n * FLOP_PER_FRAME / (lib[0] * 1e-3) / PEAK_FP32})
        if torch_ok:
            t2 = timed(lambda: by_torch(photo))
            diff = max(float(((a - b).abs().max() / b.abs().max())) for a, b in zip(maps, want_maps))
            run.update({"torch_ms_median_before": t1[0], "torch_ms_median_after": t2[0], "torch_ms_min": min(t1[1], t2[1]),
                        "torch_ms_per_frame": min(t1[0], t2[0]) / n, "torch_max_rel_diff_scores": diff,
                        "torch_max_abs_diff_orientation": float((o - want_ori).abs().max())})
        print(json.dumps(run))
        result["runs"].append(run)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
