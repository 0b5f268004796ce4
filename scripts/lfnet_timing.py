#!/usr/bin/env python3
"""Times the keypoint head (btba_lfnet_*) and writes profiles/lfnet_timing.json.

At the detector's shape -- 400 x 400, the five shipped scales, default parameters -- for 1 and for 8 frames:
  heatmaps / select / crops   each stage's call on its own
  keypoints                   btba_lfnet_keypoints, the three in one call (no host wait: n_kpts stays on the device)
  torch                       the same stages as plain torch ops on the same GPU, for scale: instance norm, a gathered TF1 resize,
                              max_pool3d / conv3d for the scale-space soft-max, the soft arg-max, 24 shifted comparisons for the
                              NMS, topk, nonzero, and gathered bilinear crops.  It is not held to the library's bit rules.
Each figure is the median of device-event times over --repeats calls after --warmup calls; the torch form is measured before and
after the library, and the distance between its two medians is its own run-to-run spread.  Needs a GPU: no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lfnet_timing.json"))
    args = ap.parse_args()
    import torch
    from bundletrack_amd import lfnet
    from bundletrack_amd._lib import lfnet_params
    from bundletrack_amd.optimizer import Workspace
    if not torch.cuda.is_available():
        sys.exit("lfnet_timing.py needs a GPU")
    F = torch.nn.functional
    H = W = 400
    sf = [2.0 ** 0.5, 2.0 ** 0.25, 1.0, 2.0 ** -0.25, 2.0 ** -0.5]
    p = lfnet_params()
    K, P, L, k = p.top_k, p.patch_size, p.kp_loc_size, p.sm_ksize
    ws = Workspace()
    gen = torch.Generator(device="cuda").manual_seed(0)

    def taps(n_in, n_out):
        src = torch.arange(n_out, device="cuda", dtype=torch.float32) * (np.float32(n_in) / np.float32(n_out))
        lo = src.floor().long().clamp(max=n_in - 1)
        return lo, (lo + 1).clamp(max=n_in - 1), src - lo.float()

    def t_resize(x):
        ya, yb, fy = taps(x.shape[-2], H)
        xa, xb, fx = taps(x.shape[-1], W)
        top = x[:, ya][:, :, xa] + (x[:, ya][:, :, xb] - x[:, ya][:, :, xa]) * fx
        bot = x[:, yb][:, :, xa] + (x[:, yb][:, :, xb] - x[:, yb][:, :, xa]) * fx
        return top + (bot - top) * fy[:, None]

    def mask(r):
        m = torch.zeros((H, W), device="cuda")
        m[r:H - r, r:W - r] = 1.0
        return m

    def t_crop(img, b, n, kx, ky, a, bb, c, d):
        g = torch.linspace(-1.0, 1.0, n, device="cuda")
        gx, gy = g[None, None, :], g[None, :, None]
        x = (a[:, None, None] * gx + bb[:, None, None] * gy) * n / 2.0 + kx[:, None, None]
        y = (c[:, None, None] * gx + d[:, None, None] * gy) * n / 2.0 + ky[:, None, None]
        x0, y0 = x.floor().long(), y.floor().long()
        x1, y1 = (x0 + 1).clamp(0, W - 1), (y0 + 1).clamp(0, H - 1)
        x0, y0 = x0.clamp(0, W - 1), y0.clamp(0, H - 1)
        bi = b[:, None, None]
        return ((x1 - x) * (y1 - y)) * img[bi, y0, x0] + ((x1 - x) * (y - y0)) * img[bi, y1, x0] + ((x - x0) * (y1 - y)) * img[bi, y0, x1] + \
               ((x - x0) * (y - y0)) * img[bi, y1, x1]

    def t_heat(maps):
        logits = []
        for m in maps:
            mean, var = m.mean((1, 2), keepdim=True), m.var((1, 2), unbiased=False, keepdim=True)
            inv = torch.rsqrt(var + 1e-3)
            logits.append(t_resize(m * inv - mean * inv))
        x = torch.stack(logits, 1)                                                   # [n, S, H, W]
        S = x.shape[1]
        mx = F.max_pool3d(x[:, None], (S, k, k), stride=(S, 1, 1), padding=(0, k // 2, k // 2))[:, 0]
        e = torch.exp(p.com_strength * (x - mx))
        sm = F.conv3d(e[:, None], torch.ones((1, 1, S, k, k), device="cuda"), stride=(S, 1, 1), padding=(0, k // 2, k // 2))[:, 0]
        pr = e / (sm + 1e-6)
        a = torch.softmax(p.score_com_strength * pr, 1)
        b = torch.softmax(p.scale_com_strength * pr, 1)
        return (pr * a).sum(1) * mask(p.pad_size), (torch.tensor(sf, device="cuda")[None, :, None, None] * b).sum(1)

    def t_select(heat):
        hk = p.nms_ksize // 2
        works = torch.where(heat < p.nms_thresh, torch.zeros_like(heat), heat)
        pad = F.pad(works, (hk, hk, hk, hk))
        peak = torch.ones_like(heat, dtype=torch.bool)
        for dy in range(p.nms_ksize):
            for dx in range(p.nms_ksize):
                if dy != hk or dx != hk:
                    peak &= works > pad[:, dy:dy + H, dx:dx + W]
        score = heat * peak * mask(p.crop_radius)
        idx = score.reshape(score.shape[0], -1).topk(K, sorted=False).indices
        top = torch.zeros_like(score).reshape(score.shape[0], -1).scatter_(1, idx, 1.0).reshape(score.shape) * peak
        return torch.nonzero(top > 0)                                                # [m, 3] (b, y, x): the host learns m here

    def t_crops(photo, ori, heat, scl, byx):
        b, ky, kx = byx[:, 0], byx[:, 1], byx[:, 2]
        s, o = scl[b, ky, kx], ori[b, ky, kx]
        z = torch.zeros_like(s)
        v = t_crop(heat, b, L, kx.float(), ky.float(), s, z, z, s)
        w = torch.softmax((p.kp_com_strength * v).reshape(len(b), -1), 1).reshape(v.shape)
        g = torch.linspace(-1.0, 1.0, L, device="cuda")
        rx = kx.float() + (w * g[None, None, :]).sum((1, 2)) * s * L / 2
        ry = ky.float() + (w * g[None, :, None]).sum((1, 2)) * s * L / 2
        return t_crop(photo, b, P, rx, ry, s * o[:, 0], -s * o[:, 1], s * o[:, 1], s * o[:, 0])

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

    result = {"shape": dict(H=H, W=W, S=len(sf), top_k=K, sm_ksize=k, patch_size=P), "repeats": args.repeats, "warmup": args.warmup, "runs": []}
    for n in (1, 8):
        maps = [torch.rand((n, int(H / s + 0.5), int(W / s + 0.5)), generator=gen, device="cuda") for s in sf]
        photo = torch.rand((n, H, W), generator=gen, device="cuda")
        ang = torch.rand((n, H, W), generator=gen, device="cuda") * 6.2831853
        ori = torch.stack((ang.cos(), ang.sin()), -1).contiguous()
        heat, scl = lfnet.lfnet_heatmaps(ws, maps, sf, H, W, p)
        kxy, cnt = lfnet.lfnet_select(ws, heat, p)
        torch.cuda.synchronize()
        th, ts_ = t_heat(maps)
        err_heat = float((th - heat).abs().max())
        n_lib, n_torch = int(cnt.sum()), int(t_select(heat).shape[0])

        def by_torch():
            h, s = t_heat(maps)
            return t_crops(photo, ori, h, s, t_select(h))

        t1 = timed(by_torch)
        a = timed(lambda: lfnet.lfnet_heatmaps(ws, maps, sf, H, W, p))
        b = timed(lambda: lfnet.lfnet_select(ws, heat, p))
        c = timed(lambda: lfnet.lfnet_crops(ws, photo, ori, heat, scl, kxy, cnt, p))
        whole = timed(lambda: lfnet.lfnet_keypoints(ws, maps, sf, photo, ori, p, wait=False))
        t_a = timed(lambda: t_heat(maps))
        t2 = timed(by_torch)
        run = {"frames": n, "keypoints": n_lib, "torch_keypoints_on_the_same_heat": n_torch, "torch_heat_max_abs_diff": err_heat,
               "heatmaps_ms_median": a[0], "select_ms_median": b[0], "crops_ms_median": c[0], "keypoints_ms_median": whole[0],
               "keypoints_ms_min": whole[1], "torch_heatmaps_ms_median": t_a[0], "torch_ms_median_before": t1[0], "torch_ms_median_after": t2[0],
               "torch_ms_min": min(t1[1], t2[1])}
        print(json.dumps(run))
        result["runs"].append(run)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
