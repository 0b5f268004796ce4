#!/usr/bin/env python3
"""Times the segmentation backbone (btba_vos_features) and writes profiles/vos_net_timing.json.

resnet50 (Bottleneck, 3 / 4 / 6 / 3) with seeded weights on 480 x 640 frames, 1 and 8 frames:
  features      one btba_vos_features call (no host wait) into a preallocated output, per call and per frame
  share         of the 157.3 TFLOP/s fp32 peak, from the multiply-adds of the net's convolutions (2 FLOP each) derived from the layer
                table and the output-size rule: a whole-call rate over peak, launches and the memory-bound stem and pool included
  torch         the same net with the same weights as torch ops on the same GPU (what a caller does today): conv2d, the folded
                norms, relu, max_pool2d.  If torch's convolution cannot run there the JSON says so.
  stem and pool the stem convolution and the max pool are two launches with the 64-channel map stored in between.  With
                --kernel-stats (the *_kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this script, taken in a run
                of its own) the average time of each of the three kernels goes into the JSON; a fused single launch has not been built.
Each figure is the median of device-event times over --repeats calls after --warmup calls; the torch form is measured before and
after the library, and the distance between its two medians is its own run-to-run spread.  Needs a GPU: no CPU fallback."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_FP32 = 157.3e12


def macs_per_frame(R, cfg, H, W):
    """Multiply-adds of one H x W frame: every convolution's outputs x its K, sizes by (in + 2 pad - k) // stride + 1."""
    size = lambda v, k, s: (v + 2 * (k // 2) - k) // s + 1
    table = {t[0]: t for t in R.layer_table(cfg)}
    total = 0.0

    def conv(name, hw):
        nonlocal total
        _, _, cout, cin, k, stride = table[name]
        hw = (size(hw[0], k, stride), size(hw[1], k, stride))
        total += float(hw[0] * hw[1] * cout) * k * k * cin
        return hw

    hw = conv("backbone.0", (H, W))
    hw = (size(hw[0], 3, 2), size(hw[1], 3, 2))
    for s in range(4):
        for b in range(cfg["layers"][s]):
            p = f"backbone.{4 + s}.{b}"
            if f"{p}.downsample.0" in table:
                conv(f"{p}.downsample.0", hw)
            hw = conv(f"{p}.conv1", hw)
            hw = conv(f"{p}.conv2", hw)
            if cfg["block"] == R.BOTTLENECK:
                hw = conv(f"{p}.conv3", hw)
    if cfg["block"] == R.BOTTLENECK:
        conv("adjust_dim", hw)
    return total


def kernel_stats(path):
    """{kernel: {calls, average_us, us_per_forward}} of the backbone's kernels out of rocprofv3's kernel stats (Name, Calls,
    TotalDurationNs) or its kernel trace (Kernel_Name, Start_Timestamp, End_Timestamp); a forward is one k_vos_stem call."""
    calls, total = {}, {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("Kernel_Name") or ""
            for k in ("k_vos_stem", "k_vos_pool", "k_vos_conv"):
                if k in name:
                    if "TotalDurationNs" in row:
                        calls[k] = calls.get(k, 0) + int(row["Calls"])
                        total[k] = total.get(k, 0.0) + float(row["TotalDurationNs"])
                    else:
                        calls[k] = calls.get(k, 0) + 1
                        total[k] = total.get(k, 0.0) + float(row["End_Timestamp"]) - float(row["Start_Timestamp"])
    forwards = max(calls.get("k_vos_stem", 1), 1)
    return {k: {"calls": calls[k], "average_us": total[k] / calls[k] / 1e3, "us_per_forward": total[k] / forwards / 1e3} for k in calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch form (a profiler run)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv of a separate run of this script")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vos_net_timing.json"))
    args = ap.parse_args()
    import torch
    import vos_net_ref as R
    from bundletrack_amd import _lib, vos_net
    from bundletrack_amd.optimizer import Workspace
    if not torch.cuda.is_available():
        sys.exit("vos_net_timing.py needs a GPU")
    F = torch.nn.functional
    cfg = R.config()
    weights = R.model_weights(R.make_model(7, cfg))
    ws = Workspace()
    net = vos_net.VosBackbone(ws, weights, cfg)
    H, W = args.height, args.width
    macs = macs_per_frame(R, cfg, H, W)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    table = {t[0]: t for t in R.layer_table(cfg)}
    layers = {}
    for name, (_, bn, _, _, k, stride) in table.items():
        scale, shift = R.fold(weights, bn, cfg["bn_eps"], np.float32)
        layers[name] = (dev(weights[f"{name}.weight"]), dev(scale)[None, :, None, None], dev(shift)[None, :, None, None], stride, k // 2)

    def cb(x, name, relu, res=None):
        w, scale, shift, stride, pad = layers[name]
        y = F.conv2d(x, w, stride=stride, padding=pad) * scale + shift
        if res is not None:
            y = y + res
        return F.relu(y) if relu else y

    def by_torch(x):
        v = F.max_pool2d(cb(x, "backbone.0", True), 3, 2, 1)
        for s in range(4):
            for b in range(cfg["layers"][s]):
                p = f"backbone.{4 + s}.{b}"
                t = cb(cb(v, f"{p}.conv1", True), f"{p}.conv2", True)
                res = cb(v, f"{p}.downsample.0", False) if f"{p}.downsample.0" in layers else v
                v = cb(t, f"{p}.conv3", True, res)
        return cb(v, "adjust_dim", False)

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

    result = {"shape": dict(block=cfg["block"], layers=cfg["layers"], bn_eps=cfg["bn_eps"], H=H, W=W), "gmac_per_frame": macs / 1e9,
              "flop_per_frame": 2.0 * macs, "peak_fp32_flops": PEAK_FP32, "repeats": args.repeats, "warmup": args.warmup,
              "stem_and_pool": {"launches": 2, "fused_single_launch": "not built"}, "runs": []}
    if args.kernel_stats:
        result["stem_and_pool"]["kernels"] = kernel_stats(args.kernel_stats)
    gen = torch.Generator(device="cuda").manual_seed(0)
    L = _lib.lib()
    for n in args.frames:
        rgb = torch.randn((n, 3, H, W), generator=gen, device="cuda")
        run = {"frames": n}
        torch_ok = False
        if not args.no_torch:
            try:
                want = by_torch(rgb)
                torch.cuda.synchronize()
                t1 = timed(lambda: by_torch(rgb))
                torch_ok = True
            except RuntimeError as e:
                run["torch"] = f"torch's convolution could not run here: {str(e).splitlines()[0]}"
        out = net.features(rgb)                              # the call itself, without the allocation, is what is timed
        call = lambda: _lib.check(L.btba_vos_features(ws.handle, net.handle, n, H, W, rgb.data_ptr(), out.data_ptr()), "btba_vos_features")
        torch.cuda.synchronize()
        lib = timed(call)
        run.update({"features_ms_median": lib[0], "features_ms_min": lib[1], "ms_per_frame": lib[0] / n,
                    "share_of_fp32_peak": n * 2.0 * macs / (lib[0] * 1e-3) / PEAK_FP32})
        if torch_ok:
            t2 = timed(lambda: by_torch(rgb))
            run.update({"torch_ms_median_before": t1[0], "torch_ms_median_after": t2[0], "torch_ms_min": min(t1[1], t2[1]),
                        "torch_ms_per_frame": min(t1[0], t2[0]) / n, "torch_max_rel_diff": float((out - want).abs().max() / want.abs().max())})
        print(json.dumps(run), flush=True)
        result["runs"].append(run)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
