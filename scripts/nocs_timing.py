"""Timing of btba_nocs_errors (the NOCS evaluation) at four sizes, written to profiles/nocs_timing.json.  GPU box only.
    python scripts/nocs_timing.py [--reps 20] [--out profiles/nocs_timing.json]
Cases: n = 1 (the tracker's per-frame case), 10^3 (a sequence), 10^5 and 10^6 (experiments x thresholds x noise sweeps) items of
mixed classes.  Per case the median over --reps calls after 3 warm-up calls, hipEvent time around the whole call:
  device_us    : poses and outputs on the device (device_resident = 1); the class / box tables still come from the host
  host_us      : poses and outputs in host memory (staged through the workspace)
  cpu_us       : the CPU restatement (tests/cpp/nocs_host.cpp, one thread) on the same items, wall clock
Nothing here asserts a time."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SIZES = (1, 1000, 100000, 1000000)


def inputs(n):
    import nocs_ref as N
    base = N.make_cases(min(n, 997), 7)
    idx = np.arange(n) % base["pred"].shape[0]
    return {k: (v if k == "boxes" else np.ascontiguousarray(v[idx])) for k, v in base.items()}


def event_us(ws, cs, device, reps):
    import torch
    from bundletrack_amd.nocs_eval import nocs_errors
    pred, gt = cs["pred"], cs["gt"]
    if device:
        pred, gt = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()

    def call():
        nocs_errors(ws, cs["boxes"], cs["class_id"], cs["box_index"], pred, gt, cs["handle_visible"])
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)) * 1e3


def cpu_us(cs, reps):
    import nocs_ref as N
    N.restate_cases(cs)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        N.restate_cases(cs)
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nocs_timing.json"))
    a = ap.parse_args()
    import torch
    from bundletrack_amd.optimizer import Workspace
    ws = Workspace()
    out = {"what": "btba_nocs_errors", "device": torch.cuda.get_device_name(0), "reps": a.reps, "cases": {}}
    for n in SIZES:
        cs = inputs(n)
        reps = a.reps if n < 1000000 else max(3, a.reps // 4)
        row = {"items": n, "device_us": round(event_us(ws, cs, True, reps), 1), "host_us": round(event_us(ws, cs, False, reps), 1),
               "cpu_us": round(cpu_us(cs, 3 if n >= 100000 else reps), 1)}
        row["items_per_s_device"] = float(f"{n / (row['device_us'] * 1e-6):.4g}")
        out["cases"][f"n_{n}"] = row
    ws.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
