"""Timing of the window assembly (btba_marshal_windows, btba_procrustes_pairs), one JSON line per case.  GPU box only.
    python scripts/window_timing.py --case tracker      one K = 15 window, 105 pairs of 200 .. 1000 matches; Kabsch of 1 and of 14 pairs
    python scripts/window_timing.py --case batch        32 windows x 105 pairs x 2000 matches; Kabsch of all 3360 pairs
    python scripts/window_timing.py --case bundler      a Bundler step (process_new_frame, 5-frame windows) with device_window off / on
Run the cases as separate commands, each under a time limit of its own, chained with &&:
    timeout -k 10 300 python scripts/window_timing.py --case tracker && timeout -k 10 400 python scripts/window_timing.py --case batch && ...
Per case: hipEvent time per call (median), the rocprofv3 --kernel-trace --stats kernel sum of the same calls in a fresh child process
(--no-rocprof skips it), and next to it the host stand-in -- what the default path does for the same work: download of the records,
bundler.marshal_window, upload of the EntryJ array (and of the offsets), and bundler.procrustes_by_correspondence (numpy fp32 Kabsch).
byte_bound_us: 72 B (96 B with corr24) per match at 6.3 TB/s; byte_frac = byte_bound_us / kernel time of k_window_marshal."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

HBM_BYTES_PER_S = 6.3e12
CASES = {"tracker": (1, 15, (200, 1000)), "batch": (32, 15, (2000, 2000))}


def inputs(name):
    """(records MATCH_DTYPE, segments int64 [nw, P, 2], poses float32 [n_frames, 4, 4])"""
    from bundletrack_amd import _lib
    from bundletrack_amd import synthetic as S
    nw, n_frames, (lo, hi) = CASES[name]
    P = n_frames * (n_frames - 1) // 2
    rng = np.random.default_rng(5)
    counts = rng.integers(lo, hi + 1, size=(nw, P))
    first = np.concatenate([[0], np.cumsum(counts.reshape(-1))[:-1]]).reshape(nw, P)
    n = int(counts.sum())
    rec = np.zeros(n, _lib.MATCH_DTYPE)
    a = rng.normal(scale=0.05, size=(n, 3)) + [0.0, 0.0, 0.6]
    rec["ptA_cam"], rec["ptB_cam"] = a, a + rng.normal(scale=0.001, size=(n, 3))
    poses = np.stack([np.eye(4, dtype=np.float32) for _ in range(n_frames)])
    for k in range(n_frames):
        poses[k, :3, :3] = S.so3_exp(rng.normal(size=3) * 0.01)
    return rec, np.stack([first, counts], -1).astype(np.int64), poses


def _events(fn, reps):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3)
    return round(float(np.median(t)), 1)


def device_calls(name, reps, which=("marshal", "marshal24", "kabsch")):
    """hipEvent microseconds per call."""
    import torch
    from bundletrack_amd.optimizer import Workspace
    from bundletrack_amd.window import marshal_windows, procrustes_pairs, window_layout
    rec, segs, poses = inputs(name)
    nw, n_frames, _ = CASES[name]
    ws = Workspace()
    dev_rec = torch.from_numpy(rec.view(np.int32).reshape(-1, 10).copy()).cuda()
    dev_seg = torch.from_numpy(segs.astype(np.int32)).cuda()
    lay = window_layout(segs[..., 1], n_frames, n_frames - 1, 5)
    out = {"matches": int(segs[..., 1].sum())}
    if "marshal" in which:
        bufs = marshal_windows(ws, dev_rec, dev_seg, n_frames, lay)
        out["marshal_us"] = _events(lambda: marshal_windows(ws, dev_rec, dev_seg, n_frames, lay, out=bufs), reps)
    if "marshal24" in which:
        bufs24 = marshal_windows(ws, dev_rec, dev_seg, n_frames, lay, corr24=True)
        out["marshal_corr24_us"] = _events(lambda: marshal_windows(ws, dev_rec, dev_seg, n_frames, lay, corr24=True, out=bufs24), reps)
    if "kabsch" in which:
        pairs = [(i, j) for i in range(n_frames) for j in range(i + 1, n_frames)]
        sets = {"kabsch_1_pair_us": [(0, len(pairs) - 1)], "kabsch_newframe_pairs_us": [(0, p) for p, (i, j) in enumerate(pairs) if j == n_frames - 1]}
        if nw > 1:
            sets = {"kabsch_all_pairs_us": [(w, p) for w in range(nw) for p in range(len(pairs))]}
        for key, sel in sets.items():
            sg = np.stack([segs[w, p] for w, p in sel])
            TA = np.stack([poses[pairs[p][1]] for _, p in sel])
            TB = np.stack([poses[pairs[p][0]] for _, p in sel])
            out[key] = _events(lambda: procrustes_pairs(ws, dev_rec, sg, TA, TB), reps)
            out[key.replace("_us", "_n")] = len(sel)
    ws.close()
    return out


def host_standin(name, reps):
    """The default path's work for the same input, microseconds (median): download, marshal_window, upload, numpy Kabsch."""
    import torch
    from bundletrack_amd.bundler import FrameRef, marshal_window, procrustes_by_correspondence
    rec, segs, poses = inputs(name)
    nw, n_frames, _ = CASES[name]
    dev_rec = torch.from_numpy(rec.view(np.int32).reshape(-1, 10).copy()).cuda()
    pairs = [(i, j) for i in range(n_frames) for j in range(i + 1, n_frames)]
    frames = [FrameRef(id=k, pose_in_model=poses[k]) for k in range(n_frames)]
    t = {"download_us": [], "marshal_window_us": [], "upload_us": [], "numpy_kabsch_1_pair_us": []}
    for _ in range(max(3, reps // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = dev_rec.cpu().numpy().view(rec.dtype).reshape(-1)
        t1 = time.perf_counter()
        wins = []
        for w in range(nw):
            matches = {(j, i): (np.ascontiguousarray(host["ptA_cam"][f:f + n]), np.ascontiguousarray(host["ptB_cam"][f:f + n]))
                       for (i, j), (f, n) in zip(pairs, segs[w])}
            wins.append(marshal_window(frames, matches, frames[-1], 5))
        t2 = time.perf_counter()
        corr = np.zeros((nw, max(len(x.corr) for x in wins)), wins[0].corr.dtype)
        for w, x in enumerate(wins):
            corr[w, :len(x.corr)] = x.corr
        up = torch.from_numpy(corr.view(np.uint8).reshape(nw, -1, 32)).cuda()
        off = torch.from_numpy(np.stack([np.concatenate([[0], np.cumsum(x.n_match_per_pair)]) for x in wins]).astype(np.int32)).cuda()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        procrustes_by_correspondence(matches, frames[-1], frames[-2])
        t4 = time.perf_counter()
        del up, off
        for key, v in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            t[key].append(v * 1e6)
    return {k: round(float(np.median(v)), 1) for k, v in t.items()}


def rocprof_us(name, reps):
    """Kernel microseconds per call from rocprofv3 --kernel-trace --stats, each device call kind in a fresh child process."""
    per = {}
    for which in ("marshal", "marshal24", "kabsch"):
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "window", "--", sys.executable, os.path.abspath(__file__),
                   "--child", name, "--which", which, "--reps", str(reps)]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=300)
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                raise RuntimeError("no kernel stats from rocprofv3")
            for row in csv.DictReader(open(stats[0])):
                if "k_window" in row["Name"] or "k_kabsch" in row["Name"]:
                    kname = row["Name"].split("(")[0].split("::")[-1]
                    per[f"{which}:{kname}"] = {"total_us": round(float(row["TotalDurationNs"]) / 1e3, 1), "calls": int(row["Calls"]),
                                               "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
    return per


def bundler_step(reps):
    """Wall microseconds of Bundler.process_new_frame (frames 2 .. 5 of a six-frame session, 5-frame windows; device synchronised)
    with device_window off and on, median over frames and `reps` sessions."""
    import torch
    from bundletrack_amd import synthetic as S
    from bundletrack_amd.bundler import Bundler, FrameRef
    from bundletrack_amd.correspondence import GpuFeatureManager
    from bundletrack_amd.optimizer import OptimizerGpu, Workspace
    from match_ref import scene_frames
    pb = S.make_problem(7, 10, seed=31, background=False, rot_step_deg=(4.0, 5.0))
    kp = S.make_keypoints(pb, 650, 60, D=64, seed=31)
    frames = scene_frames(pb, kp)[:6]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    dev = [dict(kpts_gpu=t(f.kpts), desc_gpu=t(f.desc), depth_gpu=t(f.depth), normal_gpu=t(f.normal)) for f in frames]
    ws = Workspace()
    out = {}
    for mode in (False, True, False, True):
        times = []
        for _ in range(reps + 1):
            fm = GpuFeatureManager(ws, pb.K, pb.H, pb.W)
            b = Bundler(OptimizerGpu(workspace=ws), fm, pb.K, pb.H, pb.W, window_size=5, max_BA_frames=5, device_window=mode)
            row = []
            for k in range(6):
                fr = FrameRef(id=0, pose_in_model=np.asarray(pb.poses_gt[0], np.float32) if k == 0 else np.eye(4, dtype=np.float32), **dev[k])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                b.process_new_frame(fr)
                torch.cuda.synchronize()
                row.append((time.perf_counter() - t0) * 1e6)
            times.append(row[2:])
            fm.close()
        out.setdefault("device_window_on_us" if mode else "device_window_off_us", []).append(round(float(np.median(times[1:])), 1))
    ws.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["tracker", "batch", "bundler"], default="tracker")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--which", default="marshal")
    a = ap.parse_args()
    if a.child:                                   # under rocprofv3: warm-up + reps calls of one kind, no output
        device_calls(a.child, a.reps, (a.which,))
        return
    if a.case == "bundler":
        print(json.dumps({"what": "Bundler.process_new_frame", **bundler_step(max(2, a.reps // 5))}))
        return
    out = {"what": "window assembly", "case": a.case, **device_calls(a.case, a.reps)}
    out["byte_bound_us"] = round(72 * out["matches"] / HBM_BYTES_PER_S * 1e6, 1)
    out["byte_bound_corr24_us"] = round(96 * out["matches"] / HBM_BYTES_PER_S * 1e6, 1)
    out["host_standin"] = host_standin(a.case, a.reps)
    if not a.no_rocprof:
        per = rocprof_us(a.case, a.reps)
        out["rocprof_kernels"] = per
        for which, bound in (("marshal", "byte_bound_us"), ("marshal24", "byte_bound_corr24_us")):
            k = per.get(f"{which}:k_window_marshal")
            if k:
                out[f"byte_frac_{which}"] = round(out[bound] / k["avg_us"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
