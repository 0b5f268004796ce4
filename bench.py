#!/usr/bin/env python
"""bench.py -- Gauss-Newton iterations/s of the bundle-adjustment hot path on MI355X.

A "step" = one pass of the hot path over one batch of synthetic input: `--instances` (default 32)
independent tracking instances per GPU, each a BASELINE.json configs[2] problem (K=15 keyframes, 2 000
correspondences per frame pair, feature + dense point-to-plane ICP residuals with Huber, 160x120 dense
images, 7 Gauss-Newton x 5 PCG iterations), resident in HBM before the timed region.  32 per GPU is
configs[4]'s share (256 instances over 8 GPUs): per-GPU work is fixed as N grows (weak scaling); the data
path has no collective, one all-gather of {seconds, iterations} closes the run (RCCL via backend nccl).

    python bench.py [--gpus N --steps K --warmup W]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

METRIC = "Gauss-Newton iters/sec (K=15, 2k corr/frame-pair) + achieved HBM GB/s"
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s measured achievable)
VALU_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: fp32 vector peak = dense f32 MFMA peak (64 flop/clk/SIMD, unpacked v_fma_f32; profiles/r02/valu_calibration.md)
L1_RETURN_PEAK_TBS = 39.3    # vector L1 / texture-addresser return rate: 256 CUs x 64 B per clock x 2.4 GHz; MEASURED, not from the guide: one more 16-byte-per-lane gather per trip adds 15 clocks per wave-trip and CU (profiles/r06/bound_probes.json: 1 KB in 15-16 clocks)
CONFIGS = {
    "c2": dict(K=10, m=1000, w_dense=0.0, config=2, desc="K=10, 1k corr/pair, feature residuals only"),
    "c3": dict(K=15, m=2000, w_dense=1.0, config=3, desc="K=15, 2k corr/pair, feature + dense point-to-plane ICP + Huber"),
    "c4": dict(K=30, m=4000, w_dense=1.0, config=4, desc="K=30, 4k corr/pair, feature + dense point-to-plane ICP + Huber"),
}


def _gen(args):
    from bundletrack_amd import synthetic as S
    K, m, seed, masked = args
    angles = S.pruned_pool_angles(60, 30, seed) if K == 30 else None        # c4: 60-keyframe pool pruned to 30 (greedy-rot) before the timed region
    pb = S.make_problem(K, m, seed, background=not masked, full_res=False, angles=angles)
    campos, normals, intr = S.analytic_cache(pb)
    zn = S.compact_cache(pb)       # compact cache: (z, nx, ny, nz)
    return dict(campos=campos, normals=normals, intr=intr, corr=pb.corr, poses=pb.poses_init, zn=zn, K=pb.K, H=pb.H, W=pb.W)


def generate_instances(cfg, ids, masked=False):
    """Synthetic instances with seeds 1234 + 1000*config + instance, generated in parallel."""
    from bundletrack_amd import synthetic as S
    jobs = [(cfg["K"], cfg["m"], S.config_seed(5 if cfg["config"] == 3 else cfg["config"], i), masked) for i in ids]
    from bundletrack_amd import sharding
    # worker pool of THIS rank: its share of the CPUs the container may really use (affinity mask capped by the cgroup quota -- os.cpu_count() says
    # 256 on a box that grants 16: eight ranks x 8 workers would queue 64 generator processes on 16 CPUs before the timed region)
    nproc = min(len(jobs), 8, max(1, sharding.usable_cpus() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))))
    nproc = int(os.environ.get("BTBA_BENCH_NPROC", nproc))      # 1 under rocprofv3 --pmc (no child processes)
    cache = os.environ.get("BTBA_BENCH_CACHE")                  # profiling passes of one workload: generate once, reuse (scripts/profile_bench.sh)
    if cache:                                                   # an .npz of plain arrays (never a pickle: np.load(allow_pickle=False))
        key = json.dumps([cfg["K"], cfg["m"], list(ids), bool(masked)])
        if os.path.exists(cache):
            with np.load(cache, allow_pickle=False) as z:
                if str(z["key"]) == key:
                    fields = [f for f in ("campos", "normals", "intr", "corr", "poses", "zn", "K") if f"{f}0" in z]
                    return [dict({f: (z[f"{f}{i}"].view(_lib_entryj()) if f == "corr" else z[f"{f}{i}"]) for f in fields}, H=int(z["H"]), W=int(z["W"])) for i in range(len(ids))]
        data = [_gen(j) for j in jobs] if nproc <= 1 else None
        if data is None:
            import multiprocessing as mp
            with mp.get_context("spawn").Pool(nproc) as pool:
                data = pool.map(_gen, jobs)
        arrs = {"key": np.array(key), "H": np.int32(data[0]["H"]), "W": np.int32(data[0]["W"])}
        for i, q in enumerate(data):
            for f in ("campos", "normals", "intr", "poses", "zn", "K"):
                arrs[f"{f}{i}"] = np.asarray(q[f])
            arrs[f"corr{i}"] = np.ascontiguousarray(q["corr"]).view(np.uint8)
        np.savez(cache, **arrs)
        return data
    if nproc > 1:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(nproc) as pool:
            return pool.map(_gen, jobs)
    return [_gen(j) for j in jobs]


def _lib_entryj():
    from bundletrack_amd import _lib
    return _lib.ENTRYJ_DTYPE


SOLVER_SOURCES = ("btba_kernels.hpp", "btba_solve_small.hpp", "btba_solve_mid.hpp", "btba_device.hpp", "btba_api.hip")      # what the sweep / solve kernels are built from


def kernel_source_hash():
    """sha256 over the SOLVER's sources (the sweep and solve kernels and the code that launches them): counter summaries under profiles/ are only
    quoted for the kernels they were taken on -- an edit of the image or RANSAC kernels does not invalidate them."""
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(ROOT, "bundletrack_amd", "csrc")
    for f in SOLVER_SOURCES:
        h.update(open(os.path.join(src, f), "rb").read())
    return h.hexdigest()[:16]


def profiled_counters(config, B, masked, float4_cache, fused, distinct=None, entryj=False):
    """PMC summary of the dominant kernel written by scripts/summarize_profiles.py -- only if it was taken on THESE sources and THIS workload
    (config, instances, distinct instances, mask, cache and correspondence layout); profiles/sweep_counters.json holds one record per workload."""
    tp = os.path.join(ROOT, "profiles", "sweep_counters.json")
    try:
        tj = json.load(open(tp))
    except Exception:
        return None
    records = tj.get("records", [tj]) if isinstance(tj, dict) else tj
    for r in records:
        if (r.get("kernel_source_hash") == kernel_source_hash() and r.get("instances") == B and r.get("config") == config
                and bool(r.get("fused")) == fused and bool(r.get("masked")) == masked and bool(r.get("float4_cache")) == float4_cache
                and r.get("distinct") == distinct and bool(r.get("entryj")) == bool(entryj)):
            return r
    return None


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg, insts, budget_s=24.0):
    """The CPU oracle (a port: the reference has no CPU path) timed on this box's host cores on a bounded sample of the same
    workload: whole solves (7 GN x 5 PCG) -- one instance on 1 thread, one instance on 16 OpenMP threads (frame pairs / correspondence
    chunks), and the c5 way: ALL host CPUs, one single-threaded solve per CPU over distinct instances (the GPU path's own sharding)."""
    from oracle import oracle as O
    try:
        ncpu = len(os.sched_getaffinity(0))
    except AttributeError:
        ncpu = os.cpu_count() or 1
    inst = insts[0]
    out = {}
    nmt = min(ncpu, 16)       # one instance parallelises over frame pairs / frames: more threads than that only add overhead
    for label, nt, share in (("1t", 1, 0.25), ("omp", nmt, 0.25)):
        prm = O.default_params(weight_dense_depth=cfg["w_dense"], n_threads=nt)
        t0 = time.perf_counter()
        n = 0
        while True:
            O.solve(inst["campos"], inst["normals"], inst["intr"], inst["corr"], inst["poses"], params=prm, want_trace=False)
            n += 1
            if time.perf_counter() - t0 > budget_s * share and n >= 3:
                break
        dt = time.perf_counter() - t0
        out[label] = (7.0 * n / dt, n, dt, nt)
    # all CPUs, instance-parallel (the c5 way): one single-threaded solve per CPU over distinct instances, in a worker process bounded by a timeout
    import subprocess, tempfile
    n_inst = min(len(insts), 8)
    all_err, all_info = None, None
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "instances.npz")
        arrs = {"n": np.int32(n_inst)}
        for b in range(n_inst):
            q = insts[b]
            arrs.update({f"campos{b}": q["campos"], f"normals{b}": q["normals"], f"intr{b}": q["intr"], f"corr{b}": np.ascontiguousarray(q["corr"]).view(np.uint8), f"poses{b}": q["poses"]})
        np.savez(path, **arrs)
        lines = []
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "cpu_all_cores.py"), path, str(ncpu), str(cfg["w_dense"]), str(budget_s * 0.5)],
                               capture_output=True, text=True, timeout=budget_s * 2.5)
            lines = r.stdout.strip().splitlines()
        except subprocess.TimeoutExpired as e:      # keep the stages that did finish
            lines = (e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")).strip().splitlines()
            all_err = "worker stopped after %.0f s" % (budget_s * 2.5)
        except Exception as e:                      # a baseline that cannot be measured is reported as such, it must never take the bench line down
            all_err = f"{type(e).__name__}: {e}"[:200]
        stages = []
        for l in lines:
            try:
                j = json.loads(l)
            except Exception:
                continue
            if "stage" in j:
                stages.append(j["stage"])
            if "best" in j:
                all_info = j
        if stages:
            bst = max(stages, key=lambda st: st["gn_iters_per_s"])
            out["all"] = (bst["gn_iters_per_s"], bst["solves"], bst["seconds"], bst["workers"])
            all_info = all_info or {"stages": stages, "cpu_quota": None}
    best = max(out.values(), key=lambda v: v[0])
    ref_note = None
    try:        # the reference's own solver, compiled for the CPU and run through the sequential launch emulator (oracle/_ref):
        from oracle import reference as R           # one thread by construction, every sum through emulated atomics -- context, not the baseline
        if os.path.exists(R.SO_SOLVER) and cfg["K"] <= 15:
            t0 = time.perf_counter()
            R.solve(inst["campos"], inst["normals"], inst["intr"], inst["corr"], inst["poses"], weight_dense=cfg["w_dense"])
            ref_note = {"gn_iters_per_s": round(7.0 / (time.perf_counter() - t0), 3), "cores": 1,
                        "what": "wenbowen123/BundleTrack solveBundlingStub + all kernels, emulated thread by thread on the host (oracle/_ref/libbtba_ref_solver.so)"}
    except Exception:
        ref_note = None
    return {"value": round(best[0], 3), "unit": "GN iterations/s", "cores": best[3], "kind": "port", "reference_emulated": ref_note,
            "sample": f"{best[1]} full solves (7 GN x 5 PCG) of {cfg['desc']} instances in {best[2]:.1f} s; "
                      f"1 thread, 1 instance: {out['1t'][0]:.2f} it/s; {nmt} OpenMP threads, 1 instance: {out['omp'][0]:.2f} it/s; "
                      + (f"instance-parallel over the host CPUs ({out['all'][3]} single-threaded workers, {n_inst} distinct instances round-robin; best of the worker ladder): {out['all'][0]:.2f} it/s" if "all" in out else f"all-CPU run failed ({all_err})")
                      + " (gcc -O3 AVX2 + OpenMP, oracle/btba_oracle.c)",
            "one_thread": round(out["1t"][0], 3), "omp_single_instance": {"value": round(out["omp"][0], 3), "threads": nmt},
            "all_cpus_instance_parallel": ({"value": round(out["all"][0], 3), "workers": out["all"][3], "solves": out["all"][1], "seconds": round(out["all"][2], 2),
                                            "stages": all_info.get("stages"), "cpu_quota": all_info.get("cpu_quota"), "note": all_err} if "all" in out else {"value": None, "error": all_err}),
            "host_cpus": ncpu, "host_cpu_model": _cpu_model()}


def oracle_parity(cfg, insts, picks, gpu_poses, bar=1e-4):
    """The timed run's OUTPUT against the CPU oracle (oracle/btba_oracle.c, pinned against the reference's own solveBundlingStub: DESIGN.md
    section 3) on a few of the instances the GPU has just solved: what was measured is also what is right.  picks: instance indices."""
    from bundletrack_amd import synthetic as S
    from oracle import oracle as O
    try:
        nt = min(len(os.sched_getaffinity(0)), 16)
    except AttributeError:
        nt = 1
    prm = O.default_params(weight_dense_depth=cfg["w_dense"], n_threads=nt)
    worst_r = worst_t = 0.0
    worst_at = None
    for b in picks:
        q = insts[b]
        ref = O.solve(q["campos"], q["normals"], q["intr"], q["corr"], q["poses"], params=prm, want_trace=False)
        for k in range(cfg["K"]):
            r, t = S.pose_error(gpu_poses[b, k], ref.poses[k])
            if max(r, t) > max(worst_r, worst_t):
                worst_at = int(b)
            worst_r, worst_t = max(worst_r, r), max(worst_t, t)
    which = list(picks) if len(picks) <= 8 else f"all {len(picks)} distinct instances of the batch"
    return {"instances": len(picks), "which": which, "worst_rot": float(f"{worst_r:.3e}"), "worst_trans": float(f"{worst_t:.3e}"), "worst_instance": worst_at, "bar": bar,
            "ok": bool(worst_r < bar and worst_t < bar), "against": "CPU oracle (oracle/btba_oracle.c) on the same inputs, final poses after 7 GN x 5 PCG"}


def tracker_call(dev, reps=40):
    """The call the reference actually makes (Bundler.cpp:350-351 -> OptimizerGpu::optimizeFrames, LossGPU.cu:53-139): ONE window of object-masked
    frames per new frame, host EntryJ[] + host poses in, host poses out, K borrowed full-resolution device depth / normal maps -- through
    btba_optimize_frames_keyed (frames kept in the workspace under their ids: the steady state of a tracker caches one new frame per call).
    c3's window: K = 15 x 2 000 matches per pair, 640 x 480 frames masked to the object.  Wall clock around the call including PCIe (median), and
    the library's own hipEvent split of a call.  Measured AFTER the headline region; never part of `value`."""
    import torch
    from bundletrack_amd import _lib, synthetic as S
    from bundletrack_amd.optimizer import OptimizerGpu, Workspace
    K, m = 15, 2000
    pb = S.make_problem(K, m, seed=S.config_seed(3, 0) + K, background=False)          # 640 x 480 frames, object mask
    depths = [torch.from_numpy(pb.depth[k]).to(dev) for k in range(K)]
    normals = [torch.from_numpy(pb.normals[k]).to(dev) for k in range(K)]
    opt = OptimizerGpu(workspace=Workspace())
    walls, stats = [], None
    for rep in range(reps + 10):
        poses = pb.poses_init.copy()
        keys = list(range(K - 1)) + [1000 + rep]                                        # one frame not seen before
        if rep == reps + 5:
            opt.params.flags |= _lib.FLAG_TIME_KERNELS                                  # the last calls: per-kernel split (every launch bracketed, ~4 % slower)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.optimizeFrames(pb.corr, pb.n_match_per_pair, K, pb.H, pb.W, depths, None, normals, poses, pb.K, frame_keys=keys)
        dt = time.perf_counter() - t0
        if 5 <= rep < reps + 5:
            walls.append(dt * 1e3)
            stats = opt.last_stats
    st_k = opt.last_stats
    n_launch = max(1, st_k["n_solve_launches"])
    return {"entry_point": "btba_optimize_frames_keyed", "window": f"K={K} x {m} matches per pair, 640x480 frames masked to the object (~5 % valid), B = 1", "n_corr": int(len(pb.corr)),
            "ms_per_call": round(float(np.median(walls)), 4), "ms_per_call_min": round(float(np.min(walls)), 4), "calls": len(walls), "includes": "H2D of EntryJ[] + poses, one new frame cached, 7 GN x 5 PCG, D2H of poses",
            "ms_solve": round(float(stats["ms_solve"]), 4), "ms_cache": round(float(stats["ms_cache"]), 4), "ms_upload": round(float(stats["ms_upload"]), 4), "ms_total": round(float(stats["ms_total"]), 4),
            "gn_iters_per_s": round(7e3 / float(np.median(walls)), 1),
            "kernels_us_per_launch": {"sweeps": round(1e3 * (st_k["ms_dense_sweep"] / max(1, st_k["n_dense_launches"]) + st_k["ms_sparse_sweep"] / max(1, st_k["n_sparse_launches"])), 2),
                                      "system_solve": round(1e3 * st_k["ms_system_solve"] / n_launch, 2), "dense_tiles": st_k["dense_tiles"], "sparse_chunks": st_k["sparse_chunks"]}}


def measured_copy_bandwidth(torch, dev, nbytes=1 << 30, reps=10):
    """Device-to-device copy bandwidth of this box (read + write bytes / time), SURVEY.md 8(d): fractions are quoted
    against the nominal 8 TB/s AND against what the part actually streams."""
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    for _ in range(2):
        dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * nbytes * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


def spawn_ranks(n):
    """`python bench.py --gpus N` started by hand: re-run this command line under torch.distributed.run with N ranks on this node and pass
    rank 0's JSON line through.  Refuses to pretend: fewer than N visible GPUs is an error unless BTBA_DIST_BACKEND=gloo is forced
    (the functional test that runs two ranks on a one-GPU box)."""
    import socket
    import subprocess
    import torch
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < n and os.environ.get("BTBA_DIST_BACKEND", "") != "gloo":
        raise SystemExit(f"bench.py --gpus {n}: only {have} GPU(s) visible on this node (set BTBA_DIST_BACKEND=gloo to share GPUs in a functional test)")
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    note(f"--gpus {n} without a launcher: starting {n} ranks under torch.distributed.run on port {port}")
    r = subprocess.run(cmd, env=env)
    raise SystemExit(r.returncode)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, poses, rank=None):
    """--dump-outputs: the poses of the last timed step, [B, K, 4, 4] float32.  Above DUMP_LIMIT_BYTES a fixed, seeded sample of the instances is
    written instead, with their batch indices next to it (poses_instances.npy, float64)."""
    os.makedirs(out_dir, exist_ok=True)
    suffix = "" if rank is None else f"_rank{rank}"
    per_instance = poses[0].nbytes if len(poses) else 1
    if poses.nbytes > DUMP_LIMIT_BYTES:
        keep = np.sort(np.random.default_rng(0).choice(len(poses), DUMP_LIMIT_BYTES // 2 // per_instance, replace=False))
        np.save(os.path.join(out_dir, f"poses_instances{suffix}.npy"), keep.astype(np.float64))
        poses = poses[keep]
    np.save(os.path.join(out_dir, f"poses{suffix}.npy"), np.ascontiguousarray(poses, dtype=np.float32))
    note(f"wrote {poses.shape} poses to {out_dir}")


_T0 = time.perf_counter()


def note(msg):
    """Progress on stderr (the JSON line on stdout stays alone): where the wall clock goes when a run is slow."""
    print(f"[bench +{time.perf_counter() - _T0:6.1f}s] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=250, help="timed steps (default: ~0.35 s of GPU time at c3 x 32, long enough for an external busy sampler to see)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--instances", type=int, default=32, help="instances per GPU")
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--distinct", type=int, default=32, help="distinct synthetic instances generated per GPU (seeds 1234 + 1000 config + global instance id; tiled to --instances if fewer)")
    ap.add_argument("--masked", action="store_true", help="realistic ~5%%-valid object mask instead of the 100%%-valid roofline variant")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the cpu_baseline leg (and, unless --parity is given, the parity leg: both run the CPU oracle)")
    ap.add_argument("--parity", action="store_true", help="run the parity leg (the timed output of every distinct instance against the CPU oracle) even with --no-cpu-baseline: lines of record for the other configs are self-checking without the 25 s baseline")
    ap.add_argument("--no-tracker-call", action="store_true", help="skip the extra field `tracker_call` (one object-masked c3 window per call through btba_optimize_frames_keyed, measured after the timed region)")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--float4-cache", action="store_true", help="reference-layout float4 camPos + float4 normal caches (32 B/pixel) instead of the compact (z, n) cache")
    ap.add_argument("--latency", action="store_true", help="also measure single-instance latency mode (extra field; always on at --gpus 1 unless --no-single-instance)")
    ap.add_argument("--no-single-instance", action="store_true", help="skip the `single_instance` leg: profiling passes, whose per-kernel averages must be those of the benched launches alone (the B = 1 solves launch the same kernels)")
    ap.add_argument("--same-instances", action="store_true", help="every rank solves the SAME instances (global ids 0 ..): the per-rank pose checksums must then agree -- a consistency check of the sharded run, not a benchmark")
    ap.add_argument("--entryj", action="store_true", help="keep the device-resident correspondences as 32-byte EntryJ instead of packing them to 24-byte records before the timed region")
    ap.add_argument("--corr24", action="store_true", help="24-byte records also with --masked (default there: EntryJ, which measured 4 %% faster on the masked launch: profiles/r03)")
    ap.add_argument("--settle-ms", type=float, default=200.0, help="untimed steps run for this long BEFORE the --warmup steps: a process that has just started finds the GPU at idle clocks, and "
                                                                    "5 warm-up steps (7 ms) do not ramp them -- the same command measured 5 %% slower at --steps 20 than at --steps 250 (0 disables)")
    ap.add_argument("--no-incl-pack", action="store_true", help="skip the second timed region (value_incl_pack): profiling passes, whose per-kernel averages must be those of the first region")
    ap.add_argument("--baseline-n1", type=float, default=None, help="the N = 1 value of the same command: rank 0 then also reports efficiency = value / (N x this)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step returned (the solved poses, float32) "
                                                                         "as DIR/poses.npy (DIR/poses_rank<r>.npy per rank when N > 1), so that two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    # --gpus N without a launcher: become the launcher (one rank per GPU under torch.distributed.run, RCCL via backend nccl)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args.gpus)

    import torch
    from bundletrack_amd import _lib, sharding
    from bundletrack_amd.optimizer import BatchSolver, Workspace

    rank, world, local = sharding.init_from_env()
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    local_dev = local % torch.cuda.device_count()        # == local on a real node; lets a functional test run 2 ranks on 1 GPU
    torch.cuda.set_device(local_dev)
    cpu_binding = sharding.bind_rank_to_cpus(local, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))), local_dev) if world > 1 else {"bound": False, "why": "single rank"}
    dev = torch.device(f"cuda:{local_dev}")
    cfg = CONFIGS[args.config]
    B, K = args.instances, cfg["K"]

    # ---- synthetic inputs, resident in HBM before the timed region
    n_distinct = max(1, min(args.distinct, B))
    # the partition SURVEY.md 8(e) / DESIGN.md 6 state: global instance n of the job's world x B instances runs on rank n mod world
    # (sharding.instances_for_rank); --same-instances gives every rank rank 0's share
    ids = sharding.instances_for_rank(world * B, 0 if args.same_instances else rank, world)[:n_distinct]       # global instance ids of this rank's distinct seeds
    note(f"generating {n_distinct} synthetic instances")
    inst = generate_instances(cfg, ids, args.masked)
    note("instances ready; uploading")
    pick = [inst[b % n_distinct] for b in range(B)]
    ws = Workspace()
    bs = BatchSolver(ws, weight_dense_depth=cfg["w_dense"])
    if not args.no_kernel_timing:
        bs.params.flags |= _lib.FLAG_TIME_KERNELS | _lib.FLAG_TIME_SAMPLED      # one Gauss-Newton iteration of every solve is bracketed with hipEvents (rotating): every launch costs ~4 %
    bs.params.flags |= int(os.environ.get("BTBA_BENCH_FLAGS", "0"))          # developer A/B of tuning flags
    bs.params.dense_tiles = int(os.environ.get("BTBA_BENCH_TILES", "0"))     # 0 = the library's choice
    bs.params.sparse_chunks = int(os.environ.get("BTBA_BENCH_CHUNKS", "0"))  # 0 = the library's choice
    if args.masked and not args.float4_cache:
        bs.params.flags |= _lib.FLAG_COMPACTION         # workload hint: masked frames -> walk valid-pixel lists (optimize_frames decides this by itself)
    corr, offs, mx = bs.pack_correspondences([p["corr"] for p in pick], K)
    if args.float4_cache:
        cam_d = torch.from_numpy(np.stack([p["campos"] for p in pick])).to(dev)
        nrm_d = torch.from_numpy(np.stack([p["normals"] for p in pick])).to(dev)
    else:
        cam_d = torch.from_numpy(np.stack([p["zn"] for p in pick])).to(dev)      # [B, K, Hd, Wd, 4] = (z, nx, ny, nz)
        nrm_d = None
    corr_d = torch.from_numpy(corr.view(np.uint8).reshape(B, -1, 32)).to(dev)
    offs_d = torch.from_numpy(offs.astype(np.int32)).to(dev)
    poses0 = torch.from_numpy(np.stack([p["poses"] for p in pick])).to(dev)
    poses_d = poses0.clone()
    intr = pick[0]["intr"]
    n_corr = int(sum(len(p["corr"]) for p in pick))

    # what the solve derives from the caches alone (per-block depth ranges; the valid-pixel lists of masked frames) belongs to the frame
    # cache: built here, with the caches, once
    aux_d = None if args.float4_cache else bs.cache_aux(cam_d, valid_lists=bool(bs.params.flags & _lib.FLAG_COMPACTION))
    # ... and so does the device layout of the correspondences: a batch that stays resident keeps them as 24-byte records (pos_i, pos_j --
    # the frame indices are implied by the pair-major segment), packed once here from the EntryJ wire format (btba_pack_correspondences24)
    use_c24 = not args.entryj and not args.float4_cache and n_corr > 0 and (args.corr24 or not args.masked)
    if use_c24:
        aux_d["corr24"], order_flag = bs.pack_correspondences24(corr_d, offs_d, mx, K, check_order=True)
        torch.cuda.synchronize()
        assert int(order_flag.cpu()[0]) == 0, "synthetic correspondences are pair-major"

    def step():
        poses_d.copy_(poses0)                               # pose in ...
        if args.float4_cache:
            bs.solve(cam_d, nrm_d, intr, corr_d, offs_d, mx, poses_d)   # ... pose out (7 GN iterations per instance)
        else:
            bs.solve_zn(cam_d, pick[0]["H"], pick[0]["W"], pick[0]["K"], None if use_c24 else corr_d, offs_d, mx, poses_d, aux=aux_d, corr_stride=corr_d.shape[1])

    note("warm-up")
    settle_steps = 0
    if args.settle_ms > 0:                                  # bring the device to its working clocks (untimed, disclosed in the line: "settle")
        t_s = time.perf_counter()
        while (time.perf_counter() - t_s) * 1e3 < args.settle_ms:
            for _ in range(5):
                step()
            torch.cuda.synchronize()
            settle_steps += 5
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if not args.no_kernel_timing:
        ws.collect_stats()                                  # drop warm-up events
    sharding.barrier(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    sharding.barrier(dev)
    t1 = time.perf_counter()
    seconds = t1 - t0
    note(f"timed region done: {seconds:.3f} s")
    st = ws.collect_stats()
    out_poses = poses_d.cpu().numpy()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out_poses, rank if world > 1 else None)
    # (non-finite poses: caught below through the gathered pose checksums, so that every rank leaves together instead of one rank hanging the gather)
    # What a tracker pays: its correspondences are NEW on every call, so nothing about them can be prepared outside the call.  Same steps again,
    # handing the solve the EntryJ array (already in HBM) as it is -- the library's default for fresh matches reads the 32-byte wire format in
    # every iteration (an in-sweep re-layout, BTBA_OPT_RELAYOUT, and a separate pack pass both measured no better: profiles/r04/relayout.json).
    seconds_incl_pack = None
    if use_c24 and not args.no_incl_pack:
        aux_fresh = {k: v for k, v in aux_d.items() if k != "corr24"}
        def step_incl_pack():                               # (same flags as the first region: its hipEvent brackets are part of both)
            poses_d.copy_(poses0)
            bs.solve_zn(cam_d, pick[0]["H"], pick[0]["W"], pick[0]["K"], corr_d, offs_d, mx, poses_d, aux=aux_fresh, corr_stride=corr_d.shape[1])
        for _ in range(2):
            step_incl_pack()
        torch.cuda.synchronize()
        sharding.barrier(dev)
        ta = time.perf_counter()
        for _ in range(args.steps):
            step_incl_pack()
        torch.cuda.synchronize()
        sharding.barrier(dev)
        seconds_incl_pack = time.perf_counter() - ta
        if not args.no_kernel_timing:
            ws.collect_stats()                              # (the kernel times reported below are the first region's: `st`)
        note(f"pack-inclusive region done: {seconds_incl_pack:.3f} s")
    # work the dense sweep actually executes: 8 x 8 blocks walked (the hull test removes the provably dead ones), one counted solve
    live_blocks_per_solve = None
    if not args.float4_cache and not args.masked and cfg["w_dense"] > 0:
        ws.set_option(_lib.OPT_COUNT_LIVE, 1)
        step()
        live_blocks_per_solve = ws.live_blocks()
        ws.set_option(_lib.OPT_COUNT_LIVE, 0)
        ws.collect_stats()

    gn_iters = float(B * bs.params.n_gn_iters * args.steps)
    backend = sharding.backend_name()                   # None: single process without a process group
    gather_dev = dev if backend == "nccl" else "cpu"
    per_rank = sharding.gather_throughput(seconds, gn_iters, device=gather_dev, checksum=float(np.abs(out_poses.astype(np.float64)).sum()))
    value, slowest = sharding.aggregate(per_rank)
    checksums = list(sharding.gather_throughput.checksums)
    if not all(np.isfinite(c) for c in checksums):          # a rank that produced non-finite poses: no line (every rank sees the same gathered list and stops)
        print(f"bench.py: non-finite pose checksum on rank(s) {[r for r, c in enumerate(checksums) if not np.isfinite(c)]} -- no result line", file=sys.stderr)
        if backend is not None:
            import torch.distributed as dist
            dist.destroy_process_group()
        raise SystemExit(4)
    value_incl_pack = None
    if seconds_incl_pack is not None:
        pr2 = sharding.gather_throughput(seconds_incl_pack, gn_iters, device=gather_dev)
        value_incl_pack, _ = sharding.aggregate(pr2)

    if rank == 0:
        npix = int(cam_d.shape[2] * cam_d.shape[3])
        P = K * (K - 1) // 2
        res = {
            "metric": METRIC, "value": round(value, 1), "unit": "GN iterations/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "settle": {"ms": args.settle_ms, "untimed_steps": settle_steps, "why": "device clocks ramp over ~100 ms of load; run before the warm-up steps"},
            "ms_per_step": round(1e3 * slowest / args.steps, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{args.config} x {B} instances/GPU: {cfg['desc']}, 160x120 dense images, "
                                   f"{'~5%-valid object mask' if args.masked else '100%-valid (object + background)'}, 7 GN x 5 PCG, pair policy TARGET_LOWER",
                       "keyframes": K, "corr_per_pair": cfg["m"], "instances_per_gpu": B, "distinct_instances_per_gpu": n_distinct,
                       "gn_iters": int(bs.params.n_gn_iters), "pcg_iters": int(bs.params.n_pcg_iters),
                       "dense_tiles": st["dense_tiles"], "sparse_chunks": st["sparse_chunks"], "frame_cache": "float4 camPos + float4 normal (32 B/px)" if args.float4_cache else "compact z + normal (16 B/px)",
                       "correspondences": ("`value`: 24-byte records (pos_i, pos_j) resident in HBM, packed from EntryJ BEFORE the timed region; `value_incl_pack`: the same steps with the "
                                           "EntryJ array (32-byte wire format) handed to every solve as it is, nothing prepared outside the timed region -- what a tracker "
                                           "with fresh matches on every call pays") if use_c24 else "EntryJ (32 B), every iteration",
                       "parallelism": f"instances sharded over {world} GPU(s), no data-path collective"},
            "value_incl_pack": round(value_incl_pack, 1) if value_incl_pack else None,
            "ms_per_step_incl_pack": round(1e3 * seconds_incl_pack / args.steps, 4) if seconds_incl_pack else None,
            "per_rank": [{"seconds": round(s, 6), "gn_iters": g, "ms_per_step": round(1e3 * s / args.steps, 4), "pose_checksum": round(c, 6)} for (s, g), c in zip(per_rank, checksums)],
            "rank_spread": {"ms_per_step_min": round(1e3 * min(s for s, _ in per_rank) / args.steps, 4), "ms_per_step_max": round(1e3 * max(s for s, _ in per_rank) / args.steps, 4)},
            "instance_ids_rank0": {"first": ids[:4], "rule": "global instance n -> rank n mod n_gpus (sharding.instances_for_rank)"},
            "collective": {"backend": backend, "rccl_ranks": world if backend == "nccl" else 0,
                           "what": "one all-gather of {seconds, GN iterations, pose checksum} per rank after the timed region; no data-path collective"},
            "cpu_binding_rank0": cpu_binding,
        }
        if args.baseline_n1:
            res["efficiency_vs_n1"] = {"value": round(value / (world * args.baseline_n1), 4), "formula": "value / (n_gpus x the N = 1 value passed with --baseline-n1)", "n1_value": args.baseline_n1}
        if not args.no_kernel_timing and st["n_dense_launches"] > 0:
            # Dominant kernel = the Jacobian sweep (fused: dense + sparse workgroups in one launch).  It is bound by VALU issue, not by
            # HBM (PMC: the vector pipe is ~87 % busy, HBM at ~0.2 of peak), so the roofline is the fp32 vector peak -- 157.3 TFLOP/s on
            # MI355X, equal to the dense f32 MFMA peak -- against SURVEY.md 8(d)'s ALGORITHMIC flops: 200 per (frame pair, valid source
            # pixel), 120 per correspondence.  The 8(d) HBM accounting (64 B per pair-pixel, 32 B per correspondence, no credit for the
            # reuse of a frame by its 14 pairs) is kept as context with the measured traffic next to it.
            avg_ms = st["ms_dense_sweep"] / st["n_dense_launches"]
            fused = bool(st.get("fused_sweeps", 0))
            # chained launch (k_chain): ONE launch per solve carries the sweeps of all Gauss-Newton iterations (and the system solves of all
            # but the last): per launch it does `chained` times the algorithmic work of a fused sweep launch
            chained = int(st.get("chain_iterations", 0))
            sweeps_per_launch = chained if chained else 1
            n_it_count = int(bs.params.n_gn_iters)
            depth = np.stack([p["zn"][..., 0] for p in pick]) if not args.float4_cache else np.stack([p["campos"][..., 2] for p in pick])
            nvalid = (depth >= 0.1).reshape(B, K, -1).sum(-1)                        # valid source pixels per frame
            pair_pixels = int((nvalid * np.arange(K)[None, :]).sum())                # frame j is the source of its j pairs (i < j)
            flops_alg = sweeps_per_launch * (200.0 * pair_pixels + (120.0 * n_corr if fused else 0.0))
            bytes_alg = sweeps_per_launch * (64 * pair_pixels + (32 * n_corr if fused else 0))
            tflops = flops_alg / (avg_ms * 1e-3) / 1e12
            pc = profiled_counters(args.config, B, args.masked, args.float4_cache, fused, n_distinct, not use_c24)
            traffic = pc.get("hbm_bytes_per_launch") if pc else None
            corr_bytes = 24 if use_c24 else 32
            if args.masked:
                # object-masked frames (the tracker's operating point): the launch streams every correspondence once and touches ~5 % of
                # the pixels -- it is bound by that stream, not by the vector pipe.  Algorithmic bytes (SURVEY.md 8(d)'s 32 B per
                # correspondence; every valid cached pixel once, 16 B) over the launch time against the HBM peak; the 24-byte device
                # records do the same algorithmic work on 3/4 of the correspondence bytes, `layout_bytes_per_launch` is what they move.
                alg = sweeps_per_launch * (32 * n_corr + 16 * int(nvalid.sum()))
                lay = sweeps_per_launch * (corr_bytes * n_corr + 16 * int(nvalid.sum()))      # what the device layout moves: `achieved` / `frac` never exceed the bandwidth actually sustained
                gbs = lay / (avg_ms * 1e-3) / 1e9
                res["roofline"] = {"bound": "hbm", "kernel": "k_fused_sweeps (dense + sparse workgroups)" if fused else "k_dense_sweep",
                                   "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4), "traffic": traffic,
                                   "layout_bytes_per_launch": lay, "algorithmic_bytes_per_launch": alg,
                                   "algorithmic_32B_GBps": round(alg / (avg_ms * 1e-3) / 1e9, 1),
                                   "avg_launch_ms": round(avg_ms, 5), "launches_timed": st["n_dense_launches"],
                                   "valu_context": {"achieved_TFLOPs": round(tflops, 2), "frac_of_vector_peak": round(tflops / VALU_PEAK_TFLOPS, 4), "algorithmic_flops_per_launch": flops_alg},
                                   "note": "HBM roofline: (bytes per correspondence of the device layout x correspondences + 16 B x valid cached pixels) / launch time against 8 TB/s; "
                                           "algorithmic_32B_GBps is the same with SURVEY.md 8(d)'s 32 B per correspondence; durations from hipEvents on the workspace stream inside the timed region"}
            else:
                res["roofline"] = {"bound": "valu", "kernel": (f"k_chain (ONE launch per solve: the dense + sparse sweep items of all {chained} Gauss-Newton iterations and {chained - 1} in-launch system solves)" if chained
                                                              else "k_fused_sweeps (dense + sparse workgroups)" if fused else "k_dense_sweep"),
                                   "achieved": round(tflops, 2), "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tflops / VALU_PEAK_TFLOPS, 4),
                                   "traffic": traffic, "algorithmic_flops_per_launch": flops_alg, "pair_pixels_per_launch": sweeps_per_launch * pair_pixels, "sweeps_per_launch": sweeps_per_launch,
                                   "avg_launch_ms": round(avg_ms, 5), "launches_timed": st["n_dense_launches"],
                                   "note": "fp32 vector (VALU) roofline: algorithmic flops / launch time against 157.3 TFLOP/s (256 CUs x 4 SIMDs x 64 flop/clk x 2.4 GHz = the "
                                           "dense f32 MFMA peak); durations from hipEvents on the workspace stream inside the timed region"}
            if not args.masked and live_blocks_per_solve:
                # the contract number above charges 200 flop to every (frame pair, valid source pixel) of SURVEY.md 8(d); the kernel proves about
                # half of the 8 x 8 blocks dead before it walks them (hull test, exact: tests/test_gpu_fullsize.py::test_dead_block_skip_is_exact)
                # and never evaluates their pixels.  On the work it EXECUTES: walked blocks x 64 pixels x 200 + correspondences x 120.
                live_px = 64.0 * live_blocks_per_solve / n_it_count * sweeps_per_launch
                flops_exec = 200.0 * live_px + sweeps_per_launch * (120.0 * n_corr if fused else 0.0)
                res["roofline"]["executed"] = {"frac": round(flops_exec / (avg_ms * 1e-3) / 1e12 / VALU_PEAK_TFLOPS, 4), "achieved": round(flops_exec / (avg_ms * 1e-3) / 1e12, 2),
                                               "walked_pair_pixels_per_launch": int(live_px), "share_of_pair_pixels_walked": round(live_px / (sweeps_per_launch * pair_pixels), 4),
                                               "what": "flops of the blocks the dense sweep walks (counted by the kernel: BTBA_OPT_COUNT_LIVE, one solve) + the sparse items', over the same launch time and peak"}
                # round 6 (profiles/r06/bound_probes.json): the pixel loop waits on the texture addresser / L1 return path -- one more 16-byte gather per trip costs the
                # launch 13.4 us, linearly.  Gather bytes of the walked blocks (64 lanes x 5 gathers x 16 B: an upper bound, trips that end early issue one gather and lanes
                # outside the target none) against the chip's L1 return rate, 256 CUs x 64 B / clock x 2.4 GHz.
                gather_bytes = 80.0 * live_px
                res["roofline"]["l1_gather"] = {"achieved_TBps": round(gather_bytes / (avg_ms * 1e-3) / 1e12, 2), "peak_TBps": L1_RETURN_PEAK_TBS,
                                                "frac": round(gather_bytes / (avg_ms * 1e-3) / 1e12 / L1_RETURN_PEAK_TBS, 4), "gather_bytes_per_launch": int(gather_bytes),
                                                "what": "walked blocks x 64 lanes x (1 source + 4 tap gathers) x 16 B over the launch time, against 256 CUs x 64 B/clk x 2.4 GHz; "
                                                        "the pipe whose service time the loop exposes (profiles/r06/bound_probes.json)"}
            if pc and pc.get("valu_busy_frac") is not None:
                res["roofline"]["valu_issue"] = {"busy_frac": pc["valu_busy_frac"], "cycles_per_instruction": pc.get("valu_cycles_per_inst"),
                                                 "dual_issued_frac": pc.get("valu_dual_issued_frac"), "waves_per_simd": pc.get("waves_per_simd"),
                                                 "source": pc.get("source_sq"), "kernel_source_hash": pc.get("kernel_source_hash"),
                                                 "formula": "4 (SQ_ACTIVE_INST_VALU - SQ_ACTIVE_INST_VALU2) / 1024 SIMDs / (SQ_BUSY_CYCLES / 32); units pinned in profiles/r02/valu_calibration.md"}
            else:
                res["roofline"]["valu_issue"] = None          # no counter pass on these sources / this workload (scripts/profile_bench.sh)
            hb = {"achieved_GBps": round(bytes_alg / (avg_ms * 1e-3) / 1e9, 1), "peak_GBps": HBM_PEAK_GBS, "algorithmic_bytes_per_launch": bytes_alg,
                  "note": "SURVEY.md 8(d) accounting; it exceeds the HBM peak because every pair is charged both frames while a frame is reused by its 14 pairs "
                          "out of L2 -- not a bandwidth measurement"}
            if traffic:
                compulsory = (32 if args.float4_cache else 16) * (int(nvalid.sum()) if args.masked else B * K * npix) + (corr_bytes * n_corr if fused else 0)       # every (valid) cached pixel and every correspondence once
                hb.update({"hbm_traffic_GBps": round(traffic / (avg_ms * 1e-3) / 1e9, 1), "hbm_traffic_frac_of_peak": round(traffic / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           "algorithmic_over_traffic": round(bytes_alg / traffic, 2), "traffic_over_compulsory": round(traffic / compulsory, 2),
                           "source": pc.get("source_hbm")})
            res["roofline"]["hbm_algorithmic"] = hb
            if world == 1:
                copy_bw = measured_copy_bandwidth(torch, dev)
                res["roofline"]["hbm_algorithmic"]["peak_measured_copy_GBps"] = round(copy_bw, 1)
            # per-step kernel time = average timed launch x launches per step (one iteration of every solve is timed)
            n_it = int(bs.params.n_gn_iters)
            per_step = lambda ms, n: ms / max(n, 1) * (1 if chained else n_it)      # chained: one sweep launch (all iterations) and one stand-alone system solve (the last) per step
            res["kernels_ms_per_step"] = {
                "fused_sweeps": fused,            # fused: ONE launch per iteration carries both sweeps
                "sweeps": round(per_step(st["ms_dense_sweep"], st["n_dense_launches"]) + per_step(st["ms_sparse_sweep"], st["n_sparse_launches"]), 4),
                "dense_sweep": None if fused else round(per_step(st["ms_dense_sweep"], st["n_dense_launches"]), 4),
                "sparse_sweep": None if fused else round(per_step(st["ms_sparse_sweep"], st["n_sparse_launches"]), 4),
                "system_solve": round(per_step(st["ms_system_solve"], st["n_solve_launches"]), 4), "solve_region": round(st["ms_solve"] / args.steps, 4),
                "launches_timed": {"sweep": st["n_dense_launches"], "system_solve": st["n_solve_launches"], "of_per_step": 1 if chained else n_it},
                "chained_iterations": chained,
                "sparse_alg_GBps": (round(32 * n_corr / max(st["ms_sparse_sweep"] / max(st["n_sparse_launches"], 1), 1e-9) / 1e6, 1) if st["n_sparse_launches"] else None)}
        elif cfg["w_dense"] == 0.0 and not args.no_kernel_timing and st["n_sparse_launches"] > 0:
            avg_ms = st["ms_sparse_sweep"] / st["n_sparse_launches"]
            achieved = (24 if use_c24 else 32) * n_corr / (avg_ms * 1e-3) / 1e9       # the bytes the device layout moves (SURVEY.md 8(d)'s 32 B per correspondence: algorithmic_32B_GBps)
            pc = profiled_counters(args.config, B, args.masked, args.float4_cache, False, n_distinct, not use_c24)
            res["roofline"] = {"bound": "hbm", "kernel": "k_sparse_sweep", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": pc.get("hbm_bytes_per_launch") if pc else None, "algorithmic_bytes_per_launch": 32 * n_corr,
                               "algorithmic_32B_GBps": round(32 * n_corr / (avg_ms * 1e-3) / 1e9, 1),
                               "layout_bytes_per_launch": (24 if use_c24 else 32) * n_corr,
                               "avg_launch_ms": round(avg_ms, 5), "launches_timed": st["n_sparse_launches"],
                               "valu_issue": ({"busy_frac": pc["valu_busy_frac"], "cycles_per_instruction": pc.get("valu_cycles_per_inst"), "dual_issued_frac": pc.get("valu_dual_issued_frac"),
                                               "waves_per_simd": pc.get("waves_per_simd"), "source": pc.get("source_sq"), "kernel_source_hash": pc.get("kernel_source_hash")}
                                              if pc and pc.get("valu_busy_frac") is not None else None),
                               "note": "HBM roofline of the sparse sweep: bytes the device layout moves per launch / launch time (hipEvents on the workspace stream) against 8 TB/s; the launch is 9 us long -- "
                                       "mostly ramp-up and drain -- so `traffic` (L2 fetch bytes from the counter pass) over its duration is far below what the part streams"}
        if args.latency or (world == 1 and not args.no_single_instance):
            # BASELINE.json's metric read literally -- ONE K=15 x 2k problem at a time (B = 1), resident inputs, pose in -> pose out: always in the
            # single-GPU line (10 ms of GPU time); `value` above is the batch of 32 such problems per GPU that SURVEY.md 8(d) names for the headline
            bs1 = BatchSolver(ws, weight_dense_depth=cfg["w_dense"])
            c1, o1, m1 = bs1.pack_correspondences([pick[0]["corr"]], K)
            c1d = torch.from_numpy(c1.view(np.uint8).reshape(1, -1, 32)).to(dev)
            o1d = torch.from_numpy(o1.astype(np.int32)).to(dev)
            p1 = poses0[:1].clone()
            aux1 = None if aux_d is None else {k: v[:K] for k, v in aux_d.items() if k != "corr24"}
            if use_c24:
                aux1["corr24"] = bs1.pack_correspondences24(c1d, o1d, m1, K)

            def one(p):
                if args.float4_cache:
                    bs1.solve(cam_d[:1], nrm_d[:1], intr, c1d, o1d, m1, p)
                else:
                    bs1.solve_zn(cam_d[:1], pick[0]["H"], pick[0]["W"], pick[0]["K"], None if use_c24 else c1d, o1d, m1, p, aux=aux1, corr_stride=c1d.shape[1])
            for _ in range(5):
                p1.copy_(poses0[:1]); one(p1)
            torch.cuda.synchronize()
            ta = time.perf_counter()
            reps = 50
            for _ in range(reps):
                p1.copy_(poses0[:1]); one(p1)
            torch.cuda.synchronize()
            tb = time.perf_counter()
            res["single_instance"] = {"gn_iters_per_s": round(7 * reps / (tb - ta), 1), "ms_per_solve": round(1e3 * (tb - ta) / reps, 4), "solves": reps,
                                      "what": f"ONE {args.config} problem per solve (B = 1: {cfg['desc']}), inputs resident in HBM, 7 GN x 5 PCG, back to back on one stream"}
        if world == 1 and not args.no_tracker_call:
            note("tracker-mode call (btba_optimize_frames_keyed, one masked c3 window)")
            res["tracker_call"] = tracker_call(dev)
        if world == 1 and not args.no_cpu_baseline:
            note("CPU baseline (oracle on the host cores)")
            res["cpu_baseline"] = cpu_baseline(cfg, inst)
            note("CPU baseline done")
        parity_ok = True
        if not args.no_cpu_baseline or args.parity:
            picks = list(range(n_distinct))       # every distinct instance of the timed batch (instance b of the batch is inst[b % n_distinct]); ~70 ms each on 16 threads
            res["parity"] = oracle_parity(cfg, inst, picks, out_poses.reshape(B, K, 4, 4))
            parity_ok = res["parity"]["ok"]
            note(f"parity of the timed output against the oracle: {res['parity']['worst_rot']:.2e} rad / {res['parity']['worst_trans']:.2e} m on {len(picks)} instances (worst: {res['parity']['worst_instance']})")
        print(json.dumps(res), flush=True)
        if not parity_ok:
            print("bench.py: the timed run's poses differ from the oracle's by more than the bar", file=sys.stderr)
            if backend is not None:
                import torch.distributed as dist
                dist.destroy_process_group()
            raise SystemExit(3)
    if backend is not None:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
