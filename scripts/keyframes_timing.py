"""Time of the device keyframe memory -> profiles/keyframes_timing.json: btba_keyframes_check_add and btba_keyframes_select for 1 and for 32
sessions at pools of 20, 40, 100 and 1000 keyframes (random rotations, every session its own), max_BA_frames 15: medians of 30 device-event
times after 5 warm-up calls on the workspace stream.  check_add is timed on a frame the gate refuses (a copy of a pool member): the kernel
scans the whole pool either way and the pool stays as it is.  Beside them, in the same run on the same poses, the two host memories --
bundler.KeyframeMemory (numpy, one libm acosf call per pair) and btba::KeyframeMemory (C++, through tests/cpp/keyframes_driver.cpp) -- for
ONE session: select_keyframes_for_ba, and a check_and_add_keyframe that scans the whole pool (medians of 30 host-clock times; the numpy
select at 1000 keyframes takes seconds and is measured 3 times).  No time was fixed beforehand: the JSON records what was measured.  GPU box only.
    python scripts/keyframes_timing.py [--out profiles/keyframes_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

MAX_BA, WARMUP, REPS, POOLS, SESSIONS = 15, 5, 30, (20, 40, 100, 1000), (1, 32)


def rotations(n, seed):
    from scipy.spatial.transform import Rotation
    T = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    T[:, :3, :3] = Rotation.random(n, random_state=seed).as_matrix().astype(np.float32)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframes_timing.json"))
    args = ap.parse_args()
    import torch
    from bundletrack_amd import _lib
    from bundletrack_amd.bundler import FrameRef, KeyframeMemory
    from bundletrack_amd.keyframes import DeviceKeyframeMemory
    from bundletrack_amd.optimizer import Workspace
    assert torch.cuda.is_available(), "needs a GPU"
    drv = C.CDLL(_lib.build_driver("keyframes_driver"))
    drv.keyframes_driver_host_loop.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    ws = Workspace()

    def device_ms(fn):
        for _ in range(WARMUP):
            fn()
        times = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times))

    res = {"gpu": torch.cuda.get_device_name(0), "max_BA_frames": MAX_BA, "reps": REPS, "unit": "ms", "cases": []}
    for P in POOLS:
        case = {"pool": P}
        for S in SESSIONS:
            T = np.stack([rotations(P + 1, 1000 * S + s) for s in range(S)])                 # [S, P + 1, 4, 4]
            mem = DeviceKeyframeMemory(ws, S, P + 8, MAX_BA)
            ids = torch.zeros(S, dtype=torch.int32, device="cuda")
            for k in range(P):
                mem.check_add(torch.from_numpy(T[:, k]).cuda(), ids + k, min_rot_deg=0.0)
            assert mem.export()["count"].tolist() == [P] * S
            fresh, dup, new_id = torch.from_numpy(T[:, P]).cuda(), torch.from_numpy(T[:, P - 1]).cuda(), ids + P
            added, w = torch.zeros(S, dtype=torch.int32, device="cuda"), mem.empty_windows()
            keys, ones = torch.zeros(S, dtype=torch.int64, device="cuda"), torch.ones(S, dtype=torch.int32, device="cuda")
            L = _lib.lib()
            add = lambda: L.btba_keyframes_check_add(mem._h, 10.0, 0, None, dup.data_ptr(), new_id.data_ptr(), keys.data_ptr(), ones.data_ptr(), ones.data_ptr(),
                                                     added.data_ptr())
            sel = lambda: L.btba_keyframes_select(mem._h, None, fresh.data_ptr(), new_id.data_ptr(), keys.data_ptr(), w.n_window.data_ptr(), w.slot.data_ptr(),
                                                  w.frame_id.data_ptr(), w.frame_key.data_ptr(), w.pose.data_ptr(), w.newframe_index.data_ptr())
            case[f"check_add_{S}"] = device_ms(add)
            case[f"select_{S}"] = device_ms(sel)
            assert added.cpu().tolist() == [0] * S and mem.export()["count"].tolist() == [P] * S
            if S == 1:
                device_window = w.frame_id.cpu().numpy()[0, : int(w.n_window.cpu()[0])].tolist()
                # the numpy host memory on the same poses
                host = KeyframeMemory(min_rot_deg=0.0, max_BA_frames=MAX_BA)
                frames = [FrameRef(id=k, pose_in_model=T[0, k], n_keypts=100) for k in range(P + 1)]
                for fr in frames[:P]:
                    assert host.check_and_add_keyframe(fr)
                t_sel, t_add = [], []
                for _ in range(REPS if P < 1000 else 3):
                    t0 = time.perf_counter(); chosen = host.select_keyframes_for_ba(frames[P]); t_sel.append(1e3 * (time.perf_counter() - t0))
                for _ in range(REPS):
                    t0 = time.perf_counter(); ok = host.check_and_add_keyframe(frames[P]); t_add.append(1e3 * (time.perf_counter() - t0))
                    assert ok
                    host.keyframes.pop()
                case["numpy_host_select_1"], case["numpy_host_check_add_1"] = float(np.median(t_sel)), float(np.median(t_add))
                case["device_window_equals_numpy_host"] = device_window == [f.id for f in chosen]
                # the C++ host memory
                ms = np.zeros(2 * REPS, np.float64)
                flat = np.ascontiguousarray(T[0].reshape(-1, 16))
                assert drv.keyframes_driver_host_loop(flat.ctypes.data, P, MAX_BA, REPS, ms.ctypes.data) == 0
                case["cpp_host_select_1"], case["cpp_host_check_add_1"] = float(np.median(ms[:REPS])), float(np.median(ms[REPS:]))
            mem.close()
        print(json.dumps(case))
        res["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
