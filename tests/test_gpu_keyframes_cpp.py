"""The C++ host layer's btba::DeviceKeyframeMemory (tests/cpp/keyframes_driver.cpp) on the four-session case of tests/test_gpu_keyframes.py:
pools, windows, the write-back and the distances are, byte for byte, those of the Python path (bundletrack_amd/keyframes.py), which
tests/test_gpu_keyframes.py holds to the numpy restatement."""
import ctypes as C

import numpy as np
import pytest

import keyframes_ref as G
from bundletrack_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
CAP, MAX_BA = 320, 6


def test_cpp_layer_returns_the_python_paths_bytes():
    import torch
    from bundletrack_amd.keyframes import DeviceKeyframeMemory, rotation_distances
    from bundletrack_amd.optimizer import Workspace
    drv = C.CDLL(_lib.build_driver("keyframes_driver"))
    drv.keyframes_driver_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]
    drv.keyframes_driver_destroy.restype = None
    drv.keyframes_driver_add.argtypes = [C.c_void_p] * 7
    drv.keyframes_driver_select.argtypes = [C.c_void_p] * 9
    drv.keyframes_driver_writeback.argtypes = [C.c_void_p] * 3
    drv.keyframes_driver_export.argtypes = [C.c_void_p] * 5
    drv.keyframes_driver_distances.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
    ws = Workspace()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    poses, ids, keys, new_pose, new_id, new_key = G.select_case()
    S = 4
    py = DeviceKeyframeMemory(ws, S, CAP, MAX_BA)
    assert drv.keyframes_driver_create(ws.handle.value, S, CAP, MAX_BA, 0.0, 0) == 0          # min_rot 0: every frame joins
    ones = t(np.ones(S, np.int32))
    added = torch.zeros(S, dtype=torch.int32, device="cuda")
    for k in range(max(len(p) for p in poses)):
        active = np.array([k < len(p) for p in poses], np.int32)
        pose = np.stack([p[min(k, len(p) - 1)] for p in poses])
        fid = np.array([i[min(k, len(i) - 1)] for i in ids], np.int32)
        key = np.array([q[min(k, len(q) - 1)] for q in keys], np.uint64)
        py.check_add(pose, fid, key, active=active, min_rot_deg=0.0)
        a, p_, f_, k_ = t(active), t(pose), t(fid), t(key.view(np.int64))
        assert drv.keyframes_driver_add(a.data_ptr(), p_.data_ptr(), f_.data_ptr(), k_.data_ptr(), ones.data_ptr(), ones.data_ptr(), added.data_ptr()) == 0
        assert added.cpu().numpy()[active != 0].tolist() == [1] * int(active.sum())

    def export():
        e = dict(count=np.zeros(S, np.int32), overflow=np.zeros(S, np.int32), frame_id=np.zeros((S, CAP), np.int32), frame_key=np.zeros((S, CAP), np.uint64),
                 poses=np.zeros((S, CAP, 4, 4), F))
        assert drv.keyframes_driver_export(*[e[k].ctypes.data for k in ("count", "overflow", "frame_id", "frame_key", "poses")]) == 0
        return e

    def same_state():
        a, b = export(), py.export()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        return a

    assert same_state()["count"].tolist() == [3, 5, 6, 300]
    np_, ni, nk = t(new_pose), t(new_id), t(new_key.view(np.int64))
    w_py = py.select(np_, ni, nk)
    w = py.empty_windows()
    assert drv.keyframes_driver_select(np_.data_ptr(), ni.data_ptr(), nk.data_ptr(), w.n_window.data_ptr(), w.slot.data_ptr(), w.frame_id.data_ptr(),
                                       w.frame_key.data_ptr(), w.pose.data_ptr(), w.newframe_index.data_ptr()) == 0
    for name in ("n_window", "slot", "frame_id", "frame_key", "pose", "newframe_index"):
        assert getattr(w, name).cpu().numpy().tobytes() == getattr(w_py, name).cpu().numpy().tobytes(), name
    assert w.n_window.cpu().numpy().tolist() == [4, 6, 6, 6] and w.slot.cpu().numpy()[3].tolist()[:3] == [0, 5, 70]      # the restatement's decisions once more
    solved = w.pose + 0.001
    py.writeback(w.n_window, w.slot, solved)
    assert drv.keyframes_driver_writeback(w.n_window.data_ptr(), w.slot.data_ptr(), solved.data_ptr()) == 0
    assert same_state()["poses"][3, 5].tobytes() == solved.cpu().numpy()[3, 1].tobytes()
    A, B = t(G.random_rotations(100, 1)), t(G.random_rotations(100, 2))
    d = torch.zeros(100, dtype=torch.float32, device="cuda")
    assert drv.keyframes_driver_distances(ws.handle.value, 100, A.data_ptr(), B.data_ptr(), d.data_ptr()) == 0
    assert d.cpu().numpy().tobytes() == rotation_distances(ws, A, B).cpu().numpy().tobytes()
    assert drv.keyframes_driver_create(ws.handle.value, 1, 1024, 40, 10.0, 0) == _lib.BTBA_EINVAL      # btba::Error's status; the old memory is gone
    drv.keyframes_driver_destroy()
    py.close()
    ws.close()
