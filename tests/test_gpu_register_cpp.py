"""The C++ host layer's btba::registerIndex and btba::registerFrames (tests/cpp/register_driver.cpp) on two ellipsoid frames and a point list:
the cell index, the poses, results and trace are, byte for byte, those of the Python path (bundletrack_amd/registration.py), which
tests/test_gpu_register.py holds to the numpy restatement; and the restatement's own decisions are checked once more here."""
import ctypes as C

import numpy as np
import pytest

import register_ref as G
from bundletrack_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32


def test_cpp_layer_returns_the_python_paths_bytes(oracle):
    import torch
    from bundletrack_amd.fusion import ObjectCloud, Segment
    from bundletrack_amd.optimizer import Workspace
    from bundletrack_amd.registration import build_index, register_frames
    drv = C.CDLL(_lib.build_driver("register_driver"))
    drv.register_driver_index.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3
    drv.register_driver_frames.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    sc = G.ellipsoid_scene(oracle)
    model, box, leaf, H, W = sc["model"], sc["box"], sc["leaf"], sc["H"], sc["W"]
    n_iters = 4
    ws = Workspace()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cap = model["n_out"] + 3
    pad = lambda a, fill=0: np.concatenate([a, np.full((cap - len(a),) + a.shape[1:], fill, a.dtype)])
    xyz, nrm, lin, n_out = t(pad(model["xyz"])), t(pad(model["normal"])), t(pad(model["lin"], -7)), t(np.array([model["n_out"]], np.int32))
    V = int(np.prod(box[0, 3:]))
    cells = torch.full((V,), 5, dtype=torch.int32, device="cuda")
    assert drv.register_driver_index(ws.handle.value, box.ctypes.data, cap, lin.data_ptr(), n_out.data_ptr(), cells.data_ptr()) == 0
    ws.sync()
    assert np.array_equal(cells.cpu().numpy(), G.cell_index(model, box[0]))

    views = (2, 4)
    poses = [G.perturbed(sc["segs"][v]["pose"], 3.0, 6.0, seed=50 + v) for v in views] + [G.perturbed(np.eye(4, dtype=F), 2.0, 3.0, seed=60)]
    pts = np.ascontiguousarray(model["xyz"][::3])
    depth = [t(sc["segs"][v]["depth"]) for v in views]
    normal = [t(sc["segs"][v]["normal"]) for v in views]
    pts_dev = t(pts)
    ptr = lambda ts: (C.c_void_p * len(ts))(*[x.data_ptr() for x in ts])
    Kf = np.ascontiguousarray(sc["K"], F).reshape(9)
    P = np.ascontiguousarray(np.stack(poses), F)
    pose_out = torch.zeros((3, 12), dtype=torch.float32, device="cuda")
    result = torch.zeros((3, 32), dtype=torch.uint8, device="cuda")
    trace = torch.zeros((3, n_iters, 344), dtype=torch.uint8, device="cuda")
    args = lambda leaf_: (ws.handle.value, leaf_, n_iters, 2, H, W, Kf.ctypes.data, P.ctypes.data, ptr(depth), ptr(normal), pts_dev.data_ptr(), len(pts),
                          box.ctypes.data, cap, xyz.data_ptr(), nrm.data_ptr(), cells.data_ptr(), pose_out.data_ptr(), result.data_ptr(), trace.data_ptr())
    assert drv.register_driver_frames(*args(leaf)) == 0
    ws.sync()

    cloud = ObjectCloud(xyz=xyz[None], normal=nrm[None], colour=None, count=None, lin=lin[None], n_out=n_out, n_outside=None, status=None, box=box, leaf=leaf)
    segs = [Segment(0, poses[k], depth=depth[k], normal=normal[k]) for k in range(2)] + [Segment(0, poses[2], xyz=pts_dev)]
    py = register_frames(ws, build_index(ws, cloud), segs, sc["K"], trace=True, n_iters=n_iters)
    torch.cuda.synchronize()
    assert pose_out.cpu().numpy().tobytes() == py.pose.cpu().numpy().tobytes()
    assert result.cpu().numpy().tobytes() == py.result_dev.cpu().numpy().tobytes() and trace.cpu().numpy().tobytes() == py.trace_dev.cpu().numpy().tobytes()
    res = result.cpu().numpy().reshape(-1).view(_lib.REGISTER_RESULT_DTYPE)
    for k, v in enumerate(views):                                       # the decisions, against the restatement from the same start
        seg = dict(sc["segs"][v], pose=poses[k])
        first = G.step(seg, poses[k][:3], model, box[0], G.params(leaf), sc["Ki"])
        e = py.trace[k, 0]
        assert (e["n_valid"], e["n_matched"], e["n_beyond"]) == (first["n_valid"], first["n_matched"], first["n_beyond"])
    print(res["status"], res["iters_done"], res["n_matched"])
    assert (res["n_matched"] > 300).all() and res["status"].max() <= G.MAX_ITERS
    assert drv.register_driver_frames(*args(0.0)) == _lib.BTBA_EINVAL        # leaf 0: btba::Error's status
    ws.close()
