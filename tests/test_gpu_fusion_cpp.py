"""The C++ host layer's btba::fuseBounds, btba::fuseFrames and btba::voxelDownsample (tests/cpp/fusion_driver.cpp) on the three sphere
frames and on a random cloud: the bytes of the numpy restatement (tests/fusion_ref.py), which the Python path is held to as well."""
import ctypes as C

import numpy as np
import pytest

import fusion_ref as R
from bundletrack_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
H, W, LEAF = 48, 64, 0.01


def test_cpp_layer_returns_the_references_bytes(oracle):
    import torch
    from bundletrack_amd.optimizer import Workspace
    drv = C.CDLL(_lib.build_driver("fusion_driver"))
    drv.fusion_driver_frames.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 8
    drv.fusion_driver_downsample.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    K = R.small_K(H, W)
    Ki = R.kinv4(oracle, K)
    views = R.sphere_segments(R.THREE_VIEWS, 0, K, H, W)
    box = R.bounds(views, 1, Ki, LEAF)
    ref = R.fuse(views, 1, Ki, box, LEAF)[0]
    ws = Workspace()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    maps = {k: [t(s[k]) for s in views] for k in ("depth", "normal", "colour")}
    ptr = lambda ts: (C.c_void_p * len(ts))(*[x.data_ptr() for x in ts])
    poses = np.ascontiguousarray(np.stack([s["pose"] for s in views]), F)
    Kf = np.ascontiguousarray(K, F).reshape(9)
    cap = ref["n_out"] + 5
    new = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    out = {"xyz": new((cap, 4), torch.float32), "normal": new((cap, 4), torch.float32), "colour": new((cap, 4), torch.uint8), "count": new((cap,), torch.int32),
           "lin": new((cap,), torch.int32), "n_out": new((1,), torch.int32), "n_outside": new((1,), torch.int32), "status": new((1,), torch.int32)}
    box_dev = new((1, 6), torch.int32)
    common = (3, H, W, Kf.ctypes.data, poses.ctypes.data, ptr(maps["depth"]), ptr(maps["normal"]), ptr(maps["colour"]))
    outs = [out[k].data_ptr() for k in ("xyz", "normal", "colour", "count", "lin", "n_out", "n_outside", "status")]
    assert drv.fusion_driver_frames(ws.handle.value, 0, LEAF, *common, box_dev.data_ptr(), None, 0, *([None] * 8)) == 0
    ws.sync()
    assert np.array_equal(box_dev.cpu().numpy(), box)
    assert drv.fusion_driver_frames(ws.handle.value, 1, LEAF, *common, None, box.ctypes.data, cap, *outs) == 0
    ws.sync()
    n = int(out["n_out"].item())
    assert n == ref["n_out"] and int(out["n_outside"].item()) == ref["n_outside"] and int(out["status"].item()) == 0
    for k in ("xyz", "normal", "colour", "count", "lin"):
        assert out[k][:n].cpu().numpy().tobytes() == ref[k].tobytes(), k
    assert drv.fusion_driver_frames(ws.handle.value, 1, 0.0, *common, None, box.ctypes.data, cap, *outs) == _lib.BTBA_EINVAL      # leaf 0: btba::Error's status

    rng = np.random.default_rng(8)
    pts = np.concatenate([rng.normal(size=(700, 3)) * 0.05, np.ones((700, 1))], 1).astype(F)
    dref, dbox = R.voxel_downsample(pts, 0.015)
    assert dref["n_out"] < cap
    pts_dev = t(pts)
    assert drv.fusion_driver_downsample(ws.handle.value, 0.015, pts_dev.data_ptr(), 700, dbox.ctypes.data, cap, *[out[k].data_ptr() for k in ("xyz", "count", "lin", "n_out", "n_outside", "status")]) == 0
    ws.sync()
    n = int(out["n_out"].item())
    assert n == dref["n_out"]
    for k in ("xyz", "count", "lin"):
        assert out[k][:n].cpu().numpy().tobytes() == dref[k].tobytes(), k
    ws.close()
