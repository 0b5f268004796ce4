"""The C++ host layer's btba::linearizeBatchZn and btba::poseCovariances (tests/cpp/marginals_driver.cpp) on one K = 3 window: the bits of
the Python path (BatchSolver.linearize_zn, covariance.pose_covariances)."""
import ctypes as C

import numpy as np
import pytest

import solve_ref as SR
from bundletrack_amd import _lib, synthetic as S

pytestmark = pytest.mark.gpu


def test_cpp_layer_returns_the_python_paths_bits():
    import torch
    from bundletrack_amd.covariance import pose_covariances
    from bundletrack_amd.optimizer import BatchSolver, Workspace
    drv = C.CDLL(_lib.build_driver("marginals_driver"))
    drv.marginals_driver.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_uint32] + [C.c_void_p] * 7
    dev = torch.device("cuda:0")
    K = 3
    pb, corr = SR.window(K, 532)
    ws = Workspace()
    bs = BatchSolver(ws)
    corr_h, offs, mx = bs.pack_correspondences([corr], K)
    zn = torch.from_numpy(S.compact_cache(pb)[None]).to(dev)
    corr_d = torch.from_numpy(corr_h.view(np.uint8).reshape(1, -1, 32)).to(dev)
    offs_d = torch.from_numpy(offs.astype(np.int32)).to(dev)
    poses = torch.from_numpy(pb.poses_init[None].astype(np.float32)).to(dev)
    info, rhs = bs.linearize_zn(zn, pb.H, pb.W, pb.K, corr_d, offs_d, mx, poses, rhs=True)
    py = pose_covariances(ws, info, full=True)
    ws.sync()

    na = 6 * (K - 1)
    info2, rhs2 = torch.zeros_like(info), torch.zeros_like(rhs)
    blocks, full = torch.zeros((1, K, 6, 6), dtype=torch.float64, device=dev), torch.zeros((1, na, na), dtype=torch.float64, device=dev)
    ratio, status = torch.zeros((1,), dtype=torch.float64, device=dev), torch.full((1,), -1, dtype=torch.int32, device=dev)
    Kf = np.ascontiguousarray(pb.K, np.float32).reshape(9)
    rc = drv.marginals_driver(ws.handle.value, 7, 1, K, pb.H, pb.W, Kf.ctypes.data, zn.data_ptr(), corr_d.data_ptr(), corr_d.shape[1], offs_d.data_ptr(), mx,
                              poses.data_ptr(), info2.data_ptr(), rhs2.data_ptr(), blocks.data_ptr(), full.data_ptr(), ratio.data_ptr(), status.data_ptr())
    assert rc == 0
    ws.sync()
    same = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert same(info2, info) and same(rhs2, rhs)
    assert same(blocks, py.blocks) and same(full, py.full) and same(ratio, py.pivot_ratio) and same(status, py.status)
    assert int(status[0]) == 0 and np.isfinite(full.cpu().numpy()).all()
