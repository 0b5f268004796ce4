"""The C++ host layer's btba::objectiveBatchZn and btba::residualVariance (tests/cpp/objective_driver.cpp) on one scene with a mixed explicit
pair list: the bytes of the Python path (BatchSolver.objective_zn, objective.residual_variance)."""
import ctypes as C

import numpy as np
import pytest

import sweep_ref as R
from bundletrack_amd import _lib
from bundletrack_amd.objective import residual_variance

pytestmark = pytest.mark.gpu


def test_cpp_layer_returns_the_python_paths_bytes(oracle):
    import torch
    from bundletrack_amd.optimizer import BatchSolver, Workspace, pack_zn
    drv = C.CDLL(_lib.build_driver("objective_driver"))
    drv.objective_driver.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32,
                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    drv.objective_driver_variance.argtypes, drv.objective_driver_variance.restype = [C.c_void_p, C.c_int], C.c_double
    dev = torch.device("cuda:0")
    sc = R.scene("bg50x30")
    ws = Workspace()
    zn = pack_zn(ws, torch.from_numpy(sc["campos"][None]).to(dev), torch.from_numpy(sc["normals"][None]).to(dev))
    corr_d = torch.from_numpy(sc["corr"].view(np.uint8).reshape(1, -1, 32)).to(dev)
    offs_d = torch.from_numpy((np.arange(4, dtype=np.int32) * 40)[None]).to(dev)
    poses = torch.from_numpy(sc["poses"][None].copy()).to(dev)
    pairs = np.array([(2, 0), (0, 1), (1, 2), (1, 0)], np.int32)
    total, sparse, dense = BatchSolver(ws).objective_zn(zn, sc["H"], sc["W"], sc["K"], corr_d, offs_d, 40, poses, dense_pairs=pairs)

    t2 = torch.zeros((1, 64), dtype=torch.uint8, device=dev)
    s2, d2 = torch.zeros((1, 3, 40), dtype=torch.uint8, device=dev), torch.zeros((1, 4, 40), dtype=torch.uint8, device=dev)
    Kf = np.ascontiguousarray(sc["K"], np.float32).reshape(9)
    rc = drv.objective_driver(ws.handle.value, 1, 3, sc["H"], sc["W"], Kf.ctypes.data, zn.data_ptr(), corr_d.data_ptr(), corr_d.shape[1], offs_d.data_ptr(), 40,
                              pairs.ctypes.data, 4, poses.data_ptr(), t2.data_ptr(), s2.data_ptr(), d2.data_ptr())
    assert rc == 0
    ws.sync()
    t2h = t2.cpu().numpy()
    print(f"objective {total['objective'][0]!r}; dense counts {dense[0]['count']}; C++ bytes equal: total {t2h.tobytes() == total.tobytes()}, "
          f"sparse {s2.cpu().numpy().tobytes() == sparse.tobytes()}, dense {d2.cpu().numpy().tobytes() == dense.tobytes()}")
    assert t2h.tobytes() == total.tobytes() and s2.cpu().numpy().tobytes() == sparse.tobytes() and d2.cpu().numpy().tobytes() == dense.tobytes()
    assert dense[0]["count"].all() and total["objective"][0] > 0
    var = drv.objective_driver_variance(np.ascontiguousarray(t2h).ctypes.data, 3)
    assert var == residual_variance(total, 3)[0] and var > 0
