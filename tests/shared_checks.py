"""Helpers that more than one GPU test module uses (one copy each).

- device_matrices: T = Exp(Log(pose)), its inverse and x = Log(pose) as the device forms them, through the library's own SE(3) seams
  (tests/test_gpu_sweep_sums.py, tests/test_gpu_solve_stages.py).
- The A / B rule of the device's SE(3) functions (tests/test_gpu_device_math.py, tests/test_gpu_solve_stages.py): every output component
  within A e_oracle + B ulp(scale) of the float64 truth, e_oracle being the fp32 CPU oracle's own error on the same input."""
import numpy as np

F32 = np.float32
A_IEEE, B_IEEE, A_FAST, B_FAST, FAST_VS_IEEE_ULPS = 2.0, 4.0, 4.0, 8.0, 8.0


def device_poses_and_matrices(g, poses):
    """(x [n, 6], T [n, 4, 4], Tinv [n, 4, 4]): x = Log(pose) in (rot, trans) order, T = Exp(x) and its inverse as k_prepare forms them
    (the same device functions behind btba_matrices_to_poses / btba_poses_to_matrices).  g: an object with .torch, .dev and .ws."""
    from bundletrack_amd import _lib
    n = poses.shape[0]
    P_d = g.torch.from_numpy(np.ascontiguousarray(poses, np.float32).reshape(n, 16)).to(g.dev)
    x_d, T_d, Ti_d = g.torch.zeros((n, 6), device=g.dev), g.torch.zeros((n, 16), device=g.dev), g.torch.zeros((n, 16), device=g.dev)
    L = _lib.lib()
    _lib.check(L.btba_matrices_to_poses(g.ws.handle, n, P_d.data_ptr(), x_d.data_ptr()), "m2p")
    _lib.check(L.btba_poses_to_matrices(g.ws.handle, n, x_d.data_ptr(), T_d.data_ptr(), Ti_d.data_ptr()), "p2m")
    g.ws.sync()
    return x_d.cpu().numpy(), T_d.cpu().numpy().reshape(n, 4, 4), Ti_d.cpu().numpy().reshape(n, 4, 4)


def device_matrices(g, poses):
    """T = Exp(Log(pose)) and its inverse as k_prepare forms them (the same device functions behind the library's SE(3) seams)."""
    return device_poses_and_matrices(g, poses)[1:]


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)


def _bound(stats, labels, name, dev, ora, truth, scale, A, B):
    """assert |dev - truth| <= A |ora - truth| + B ulp(scale) per component; record the worst ratio per branch"""
    dev, ora, truth = (np.asarray(v, np.float64) for v in (dev, ora, truth))
    u = _ulp(scale)
    while u.ndim < dev.ndim:
        u = u[..., None]
    e_dev, e_ora = np.abs(dev - truth), np.abs(ora - truth)
    ratio = (e_dev / (A * e_ora + B * u)).reshape(len(dev), -1).max(1)
    ulps = (e_dev / u).reshape(len(dev), -1).max(1)
    for lab in np.unique(labels):
        m = labels == lab
        key = (name, lab)
        r, q = float(ratio[m].max()), float(ulps[m].max())
        old = stats.get(key, (0.0, 0.0))
        stats[key] = (max(old[0], r), max(old[1], q))
    bad = np.nonzero(~(ratio <= 1.0))[0]
    return [(name, labels[i], i, float(ratio[i])) for i in bad]
