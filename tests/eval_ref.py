"""Test-side references for btba_pose_errors: the CPU restatement (tests/cpp/eval_host.cpp, bit-exact contract), an independent
fp64 evaluation in the reference's terms (scripts/Utils.py:69-95: transform the model by both poses, ADD = mean point distance,
ADD-S = mean nearest-neighbour distance on a cKDTree of the predicted points), the VOCap closed form, and scene generators."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from bundletrack_amd import synthetic as S

from match_ref import HERE, _build

_host = None


def host_lib():
    """tests/cpp/libeval_host.so (built on first use with g++ -O2 -ffp-contract=off)."""
    global _host
    if _host is None:
        _host = C.CDLL(_build("libeval_host.so", [os.path.join(HERE, "cpp", "eval_host.cpp")], []))
        _host.eval_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _host.eval_host.restype = None
    return _host


def _as_list(models):
    return [models] if isinstance(models, np.ndarray) and models.ndim == 2 else list(models)


def restate(models, poses_pred, poses_gt, model_index=None):
    """eval_host: (add, adds) float32 [n], bit for bit what btba_pose_errors must return."""
    models = [np.ascontiguousarray(np.asarray(m, np.float32).reshape(-1, 3)) for m in _as_list(models)]
    pp = np.ascontiguousarray(np.asarray(poses_pred, np.float32).reshape(-1, 16))
    pg = np.ascontiguousarray(np.asarray(poses_gt, np.float32).reshape(-1, 16))
    n = pp.shape[0]
    mi = np.zeros(n, np.int32) if model_index is None else np.ascontiguousarray(np.asarray(model_index, np.int32))
    ptrs = (C.c_void_p * len(models))(*[m.ctypes.data for m in models])
    n_pts = np.array([m.shape[0] for m in models], np.int32)
    add, adds = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    host_lib().eval_host(len(models), C.cast(ptrs, C.c_void_p), n_pts.ctypes.data, n, mi.ctypes.data, pp.ctypes.data, pg.ctypes.data,
                         add.ctypes.data, adds.ctypes.data, min(16, os.cpu_count() or 1))
    return add[:n], adds[:n]


def _nearest(cand, query):
    """Distance from every query to its nearest candidate, fp64: cKDTree when scipy is there, else a chunked brute force."""
    try:
        from scipy.spatial import cKDTree
        return cKDTree(cand).query(query, k=1, workers=min(16, os.cpu_count() or 1))[0]
    except ImportError:
        out = np.empty(query.shape[0])
        for s in range(0, query.shape[0], 1024):
            d = ((query[s:s + 1024, None, :] - cand[None, :, :]) ** 2).sum(-1)
            out[s:s + 1024] = np.sqrt(d.min(1))
        return out


def fp64(models, poses_pred, poses_gt, model_index=None):
    """(add, adds) float64 [n]: the poses (as given, fp32 values) and points transformed in fp64, exact distances."""
    models = [np.asarray(m, np.float32).reshape(-1, 3).astype(np.float64) for m in _as_list(models)]
    pp = np.asarray(poses_pred, np.float32).reshape(-1, 4, 4).astype(np.float64)
    pg = np.asarray(poses_gt, np.float32).reshape(-1, 4, 4).astype(np.float64)
    mi = np.zeros(pp.shape[0], np.int64) if model_index is None else np.asarray(model_index)
    add, adds = np.zeros(pp.shape[0]), np.zeros(pp.shape[0])
    for e in range(pp.shape[0]):
        x = models[mi[e]]
        c = x @ pp[e, :3, :3].T + pp[e, :3, 3]
        q = x @ pg[e, :3, :3].T + pg[e, :3, 3]
        add[e] = np.linalg.norm(q - c, axis=1).mean()
        adds[e] = _nearest(c, q).mean()
    return add, adds


def vocap(errors, thr=0.1):
    """The VOCap closed form, vectorised (a second statement of evaluation.vocap_auc): over the distinct errors v below thr,
    ascending, the step from the previous one (from 0) times k / n, k the rank of v's first occurrence; then the last step out
    to thr times m / n (m errors below thr)."""
    e = np.sort(np.asarray(errors, np.float64).reshape(-1))
    b = e[e < thr]
    if e.size == 0 or b.size == 0:
        return 0.0
    vals = np.unique(b)
    k_first = np.searchsorted(b, vals, side="left") + 1
    steps = vals - np.concatenate([[0.0], vals[:-1]])
    return float(((steps * k_first).sum() / e.size + (thr - vals[-1]) * b.size / e.size) / thr)


def random_rotation(rng) -> np.ndarray:
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene_poses(n, seed, rot_deg=3.0, trans_m=0.01):
    """(pred, gt) float32 [n, 4, 4] object-in-camera: the object 0.5 .. 1 m in front of the camera, the prediction off by up to
    rot_deg about a random axis and up to trans_m per axis."""
    rng = np.random.default_rng(seed)
    gt, pred = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))
    for e in range(n):
        G = np.eye(4)
        G[:3, :3] = random_rotation(rng)
        G[:3, 3] = [rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(0.5, 1.0)]
        w = rng.normal(size=3)
        w *= np.deg2rad(rng.uniform(0, rot_deg)) / np.linalg.norm(w)
        D = S.se3_exp(w, rng.uniform(-trans_m, trans_m, size=3))
        gt[e], pred[e] = G, G @ D
    return pred.astype(np.float32), gt.astype(np.float32)


def symmetric_model(n, seed):
    """float32 [2n, 3] closed under diag(-1, 1, -1): n surface points and their mirrors (-x, y, -z)."""
    p = S.model_points(n, seed)
    return np.concatenate([p, p * np.array([-1, 1, -1], np.float32)])


_driver = None


def driver():
    """tests/cpp/libeval_driver.so: btba::poseErrors and btba::vocapAuc of the C++ host layer, linked against libbtba.so."""
    global _driver
    if _driver is None:
        from bundletrack_amd import _lib
        so = _lib.build_driver("eval_driver")
        _driver = C.CDLL(so)
        _driver.pose_errors_driver.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
        _driver.vocap_driver.argtypes = [C.c_void_p, C.c_int, C.c_double]
        _driver.vocap_driver.restype = C.c_double
    return _driver


def session_errors(frames, seq, model):
    """(add, adds) of a tracking session's final poses (camera -> model, FrameRef.pose_in_model) against the sequence's ground
    truth, through the CPU restatement."""
    from bundletrack_amd.evaluation import ob_in_cam
    pred = ob_in_cam(np.stack([f.pose_in_model for f in frames]))
    gt = ob_in_cam(seq.poses_gt[: len(frames)])
    return restate(model, pred, gt)
