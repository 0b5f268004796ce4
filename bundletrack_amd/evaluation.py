"""Pose accuracy on the MI355X: ADD, ADD-S and their VOCap AUC, the figures BundleTrack's users quote.

Mirrors the reference's evaluation (scripts/eval_ycbineoat.py:54-163 with scripts/Utils.py:69-95): per frame the mean distance
of the model points under the predicted and the ground-truth pose (ADD) and the mean distance of every ground-truth point to
its nearest predicted point (ADD-S, the reference's `adi` on a cKDTree); per object and overall the area under the accuracy
curve up to 0.1 m.  The errors of any number of frames, sequences and models come from one btba_pose_errors call
(include/btba.h fixes the arithmetic); the AUC is a sort on the host.  Poses are OBJECT-IN-CAMERA, as the reference's
poses/*.txt files hold them; `ob_in_cam` turns the tracker's camera -> model poses into that convention."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib


def ob_in_cam(poses_cam2model):
    """Object-in-camera poses from camera -> model poses ([4,4] or [n,4,4]): the inverse in fp64, rounded to fp32."""
    T = np.asarray(poses_cam2model, np.float64)
    return np.linalg.inv(T).astype(np.float32)


def load_points_xyz(path: str) -> np.ndarray:
    """A model's points.xyz (one 'x y z' line per point, whitespace separated) as float32 [N, 3]."""
    return np.loadtxt(path, dtype=np.float64, ndmin=2)[:, :3].astype(np.float32)


def vocap_auc(errors, max_threshold: float = 0.1) -> float:
    """Area under the accuracy-vs-threshold curve on [0, max_threshold], divided by max_threshold (the reference's VOCap,
    eval_ycbineoat.py:54-81, in closed form).  The errors strictly below the threshold, sorted, are b_1 <= .. <= b_m of n;
    from prev = 0, every k with b_k != prev adds (b_k - prev) k / n and sets prev = b_k; then (thr - prev) m / n is added
    and the sum is divided by thr.  No errors, or none below the threshold: 0."""
    e = np.sort(np.asarray(errors, np.float64).reshape(-1))
    n = e.size
    thr = float(max_threshold)
    if n == 0:
        return 0.0
    b = e[e < thr]
    m = b.size
    if m == 0:
        return 0.0
    area, prev = 0.0, 0.0
    for k in range(1, m + 1):
        if b[k - 1] != prev:
            area += (b[k - 1] - prev) * k / n
            prev = b[k - 1]
    area += (thr - prev) * m / n
    return area / thr


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def pose_errors(ws, models, poses_pred, poses_gt, model_index=None):
    """btba_pose_errors: (add, adds) float32 [n] for n evaluations.

    models: one [N, 3] point set or a list of them (numpy, or float32 CUDA tensors that are used in place).
    poses_pred, poses_gt: [n, 4, 4] (or [4, 4]) object-in-camera.  numpy poses: the call reads and writes host memory and
    returns numpy arrays; CUDA tensors: device_resident, the outputs are CUDA tensors and nothing crosses to the host.
    model_index: int [n] into models (default: all 0)."""
    import torch
    from .optimizer import _dev_ptr
    if _is_torch(models) or (isinstance(models, np.ndarray) and models.ndim == 2):
        models = [models]
    dev_models = []
    for k, m in enumerate(models):
        t = m if _is_torch(m) else torch.from_numpy(np.ascontiguousarray(np.asarray(m, np.float32).reshape(-1, 3)))
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise ValueError(f"model {k}: expected float32 [N, 3], got {tuple(t.shape)} {t.dtype}")
        dev_models.append(t.contiguous().cuda() if not t.is_cuda else t.contiguous())
    n_pts = np.array([t.shape[0] for t in dev_models], np.int32)
    ptrs = (C.c_void_p * len(dev_models))(*[_dev_ptr(t, f"model {k}") for k, t in enumerate(dev_models)])
    device = _is_torch(poses_pred)
    if device != _is_torch(poses_gt):
        raise ValueError("poses_pred and poses_gt must both be numpy arrays or both CUDA tensors")
    if device:
        pp = poses_pred.to(torch.float32).reshape(-1, 16).contiguous()
        pg = poses_gt.to(torch.float32).reshape(-1, 16).contiguous()
    else:
        pp = np.ascontiguousarray(np.asarray(poses_pred, np.float32).reshape(-1, 16))
        pg = np.ascontiguousarray(np.asarray(poses_gt, np.float32).reshape(-1, 16))
    n = pp.shape[0]
    if pg.shape[0] != n:
        raise ValueError(f"{n} predicted poses but {pg.shape[0]} ground-truth poses")
    mi = np.zeros(n, np.int32) if model_index is None else np.ascontiguousarray(np.asarray(model_index, np.int32).reshape(-1))
    if mi.shape[0] != n:
        raise ValueError(f"model_index has {mi.shape[0]} entries for {n} evaluations")
    if device:
        add = torch.empty(max(n, 1), dtype=torch.float32, device=pp.device)
        adds = torch.empty(max(n, 1), dtype=torch.float32, device=pp.device)
        args = (_dev_ptr(pp, "poses_pred"), _dev_ptr(pg, "poses_gt"), _dev_ptr(add, "add"), _dev_ptr(adds, "adds"))
    else:
        add, adds = np.empty(max(n, 1), np.float32), np.empty(max(n, 1), np.float32)
        args = (pp.ctypes.data, pg.ctypes.data, add.ctypes.data, adds.ctypes.data)
    check(lib().btba_pose_errors(ws.handle, int(device), len(dev_models), C.cast(ptrs, C.c_void_p), n_pts.ctypes.data, n, mi.ctypes.data, *args),
          "btba_pose_errors")
    return add[:n], adds[:n]


def evaluate_sequences(sequences: dict, ws=None, max_threshold: float = 0.1) -> dict:
    """eval_ycbineoat.py's report: sequences = {name: (model_pts [N, 3], pred [n, 4, 4], gt [n, 4, 4])} with object-in-camera
    poses; every key is one row (the reference's rows are objects: concatenate an object's sequences under one key).
    Returns {name: {"n", "add_auc", "adds_auc"}, ..., "overall": {...}} with the AUCs x 100 ("overall" over all frames), and
    the per-frame errors under "errors" ({name: (add, adds)}).  One btba_pose_errors call for all frames; ws: a Workspace,
    or None for a temporary one."""
    from .optimizer import Workspace
    own = ws is None
    ws = Workspace() if own else ws
    try:
        names = list(sequences)
        models, pred, gt, index = [], [], [], []
        for m, name in enumerate(names):
            pts, p, g = sequences[name]
            p = np.asarray(p, np.float32).reshape(-1, 4, 4)
            g = np.asarray(g, np.float32).reshape(-1, 4, 4)
            if p.shape != g.shape:
                raise ValueError(f"{name}: {p.shape[0]} predicted poses but {g.shape[0]} ground-truth poses")
            models.append(np.asarray(pts, np.float32).reshape(-1, 3))
            pred.append(p)
            gt.append(g)
            index.append(np.full(p.shape[0], m, np.int32))
        add, adds = pose_errors(ws, models, np.concatenate(pred), np.concatenate(gt), np.concatenate(index))
    finally:
        if own:
            ws.close()
    out, errors, o = {}, {}, 0
    for name, p in zip(names, pred):
        a, s = add[o:o + p.shape[0]], adds[o:o + p.shape[0]]
        o += p.shape[0]
        errors[name] = (a, s)
        out[name] = {"n": int(p.shape[0]), "add_auc": 100.0 * vocap_auc(a, max_threshold), "adds_auc": 100.0 * vocap_auc(s, max_threshold)}
    out["overall"] = {"n": int(add.shape[0]), "add_auc": 100.0 * vocap_auc(add, max_threshold), "adds_auc": 100.0 * vocap_auc(adds, max_threshold)}
    out["errors"] = errors
    return out
