"""Frame-to-model registration on the MI355X (btba_register_index, btba_register_frames, btba_register_associate): batched point-to-plane ICP
of frames or point lists against the cloud fusion.fuse_frames / voxel_downsample made.

What it is for: bringing a frame the tracker lost back against what the session has learned of the object; the numeric half of a pose check
(n_iters=0: the points of a frame that lie on the model at a pose, and their point-to-plane error); a per-frame drift figure where no CAD
model exists.  The exact rules are in include/btba.h ("frame-to-model registration"); tests/register_ref.py restates them.  Fuse the model
with normalize_normals=True: the model normals are used as they are."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from ._lib import REG_STATUS_NAMES, REGISTER_ITER_DTYPE, REGISTER_RESULT_DTYPE, check, lib, register_params
from .fusion import ObjectCloud, _K, _segment_array, fuse_layout


@dataclass
class ModelIndex:
    """An ObjectCloud with the cell index the registration looks candidates up in: int32 [V], -1 or the record of the voxel."""
    cloud: ObjectCloud
    cell_index: object          # CUDA int32 [max(V, 1)]
    voxel_offsets: np.ndarray   # int64 [B + 1], host


def build_index(ws, cloud: ObjectCloud) -> ModelIndex:
    """btba_register_index over an ObjectCloud (asynchronous on the workspace stream); build it once per cloud and reuse it."""
    import torch
    if cloud.normal is None:
        raise ValueError("registration needs a cloud with normals (fuse with want_normals=True, normalize_normals=True)")
    B, capacity = int(cloud.xyz.shape[0]), int(cloud.xyz.shape[1])
    box = np.ascontiguousarray(cloud.box, np.int32).reshape(B, 6)
    off, _ = fuse_layout(box)
    cells = torch.empty((max(int(off[-1]), 1),), dtype=torch.int32, device="cuda")
    check(lib().btba_register_index(ws.handle, B, box.ctypes.data, capacity, cloud.lin.data_ptr(), cloud.n_out.data_ptr(), cells.data_ptr()), "btba_register_index")
    return ModelIndex(cloud, cells, off)


@dataclass
class Registration:
    """The outcome of register_frames.  pose is on the device ([n, 3, 4] float32, rows 0 .. 2 of camera -> model); everything else is read
    back on first use (one synchronisation) from the device records."""
    pose: object
    result_dev: object                 # CUDA uint8 [n, 32]: btba_register_result
    trace_dev: object = None           # CUDA uint8 [n, n_iters, 344]: btba_register_iter, or None
    _host: dict = field(default_factory=dict, repr=False)

    @property
    def result(self) -> np.ndarray:
        """btba_register_result of every item as a structured array (synchronises)."""
        if "result" not in self._host:
            self._host["result"] = self.result_dev.cpu().numpy().reshape(-1).view(REGISTER_RESULT_DTYPE)
        return self._host["result"]

    @property
    def trace(self):
        """btba_register_iter [n, n_iters] as a structured array, or None (synchronises)."""
        if self.trace_dev is None:
            return None
        if "trace" not in self._host:
            n, it = self.trace_dev.shape[:2]
            self._host["trace"] = self.trace_dev.cpu().numpy().reshape(-1).view(REGISTER_ITER_DTYPE).reshape(n, it)
        return self._host["trace"]

    status = property(lambda self: self.result["status"])
    iterations = property(lambda self: self.result["iters_done"])
    n_valid = property(lambda self: self.result["n_valid"])
    n_matched = property(lambda self: self.result["n_matched"])
    n_beyond = property(lambda self: self.result["n_beyond"])
    cost = property(lambda self: self.result["cost"])

    @property
    def status_names(self):
        return [REG_STATUS_NAMES[s] for s in self.status]

    @property
    def fitness(self) -> np.ndarray:
        """n_matched / n_valid at pose (0 without a valid point)."""
        return self.n_matched / np.maximum(self.n_valid, 1)

    @property
    def rms(self) -> np.ndarray:
        """sqrt(cost / n_matched) at pose: the Huber cost per matched point as a length (nan without a match)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.sqrt(self.cost / self.n_matched)

    def poses4(self) -> np.ndarray:
        """pose as [n, 4, 4] float32 on the host (synchronises)."""
        p = self.pose.cpu().numpy()
        out = np.tile(np.eye(4, dtype=np.float32), (p.shape[0], 1, 1))
        out[:, :3] = p
        return out


class _Call:
    """The arguments register_frames and associate share, marshalled once.  The C ABI reads the host arrays (segments, K, box, params) during the
    call only; this object owns them, so they live until the caller has made the call and dropped it."""

    def __init__(self, ws, model, segments, K, params):
        self.index = model if isinstance(model, ModelIndex) else build_index(ws, model)
        cloud = self.index.cloud
        self.segments = list(segments)
        B, capacity = int(cloud.xyz.shape[0]), int(cloud.xyz.shape[1])
        self.arr, self.H, self.W, _, self.keep = _segment_array(self.segments, B)
        self.Kf, Kp = _K(K, self.H > 0)
        self.prm = register_params(leaf=float(cloud.leaf), **params)
        self.box = np.ascontiguousarray(cloud.box, np.int32).reshape(B, 6)
        self.head = (ws.handle, C.byref(self.prm), B, len(self.segments), C.cast(self.arr, C.c_void_p), self.H, self.W, Kp, self.box.ctypes.data, capacity,
                     cloud.xyz.data_ptr(), cloud.normal.data_ptr(), self.index.cell_index.data_ptr())


def register_frames(ws, model, segments, K=None, *, trace=False, **params) -> Registration:
    """btba_register_frames on fusion.Segment objects (pose = the initial camera -> model pose, instance = the model within the cloud).
    model: an ObjectCloud (its index is built here) or a ModelIndex.  params: the fields of btba_register_params but leaf, which is the
    cloud's (search_radius, max_dist, min_cos, huber_delta, n_iters, eps_rot, eps_trans, min_matches, require_normals).  Asynchronous on
    the workspace stream; trace=True also records every iteration."""
    import torch
    call = _Call(ws, model, segments, K, params)
    n = len(call.segments)
    pose = torch.empty((n, 3, 4), dtype=torch.float32, device="cuda")
    result = torch.empty((n, REGISTER_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    tr = torch.empty((n, int(call.prm.n_iters), REGISTER_ITER_DTYPE.itemsize), dtype=torch.uint8, device="cuda") if trace else None
    check(lib().btba_register_frames(*call.head, pose.data_ptr(), result.data_ptr(), tr.data_ptr() if trace and tr.numel() else None), "btba_register_frames")
    del call                                                     # (held until here: the call has returned)
    return Registration(pose, result, tr)


def associate(ws, model, segments, K=None, **params):
    """btba_register_associate: one association pass at the segments' poses, a CUDA int32 tensor per segment ([H, W] or [n]): the matched
    model record, -1 no candidate, -2 beyond max_dist, -3 failed the normal gate (or the model normal is zero), -4 the point was dropped."""
    import torch
    call = _Call(ws, model, segments, K, params)
    out = [torch.empty((call.H, call.W) if s.xyz is None else (int(s.xyz.shape[0]),), dtype=torch.int32, device="cuda") for s in call.segments]
    table = (C.c_void_p * max(len(out), 1))(*[t.data_ptr() if t.numel() else None for t in out])
    check(lib().btba_register_associate(*call.head, C.cast(table, C.c_void_p)), "btba_register_associate")
    del call                                                     # (held until here: the call has returned)
    return out
