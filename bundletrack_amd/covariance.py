"""Pose covariances on the MI355X: the inverse of the solver's Gauss-Newton matrix, batched, in fp64 (btba_pose_covariances).

The matrix comes from BatchSolver.linearize_zn (the solver's system at given poses; include/btba.h says what it is and is not: the sparse
share without a Huber weight, the dense share with it -- the inverse is to be scaled by a residual variance of the caller's).  The unknowns are
those of frames 1 .. N - 1 in the public (rot, trans) order; frame 0 is fixed and gets a zero block."""
from __future__ import annotations

from typing import NamedTuple

from ._lib import check, lib
from .optimizer import _dev_ptr

MAX_FRAMES = 31      # BTBA_MAX_FRAMES_LDS


class PoseCovariances(NamedTuple):
    blocks: object        # CUDA float64 [B, N, 6, 6]: each frame's marginal covariance block, frame 0 zeros
    full: object          # CUDA float64 [B, na, na], or None
    pivot_ratio: object   # CUDA float64 [B]: min_j d_j / H_jj over the Cholesky pivots; 0 where status != 0
    status: object        # CUDA int32 [B]: 0, or 1 + the first unknown whose pivot is not positive and finite (outputs NaN)


def pose_covariances(ws, info, full=False) -> PoseCovariances:
    """info: CUDA float32 [B, na, na] (na = 6 (N - 1), 2 <= N <= 31), symmetric positive definite; its lower triangle is read.
    Asynchronous on the workspace stream; nothing crosses to the host."""
    import torch
    if info.dim() != 3 or info.shape[1] != info.shape[2] or info.shape[1] % 6 or info.dtype != torch.float32:
        raise ValueError(f"info: expected float32 [B, na, na] with na a multiple of 6, got {info.dtype} {tuple(info.shape)}")
    B, na = int(info.shape[0]), int(info.shape[1])
    N = na // 6 + 1
    dev = info.device
    blocks = torch.empty((B, N, 6, 6), dtype=torch.float64, device=dev)
    cov = torch.empty((B, na, na), dtype=torch.float64, device=dev) if full else None
    ratio = torch.empty((B,), dtype=torch.float64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib().btba_pose_covariances(ws.handle, B, N, _dev_ptr(info, "info"), na * na, blocks.data_ptr(), cov.data_ptr() if full else None,
                                      ratio.data_ptr(), _dev_ptr(status, "status")), "btba_pose_covariances")
    return PoseCovariances(blocks, cov, ratio, status)
