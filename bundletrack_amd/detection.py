"""Detector front end on the MI355X (btba_detector_inputs, btba_detector_keypoints_to_image): the step between the mask and the
matcher.

Mirrors the image and point arithmetic of Lfnet::detectFeature (src/FeatureManager.cpp:811-908, called by
Bundler::processNewFrame, src/Bundler.cpp:103-117) with rot_deg = 0: the masked colour image cropped to the ROI, zero-padded into
a square and resized to out_size x out_size (400 in the reference) with OpenCV's fixed-point INTER_LINEAR, the grey float image
the LF-Net server makes of it (lf-net-release/run_server.py:160-165), and the detector's keypoints mapped back to full-resolution
pixels by the inverse of the crop-and-scale transform.  The detector itself is the caller's (for example a torch model fed the
grey tensor).  The exact rules are in include/btba.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, detector_params, lib


def detector_transform(roi, out_size: int = 400):
    """btba_detector_transform: the forward (full-resolution -> detector pixels) and backward 3 x 3 float32 matrices of a ROI
    (umin, umax, vmin, vmax).  Host only."""
    r = np.ascontiguousarray(roi, np.float32).reshape(4)
    fwd, bwd = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
    check(lib().btba_detector_transform(C.byref(detector_params(out_size=int(out_size))), r.ctypes.data, fwd.ctypes.data, bwd.ctypes.data),
          "btba_detector_transform")
    return fwd, bwd


def _rois(frames):
    roi = np.ascontiguousarray([f.roi for f in frames], np.float32).reshape(len(frames), 4)
    return roi


def prepare_detector_inputs(ws, frames, out_size: int = 400, want_bgr: bool = True, want_gray: bool = True):
    """btba_detector_inputs on FrameRef-like objects with color_gpu [H,W,4] uint8 (the masked colour map) and roi set (as
    segmentation.apply_masks leaves them).  Returns (bgr, gray): CUDA tensors uint8 [n,S,S,3] (the bytes the reference sends the
    detector) and float32 [n,1,S,S] (g / 255), either None when not wanted.  Asynchronous on the workspace stream."""
    import torch
    from .optimizer import _dev_ptr
    n, S = len(frames), int(out_size)
    if n == 0:
        raise ValueError("no frames")
    c0 = frames[0].color_gpu
    if c0 is None or c0.dim() != 3 or c0.shape[2] != 4 or c0.dtype != torch.uint8:
        raise ValueError("frame 0: color_gpu must be a [H, W, 4] uint8 CUDA tensor")
    H, W = int(c0.shape[0]), int(c0.shape[1])
    for k, f in enumerate(frames):
        c = f.color_gpu
        if c is None or tuple(c.shape) != (H, W, 4) or c.dtype != torch.uint8 or not c.is_contiguous():
            raise ValueError(f"frame {k}: color_gpu must be a contiguous [{H}, {W}, 4] uint8 CUDA tensor")
    roi = _rois(frames)
    table = (C.c_void_p * n)(*[_dev_ptr(f.color_gpu, f"frame {k} colour") for k, f in enumerate(frames)])
    dev = c0.device
    bgr = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev) if want_bgr else None
    gray = torch.empty((n, 1, S, S), dtype=torch.float32, device=dev) if want_gray else None
    check(lib().btba_detector_inputs(ws.handle, C.byref(detector_params(out_size=S)), n, H, W, C.cast(table, C.c_void_p), roi.ctypes.data,
                                     bgr.data_ptr() if want_bgr else None, gray.data_ptr() if want_gray else None),
          "btba_detector_inputs")
    return bgr, gray


def keypoints_to_image(ws, frames, kpts, out_size: int = 400, out=None):
    """btba_detector_keypoints_to_image: kpts[k] is a float32 CUDA tensor [m_k, 2] of frame k's keypoints in detector pixels.
    Sets frame.kpts_gpu (float32 [m_k, 2] in full-resolution pixels, btba_match_pairs' format) and frame.n_keypts.  out: None
    (new tensors), "inplace" (kpts[k] is overwritten and becomes kpts_gpu) or a list of [m_k, 2] float32 tensors.
    Asynchronous on the workspace stream."""
    import torch
    from .optimizer import _dev_ptr
    n = len(frames)
    if n == 0 or len(kpts) != n:
        raise ValueError("one keypoint tensor per frame")
    for k, t in enumerate(kpts):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 2 or not t.is_contiguous():
            raise ValueError(f"frame {k}: keypoints must be a contiguous [m, 2] float32 CUDA tensor")
    if out is None:
        outs = [torch.empty_like(t) for t in kpts]
    elif isinstance(out, str) and out == "inplace":
        outs = list(kpts)
    else:
        outs = list(out)
        if len(outs) != n or any(o.shape != t.shape or o.dtype != torch.float32 or not o.is_contiguous() for o, t in zip(outs, kpts)):
            raise ValueError("out: one contiguous float32 tensor of each keypoint tensor's shape")
    counts = np.array([int(t.shape[0]) for t in kpts], np.int32)
    ptr = lambda ts, what: (C.c_void_p * n)(*[_dev_ptr(t, f"frame {k} {what}") if t.numel() else None for k, t in enumerate(ts)])
    roi = _rois(frames)
    check(lib().btba_detector_keypoints_to_image(ws.handle, C.byref(detector_params(out_size=int(out_size))), n, roi.ctypes.data,
                                                 C.cast(ptr(kpts, "keypoints"), C.c_void_p), counts.ctypes.data,
                                                 C.cast(ptr(outs, "keypoints out"), C.c_void_p)),
          "btba_detector_keypoints_to_image")
    for f, o, m in zip(frames, outs, counts):
        f.kpts_gpu = o
        f.n_keypts = int(m)
    return outs
