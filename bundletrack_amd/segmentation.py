"""Foreground-mask segmentation on the MI355X (btba_apply_masks): the first step of every frame.

Mirrors Frame::segmentationByMaskFile minus the PNG read (src/Frame.cpp:236-373), which Bundler::processNewFrame calls before
anything else uses the frame (src/Bundler.cpp:80,84): optionally the largest 8-connected component's filled convex hull (the
NOCS configuration), a dilation (5 x 5 in the reference), colour / depth / normals zeroed outside the mask in place, and the
mask's ROI, which decides whether the frame is FAIL (Bundler.cpp:88-93).  The reference does this with OpenCV on the host and
uploads the three maps again; here one call does it for any number of frames without leaving the device.  The exact rules are
in include/btba.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib, mask_params


def apply_masks(ws, frames, masks=None, *, largest_component_hull: bool = False, dilate: int = 5, want_mask: bool = True,
                want_roi: bool = True):
    """btba_apply_masks on FrameRef-like objects with depth_gpu [H,W] float32, normal_gpu [H,W,4] float32 and optionally
    color_gpu [H,W,4] uint8 (CUDA tensors, updated in place).  masks: one [H,W] uint8 / bool CUDA tensor per frame, nonzero =
    foreground; None (or a None entry) takes the frame's mask_gpu.  Sets every frame's roi = (umin, umax, vmin, vmax) (with
    want_roi; the call is then synchronous, otherwise asynchronous on the workspace stream) and fg_mask_gpu = the final 0 / 1
    mask (with want_mask).  Returns the ROIs as float32 [n, 4], or None without want_roi."""
    import torch
    from .optimizer import _dev_ptr
    n = len(frames)
    if n == 0:
        return np.zeros((0, 4), np.float32) if want_roi else None
    masks = [f.mask_gpu for f in frames] if masks is None else [m if m is not None else f.mask_gpu for f, m in zip(frames, masks)]
    if len(masks) != n or any(m is None for m in masks):
        raise ValueError("every frame needs a mask")
    H, W = (int(s) for s in masks[0].shape[:2])
    for k, (f, m) in enumerate(zip(frames, masks)):
        if m.numel() != H * W or f.depth_gpu is None or f.depth_gpu.numel() != H * W or f.normal_gpu is None or f.normal_gpu.numel() != 4 * H * W:
            raise ValueError(f"frame {k}: mask, depth and normals must all be {H} x {W}")
        if f.color_gpu is not None and f.color_gpu.numel() * f.color_gpu.element_size() != 4 * H * W:
            raise ValueError(f"frame {k}: colour must be {H} x {W} x 4 bytes")
        if m.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"frame {k}: the mask must be uint8 or bool, got {m.dtype}")

    def table(ts, what):
        arr = (C.c_void_p * n)()
        for k, t in enumerate(ts):
            arr[k] = _dev_ptr(t, f"frame {k} {what}") if t is not None else None
        return arr

    outs = [torch.empty((H, W), dtype=torch.uint8, device=m.device) for m in masks] if want_mask else None
    has_color = any(f.color_gpu is not None for f in frames)
    roi = np.zeros((n, 4), np.float32) if want_roi else None
    prm = mask_params(largest_component_hull=int(bool(largest_component_hull)), dilate=int(dilate))
    check(lib().btba_apply_masks(ws.handle, C.byref(prm), n, H, W, C.cast(table(masks, "mask"), C.c_void_p),
                                 C.cast(table([f.depth_gpu for f in frames], "depth"), C.c_void_p),
                                 C.cast(table([f.normal_gpu for f in frames], "normals"), C.c_void_p),
                                 C.cast(table([f.color_gpu for f in frames], "colour"), C.c_void_p) if has_color else None,
                                 C.cast(table(outs, "mask_out"), C.c_void_p) if want_mask else None,
                                 roi.ctypes.data if want_roi else None),
          "btba_apply_masks")
    for k, f in enumerate(frames):
        if want_mask:
            f.fg_mask_gpu = outs[k]
        if want_roi:
            f.roi = tuple(float(v) for v in roi[k])
    return roi
