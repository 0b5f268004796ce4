"""Frame ingest on the MI355X (btba_ingest_frames): from a frame's two images to the maps the rest of the pipeline reads.

Mirrors the body of Frame's constructor after the two imreads (src/Frame.cpp:45-89 with Utils::readDepthImage,
src/Utils.cpp:50-69): the 16-bit depth codes decoded to metres, the BGR image packed into the uchar4 colour map,
Frame::processDepth and Frame::depthToCloudAndNormals.  The reference does this frame by frame with a host loop per image and
five launches; here one call does it for any number of frames, two launches per 32 of them, and its outputs equal
optimizer.process_depth + optimizer.depth_to_normals on the decoded depth bit for bit.  The exact rules are in include/btba.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, ingest_params, lib

DEPTH_CODES, DEPTH_METRES = 0, 1          # btba_ingest_params.depth_format


def _code_dtypes(torch):
    return tuple(getattr(torch, n) for n in ("uint16", "int16") if hasattr(torch, n))      # the same 16 bits either way


def ingest_frames(ws, frames, depth=None, bgr=None, K=None, *, depth_format=None, want_xyz=False, want_raw=False, **depth_processing):
    """btba_ingest_frames on FrameRef-like objects.  depth: one [H,W] CUDA tensor per frame, torch.uint16 / torch.int16
    millimetre codes (depth_format 0) or float32 metres (depth_format 1; the call is then a batched process_depth +
    depth_to_normals); None (or a None entry) takes the frame's depth_code_gpu.  bgr: one [H,W,3] uint8 CUDA tensor per frame, None
    (or a None entry) takes the frame's bgr_gpu; a frame without one gets no colour map.  depth_format None reads it off the
    first tensor's dtype.  depth_processing: optimizer.process_depth's keywords.  Sets every frame's depth_gpu [H,W] float32,
    normal_gpu [H,W,4] float32 and, with a BGR image, color_gpu [H,W,4] uint8; with want_xyz also xyz_gpu [H,W,4] float32 and with
    want_raw depth_raw_gpu [H,W] float32 (the decoded, unfiltered depth).  Asynchronous on the workspace stream."""
    import torch
    from .optimizer import DEPTH_PROCESSING_DEFAULTS, _dev_ptr
    if K is None:
        raise ValueError("ingest_frames needs the intrinsics K")
    n = len(frames)
    if n == 0:
        return
    depth = [getattr(f, "depth_code_gpu", None) for f in frames] if depth is None else \
        [d if d is not None else getattr(f, "depth_code_gpu", None) for f, d in zip(frames, depth)]
    bgr = [getattr(f, "bgr_gpu", None) for f in frames] if bgr is None else \
        [b if b is not None else getattr(f, "bgr_gpu", None) for f, b in zip(frames, bgr)]
    if len(depth) != n or len(bgr) != n or any(d is None for d in depth):
        raise ValueError("every frame needs a depth image")
    if depth_format is None:
        depth_format = DEPTH_METRES if depth[0].dtype == torch.float32 else DEPTH_CODES
    if depth_format not in (DEPTH_CODES, DEPTH_METRES):
        raise ValueError(f"depth_format must be 0 (uint16 codes) or 1 (float32 metres), got {depth_format}")
    want = (torch.float32,) if depth_format == DEPTH_METRES else _code_dtypes(torch)
    H, W = (int(s) for s in depth[0].shape[:2])
    in_ptrs = (C.c_void_p * n)()
    for k, (d, b) in enumerate(zip(depth, bgr)):
        if d.dtype not in want:
            raise ValueError(f"frame {k}: depth_format {depth_format} needs {' / '.join(str(t) for t in want)}, got {d.dtype}")
        if d.numel() != H * W:
            raise ValueError(f"frame {k}: the depth image must be {H} x {W}")
        if d.element_size() == 2:           # _dev_ptr takes 4-byte and byte elements only
            if not d.is_cuda or not d.is_contiguous():
                raise ValueError(f"frame {k} depth codes: expected a contiguous CUDA tensor")
            in_ptrs[k] = d.data_ptr()
        else:
            in_ptrs[k] = _dev_ptr(d, f"frame {k} depth")
        if b is not None and (b.dtype != torch.uint8 or b.numel() != 3 * H * W):
            raise ValueError(f"frame {k}: the BGR image must be uint8 {H} x {W} x 3")

    def table(ts, what):
        arr = (C.c_void_p * n)()
        for k, t in enumerate(ts):
            arr[k] = _dev_ptr(t, f"frame {k} {what}") if t is not None else None
        return C.cast(arr, C.c_void_p)

    def new(k, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=depth[k].device)

    d_out = [new(k, (H, W), torch.float32) for k in range(n)]
    n_out = [new(k, (H, W, 4), torch.float32) for k in range(n)]
    c_out = [new(k, (H, W, 4), torch.uint8) if bgr[k] is not None else None for k in range(n)]
    raw = [new(k, (H, W), torch.float32) for k in range(n)] if want_raw else None
    xyz = [new(k, (H, W, 4), torch.float32) for k in range(n)] if want_xyz else None
    has_color = any(b is not None for b in bgr)
    p = dict(DEPTH_PROCESSING_DEFAULTS)
    p.update(depth_processing)
    prm = ingest_params(depth_format=int(depth_format), erode_radius=int(p["erode_radius"]), erode_diff=float(p["erode_diff"]),
                        erode_ratio=float(p["erode_ratio"]), bf_radius=int(p["bf_radius"]), sigma_d=float(p["sigma_d"]), sigma_r=float(p["sigma_r"]))
    Kf = np.ascontiguousarray(K, np.float32).reshape(9)
    check(lib().btba_ingest_frames(ws.handle, C.byref(prm), n, H, W, Kf.ctypes.data, C.cast(in_ptrs, C.c_void_p),
                                   table(bgr, "bgr") if has_color else None, table(d_out, "depth_out"), table(n_out, "normal_out"),
                                   table(c_out, "color_out") if has_color else None, table(raw, "depth_raw_out") if want_raw else None,
                                   table(xyz, "xyz_out") if want_xyz else None), "btba_ingest_frames")
    for k, f in enumerate(frames):
        f.depth_gpu, f.normal_gpu = d_out[k], n_out[k]
        if c_out[k] is not None:
            f.color_gpu = c_out[k]
        if want_raw:
            f.depth_raw_gpu = raw[k]
        if want_xyz:
            f.xyz_gpu = xyz[k]
