"""LF-Net's keypoint head on the MI355X (btba_lfnet_*): everything between the detector's two conv nets.

Mirrors lf-net-release/inference.py::build_multi_scale_deep_detector_3DNMS and build_patch_extraction (on det_tools.py and
spatial_transformer.py) as run_server.py runs them: instance normalisation of every scale's score map, TF1's resize to the photo's
size, the 15 x 15 x S soft-max in scale space, the soft max / arg-max over scale, the frame masks, 5 x 5 NMS and top-k, the keypoints
in raster order, the 9 x 9 soft-arg-max refinement and the scaled, rotated 32 x 32 crop per keypoint.  The two conv nets stay with
the caller: LfnetDetector takes them as callables and is what Bundler(detector=...) takes.  The exact rules are in include/btba.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lfnet_params, lib

MAX_SCALES, MAX_TOP_K = 16, 2048          # BTBA_LFNET_MAX_SCALES, BTBA_LFNET_MAX_TOP_K


def _params(params):
    return lfnet_params() if params is None else (lfnet_params(**params) if isinstance(params, dict) else params)


def _f32(t, shape, what):
    import torch
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected float32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t


def _maps(score_maps, scale_factors, n):
    """The per-scale table of btba_lfnet_heatmaps: score_maps[s] is a float32 CUDA tensor with n * h_s * w_s elements whose last
    two dimensions are (h_s, w_s)."""
    import torch
    from .optimizer import _dev_ptr
    S = len(score_maps)
    if S < 1 or S > MAX_SCALES or len(scale_factors) != S:
        raise ValueError(f"1 .. {MAX_SCALES} score maps and as many scale factors")
    mh, mw = np.zeros(S, np.int32), np.zeros(S, np.int32)
    for s, m in enumerate(score_maps):
        if m.dtype != torch.float32 or m.dim() < 2 or m.numel() != n * int(m.shape[-2]) * int(m.shape[-1]):
            raise ValueError(f"score map {s}: expected float32 with {n} x h x w elements, got {m.dtype} {tuple(m.shape)}")
        mh[s], mw[s] = int(m.shape[-2]), int(m.shape[-1])
    table = (C.c_void_p * S)(*[_dev_ptr(m, f"score map {s}") for s, m in enumerate(score_maps)])
    return S, table, mh, mw, np.ascontiguousarray(scale_factors, np.float32)


def lfnet_heatmaps(ws, score_maps, scale_factors, H: int, W: int, params=None, n_frames: int | None = None):
    """btba_lfnet_heatmaps (stage A).  score_maps[s]: float32 CUDA [n, h_s, w_s] (or [n, 1, h_s, w_s]).  Returns (max_heatmaps,
    max_scales), float32 [n, H, W] each.  Asynchronous on the workspace stream."""
    import torch
    p = _params(params)
    n = int(score_maps[0].shape[0]) if n_frames is None else int(n_frames)
    S, table, mh, mw, sf = _maps(score_maps, scale_factors, n)
    heat = torch.empty((n, int(H), int(W)), dtype=torch.float32, device=score_maps[0].device)
    scales = torch.empty_like(heat)
    check(lib().btba_lfnet_heatmaps(ws.handle, C.byref(p), n, int(H), int(W), S, C.cast(table, C.c_void_p), mh.ctypes.data, mw.ctypes.data,
                                    sf.ctypes.data, heat.data_ptr(), scales.data_ptr()), "btba_lfnet_heatmaps")
    return heat, scales


def lfnet_select(ws, heat, params=None):
    """btba_lfnet_select (stage B).  heat: float32 CUDA [n, H, W] (any heat map).  Returns (kpts_xy int32 [n, top_k, 2] in raster
    order, n_kpts int32 [n]).  Asynchronous on the workspace stream."""
    import torch
    from .optimizer import _dev_ptr
    p = _params(params)
    if heat.dtype != torch.float32 or heat.dim() != 3:
        raise ValueError("lfnet_select: heat must be float32 [n, H, W]")
    n, H, W = (int(s) for s in heat.shape)
    kp = torch.empty((n, max(int(p.top_k), 1), 2), dtype=torch.int32, device=heat.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=heat.device)
    check(lib().btba_lfnet_select(ws.handle, C.byref(p), n, H, W, _dev_ptr(heat, "heat"), kp.data_ptr(), cnt.data_ptr()), "btba_lfnet_select")
    return kp, cnt


def _crop_outputs(n, p, dev):
    import torch
    K, P = max(int(p.top_k), 1), max(int(p.patch_size), 1)
    return (torch.empty((n, K, 2), dtype=torch.float32, device=dev), torch.empty((n, K), dtype=torch.float32, device=dev),
            torch.empty((n, K, 2), dtype=torch.float32, device=dev), torch.empty((n, K, P, P), dtype=torch.float32, device=dev))


def lfnet_crops(ws, photo, ori_maps, heat, scales, kpts_xy, n_kpts, params=None):
    """btba_lfnet_crops (stage C).  photo, heat, scales: float32 CUDA [n, H, W]; ori_maps: float32 [n, H, W, 2] (cos, sin); kpts_xy,
    n_kpts: lfnet_select's.  Returns (kpts [n, top_k, 2], kpts_scale [n, top_k], kpts_ori [n, top_k, 2], patches [n, top_k, P, P]),
    slots past n_kpts zero.  Asynchronous on the workspace stream."""
    import torch
    from .optimizer import _dev_ptr
    p = _params(params)
    n, H, W = (int(s) for s in heat.shape)
    _f32(photo.reshape(n, H, W), (n, H, W), "photo")
    _f32(ori_maps, (n, H, W, 2), "ori_maps")
    _f32(scales, (n, H, W), "scales")
    if kpts_xy.dtype != torch.int32 or tuple(kpts_xy.shape) != (n, int(p.top_k), 2) or n_kpts.dtype != torch.int32 or n_kpts.numel() != n:
        raise ValueError(f"lfnet_crops: kpts_xy must be int32 [{n}, {p.top_k}, 2] and n_kpts int32 [{n}]")
    kp, ksc, kor, patches = _crop_outputs(n, p, heat.device)
    check(lib().btba_lfnet_crops(ws.handle, C.byref(p), n, H, W, _dev_ptr(photo, "photo"), _dev_ptr(ori_maps, "ori_maps"), _dev_ptr(heat, "heat"),
                                 _dev_ptr(scales, "scales"), _dev_ptr(kpts_xy, "kpts_xy"), _dev_ptr(n_kpts, "n_kpts"), kp.data_ptr(),
                                 ksc.data_ptr(), kor.data_ptr(), patches.data_ptr()), "btba_lfnet_crops")
    return kp, ksc, kor, patches


def lfnet_keypoints(ws, score_maps, scale_factors, photo, ori_maps, params=None, wait: bool = True):
    """btba_lfnet_keypoints: stages A, B and C in one call.  photo: float32 CUDA [n, H, W] (or [n, 1, H, W]).  Returns a dict with
    max_heatmaps, max_scales, kpts_xy, n_kpts (device), kpts, kpts_scale, kpts_ori, patches and, with wait, n_kpts_host (numpy int32 [n];
    the call's one host wait)."""
    import torch
    from .optimizer import _dev_ptr
    p = _params(params)
    if photo.dtype != torch.float32 or photo.dim() not in (3, 4) or (photo.dim() == 4 and photo.shape[1] != 1):
        raise ValueError("lfnet_keypoints: photo must be float32 [n, H, W] or [n, 1, H, W]")
    n, H, W = int(photo.shape[0]), int(photo.shape[-2]), int(photo.shape[-1])
    _f32(ori_maps, (n, H, W, 2), "ori_maps")
    S, table, mh, mw, sf = _maps(score_maps, scale_factors, n)
    dev = photo.device
    heat = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    scales = torch.empty_like(heat)
    kxy = torch.empty((n, max(int(p.top_k), 1), 2), dtype=torch.int32, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    kp, ksc, kor, patches = _crop_outputs(n, p, dev)
    host = np.zeros(n, np.int32) if wait else None
    check(lib().btba_lfnet_keypoints(ws.handle, C.byref(p), n, H, W, S, C.cast(table, C.c_void_p), mh.ctypes.data, mw.ctypes.data, sf.ctypes.data,
                                     _dev_ptr(photo, "photo"), _dev_ptr(ori_maps, "ori_maps"), heat.data_ptr(), scales.data_ptr(), kxy.data_ptr(),
                                     cnt.data_ptr(), kp.data_ptr(), ksc.data_ptr(), kor.data_ptr(), patches.data_ptr(),
                                     host.ctypes.data if wait else None), "btba_lfnet_keypoints")
    return dict(max_heatmaps=heat, max_scales=scales, kpts_xy=kxy, n_kpts=cnt, kpts=kp, kpts_scale=ksc, kpts_ori=kor, patches=patches,
                n_kpts_host=host)


class LfnetDetector:
    """The detector Bundler(detector=...) takes, (bgr, gray) -> (kpts [m, 2], desc [m, D]), around the caller's two conv nets:
      score_net(gray [n, 1, H, W]) -> (list of S score maps [n, h_s, w_s] or [n, 1, h_s, w_s], ori_maps [n, H, W, 2])
      desc_net(patches [m, 1, P, P]) -> desc [m, D]
    with lfnet_keypoints in between.  Keypoints are in the grey image's pixels."""

    def __init__(self, ws, score_net, desc_net, scale_factors, params=None):
        self.ws, self.score_net, self.desc_net = ws, score_net, desc_net
        self.scale_factors = [float(s) for s in scale_factors]
        self.params = _params(params)
        self.last = None                                   # the last call's lfnet_keypoints result

    @classmethod
    def from_models(cls, ws, score_net, desc_net, params=None):
        """The detector around the two device nets: score_net an lfnet_det.LfnetScoreNet, whose scale_factors and pad_size the
        keypoint head takes (pad_size overrides the one in `params`), desc_net an lfnet_desc.LfnetDescriptor (or any desc_net)."""
        import copy
        p = copy.copy(_params(params))
        p.pad_size = int(score_net.pad_size)
        return cls(ws, score_net, desc_net, score_net.scale_factors, p)

    def __call__(self, bgr, gray):
        import torch
        with torch.no_grad():
            score_maps, ori_maps = self.score_net(gray)
            score_maps = [m.float().contiguous() for m in score_maps]
            r = lfnet_keypoints(self.ws, score_maps, self.scale_factors, gray.float().contiguous(), ori_maps.float().contiguous(), self.params)
            m = int(r["n_kpts_host"][0])
            P = int(self.params.patch_size)
            desc = self.desc_net(r["patches"][0, :m].reshape(m, 1, P, P))
        self.last = r
        return r["kpts"][0, :m].contiguous(), desc.float().contiguous()
