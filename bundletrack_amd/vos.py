"""Mask propagation on the MI355X (btba_vos_*): where a tracked frame's object mask comes from.

Mirrors transductive-vos.pytorch/run_video.py around its backbone: rgb_normalize, prepare_first_frame, lib/predict.py::predict with
sample_frames and the Gaussian motion model, the one-hot history entry and the upsampled arg-max mask.  The reference forms an
[n_ref * HW, HW] similarity matrix and two [HW, HW] weight tables per video; here predict is one fused pass with an online softmax
(btba_vos.hpp) and neither exists.  The backbone is a callable from normalize_inputs' output to features [C, Hd, Wd]: the caller's
torch model, or btba_vos_features (vos_net.VosBackbone).  The exact rules are in include/btba.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib, vos_params

MAX_REF, MAX_CLASSES = 32, 16          # BTBA_VOS_MAX_REF, BTBA_VOS_MAX_CLASSES


def grid_of(H: int, W: int):
    """(Hd, Wd) = (ceil(H / 8), ceil(W / 8)): the backbone's stride."""
    return (int(H) + 7) // 8, (int(W) + 7) // 8


def _params(params):
    return vos_params() if params is None else (vos_params(**params) if isinstance(params, dict) else params)


def sample_frames(frame_idx: int, params=None):
    """btba_vos_sample_frames: (history indices predict reads for target `frame_idx`, how many of the last take sigma_dense).
    Needs no GPU."""
    p = _params(params)
    idx = np.zeros(max(int(p.ref_num), 1), np.int32)
    n, n_dense = C.c_int32(), C.c_int32()
    check(lib().btba_vos_sample_frames(C.byref(p), int(frame_idx), idx.ctypes.data, C.byref(n), C.byref(n_dense)), "btba_vos_sample_frames")
    return idx[:n.value].tolist(), int(n_dense.value)


def _table(tensors, what):
    from .optimizer import _dev_ptr
    arr = (C.c_void_p * len(tensors))()
    for k, t in enumerate(tensors):
        arr[k] = _dev_ptr(t, f"{what} {k}") if t is not None else None
    return arr


def first_labels(ws, label_image, d: int, out=None):
    """btba_vos_first_labels: uint8 [H, W] CUDA label image with classes 0 .. d-1 -> float32 [d, Hd, Wd], its one-hot taken down
    bilinearly (prepare_first_frame).  Asynchronous on the workspace stream."""
    import torch
    from .optimizer import _dev_ptr
    if label_image.dtype != torch.uint8 or label_image.dim() != 2:
        raise ValueError("first_labels: the label image must be uint8 [H, W]")
    H, W = (int(s) for s in label_image.shape)
    Hd, Wd = grid_of(H, W)
    if out is None:
        out = torch.empty((int(d), Hd, Wd), dtype=torch.float32, device=label_image.device)
    elif out.numel() != int(d) * Hd * Wd or out.dtype != torch.float32:
        raise ValueError(f"first_labels: out must be float32 with {d} x {Hd} x {Wd} elements")
    check(lib().btba_vos_first_labels(ws.handle, H, W, int(d), _dev_ptr(label_image, "label image"), _dev_ptr(out, "labels out")), "btba_vos_first_labels")
    return out


def propagate(ws, refs, labels, targets, n_dense, Hd: int, Wd: int, params=None, pred_out=None, onehot_out=None, want_onehot=True):
    """btba_vos_propagate.  refs[b] / labels[b]: the b-th video's reference features (float32 [C, Hd*Wd] each, any shape with those
    elements) and labels (float32 [d, Hd*Wd] each), oldest first; targets[b]: float32 [C, Hd*Wd]; n_dense[b]: how many of the last
    references take sigma_dense.  Returns (pred, onehot): lists of float32 [d, Hd, Wd] per video (onehot None without want_onehot /
    onehot_out).  pred_out / onehot_out: lists of tensors to write into.  Asynchronous on the workspace stream."""
    import torch
    n = len(targets)
    if n == 0:
        return [], []
    if not (len(refs) == len(labels) == len(n_dense) == n) or any(len(r) != len(l) or len(r) == 0 for r, l in zip(refs, labels)):
        raise ValueError("propagate: one non-empty list of references and as many labels per target")
    HW = int(Hd) * int(Wd)
    Cn, d = targets[0].numel() // HW, labels[0][0].numel() // HW
    for b in range(n):
        if targets[b].numel() != Cn * HW or targets[b].dtype != torch.float32:
            raise ValueError(f"propagate: target {b} must be float32 with {Cn} x {HW} elements")
        for r, l in zip(refs[b], labels[b]):
            if r.numel() != Cn * HW or l.numel() != d * HW or r.dtype != torch.float32 or l.dtype != torch.float32:
                raise ValueError(f"propagate: video {b}: references must be float32 [{Cn}, {HW}], labels float32 [{d}, {HW}]")
    dev = targets[0].device
    if pred_out is None:
        pred_out = [torch.empty((d, int(Hd), int(Wd)), dtype=torch.float32, device=dev) for _ in range(n)]
    if onehot_out is None and want_onehot:
        onehot_out = [torch.empty((d, int(Hd), int(Wd)), dtype=torch.float32, device=dev) for _ in range(n)]
    for t in list(pred_out) + list(onehot_out or []):
        if t is not None and (t.numel() != d * HW or t.dtype != torch.float32):
            raise ValueError(f"propagate: outputs must be float32 with {d} x {HW} elements")
    nr = np.array([len(r) for r in refs], np.int32)
    nd = np.array([int(v) for v in n_dense], np.int32)
    check(lib().btba_vos_propagate(ws.handle, C.byref(_params(params)), n, Cn, d, int(Hd), int(Wd), nr.ctypes.data, nd.ctypes.data,
                                   _table([r for rs in refs for r in rs], "reference"), _table([l for ls in labels for l in ls], "label"),
                                   _table(targets, "target"), _table(pred_out, "pred"),
                                   _table(onehot_out, "onehot") if onehot_out is not None else None), "btba_vos_propagate")
    return pred_out, onehot_out


def masks(ws, pred, H: int, W: int, out=None):
    """btba_vos_masks: pred float32 [d, Hd, Wd] -> uint8 [H, W] class map (bilinear to H x W, arg-max; nonzero = foreground, what
    segmentation.apply_masks takes).  Asynchronous on the workspace stream."""
    import torch
    from .optimizer import _dev_ptr
    if pred.dim() != 3 or pred.dtype != torch.float32:
        raise ValueError("masks: pred must be float32 [d, Hd, Wd]")
    d, Hd, Wd = (int(s) for s in pred.shape)
    if out is None:
        out = torch.empty((int(H), int(W)), dtype=torch.uint8, device=pred.device)
    elif out.numel() != int(H) * int(W) or out.dtype != torch.uint8:
        raise ValueError(f"masks: out must be uint8 {H} x {W}")
    check(lib().btba_vos_masks(ws.handle, d, Hd, Wd, int(H), int(W), _dev_ptr(pred, "pred"), _dev_ptr(out, "mask out")), "btba_vos_masks")
    return out


def normalize_inputs(ws, bgr):
    """btba_vos_inputs: a list of uint8 [H, W, 3] CUDA BGR images (imread's layout) -> float32 [n, 3, H, W], RGB planes,
    (v / 255 - mean) / std with the ImageNet constants: the backbone's input (rgb_normalize).  Asynchronous on the workspace stream."""
    import torch
    from .optimizer import _dev_ptr
    if len(bgr) == 0:
        raise ValueError("normalize_inputs: no frames")
    H, W = (int(s) for s in bgr[0].shape[:2])
    for k, b in enumerate(bgr):
        if b.dtype != torch.uint8 or b.numel() != 3 * H * W:
            raise ValueError(f"normalize_inputs: frame {k} must be uint8 {H} x {W} x 3")
    out = torch.empty((len(bgr), 3, H, W), dtype=torch.float32, device=bgr[0].device)
    check(lib().btba_vos_inputs(ws.handle, len(bgr), H, W, _table(bgr, "bgr"), _dev_ptr(out, "rgb out")), "btba_vos_inputs")
    return out


class MaskPropagator:
    """One video's propagation state: run_video.py's feats_history / label_history as a device ring of `range + 5` slots (no frame
    older than frame_idx - range - 4 is ever sampled; the reference keeps every frame).  start(label_image, features) takes the
    annotated first frame, step(features) returns the next frame's uint8 [H, W] class map and appends the frame to the history.
    A label image whose values are not 0 .. d-1 (a 0 / 255 mask) is compacted to consecutive classes first: the reference would
    carry 254 empty classes whose rows are exactly zero and never win the arg-max."""

    def __init__(self, ws, d: int, H: int, W: int, C: int = 256, params=None):
        self.ws, self.d, self.H, self.W, self.C = ws, int(d), int(H), int(W), int(C)
        self.Hd, self.Wd = grid_of(H, W)
        self.params = _params(params)
        self.slots = int(self.params.range) + 5
        self.n_frames = 0                       # frames in the history = the next frame_idx
        self.values = None                      # the label image's original values, by class
        self._feats = self._labels = self._pred = None
        self.last_pred = None

    def _alloc(self, device):
        import torch
        HW = self.Hd * self.Wd
        self._feats = torch.empty((self.slots, self.C, HW), dtype=torch.float32, device=device)
        self._labels = torch.empty((self.slots, self.d, HW), dtype=torch.float32, device=device)
        self._pred = torch.empty((self.d, self.Hd, self.Wd), dtype=torch.float32, device=device)

    def _store(self, features, slot):
        import torch
        f = features.to(dtype=torch.float32)
        if f.numel() != self._feats[slot].numel():
            raise ValueError(f"MaskPropagator: features must have {self.C} x {self.Hd} x {self.Wd} elements, got {tuple(features.shape)}")
        self._feats[slot].copy_(f.reshape(self.C, -1))

    def start(self, label_image, features) -> None:
        """The annotated frame 0: label_image uint8 [H, W] (CUDA tensor or array), features [C, Hd, Wd] of that frame."""
        import torch
        if not torch.is_tensor(label_image):
            label_image = torch.from_numpy(np.ascontiguousarray(label_image, np.uint8)).to(features.device)
        if tuple(label_image.shape) != (self.H, self.W) or label_image.dtype != torch.uint8:
            raise ValueError(f"MaskPropagator.start: the label image must be uint8 {self.H} x {self.W}")
        vals = torch.unique(label_image).tolist()
        if vals[0] != 0:
            vals = [0] + vals                   # value 0 stays class 0, present or not
        if len(vals) > self.d:
            raise ValueError(f"MaskPropagator.start: {len(vals)} label values for d = {self.d}")
        if vals[-1] >= len(vals):               # not 0 .. n-1: compact
            lut = torch.zeros(256, dtype=torch.uint8, device=label_image.device)
            lut[torch.tensor(vals, dtype=torch.long, device=label_image.device)] = torch.arange(len(vals), dtype=torch.uint8, device=label_image.device)
            label_image = lut[label_image.long()]
        self.values = vals
        self._alloc(label_image.device)
        self._store(features, 0)
        first_labels(self.ws, label_image.contiguous(), self.d, out=self._labels[0])
        self.n_frames = 1

    def step(self, features):
        """The next frame: predict against the sampled history, the frame's one-hot labels and features into the ring, and the
        uint8 [H, W] class map (0 = background).  The prediction itself stays in last_pred ([d, Hd, Wd]) until the next step."""
        if self.n_frames < 1:
            raise RuntimeError("MaskPropagator.step before start")
        f = self.n_frames
        idx, n_dense = sample_frames(f, self.params)
        slot = f % self.slots
        self._store(features, slot)
        refs = [self._feats[i % self.slots] for i in idx]
        labs = [self._labels[i % self.slots] for i in idx]
        propagate(self.ws, [refs], [labs], [self._feats[slot]], [n_dense], self.Hd, self.Wd, self.params, pred_out=[self._pred],
                  onehot_out=[self._labels[slot]])
        self.n_frames = f + 1
        self.last_pred = self._pred
        return masks(self.ws, self._pred, self.H, self.W)

    def history(self, frame: int):
        """(features [C, HW], labels [d, HW]) of a frame still in the ring."""
        if not (0 <= frame < self.n_frames and frame > self.n_frames - 1 - self.slots):
            raise IndexError(frame)
        return self._feats[frame % self.slots], self._labels[frame % self.slots]
