"""LF-Net's detector net on the MI355X (btba_lfnet_det_*, btba_lfnet_scores): grey photos -> score maps and orientation map.

Mirrors lf-net-release/models/mso_resnet_detector.py::get_model in inference: init_conv, residual blocks of two k x k convolutions
with batch norm and activation before each, fin-bn, per scale TF1's resize and a score convolution, the orientation convolution
and l2_normalize.  LfnetScoreNet is what LfnetDetector(score_net=...) takes; with it and LfnetDescriptor photo -> keypoints ->
descriptors stay on the workspace stream (LfnetDetector.from_models).  The exact rules are in include/btba.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lfnet_model import BN_FIELDS, NpzModel, WeightMarshal, resolve_config
from ._lib import LfnetDetWeights, check, lfnet_det_config, lib

MAX_BLOCKS, MAX_SCALES = 8, 16             # BTBA_LFNET_DET_MAX_BLOCKS, BTBA_LFNET_MAX_SCALES
SCOPE = "ConvOnlyResNet"


def detector_scales(min_scale: float, max_scale: float, num_scales: int) -> np.ndarray:
    """btba_lfnet_det_scales: np.exp(np.linspace(log(max_scale), log(min_scale), num_scales)) in double, [1.0] for one scale."""
    out = np.zeros(max(int(num_scales), 1), np.float64)
    check(lib().btba_lfnet_det_scales(float(min_scale), float(max_scale), int(num_scales), out.ctypes.data), "btba_lfnet_det_scales")
    return out


def expected_names(blocks: int, num_scales: int, perform_bn: bool = True, use_bias: bool = True, scope: str = SCOPE):
    """The variables of a checkpoint of get_model(num_block=blocks, num_scales=..., perform_bn=..., use_bias=...).  ori_conv always
    has its biases (conv2d_custom)."""
    names = []

    def conv(name, bias=use_bias):
        names.append(f"{scope}/{name}/weights")
        if bias:
            names.append(f"{scope}/{name}/biases")

    def bn(name):
        if perform_bn:
            names.extend(f"{scope}/{name}/{k}" for k in BN_FIELDS)

    conv("init_conv")
    for i in range(1, blocks + 1):
        bn(f"block-{i}/pre-bn")
        conv(f"block-{i}/conv1")
        bn(f"block-{i}/mid-bn")
        conv(f"block-{i}/conv2")
    bn("fin-bn")
    for j in range(num_scales):
        conv(f"score_conv_{j}")
    conv("ori_conv", True)
    return names


def config_from_weights(weights, scope: str = SCOPE, **over):
    """The shape fields of the configuration read off the arrays (channels and ksize from init_conv, blocks and num_scales from the
    names); scale_factors, activation, leaky_alpha and bn_eps from `over`.  Without scale_factors: the release's range sqrt(2) ..
    1 / sqrt(2) over the stored number of scales."""
    blocks = 0
    while f"{scope}/block-{blocks + 1}/conv1/weights" in weights:
        blocks += 1
    scales = 0
    while f"{scope}/score_conv_{scales}/weights" in weights:
        scales += 1
    if f"{scope}/init_conv/weights" not in weights:
        raise KeyError(f"detector weights: missing {scope}/init_conv/weights; expected {expected_names(max(blocks, 1), max(scales, 1), scope=scope)}")
    w = np.shape(weights[f"{scope}/init_conv/weights"])
    if len(w) != 4 or w[0] != w[1] or w[2] != 1:
        raise ValueError(f"detector weights: init_conv {w}: expected [k, k, 1, C]")
    cfg = dict(channels=int(w[3]), ksize=int(w[0]), blocks=blocks)
    if "scale_factors" not in over:
        over = dict(over, scale_factors=detector_scales(2.0 ** -0.5, 2.0 ** 0.5, scales))
    cfg.update(over)
    return lfnet_det_config(**cfg)


class LfnetScoreNet(NpzModel):
    """A detector model on a workspace.  weights: a mapping from the checkpoint's variable names (ConvOnlyResNet/init_conv/weights,
    ConvOnlyResNet/block-1/pre-bn/gamma, .../conv1/weights, .../mid-bn/moving_mean, ConvOnlyResNet/fin-bn/..., .../score_conv_0/weights,
    .../ori_conv/biases, ...) to arrays in TensorFlow's layouts.  A convolution's `weights` must be there; absent biases mean none,
    absent moving_* no batch norm at that place, absent gamma 1 and beta 0.
    config: None (the release net), a dict of btba_lfnet_det_config fields or an LfnetDetConfig.

    Callable as score_net: gray [n, 1, H, W] -> (list of S maps [n, h_j, w_j], ori [n, H, W, 2])."""

    _destroy = "btba_lfnet_det_model_destroy"
    _default_config, _expected_names, _config_from_weights = staticmethod(lfnet_det_config), staticmethod(expected_names), staticmethod(config_from_weights)

    def __init__(self, ws, weights, config=None, scope: str = SCOPE):
        self.ws, self.config = ws, resolve_config(lfnet_det_config, config)
        cfg = self.config
        Cn, k, blocks, S = int(cfg.channels), int(cfg.ksize), int(cfg.blocks), int(cfg.num_scales)
        if not 1 <= blocks <= MAX_BLOCKS or not 1 <= S <= MAX_SCALES:
            raise ValueError(f"blocks {blocks} outside 1 .. {MAX_BLOCKS} or num_scales {S} outside 1 .. {MAX_SCALES}")
        W = LfnetDetWeights()
        m = WeightMarshal(weights, scope, "detector", expected_names(blocks, S, scope=scope))
        m.conv(W.init_conv, "init_conv", (k, k, 1, Cn))
        for i in range(blocks):
            b = W.block[i]
            m.bn(b.pre_bn, f"block-{i + 1}/pre-bn", Cn)
            m.conv(b.conv1, f"block-{i + 1}/conv1", (k, k, Cn, Cn))
            m.bn(b.conv1, f"block-{i + 1}/mid-bn", Cn)
            m.conv(b.conv2, f"block-{i + 1}/conv2", (k, k, Cn, Cn))
        m.bn(W.fin_bn, "fin-bn", Cn)
        for j in range(S):
            m.conv(W.score_conv[j], f"score_conv_{j}", (k, k, Cn, 1))
        m.conv(W.ori_conv, "ori_conv", (k, k, Cn, 2))
        h = C.c_void_p()
        check(lib().btba_lfnet_det_model_create(ws.handle, C.byref(cfg), C.byref(W), C.byref(h)), "btba_lfnet_det_model_create")
        self._h = h

    @staticmethod
    def _counts(cfg, have, scope, over):
        if cfg is not None:
            return int(cfg.blocks), int(cfg.num_scales)
        blocks = max(sum(f"{scope}/block-{i + 1}/conv1/weights" in have for i in range(MAX_BLOCKS)), 1)
        if "scale_factors" in over:
            return blocks, len(over["scale_factors"])
        return blocks, max(sum(f"{scope}/score_conv_{j}/weights" in have for j in range(MAX_SCALES)), 1)

    @classmethod
    def from_npz(cls, ws, path, config=None, perform_bn: bool = True, use_bias: bool = True, scope: str = SCOPE, **over):
        """A model from an .npz whose arrays are named as the checkpoint names its variables (INTEGRATION.md has the TF1 export).
        Every variable of get_model(perform_bn=..., use_bias=...) must be there: a missing one is an error that lists them all.
        Without `config` the shape fields come from the arrays; `over` sets scale_factors, activation, leaky_alpha, bn_eps."""
        return cls._from_npz(ws, path, config, perform_bn, use_bias, scope, over)

    @property
    def scale_factors(self):
        return [float(self.config.scale_factors[j]) for j in range(int(self.config.num_scales))]

    @property
    def pad_size(self) -> int:
        return int(lib().btba_lfnet_det_pad_size(self._h))

    def map_sizes(self, H: int, W: int):
        """btba_lfnet_det_map_sizes: (map_h, map_w), int32 [S] each."""
        S = int(self.config.num_scales)
        mh, mw = np.zeros(S, np.int32), np.zeros(S, np.int32)
        check(lib().btba_lfnet_det_map_sizes(self._h, int(H), int(W), mh.ctypes.data, mw.ctypes.data), "btba_lfnet_det_map_sizes")
        return mh, mw

    def scores(self, photo):
        """photo: float32 CUDA [n, H, W] or [n, 1, H, W].  Returns (list of S score maps float32 [n, h_j, w_j], ori float32
        [n, H, W, 2]).  Asynchronous on the workspace stream."""
        return lfnet_scores(self.ws, self, photo)

    def __call__(self, gray):
        return lfnet_scores(self.ws, self, gray)


def lfnet_scores(ws, model: LfnetScoreNet, photo):
    """btba_lfnet_scores.  photo: float32 CUDA [n, H, W] or [n, 1, H, W] -> (score maps [n, h_j, w_j] per scale, ori [n, H, W, 2])."""
    import torch
    from .optimizer import _dev_ptr
    if photo.dtype != torch.float32 or photo.dim() not in (3, 4) or (photo.dim() == 4 and photo.shape[1] != 1):
        raise ValueError(f"lfnet_scores: photo must be float32 [n, H, W] or [n, 1, H, W], got {photo.dtype} {tuple(photo.shape)}")
    n, H, W = int(photo.shape[0]), int(photo.shape[-2]), int(photo.shape[-1])
    mh, mw = model.map_sizes(H, W)
    maps = [torch.empty((n, int(h), int(w)), dtype=torch.float32, device=photo.device) for h, w in zip(mh, mw)]
    ori = torch.empty((n, H, W, 2), dtype=torch.float32, device=photo.device)
    table = (C.c_void_p * len(maps))(*[m.data_ptr() if n else None for m in maps])
    check(lib().btba_lfnet_scores(ws.handle, model.handle, n, H, W, _dev_ptr(photo, "photo") if n else None, C.cast(table, C.c_void_p),
                                  ori.data_ptr() if n else None), "btba_lfnet_scores")
    return maps, ori
