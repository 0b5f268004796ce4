"""LF-Net's descriptor net on the MI355X (btba_lfnet_desc_*, btba_lfnet_descriptors): patches -> descriptors.

Mirrors lf-net-release/models/simple_desc.py::get_model in inference: stride-2 3 x 3 convolutions with batch norm and activation,
flatten, two fully connected layers, l2_normalize.  LfnetDescriptor is what LfnetDetector(desc_net=...) takes; with it crops ->
descriptors -> matches stay on the workspace stream.  The exact rules are in include/btba.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lfnet_model import BN_FIELDS, NpzModel, WeightMarshal, resolve_config
from ._lib import LfnetDescWeights, check, lfnet_desc_config, lib

MAX_DEPTH, MAX_SLOTS = 4, 2048             # BTBA_LFNET_DESC_MAX_DEPTH, BTBA_LFNET_MAX_TOP_K
SCOPE = "SimpleDesc"


def layer_scopes(depth: int):
    """(layer scope, batch-norm scope or None) of every layer in order, as get_model names them."""
    return [(f"conv{i + 1}", f"bn{i + 1}") for i in range(depth)] + [("fc1", "fc-bn1"), ("fc2", None)]


def expected_names(depth: int, perform_bn: bool = True, use_bias: bool = True, scope: str = SCOPE):
    """The variables of a checkpoint of get_model(num_conv_layers=depth, perform_bn=..., use_bias=...)."""
    names = []
    for layer, bn in layer_scopes(depth):
        names.append(f"{scope}/{layer}/weights")
        if use_bias:
            names.append(f"{scope}/{layer}/biases")
        if bn and perform_bn:
            names += [f"{scope}/{bn}/{k}" for k in BN_FIELDS]
    return names


def config_from_weights(weights, scope: str = SCOPE, **over):
    """The shape fields of the configuration read off the arrays' shapes; activation, leaky_alpha, norm and bn_eps from `over`."""
    depth = 0
    while f"{scope}/conv{depth + 1}/weights" in weights:
        depth += 1
    need = [f"{scope}/conv1/weights", f"{scope}/fc1/weights", f"{scope}/fc2/weights"]
    if any(n not in weights for n in need):
        raise KeyError(f"descriptor weights: missing {[n for n in need if n not in weights]}; expected {expected_names(max(depth, 1), scope=scope)}")
    c1 = np.shape(weights[f"{scope}/conv1/weights"])
    fc1, fc2 = np.shape(weights[f"{scope}/fc1/weights"]), np.shape(weights[f"{scope}/fc2/weights"])
    if len(c1) != 4 or len(fc1) != 2 or len(fc2) != 2:
        raise ValueError(f"descriptor weights: conv1 {c1}, fc1 {fc1}, fc2 {fc2}: expected [3, 3, 1, C], [in, fc] and [fc, out]")
    channels = int(c1[3])
    last = channels << (depth - 1)
    side = int(round((fc1[0] / last) ** 0.5))
    cfg = dict(patch_size=side << depth, depth=depth, channels=channels, fc_dim=int(fc1[1]), out_dim=int(fc2[1]))
    cfg.update(over)
    return lfnet_desc_config(**cfg)


class LfnetDescriptor(NpzModel):
    """A descriptor model on a workspace.  weights: a mapping from the checkpoint's variable names (SimpleDesc/conv1/weights,
    SimpleDesc/conv1/biases, SimpleDesc/bn1/gamma, .../beta, .../moving_mean, .../moving_variance, SimpleDesc/fc1/weights,
    SimpleDesc/fc-bn1/..., SimpleDesc/fc2/weights, SimpleDesc/fc2/biases) to arrays in TensorFlow's layouts.  A layer's `weights`
    must be there; absent biases mean none, absent moving_* no batch norm on that layer, absent gamma 1 and beta 0.
    config: None (the release net), a dict of btba_lfnet_desc_config fields or an LfnetDescConfig.

    Callable as desc_net: (patches [m, 1, P, P] or [m, P, P]) -> [m, D]."""

    _destroy = "btba_lfnet_desc_model_destroy"
    _default_config, _expected_names, _config_from_weights = staticmethod(lfnet_desc_config), staticmethod(expected_names), staticmethod(config_from_weights)

    def __init__(self, ws, weights, config=None, scope: str = SCOPE):
        self.ws, self.config = ws, resolve_config(lfnet_desc_config, config)
        cfg = self.config
        depth = int(cfg.depth)
        if not 1 <= depth <= MAX_DEPTH:
            raise ValueError(f"depth {depth} outside 1 .. {MAX_DEPTH}")
        W = LfnetDescWeights()
        m = WeightMarshal(weights, scope, "descriptor", expected_names(depth, scope=scope))

        def fill(layer, name, bn, wshape):
            m.conv(layer, name, wshape)
            if bn:
                m.bn(layer, bn, wshape[-1])

        c_in = 1
        for i, (name, bn) in enumerate(layer_scopes(depth)[:depth]):
            c_out = int(cfg.channels) << i
            fill(W.conv[i], name, bn, (3, 3, c_in, c_out))
            c_in = c_out
        side = int(cfg.patch_size) >> depth
        fill(W.fc1, "fc1", "fc-bn1", (side * side * c_in, int(cfg.fc_dim)))
        fill(W.fc2, "fc2", None, (int(cfg.fc_dim), int(cfg.out_dim)))
        h = C.c_void_p()
        check(lib().btba_lfnet_desc_model_create(ws.handle, C.byref(cfg), C.byref(W), C.byref(h)), "btba_lfnet_desc_model_create")
        self._h = h

    @staticmethod
    def _counts(cfg, have, scope, over):
        return (int(cfg.depth) if cfg is not None else max(sum(f"{scope}/conv{i + 1}/weights" in have for i in range(MAX_DEPTH)), 1),)

    @classmethod
    def from_npz(cls, ws, path, config=None, perform_bn: bool = True, use_bias: bool = True, scope: str = SCOPE, **over):
        """A model from an .npz whose arrays are named as the checkpoint names its variables (INTEGRATION.md has the TF1 export).
        Every variable of get_model(perform_bn=..., use_bias=...) must be there: a missing one is an error that lists them all.
        Without `config` the shape fields come from the arrays; `over` sets activation, leaky_alpha, norm, bn_eps."""
        return cls._from_npz(ws, path, config, perform_bn, use_bias, scope, over)

    def describe(self, patches, n_kpts=None):
        """patches: float32 CUDA [n, K, P, P]; n_kpts: int32 CUDA [n] or None (all slots).  Returns desc float32 [n, K, D]; slots
        past a frame's count are zero.  Asynchronous on the workspace stream."""
        return lfnet_descriptors(self.ws, self, patches, n_kpts)

    def __call__(self, patches):
        P = int(self.config.patch_size)
        m = int(patches.shape[0])
        if m > MAX_SLOTS:                                   # rows are independent: the pieces give the same bits
            import torch
            return torch.cat([self(patches[i:i + MAX_SLOTS]) for i in range(0, m, MAX_SLOTS)])
        return lfnet_descriptors(self.ws, self, patches.reshape(1, m, P, P), None)[0]


def lfnet_descriptors(ws, model: LfnetDescriptor, patches, n_kpts=None):
    """btba_lfnet_descriptors.  patches: float32 CUDA [n, K, P, P] -> desc float32 [n, K, D]."""
    import torch
    from .optimizer import _dev_ptr
    P, D = int(model.config.patch_size), int(model.config.out_dim)
    if patches.dtype != torch.float32 or patches.dim() != 4 or tuple(patches.shape[2:]) != (P, P):
        raise ValueError(f"lfnet_descriptors: patches must be float32 [n, K, {P}, {P}], got {patches.dtype} {tuple(patches.shape)}")
    n, K = int(patches.shape[0]), int(patches.shape[1])
    if n_kpts is not None and (n_kpts.dtype != torch.int32 or n_kpts.numel() != n):
        raise ValueError(f"lfnet_descriptors: n_kpts must be int32 [{n}]")
    desc = torch.empty((n, K, D), dtype=torch.float32, device=patches.device)
    check(lib().btba_lfnet_descriptors(ws.handle, model.handle, n, K, _dev_ptr(patches, "patches"), _dev_ptr(n_kpts, "n_kpts"), desc.data_ptr()),
          "btba_lfnet_descriptors")
    return desc
