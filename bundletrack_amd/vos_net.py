"""The video segmentation's backbone on the MI355X (btba_vos_net_*, btba_vos_features): normalised RGB frames -> features.

Mirrors transductive-vos.pytorch/modeling/network.py::VOSNet on modeling/backbone/resnet.py in eval mode: the 7 x 7 stem and max
pool, layer1 .. layer4 of BasicBlock or Bottleneck (layer4 at 256 planes and stride 1), and for the bottleneck nets adjust_dim and
bn256.  VosBackbone is what Bundler(segmenter=...) takes; with vos.normalize_inputs before it and vos.MaskPropagator behind it frame ->
mask stays on the workspace stream.  The exact rules are in include/btba.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lfnet_model import Handle
from ._lib import VosNetConfig, VosNetLayer, check, lib, vos_net_config

BASIC, BOTTLENECK = 0, 1                   # BTBA_VOS_NET_BASIC, BTBA_VOS_NET_BOTTLENECK
MAX_BLOCKS = 64                            # BTBA_VOS_NET_MAX_BLOCKS
PLANES, STRIDES, STEM_C, OUT_C = (64, 128, 256, 256), (1, 2, 1, 1), 64, 256
BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def resolve_config(config) -> VosNetConfig:
    """None: resnet50; a dict: its fields (block, layers, bn_eps) over the defaults; a VosNetConfig: as it is."""
    return vos_net_config() if config is None else (vos_net_config(**config) if isinstance(config, dict) else config)


def layer_table(config=None):
    """The net's convolutions in the forward order of include/btba.h: a list of (convolution's name, its batch norm's name, C_out,
    C_in, k) under the checkpoint's names, e.g. ("backbone.4.0.conv1", "backbone.4.0.bn1", 64, 64, 1)."""
    cfg = resolve_config(config)
    bott = int(cfg.block) == BOTTLENECK
    expansion = 4 if bott else 1
    out = [("backbone.0", "backbone.1", STEM_C, 3, 7)]
    inplanes = STEM_C
    for s in range(4):
        planes, out_c = PLANES[s], PLANES[s] * expansion
        for b in range(int(cfg.layers[s])):
            stride = STRIDES[s] if b == 0 else 1
            p = f"backbone.{4 + s}.{b}"
            if bott:
                out += [(f"{p}.conv1", f"{p}.bn1", planes, inplanes, 1), (f"{p}.conv2", f"{p}.bn2", planes, planes, 3),
                        (f"{p}.conv3", f"{p}.bn3", out_c, planes, 1)]
            else:
                out += [(f"{p}.conv1", f"{p}.bn1", planes, inplanes, 3), (f"{p}.conv2", f"{p}.bn2", planes, planes, 3)]
            if b == 0 and (stride != 1 or inplanes != out_c):
                out.append((f"{p}.downsample.0", f"{p}.downsample.1", out_c, inplanes, 1))
            inplanes = out_c
    if bott:
        out.append(("adjust_dim", "bn256", OUT_C, inplanes, 1))
    return out


def expected_names(config=None):
    """The arrays a model needs, under the names VOSNet.state_dict() gives them, in forward order (num_batches_tracked is not one)."""
    names = []
    for conv, bn, _, _, _ in layer_table(config):
        names.append(f"{conv}.weight")
        names.extend(f"{bn}.{k}" for k in BN_KEYS)
    return names


def _plain(state_dict):
    """The state_dict without DataParallel's leading `module.` and without num_batches_tracked."""
    out = {}
    for k, v in state_dict.items():
        k = k[len("module."):] if k.startswith("module.") else k
        if not k.endswith("num_batches_tracked"):
            out[k] = v
    return out


def config_from_state_dict(state_dict, **over) -> VosNetConfig:
    """Block kind and depths read off the names: Bottleneck where backbone.4.0.conv3.weight exists, layers[s] = the blocks of
    backbone.{4 + s} that have a conv1.  `over` sets bn_eps."""
    sd = _plain(state_dict)
    block = BOTTLENECK if "backbone.4.0.conv3.weight" in sd else BASIC
    layers = []
    for s in range(4):
        n = 0
        while f"backbone.{4 + s}.{n}.conv1.weight" in sd:
            n += 1
        layers.append(max(n, 1))
    return vos_net_config(block=block, layers=layers, **over)


def out_size(H: int, W: int):
    """btba_vos_net_out_size: (Hd, Wd) = (ceil(H / 8), ceil(W / 8))."""
    hd, wd = C.c_int32(), C.c_int32()
    check(lib().btba_vos_net_out_size(int(H), int(W), C.byref(hd), C.byref(wd)), "btba_vos_net_out_size")
    return int(hd.value), int(wd.value)


class VosBackbone(Handle):
    """A backbone model on a workspace.  state_dict: a mapping from the checkpoint's own names (backbone.0.weight,
    backbone.1.running_mean, backbone.4.0.conv1.weight, backbone.5.0.downsample.0.weight, adjust_dim.weight, bn256.bias, ...) to numpy
    arrays or CPU tensors in PyTorch's layouts.  A leading `module.` (DataParallel) is accepted and num_batches_tracked ignored.
    config: None (block kind and depths read off the names), a dict of btba_vos_net_config fields or a VosNetConfig.

    Callable as Bundler's segmenter: rgb float32 CUDA [n, 3, H, W] -> features float32 [n, 256, Hd, Wd]."""

    _destroy = "btba_vos_net_model_destroy"

    def __init__(self, ws, state_dict, config=None):
        sd = _plain(state_dict)
        self.ws = ws
        self.config = config_from_state_dict(sd) if config is None else resolve_config(config)
        cfg = self.config
        if any(not 1 <= int(cfg.layers[s]) <= MAX_BLOCKS for s in range(4)) or int(cfg.block) not in (BASIC, BOTTLENECK):
            raise ValueError(f"block {int(cfg.block)} not 0 or 1, or a block count of {list(cfg.layers)} outside 1 .. {MAX_BLOCKS}")
        table = layer_table(cfg)
        want = expected_names(cfg)
        missing = [n for n in want if n not in sd]
        if missing:
            raise KeyError(f"backbone weights: missing {missing}; expected the arrays {want}")
        keep = []

        def arr(name, shape):
            v = sd[name]
            a = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float32)
            if tuple(a.shape) != tuple(shape):
                raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
            keep.append(a)
            return a.ctypes.data

        records = (VosNetLayer * len(table))()
        for r, (conv, bn, cout, cin, k) in zip(records, table):
            r.weight = arr(f"{conv}.weight", (cout, cin, k, k))
            r.bn_weight, r.bn_bias = arr(f"{bn}.weight", (cout,)), arr(f"{bn}.bias", (cout,))
            r.running_mean, r.running_var = arr(f"{bn}.running_mean", (cout,)), arr(f"{bn}.running_var", (cout,))
        h = C.c_void_p()
        check(lib().btba_vos_net_model_create(ws.handle, C.byref(cfg), C.cast(records, C.c_void_p), len(table), C.byref(h)), "btba_vos_net_model_create")
        self._h = h

    @classmethod
    def from_npz(cls, ws, path, config=None):
        """A model from an .npz whose arrays carry the state_dict's names (INTEGRATION.md has the export)."""
        with np.load(path) as z:
            return cls(ws, {k: z[k] for k in z.files}, config)

    @classmethod
    def from_checkpoint(cls, ws, path, config=None):
        """A model from a checkpoint as the reference's train.py saves it: torch.load(...)["state_dict"]."""
        import torch
        return cls(ws, torch.load(path, map_location="cpu", weights_only=True)["state_dict"], config)

    def features(self, rgb):
        """rgb: float32 CUDA [n, 3, H, W] (vos.normalize_inputs' output) -> float32 [n, 256, Hd, Wd].  Asynchronous on the workspace stream."""
        return vos_features(self.ws, self, rgb)

    def __call__(self, rgb):
        return vos_features(self.ws, self, rgb)


def vos_features(ws, model: VosBackbone, rgb):
    """btba_vos_features.  rgb: float32 CUDA [n, 3, H, W] -> features float32 [n, 256, ceil(H / 8), ceil(W / 8)]."""
    import torch
    from .optimizer import _dev_ptr
    if rgb.dtype != torch.float32 or rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError(f"vos_features: rgb must be float32 [n, 3, H, W], got {rgb.dtype} {tuple(rgb.shape)}")
    n, H, W = int(rgb.shape[0]), int(rgb.shape[2]), int(rgb.shape[3])
    Hd, Wd = out_size(H, W)
    out = torch.empty((n, OUT_C, Hd, Wd), dtype=torch.float32, device=rgb.device)
    check(lib().btba_vos_features(ws.handle, model.handle, n, H, W, _dev_ptr(rgb, "rgb") if n else None, out.data_ptr() if n else None),
          "btba_vos_features")
    return out
