"""What the numpy restatements of LF-Net's two nets (lfnet_desc_ref.py, lfnet_det_ref.py) share: int8 levels, the activation, the
fold of bias and batch norm into (scale, shift) as include/btba.h states it, the batch-norm draws of a seeded model and the stored
groups of a golden file."""
from __future__ import annotations

import numpy as np

BN = ("gamma", "beta", "moving_mean", "moving_variance")


def levels(q, mult):
    return (np.asarray(q).astype(np.float32) * np.float32(mult)).astype(np.float32)


def model_weights(q):
    return {name: levels(*v) for name, v in q.items()}


def activate(y, cfg):
    if cfg["activation"] == 0:
        return np.maximum(y, 0)
    return np.where(y >= 0, y, y * y.dtype.type(np.float32(cfg["leaky_alpha"])))


def fold(weights, scope, bn_name, n, eps, bias=None):
    """(scale, shift) of include/btba.h in fp64 for the batch norm `bn_name` behind `bias`; (1, bias) where the norm is absent."""
    g = lambda key, default: np.asarray(weights[key], np.float64) if key in weights else np.full(n, default, np.float64)
    b = np.zeros(n) if bias is None else np.asarray(bias, np.float64)
    if bn_name is None or f"{scope}/{bn_name}/moving_mean" not in weights:
        return np.ones(n), b
    scale = g(f"{scope}/{bn_name}/gamma", 1.0) / np.sqrt(g(f"{scope}/{bn_name}/moving_variance", 1.0) + np.float64(np.float32(eps)))
    return scale, g(f"{scope}/{bn_name}/beta", 0.0) + (b - g(f"{scope}/{bn_name}/moving_mean", 0.0)) * scale


def bn_levels(rs, n, big_beta=False):
    """{field: (int8 levels, fp32 multiplier)} of one batch norm, drawn from `rs` in the order of BN: gammas in [0.64, 1.27], moving
    variances in [0.5, 2]; with big_beta the betas are 0.5 .. 1 in size."""
    q = {"gamma": (rs.integers(64, 128, n).astype(np.int8), np.float32(0.01))}
    if big_beta:
        q["beta"] = ((rs.integers(64, 128, n) * rs.choice([-1, 1], n)).astype(np.int8), np.float32(1.0 / 128.0))
    else:
        q["beta"] = (rs.integers(-127, 128, n).astype(np.int8), np.float32(1.0 / 512.0))
    q["moving_mean"] = (rs.integers(-127, 128, n).astype(np.int8), np.float32(1.0 / 512.0))
    q["moving_variance"] = (rs.integers(32, 128, n).astype(np.int8), np.float32(1.0 / 64.0))
    return q


def group_model(z, group, scope, input_key):
    """The stored model and inputs of a golden group as fp32: (weights, inputs)."""
    pre = f"{group}/"
    w = {k[len(pre):]: levels(z[k], z[k + "@mult"]) for k in z.files if k.startswith(pre + scope) and not k.endswith("@mult")}
    return w, levels(z[f"{group}/{input_key}"], z[f"{group}/{input_key}@mult"])
