"""LF-Net's descriptor net restated in numpy (lf-net-release/models/simple_desc.py::get_model in inference), with a dtype argument.

float32: what a device that works in the reference's arithmetic class computes.  Every dot product is ONE chain over k in the
kernels' order ((ky, kx, c_in) for a convolution), one rounding per product and one per add: a loop over k on whole arrays.
float64: the reference for the bars (tests/golden/make_lfnet_desc_golden.py).
Weights are a mapping from the checkpoint's variable names (SimpleDesc/conv1/weights, SimpleDesc/bn1/moving_mean, ...) to arrays,
exactly what bundletrack_amd.lfnet_desc.LfnetDescriptor takes."""
from __future__ import annotations

import os

import numpy as np

from lfnet_net_ref import activate, bn_levels, fold, levels, model_weights  # noqa: F401
import lfnet_net_ref as N

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lfnet_desc", "lfnet_desc_reference.npz")
SCOPE = "SimpleDesc"
DEFAULTS = dict(patch_size=32, depth=3, channels=64, fc_dim=512, out_dim=256, activation=0, leaky_alpha=0.2, norm=0, bn_eps=1e-5)
# golden groups: name, configuration, get_model's (perform_bn, use_bias), patches.  get_model switches batch norm and biases for all
# layers at once, so group c has neither anywhere, fc1 included.
GROUPS = (("a", dict(patch_size=16, depth=2, channels=16, fc_dim=32, out_dim=16, activation=0, norm=0), (True, True), 5),
          ("b", dict(patch_size=32, depth=3, channels=16, fc_dim=64, out_dim=32, activation=1, leaky_alpha=0.2, norm=1), (True, True), 5),
          ("c", dict(patch_size=32, depth=3, channels=32, fc_dim=128, out_dim=64, activation=0, norm=0), (False, False), 5))
MODEL_SEED, PATCH_SEED = 31000, 32000      # + the group's index: the seeds of the golden file's models and patches


def config(**over):
    c = dict(DEFAULTS)
    c.update(over)
    return c


def same_pads(n: int):
    """TensorFlow's SAME for a 3-tap window with stride 2: (output size, padding before, padding after)."""
    out = -(-n // 2)
    total = max((out - 1) * 2 + 3 - n, 0)
    return out, total // 2, total - total // 2


def layer_scopes(depth):
    return [(f"conv{i + 1}", f"bn{i + 1}") for i in range(depth)] + [("fc1", "fc-bn1"), ("fc2", None)]


def conv(x, w, dtype):
    """x [m, H, W, C_in], w [3, 3, C_in, C_out] -> [m, ceil(H / 2), ceil(W / 2), C_out], stride 2, SAME."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    (Ho, hb, ha), (Wo, wb, wa) = same_pads(x.shape[1]), same_pads(x.shape[2])
    xp = np.pad(x, [(0, 0), (hb, ha), (wb, wa), (0, 0)])
    if dtype == np.float64:
        return sum(np.einsum("mhwc,cn->mhwn", xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2], w[ky, kx]) for ky in range(3) for kx in range(3))
    out = np.zeros((x.shape[0], Ho, Wo, w.shape[3]), dtype)
    for ky in range(3):
        for kx in range(3):
            tap = xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
            for c in range(x.shape[3]):
                out = out + tap[..., c, None] * w[ky, kx, c]
    return out


def dense(x, w, dtype):
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    if dtype == np.float64:
        return x @ w
    out = np.zeros((x.shape[0], w.shape[1]), dtype)
    for k in range(x.shape[1]):
        out = out + x[:, k, None] * w[k]
    return out


def flatten(x):
    """(h, w, c): NHWC as it lies."""
    return np.ascontiguousarray(x).reshape(x.shape[0], -1)


def l2_normalize(raw, dtype):
    if dtype == np.float64:
        ss = (raw * raw).sum(1, keepdims=True)
    else:
        ss = np.zeros((raw.shape[0], 1), dtype)
        for k in range(raw.shape[1]):
            ss = ss + raw[:, k, None] * raw[:, k, None]
    return raw * (dtype(1.0) / np.sqrt(np.maximum(ss, dtype(1e-12))))


def forward(weights, cfg, patches, dtype=np.float64):
    """patches [m, P, P] -> (descriptors [m, D], raw fc2 output [m, D])."""
    x = np.asarray(patches, dtype)[..., None]
    depth = cfg["depth"]
    for i, (layer, bn) in enumerate(layer_scopes(depth)):
        w = weights[f"{SCOPE}/{layer}/weights"]
        if i == depth:
            x = flatten(x)
        acc = conv(x, w, dtype) if i < depth else dense(x, w, dtype)
        scale, shift = fold(weights, SCOPE, bn, w.shape[-1], cfg["bn_eps"], weights.get(f"{SCOPE}/{layer}/biases"))
        y = acc * scale.astype(dtype) + shift.astype(dtype)
        x = activate(y, cfg) if i <= depth else y
    return (l2_normalize(x, dtype) if cfg["norm"] == 0 else x), x


def error(desc, raw, desc64, raw64, cfg):
    """The figure the bars bound: absolute on unit-norm descriptors; without the norm, relative to the case's largest |raw|."""
    if cfg["norm"] == 0:
        return float(np.abs(np.asarray(desc, np.float64) - desc64).max())
    return float(np.abs(np.asarray(raw, np.float64) - raw64).max() / np.abs(raw64).max())


# ---- seeded models and patches on int8 levels ---------------------------------------------------------------------------

def make_model(seed, cfg, perform_bn=True, use_bias=True):
    """{name: (int8 levels, fp32 multiplier)}: weights uniform with He's bound, moving variances in [0.5, 2], gammas in [0.64, 1.27]."""
    rs = np.random.default_rng(seed)
    q = {}
    c_in, depth = 1, cfg["depth"]
    shapes = []
    for i in range(depth):
        shapes.append((3, 3, c_in, cfg["channels"] << i))
        c_in = cfg["channels"] << i
    side = cfg["patch_size"] >> depth
    shapes += [(side * side * c_in, cfg["fc_dim"]), (cfg["fc_dim"], cfg["out_dim"])]
    for (layer, bn), shape in zip(layer_scopes(depth), shapes):
        K, n = int(np.prod(shape[:-1])), shape[-1]
        q[f"{SCOPE}/{layer}/weights"] = (rs.integers(-127, 128, shape).astype(np.int8), np.float32(np.sqrt(6.0 / K) / 127.0))
        if use_bias:
            q[f"{SCOPE}/{layer}/biases"] = (rs.integers(-127, 128, n).astype(np.int8), np.float32(1.0 / 512.0))
        if bn and perform_bn:
            q.update((f"{SCOPE}/{bn}/{k}", v) for k, v in bn_levels(rs, n).items())
    return q


def make_patches(seed, m, P):
    """Smooth blobs plus noise on levels 0 .. 127 of 1 / 127: (int8 [m, P, P], multiplier)."""
    rs = np.random.default_rng(seed)
    y, x = np.mgrid[0:P, 0:P] / float(P)
    out = np.zeros((m, P, P))
    for i in range(m):
        cx, cy, s = rs.uniform(0.2, 0.8), rs.uniform(0.2, 0.8), rs.uniform(0.1, 0.4)
        out[i] = 0.6 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s)) + 0.4 * rs.random((P, P))
    return np.clip(np.round(out * 127.0), 0, 127).astype(np.int8), np.float32(1.0 / 127.0)


def load_golden():
    return np.load(GOLDEN)


def group_model(z, name):
    """The stored model and patches of a group as fp32: (weights, patches [m, P, P])."""
    return N.group_model(z, name, SCOPE, "patches")
