"""The video segmentation's backbone restated in numpy (transductive-vos.pytorch/modeling/network.py::VOSNet on
modeling/backbone/resnet.py in eval mode; the rules of include/btba.h), with a dtype argument.

float64: the reference for the bars (tests/golden/make_vos_net_golden.py holds it to the reference's own fp64 run).
float32: what a device that works in the reference's arithmetic class computes.  Every convolution output is ONE chain over
(ky, kx, c_in) in that order, one rounding per product and one per add: a loop over k on whole arrays.
Weights are a mapping from the state_dict's names (backbone.0.weight, backbone.4.0.bn1.running_var, adjust_dim.weight, ...) to arrays
in PyTorch's layouts, exactly what bundletrack_amd.vos_net.VosBackbone takes.  A configuration is a dict(block=0 | 1, layers=[4 counts],
bn_eps=...)."""
from __future__ import annotations

import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "vos_net", "vos_net_reference.npz")
BASIC, BOTTLENECK = 0, 1
PLANES, STRIDES, STEM_C, OUT_C = (64, 128, 256, 256), (1, 2, 1, 1), 64, 256
BN_KEYS = ("weight", "bias", "running_mean", "running_var")
MODEL_SEED, PHOTO_SEED = 51000, 52000      # + the group's index: the seeds of the golden file's models and photos
# golden groups: name, configuration, photos (n, H, W)
GROUPS = (("a", dict(block=BASIC, layers=[1, 1, 1, 1]), (2, 40, 56)),
          ("b", dict(block=BOTTLENECK, layers=[1, 1, 1, 1]), (2, 33, 47)),
          ("c", dict(block=BOTTLENECK, layers=[3, 4, 6, 3]), (1, 40, 56)))


def config(**over):
    c = dict(block=BOTTLENECK, layers=[3, 4, 6, 3], bn_eps=1e-5)
    c.update(over)
    c["layers"] = [int(v) for v in c["layers"]]
    return c


def out_size(size):
    """Three halvings, each (in + 2 pad - k) // 2 + 1: the stem, the pool, layer2."""
    for k in (7, 3, 3):
        size = (size + 2 * (k // 2) - k) // 2 + 1
    return size


def layer_table(cfg):
    """(convolution's name, batch norm's name, C_out, C_in, k, stride) of every convolution in forward order: stem; per block conv1,
    conv2, [conv3], [downsample]; adjust_dim."""
    bott = cfg["block"] == BOTTLENECK
    expansion = 4 if bott else 1
    out = [("backbone.0", "backbone.1", STEM_C, 3, 7, 2)]
    inplanes = STEM_C
    for s in range(4):
        planes, out_c = PLANES[s], PLANES[s] * expansion
        for b in range(cfg["layers"][s]):
            stride = STRIDES[s] if b == 0 else 1
            p = f"backbone.{4 + s}.{b}"
            if bott:
                out += [(f"{p}.conv1", f"{p}.bn1", planes, inplanes, 1, 1), (f"{p}.conv2", f"{p}.bn2", planes, planes, 3, stride),
                        (f"{p}.conv3", f"{p}.bn3", out_c, planes, 1, 1)]
            else:
                out += [(f"{p}.conv1", f"{p}.bn1", planes, inplanes, 3, stride), (f"{p}.conv2", f"{p}.bn2", planes, planes, 3, 1)]
            if b == 0 and (stride != 1 or inplanes != out_c):
                out.append((f"{p}.downsample.0", f"{p}.downsample.1", out_c, inplanes, 1, stride))
            inplanes = out_c
    if bott:
        out.append(("adjust_dim", "bn256", OUT_C, inplanes, 1, 1))
    return out


# ---- the net ----------------------------------------------------------------------------------------------------------

def conv(x, w, stride, dtype):
    """x [n, H, W, C_in] NHWC, w [C_out, C_in, k, k] -> [n, Ho, Wo, C_out]: pad k // 2, no bias."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    k, p = w.shape[2], w.shape[2] // 2
    n, H, W, Cin = x.shape
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    xp = np.pad(x, [(0, 0), (p, p), (p, p), (0, 0)])
    taps = [(ky, kx, xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]) for ky in range(k) for kx in range(k)]
    if dtype == np.float64:
        return sum(t.reshape(-1, Cin) @ w[:, :, ky, kx].T for ky, kx, t in taps).reshape(n, Ho, Wo, -1)
    out = np.zeros((n * Ho * Wo, w.shape[0]), dtype)
    tmp = np.empty_like(out)
    for ky, kx, t in taps:
        a = np.ascontiguousarray(t.reshape(-1, Cin).T)             # [C_in][M]
        wk = np.ascontiguousarray(w[:, :, ky, kx].T)               # [C_in][C_out]
        for c in range(Cin):
            np.multiply(a[c][:, None], wk[c][None, :], out=tmp)
            np.add(out, tmp, out=out)
    return out.reshape(n, Ho, Wo, -1)


def max_pool(x):
    """3 x 3, stride 2, pad 1 on NHWC; the padding is -inf."""
    n, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.pad(x, [(0, 0), (1, 1), (1, 1), (0, 0)], constant_values=-np.inf)
    out = np.full((n, Ho, Wo, C), -np.inf, x.dtype)
    for ky in range(3):
        for kx in range(3):
            out = np.maximum(out, xp[:, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2])
    return out


def fold(weights, bn, eps, dtype):
    """(scale, shift) of include/btba.h: fp64, rounded once to `dtype`."""
    g = lambda k: np.asarray(weights[f"{bn}.{k}"], np.float64)
    scale = g("weight") / np.sqrt(g("running_var") + np.float64(np.float32(eps)))
    return scale.astype(dtype), (g("bias") - g("running_mean") * scale).astype(dtype)


def forward(weights, cfg, x, dtype=np.float64):
    """x [n, 3, H, W] -> features [n, 256, Hd, Wd] in `dtype`."""
    table = {t[0]: t for t in layer_table(cfg)}

    def cb(v, name, relu, res=None):
        """conv -> bn [-> + res] [-> relu]"""
        _, bn, cout, cin, k, stride = table[name]
        assert v.shape[3] == cin
        scale, shift = fold(weights, bn, cfg["bn_eps"], dtype)
        y = conv(v, weights[f"{name}.weight"], stride, dtype) * scale + shift
        if res is not None:
            y = y + res
        return np.maximum(y, 0) if relu else y

    v = max_pool(cb(np.asarray(x, dtype).transpose(0, 2, 3, 1), "backbone.0", True))
    bott = cfg["block"] == BOTTLENECK
    for s in range(4):
        for b in range(cfg["layers"][s]):
            p = f"backbone.{4 + s}.{b}"
            t = cb(v, f"{p}.conv1", True)
            if bott:
                t = cb(t, f"{p}.conv2", True)
            res = cb(v, f"{p}.downsample.0", False) if f"{p}.downsample.0" in table else v
            v = cb(t, f"{p}.conv3" if bott else f"{p}.conv2", True, res)
    if bott:
        v = cb(v, "adjust_dim", False)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2))


def error(y, y64):
    """max |y - y64| / max |y64| per frame, the worst over the frames."""
    y = np.asarray(y, np.float64)
    return max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(y, y64))


# ---- seeded models and photos on int8 levels ----------------------------------------------------------------------------

def levels(q, mult):
    return (np.asarray(q).astype(np.float32) * np.float32(mult)).astype(np.float32)


def make_model(seed, cfg):
    """{name: (int8 levels, fp32 multiplier)}: convolution weights uniform with He's bound sqrt(6 / K), batch-norm weights and running
    variances in 0.5 .. 1.5, biases and running means within +- 0.2."""
    rs = np.random.default_rng(seed)
    q = {}
    for conv_name, bn, cout, cin, k, _ in layer_table(cfg):
        K = cin * k * k
        q[f"{conv_name}.weight"] = (rs.integers(-127, 128, (cout, cin, k, k)).astype(np.int8), np.float32(np.sqrt(6.0 / K) / 127.0))
        q[f"{bn}.weight"] = (rs.integers(43, 128, cout).astype(np.int8), np.float32(1.5 / 127.0))
        q[f"{bn}.bias"] = (rs.integers(-127, 128, cout).astype(np.int8), np.float32(0.2 / 127.0))
        q[f"{bn}.running_mean"] = (rs.integers(-127, 128, cout).astype(np.int8), np.float32(0.2 / 127.0))
        q[f"{bn}.running_var"] = (rs.integers(43, 128, cout).astype(np.int8), np.float32(1.5 / 127.0))
    return q


def model_weights(q):
    return {name: levels(*v) for name, v in q.items()}


def make_photos(seed, n, H, W):
    """Normalised RGB frames, smooth blobs plus noise within about +- 2 on levels of 1 / 50: (int8 [n, 3, H, W], multiplier)."""
    rs = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    y, x = y / float(max(H, 2)), x / float(max(W, 2))
    out = np.zeros((n, 3, H, W))
    for i in range(n):
        for c in range(3):
            for _ in range(3):
                cx, cy, s = rs.uniform(0.1, 0.9), rs.uniform(0.1, 0.9), rs.uniform(0.05, 0.3)
                out[i, c] += rs.uniform(-1.5, 1.5) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
            out[i, c] += rs.uniform(-1.0, 1.0, (H, W))
    return np.clip(np.round(out * 50.0), -127, 127).astype(np.int8), np.float32(1.0 / 50.0)


def crc(q):
    """One CRC-32 over a seeded model's or photo set's levels and multipliers, names sorted."""
    if isinstance(q, tuple):
        q = {"": q}
    c = 0
    for name in sorted(q):
        lev, mult = q[name]
        c = zlib.crc32(np.float32(mult).tobytes(), zlib.crc32(np.ascontiguousarray(lev, np.int8).tobytes(), zlib.crc32(name.encode(), c)))
    return c


def load_golden():
    return np.load(GOLDEN)


def group(z, g):
    """Group g of the golden file with its model regenerated from the stored seed: dict(name, cfg, q (levels), weights (fp32), photos
    (fp32 [n, 3, H, W]), ref (the reference's fp32 output), tol, keys)."""
    name, over, _ = GROUPS[g]
    cfg = config(**over)
    q = make_model(int(z[f"{name}/model_seed"]), cfg)
    return dict(name=name, cfg=cfg, q=q, weights=model_weights(q), photos=levels(z[f"{name}/photos"], z[f"{name}/photos@mult"]),
                ref=z[f"{name}/ref"], tol=float(z[f"tol_{name}"]), keys=[str(k) for k in z[f"{name}/keys"]])
