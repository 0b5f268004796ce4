"""LF-Net's detector net restated in numpy (lf-net-release/models/mso_resnet_detector.py::get_model in inference; the rules of
include/btba.h), with a dtype argument.

float32: what a device that works in the reference's arithmetic class computes.  Every convolution output is ONE chain over
(ky, kx, c_in) in that order, one rounding per product and one per add: a loop over k on whole arrays.
float64: the reference for the bars (tests/golden/make_lfnet_det_golden.py).
Weights are a mapping from the checkpoint's variable names (ConvOnlyResNet/init_conv/weights, ConvOnlyResNet/block-1/pre-bn/gamma,
...) to arrays, exactly what bundletrack_amd.lfnet_det.LfnetScoreNet takes."""
from __future__ import annotations

import os

import numpy as np

from lfnet_net_ref import BN as _BN, activate, bn_levels, levels, model_weights  # noqa: F401
import lfnet_net_ref as N
from lfnet_ref import resize_taps

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lfnet_det", "lfnet_det_reference.npz")
SCOPE = "ConvOnlyResNet"
MODEL_SEED, PHOTO_SEED = 41000, 42000      # + the group's index: the seeds of the golden file's models and photos
ORI_FLOOR, ORI_CAP = 0.05, 0.01            # pixels whose fp64 raw norm is below ORI_FLOOR x the frame's largest are not compared; at most ORI_CAP of a frame


def scales(min_scale, max_scale, num_scales):
    """get_model's scale factors, largest first."""
    if num_scales == 1:
        return np.array([1.0])
    return np.exp(np.linspace(np.log(max_scale), np.log(min_scale), num_scales))


DEFAULTS = dict(channels=16, ksize=5, blocks=3, min_scale=2.0 ** -0.5, max_scale=2.0 ** 0.5, num_scales=5, activation=1, leaky_alpha=0.2,
                bn_eps=1e-5)
# golden groups: name, configuration, get_model's (perform_bn, use_bias), photos (n, H, W), pre-bn / fin-bn betas of at least 0.5
GROUPS = (("a", dict(channels=16, ksize=3, blocks=1, min_scale=1.0, max_scale=1.0, num_scales=1, activation=0), (True, True), (1, 20, 24), False),
          ("b", dict(channels=16, ksize=5, blocks=2, num_scales=3, activation=1, leaky_alpha=0.2), (True, True), (2, 33, 47), True),
          ("c", dict(channels=32, ksize=3, blocks=1, min_scale=0.5, max_scale=1.0, num_scales=2, activation=0), (False, False), (1, 24, 20), False))


def config(**over):
    """A configuration dict; scale_factors is derived from (min_scale, max_scale, num_scales) unless given."""
    c = dict(DEFAULTS)
    c.update(over)
    if "scale_factors" not in c:
        c["scale_factors"] = [float(s) for s in scales(c["min_scale"], c["max_scale"], c["num_scales"])]
    c["num_scales"] = len(c["scale_factors"])
    return c


def lib_config(cfg):
    """The fields of btba_lfnet_det_config out of a configuration dict."""
    return {k: cfg[k] for k in ("channels", "ksize", "blocks", "scale_factors", "activation", "leaky_alpha", "bn_eps")}


def pad_size(cfg):
    return (2 * cfg["blocks"] + 2) * (cfg["ksize"] // 2)


def map_size(s, size):
    """tf.cast(to_float(size) * (1.0 / s) + 0.5, tf.int32): fp32 product, fp32 sum, truncation."""
    return int(np.float32(np.float32(size) * np.float32(1.0 / s)) + np.float32(0.5))


def map_sizes(cfg, H, W):
    return [(map_size(s, H), map_size(s, W)) for s in cfg["scale_factors"]]


def conv(x, w, dtype):
    """x [n, H, W, C_in], w [k, k, C_in, C_out] -> [n, H, W, C_out]: stride 1, SAME (k // 2 zeros on every side)."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    k, h = w.shape[0], w.shape[0] // 2
    H, W = x.shape[1:3]
    xp = np.pad(x, [(0, 0), (h, h), (h, h), (0, 0)])
    if dtype == np.float64:
        return sum(np.einsum("nhwc,co->nhwo", xp[:, ky:ky + H, kx:kx + W], w[ky, kx]) for ky in range(k) for kx in range(k))
    out = np.zeros(x.shape[:3] + (w.shape[3],), dtype)
    for ky in range(k):
        for kx in range(k):
            tap = xp[:, ky:ky + H, kx:kx + W]
            for c in range(x.shape[3]):
                out = out + tap[..., c, None] * w[ky, kx, c]
    return out


def resize(x, h, w, dtype):
    """TF1's resize_images on NHWC: top, bottom and value lerps in that order."""
    ya, yb, fy = resize_taps(x.shape[1], h, dtype)
    xa, xb, fx = resize_taps(x.shape[2], w, dtype)
    fx, fy = fx[None, None, :, None], fy[None, :, None, None]
    tl, tr, bl, br = x[:, ya][:, :, xa], x[:, ya][:, :, xb], x[:, yb][:, :, xa], x[:, yb][:, :, xb]
    top = tl + (tr - tl) * fx
    bot = bl + (br - bl) * fx
    return (top + (bot - top) * fy).astype(dtype)


def forward(weights, cfg, photos, dtype=np.float64, pad_before_bn=False):
    """photos [n, H, W] -> (score maps: list of [n, h_j, w_j], raw orientation [n, H, W, 2], unit orientation [n, H, W, 2]).
    pad_before_bn: the WRONG rule at every pre-bn (SAME's zeros put in before batch norm and activation), for the test that shows the
    bars see it."""
    C, eps = cfg["channels"], cfg["bn_eps"]
    bias = lambda name: weights.get(f"{SCOPE}/{name}/biases")
    W = lambda name: weights[f"{SCOPE}/{name}/weights"]
    affine = lambda v, pair: v * pair[0].astype(dtype) + pair[1].astype(dtype)
    bn_pair = lambda name, n, b=None: N.fold(weights, SCOPE, name, n, eps, b)

    def conv_of(v, pair, name):
        """conv(act(bn(v))) with the zeros after (right) or before (wrong) the norm and activation."""
        if not pad_before_bn:
            return conv(activate(affine(v, pair), cfg), W(name), dtype)
        h = cfg["ksize"] // 2
        vp = activate(affine(np.pad(v, [(0, 0), (h, h), (h, h), (0, 0)]), pair), cfg)
        return conv(vp, W(name), dtype)[:, h:-h, h:-h]

    x = np.asarray(photos, dtype)[..., None]
    x = affine(conv(x, W("init_conv"), dtype), bn_pair(None, C, bias("init_conv")))
    for i in range(1, cfg["blocks"] + 1):
        b = f"block-{i}"
        t = conv_of(x, bn_pair(f"{b}/pre-bn", C), f"{b}/conv1")
        t = activate(affine(t, bn_pair(f"{b}/mid-bn", C, bias(f"{b}/conv1"))), cfg)
        x = affine(conv(t, W(f"{b}/conv2"), dtype), bn_pair(None, C, bias(f"{b}/conv2"))) + x
    fin = bn_pair("fin-bn", C)
    f = activate(affine(x, fin), cfg)
    H, Wd = x.shape[1:3]
    maps = []
    for j, (h, w) in enumerate(map_sizes(cfg, H, Wd)):
        r = f if (h, w) == (H, Wd) else resize(f, h, w, dtype)
        maps.append(affine(conv(r, W(f"score_conv_{j}"), dtype), bn_pair(None, 1, bias(f"score_conv_{j}")))[..., 0])
    raw = affine(conv(f, W("ori_conv"), dtype), bn_pair(None, 2, bias("ori_conv")))
    ss = raw[..., :1] * raw[..., :1] + raw[..., 1:] * raw[..., 1:]
    unit = raw * (dtype(1.0) / np.sqrt(np.maximum(ss, dtype(1e-12))))
    return maps, raw, unit


def error(maps, unit, maps64, raw64, unit64):
    """The figures the bars bound, the worst over the frames: dict(score = max |got - fp64| / max |fp64| per score map and frame,
    ori = the largest |unit - fp64 unit| over the pixels whose fp64 raw norm is at least ORI_FLOOR x the frame's largest,
    left_out = the largest share of a frame's pixels not compared, norm = the largest | |unit| - 1 | anywhere, worst = max(score, ori))."""
    score = 0.0
    for got, ref in zip(maps, maps64):
        for g, r in zip(np.asarray(got, np.float64), ref):
            score = max(score, float(np.abs(g - r).max() / np.abs(r).max()))
    unit = np.asarray(unit, np.float64)
    nrm = np.sqrt((raw64 ** 2).sum(-1))
    ori = left = 0.0
    for f in range(unit.shape[0]):
        keep = nrm[f] >= ORI_FLOOR * nrm[f].max()
        left = max(left, 1.0 - float(keep.mean()))
        ori = max(ori, float(np.abs(unit[f] - unit64[f])[keep].max()))
    norm = float(np.abs(np.sqrt((unit ** 2).sum(-1)) - 1.0).max()) if np.isfinite(unit).all() else float("inf")
    return dict(score=score, ori=ori, left_out=left, norm=norm, worst=max(score, ori))


# ---- seeded models and photos on int8 levels ----------------------------------------------------------------------------

def layer_shapes(cfg):
    """(name, weight shape, batch-norm name or None) of every convolution and (None, None, name) of every free-standing batch norm,
    in get_model's order."""
    C, k = cfg["channels"], cfg["ksize"]
    out = [("init_conv", (k, k, 1, C), None)]
    for i in range(1, cfg["blocks"] + 1):
        out += [(None, None, f"block-{i}/pre-bn"), (f"block-{i}/conv1", (k, k, C, C), f"block-{i}/mid-bn"), (f"block-{i}/conv2", (k, k, C, C), None)]
    out.append((None, None, "fin-bn"))
    out += [(f"score_conv_{j}", (k, k, C, 1), None) for j in range(cfg["num_scales"])]
    out.append(("ori_conv", (k, k, C, 2), None))
    return out


def make_model(seed, cfg, perform_bn=True, use_bias=True, big_beta=False):
    """{name: (int8 levels, fp32 multiplier)}: weights uniform with He's bound (the second convolution of a block at a third of it, so
    that the residual stream keeps its size), moving variances in [0.5, 2], gammas in [0.64, 1.27]; with big_beta the betas of pre-bn
    and fin-bn are 0.5 .. 1 in size.  ori_conv always has biases, near (1, 0) as the reference initialises them."""
    rs = np.random.default_rng(seed)
    C = cfg["channels"]
    q = {}
    for name, shape, bn in layer_shapes(cfg):
        if name:
            K, n = int(np.prod(shape[:-1])), shape[-1]
            gain = 1.0 / 3.0 if name.endswith("conv2") else (0.5 if name == "ori_conv" else 1.0)
            q[f"{SCOPE}/{name}/weights"] = (rs.integers(-127, 128, shape).astype(np.int8), np.float32(gain * np.sqrt(6.0 / K) / 127.0))
            if name == "ori_conv":
                q[f"{SCOPE}/{name}/biases"] = (np.array([127, -40], np.int8), np.float32(1.0 / 127.0))
            elif use_bias:
                q[f"{SCOPE}/{name}/biases"] = (rs.integers(-127, 128, n).astype(np.int8), np.float32(1.0 / 512.0))
        if bn and perform_bn:
            q.update((f"{SCOPE}/{bn}/{k}", v) for k, v in bn_levels(rs, C, big_beta and name is None).items())
    return q


def make_photos(seed, n, H, W):
    """Smooth blobs plus noise on levels 0 .. 127 of 1 / 127: (int8 [n, H, W], multiplier)."""
    rs = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    y, x = y / float(max(H, 2)), x / float(max(W, 2))
    out = np.zeros((n, H, W))
    for i in range(n):
        for _ in range(3):
            cx, cy, s = rs.uniform(0.1, 0.9), rs.uniform(0.1, 0.9), rs.uniform(0.05, 0.3)
            out[i] += 0.3 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
        out[i] += 0.4 * rs.random((H, W))
    return np.clip(np.round(out * 127.0), 0, 127).astype(np.int8), np.float32(1.0 / 127.0)


def load_golden():
    return np.load(GOLDEN)


def group_model(z, name):
    """The stored model and photos of a group as fp32: (weights, photos [n, H, W])."""
    return N.group_model(z, name, SCOPE, "photos")
