"""Test-side references for the keypoint head (btba_lfnet_*, include/btba.h): a plain numpy restatement of the three stages --
A (heat and scale maps) and C (refinement and crops) in fp32 or fp64, B (peaks, top-k, survivors) exactly -- the seeded input
makers, the comparison rules, and the loader of the reference-produced vectors (tests/golden/lfnet/lfnet_reference.npz)."""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lfnet", "lfnet_reference.npz")
DEFAULTS = dict(sm_ksize=15, com_strength=3.0, score_com_strength=100.0, scale_com_strength=100.0, nms_thresh=0.0, nms_ksize=5, top_k=500,
                pad_size=16, crop_radius=16, soft_kpts=1, kp_loc_size=9, do_softmax_kp_refine=1, kp_com_strength=1.0, patch_size=32)
SQRT2 = float(np.sqrt(2.0))
# golden groups: name, H, W, scale factors, parameter overrides, number of frames (cases)
GROUPS = (("g40x52_s3", 40, 52, (SQRT2, 1.0, 1.0 / SQRT2), {}, 2),
          ("g64x64_s5", 64, 64, (SQRT2, 2.0 ** 0.25, 1.0, 2.0 ** -0.25, 1.0 / SQRT2), {}, 1),
          ("g20x20_fill", 20, 20, (1.0,), dict(pad_size=2, crop_radius=5, top_k=64), 2))
EDGE_EPS = 1e-3            # patch samples this close to coordinate 0 or W - 1 / H - 1 sit on the crop's discontinuity
EDGE_SHARE = 0.005


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def map_sizes(H, W, scale_factors):
    """The detector's map sizes: int(H / s + 0.5)."""
    return [(int(H / s + 0.5), int(W / s + 0.5)) for s in scale_factors]


def make_inputs(seed, H, W, scale_factors):
    """Seeded inputs of one frame as int8 levels and one multiplier each: (score levels per scale, score multiplier, photo levels,
    photo multiplier, ori levels [H, W, 2], ori multiplier).  The score maps are bounded white noise: after the instance
    normalisation no logit lies more than 3.5 deviations under the maximum, so no heat value is so far under the largest that its
    neighbours' differences drown in the largest one's rounding."""
    rs = np.random.default_rng(seed)
    maps = [rs.integers(-127, 128, (h, w)).astype(np.int8) for (h, w) in map_sizes(H, W, scale_factors)]
    photo = np.clip(np.round(rs.uniform(0, 127, (H, W))), 0, 127).astype(np.int8)
    ang = rs.uniform(0, 2 * np.pi, (H, W))
    ori = np.clip(np.round(np.stack([np.cos(ang), np.sin(ang)], -1) * 127.0), -127, 127).astype(np.int8)
    return maps, np.float32(4.0 / 127.0), photo, np.float32(1.0 / 127.0), ori, np.float32(1.0 / 127.0)


def levels(q, mult):
    return (np.asarray(q).astype(np.float32) * np.float32(mult)).astype(np.float32)


# ---- stage A ---------------------------------------------------------------------------------------------------------

def normalize(x, dtype):
    """instance_normalization: x * inv - mean * inv with the biased variance and eps 1e-3."""
    x = np.asarray(x).astype(dtype)
    mean = x.mean(dtype=np.float64).astype(dtype) if dtype == np.float32 else x.mean()
    var = ((x.astype(np.float64) - np.float64(mean)) ** 2).mean().astype(dtype)
    inv = (dtype(1.0) / np.sqrt(var + dtype(1e-3))).astype(dtype)
    return (x * inv - mean * inv).astype(dtype)


def resize_taps(n_in, n_out, dtype):
    """TF1 resize_images (bilinear, no half-pixel centres) along one axis: (lower, upper, lerp)."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = (np.arange(n_out).astype(dtype) * dtype(scale)).astype(dtype)
    lo = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    up = np.minimum(lo + 1, n_in - 1)
    return lo, up, (src - lo.astype(dtype)).astype(dtype)


def resize(x, H, W, dtype):
    x = np.asarray(x).astype(dtype)
    ya, yb, fy = resize_taps(x.shape[0], H, dtype)
    xa, xb, fx = resize_taps(x.shape[1], W, dtype)
    top = x[ya][:, xa] + (x[ya][:, xb] - x[ya][:, xa]) * fx[None, :]
    bot = x[yb][:, xa] + (x[yb][:, xb] - x[yb][:, xa]) * fx[None, :]
    return (top + (bot - top) * fy[:, None]).astype(dtype)


def window_max(x, k):
    """max over the k x k window cut to the image; x [..., H, W]."""
    h = k // 2
    H, W = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(h, h), (h, h)], constant_values=-np.inf)
    out = np.full_like(x, -np.inf)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, p[..., dy:dy + H, dx:dx + W])
    return out


def window_sum(x, k):
    """sum over the k x k window, zeros outside; x [..., H, W]."""
    h = k // 2
    H, W = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(h, h), (h, h)])
    out = np.zeros_like(x)
    for dy in range(k):
        for dx in range(k):
            out = out + p[..., dy:dy + H, dx:dx + W]
    return out


def frame_mask(H, W, r):
    m = np.zeros((H, W), bool)
    m[r:H - r, r:W - r] = True
    return m


def heatmaps(score_maps, scale_factors, H, W, prm=None, dtype=np.float64):
    """Stage A of one frame: score_maps[s] [h_s, w_s] -> (max_heatmaps, max_scales) [H, W] in `dtype`."""
    prm = params(**(prm or {}))
    k, S = int(prm["sm_ksize"]), len(score_maps)
    logits = np.stack([resize(normalize(m, dtype), H, W, dtype) for m in score_maps])            # [S, H, W]
    mx = window_max(logits.max(0), k)
    e = np.exp(dtype(prm["com_strength"]) * (logits - mx[None])).astype(dtype)
    p = (e / (window_sum(e.sum(0), k)[None] + dtype(1e-6))).astype(dtype)
    pm = p.max(0, keepdims=True)
    a = np.exp(dtype(prm["score_com_strength"]) * (p - pm)).astype(dtype)
    b = np.exp(dtype(prm["scale_com_strength"]) * (p - pm)).astype(dtype)
    heat = (p * (a / (a.sum(0, keepdims=True) + dtype(1e-8)))).sum(0)
    sf = np.asarray(scale_factors, np.float32).astype(dtype).reshape(S, 1, 1)
    scl = (sf * (b / (b.sum(0, keepdims=True) + dtype(1e-8)))).sum(0)
    return (heat * frame_mask(H, W, int(prm["pad_size"]))).astype(dtype), scl.astype(dtype)


# ---- stage B (exact) -------------------------------------------------------------------------------------------------

def peaks(heat, thresh, ksize):
    """non_max_suppression: works strictly greater than all ksize^2 - 1 neighbours, zeros outside the image."""
    heat = np.asarray(heat, np.float32)
    H, W = heat.shape
    hk = ksize // 2
    works = np.where(heat < np.float32(thresh), np.float32(0.0), heat)
    p = np.pad(works, hk)
    pk = np.ones((H, W), bool)
    for dy in range(ksize):
        for dx in range(ksize):
            if dy == hk and dx == hk:
                continue
            pk &= works > p[dy:dy + H, dx:dx + W]
    return pk


def scores(heat, prm):
    heat = np.asarray(heat, np.float32)
    H, W = heat.shape
    pk = peaks(heat, prm["nms_thresh"], int(prm["nms_ksize"]))
    sc = np.where(pk & frame_mask(H, W, int(prm["crop_radius"])), heat, np.float32(0.0)).astype(np.float32)
    return sc + np.float32(0.0), pk                                   # -0 -> +0: one score


def select(heat, prm=None):
    """Stage B of one frame: int32 [m, 2] keypoints (x, y) in raster order.  tf.nn.top_k is a stable sort by descending score."""
    prm = params(**(prm or {}))
    sc, pk = scores(heat, prm)
    H, W = sc.shape
    flat = sc.reshape(-1)
    k = min(int(prm["top_k"]), flat.size)
    chosen = np.argsort(-flat.astype(np.float64), kind="stable")[:k]
    keep = np.zeros(flat.size, bool)
    keep[chosen] = True
    keep &= pk.reshape(-1)
    idx = np.flatnonzero(keep)
    return np.stack([idx % W, idx // W], -1).astype(np.int32)


def select_bruteforce(heat, prm=None):
    """The same by the definition, one position at a time: rank = positions that beat it (greater, or equal and before it)."""
    prm = params(**(prm or {}))
    sc, pk = scores(heat, prm)
    H, W = sc.shape
    flat = sc.reshape(-1).tolist()
    k = min(int(prm["top_k"]), len(flat))
    out = []
    for i in np.flatnonzero(pk.reshape(-1)).tolist():
        rank = sum(1 for j, v in enumerate(flat) if v > flat[i] or (v == flat[i] and j < i))
        if rank < k:
            out.append((i % W, i // W))
    return np.asarray(out, np.int32).reshape(-1, 2)


def decision_margin(heat64, prm=None):
    """The smallest fp64 margin by which a peak or top-k decision inside the crop frame is taken; np.inf where exact zeros decide."""
    prm = params(**(prm or {}))
    H, W = heat64.shape
    ks, hk = int(prm["nms_ksize"]), int(prm["nms_ksize"]) // 2
    works = np.where(heat64 < prm["nms_thresh"], 0.0, heat64)
    p = np.pad(works, hk)
    nb = np.full((H, W), -np.inf)
    for dy in range(ks):
        for dx in range(ks):
            if dy != hk or dx != hk:
                nb = np.maximum(nb, p[dy:dy + H, dx:dx + W])
    gap = np.abs(works - nb)                                          # peak: centre above the best neighbour; else the other way
    gap[works == 0.0] = np.inf                                        # a masked zero is no peak whatever the rounding (heat is never negative)
    m = float(gap.min())
    sc = np.sort(np.where((works > nb) & frame_mask(H, W, int(prm["crop_radius"])), heat64, 0.0).reshape(-1))[::-1]
    k = int(prm["top_k"])
    if k < sc.size and sc[k] > 0.0:                                   # more positive scores than top_k: the cut between two of them
        m = min(m, float(sc[k - 1] - sc[k]))
    return m


# ---- stage C ---------------------------------------------------------------------------------------------------------

def linspace(n, dtype):
    step = dtype(np.float32(2.0) / np.float32(n - 1))
    return (dtype(-1.0) + np.arange(n).astype(dtype) * step).astype(dtype)


def crop(img, n, kx, ky, a, b, c, d, dtype):
    """transformer_crop of one keypoint: img [H, W] -> ([n, n] values, x, y sample coordinates)."""
    img = np.asarray(img).astype(dtype)
    H, W = img.shape
    g = linspace(n, dtype)
    gx, gy = g[None, :], g[:, None]
    x = ((dtype(a) * gx + dtype(b) * gy) * dtype(n) / dtype(2.0) + dtype(kx)).astype(dtype)
    y = ((dtype(c) * gx + dtype(d) * gy) * dtype(n) / dtype(2.0) + dtype(ky)).astype(dtype)
    xf, yf = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x0, x1 = np.clip(xf, 0, W - 1), np.clip(xf + 1, 0, W - 1)
    y0, y1 = np.clip(yf, 0, H - 1), np.clip(yf + 1, 0, H - 1)
    x0f, x1f, y0f, y1f = (v.astype(dtype) for v in (x0, x1, y0, y1))
    out = ((x1f - x) * (y1f - y)) * img[y0, x0] + ((x1f - x) * (y - y0f)) * img[y1, x0] + ((x - x0f) * (y1f - y)) * img[y0, x1] + \
          ((x - x0f) * (y - y0f)) * img[y1, x1]
    return out.astype(dtype), x, y


def crops(photo, ori, heat, scales, kpts_xy, prm=None, dtype=np.float64):
    """Stage C of one frame for integer keypoints [m, 2]: (kpts [m, 2], kpts_scale [m], kpts_ori [m, 2], patches [m, P, P],
    edge [m, P, P] bool: samples on the crop's discontinuity)."""
    prm = params(**(prm or {}))
    L, P = int(prm["kp_loc_size"]), int(prm["patch_size"])
    H, W = np.asarray(photo).shape
    m = len(kpts_xy)
    kp, ksc, kor = np.zeros((m, 2), dtype), np.zeros(m, dtype), np.zeros((m, 2), dtype)
    patches, edge = np.zeros((m, P, P), dtype), np.zeros((m, P, P), bool)
    heat, scales, ori = np.asarray(heat).astype(dtype), np.asarray(scales).astype(dtype), np.asarray(ori).astype(dtype)
    gl = linspace(L, dtype)
    for i, (kx, ky) in enumerate(np.asarray(kpts_xy).tolist()):
        s, (co, sn) = scales[ky, kx], ori[ky, kx]
        rx, ry = dtype(kx), dtype(ky)
        if prm["soft_kpts"]:
            v, _, _ = crop(heat, L, kx, ky, s, 0.0, 0.0, s, dtype)
            if prm["do_softmax_kp_refine"]:
                e = np.exp(dtype(prm["kp_com_strength"]) * (v - v.max())).astype(dtype)
                v = (e / (e.sum() + dtype(1e-8))).astype(dtype)
            dx, dy = (gl[None, :] * v).sum(), (gl[:, None] * v).sum()
            rx = dtype(rx + dx * s * dtype(L) / dtype(2.0))
            ry = dtype(ry + dy * s * dtype(L) / dtype(2.0))
        kp[i], ksc[i], kor[i] = (rx, ry), s, (co, sn)
        patches[i], x, y = crop(photo, P, rx, ry, s * co, s * -sn, s * sn, s * co, dtype)
        edge[i] = (np.abs(x) < EDGE_EPS) | (np.abs(x - (W - 1)) < EDGE_EPS) | (np.abs(y) < EDGE_EPS) | (np.abs(y - (H - 1)) < EDGE_EPS)
    return kp, ksc, kor, patches, edge


# ---- comparison and the golden file -----------------------------------------------------------------------------------

def errors(heat, scl, kp, patches, heat64, scl64, kp64, patches64, edge, scale_factors, photo_range):
    """The four measured errors: heat, scale / scale range, keypoints in pixels, patches / photo range (off the discontinuity)."""
    sr = max(float(max(scale_factors) - min(scale_factors)), 1.0)
    keep = ~edge
    return dict(heat=float(np.abs(heat - heat64).max()), scale=float(np.abs(scl - scl64).max()) / sr,
                kpts=float(np.abs(kp - kp64).max()) if len(kp) else 0.0,
                patch=float(np.abs(patches - patches64)[keep].max()) / float(photo_range) if keep.any() else 0.0)


def load_golden():
    return np.load(GOLDEN)


def group_inputs(z, name, case, scale_factors):
    """The stored inputs of one case as fp32: (score maps, photo, ori)."""
    S = len(scale_factors)
    maps = [levels(z[f"{name}_{case}_score{s}"], z[f"{name}_score_mult"]) for s in range(S)]
    return maps, levels(z[f"{name}_{case}_photo"], z[f"{name}_photo_mult"]), levels(z[f"{name}_{case}_ori"], z[f"{name}_ori_mult"])


def reference_dir():
    return os.environ.get("BTBA_REFERENCE_DIR", "/root/reference")
