"""Test-side references for the mask propagation (btba_vos_*, include/btba.h): a plain numpy restatement of predict's formulas in
fp32 and fp64, of the two bilinear interpolations, of sample_frames and of the input normalisation; the case generator; the
comparison rules (measured tolerance, arg-max decisions above a margin); the loader of the reference-produced vectors
(tests/golden/vos/vos_reference.npz) and of the reference's own lib/predict.py where its checkout exists."""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "vos", "vos_reference.npz")
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
DEFAULTS = dict(ref_num=9, range=40, sigma_dense=8.0, sigma_sparse=21.0, temperature=1.0, continuous_frames=4, sparse_after=15)
# golden groups: name, Hd, Wd, H, W, C, d, feature scale, the frame_idx cases (the history has max + 1 frames)
GROUPS = (("g7x9_c24", 7, 9, 52, 68, 24, 2, 1.0, (1, 3, 9, 10, 15, 16, 17, 24, 60)), ("g7x9_c8_large", 7, 9, 52, 68, 8, 2, 7.0, (3, 17)),
          ("g15x20_c256", 15, 20, 120, 160, 256, 3, 1.0, (3, 9)))
SAMPLE_CONFIGS = ((9, 40), (5, 10), (4, 40))


def sample_frames(frame_idx, ref_num=9, take_range=40, continuous_frames=4, sparse_after=15):
    """(indices, n_dense): lib/predict.py::sample_frames and the weight rule of predict:48-55."""
    if frame_idx <= ref_num:
        idx = list(range(frame_idx))
    else:
        dense_num = continuous_frames - 1
        ref_end = frame_idx - dense_num - 1
        ref_start = max(ref_end - take_range, 0)
        idx = np.linspace(ref_start, ref_end, ref_num - dense_num).astype(int).tolist()
        idx += [frame_idx - dense_num + j for j in range(dense_num)]
    return idx, (min(continuous_frames, len(idx)) if frame_idx > sparse_after else len(idx))


def spatial_weight(Hd, Wd, sigma, dtype):
    """w[p, q] = exp(-|p - q|^2 / sigma^2) over the grid, [HW, HW]."""
    i = np.arange(Hd * Wd)
    yx = np.stack([i // Wd, i % Wd], -1).astype(dtype)
    d2 = ((yx[:, None, :] - yx[None, :, :]) ** 2).sum(-1)
    return np.exp(-d2 / dtype(sigma) ** 2).astype(dtype)


def predict(refs, labels, tgt, n_dense, Hd, Wd, sigma_dense=8.0, sigma_sparse=21.0, temperature=1.0, dtype=np.float64):
    """refs [n, C, HW], labels [n, d, HW], tgt [C, HW] -> pred [d, HW]: the formulas of include/btba.h in `dtype`."""
    refs, labels, tgt = (np.asarray(a).astype(dtype) for a in (refs, labels, tgt))
    n, C, HW = refs.shape
    keys = refs.transpose(0, 2, 1).reshape(n * HW, C)
    s = (keys @ tgt) * dtype(temperature)
    e = np.exp(s - s.max(0, keepdims=True))
    P = (e / e.sum(0, keepdims=True)).reshape(n, HW, HW)
    wd, wsp = spatial_weight(Hd, Wd, sigma_dense, dtype), spatial_weight(Hd, Wd, sigma_sparse, dtype)
    P = P * np.stack([wd if r >= n - n_dense else wsp for r in range(n)])
    return labels.transpose(1, 0, 2).reshape(labels.shape[1], n * HW) @ P.reshape(n * HW, HW)


def taps(n_in, n_out):
    """torch's bilinear, align_corners=False, along one axis in fp32: (i0, i1, w0, w1) per output index."""
    o = np.arange(n_out, dtype=np.float32)
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.maximum((scale * (o + np.float32(0.5))).astype(np.float32) - np.float32(0.5), np.float32(0.0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1.0) - w1).astype(np.float32), w1


def bilinear(img, H_out, W_out):
    """img [c, H, W] float32 -> [c, H_out, W_out] float32."""
    img = np.asarray(img, np.float32)
    y0, y1, wy0, wy1 = taps(img.shape[1], H_out)
    x0, x1, wx0, wx1 = taps(img.shape[2], W_out)
    top = wx0 * img[:, y0][:, :, x0] + wx1 * img[:, y0][:, :, x1]
    bot = wx0 * img[:, y1][:, :, x0] + wx1 * img[:, y1][:, :, x1]
    return (wy0[None, :, None] * top + wy1[None, :, None] * bot).astype(np.float32)


def grid_of(H, W):
    return (H + 7) // 8, (W + 7) // 8


def onehot(idx, d):
    """idx2onehot's scatter: [d, ...] float32, 1 where idx == c."""
    return (np.asarray(idx)[None] == np.arange(d).reshape((d,) + (1,) * np.ndim(idx))).astype(np.float32)


def first_labels(label_img, d):
    """prepare_first_frame: [d, Hd, Wd] float32."""
    H, W = label_img.shape
    return bilinear(onehot(label_img, d), *grid_of(H, W))


def masks(pred, Hd, Wd, H, W):
    """run_video.py:151-155: (class map uint8 [H, W], the upsampled prediction [d, H, W])."""
    up = bilinear(np.asarray(pred, np.float32).reshape(-1, Hd, Wd), H, W)
    return np.argmax(up, 0).astype(np.uint8), up


def normalize_inputs(bgr):
    """rgb_normalize on imread's BGR bytes [n, H, W, 3] -> float32 [n, 3, H, W]."""
    rgb = np.asarray(bgr)[..., ::-1].astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(((rgb - MEAN) / STD).astype(np.float32).transpose(0, 3, 1, 2))


def compact_labels(label_img):
    """(compacted image uint8, the sorted original values): a 0 / 255 mask becomes classes 0 / 1.  Value 0 stays class 0."""
    vals = np.unique(np.concatenate([[0], np.asarray(label_img).reshape(-1)]))
    return np.searchsorted(vals, label_img).astype(np.uint8), vals


def label_image(H, W, d, shift, seed=0):
    """A coherent d-class label image whose regions drift with `shift`."""
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(seed)
    a, b = rng.integers(9, 17), rng.integers(11, 19)
    return ((((x + 2 * shift) // a) + (y + shift) // b) % d).astype(np.uint8)


def make_history(seed, Hd, Wd, H, W, C, d, n_frames, scale=1.0):
    """(q int8 [n_frames, C, HW], mult float32, labels float32 [n_frames, d, HW]): the features are q * mult -- a shared base plus
    noise, so a target's softmax spreads over the references, on a grid of thirds so that a history stores small; frame 0's labels
    are soft, the others one-hot."""
    rng = np.random.default_rng(seed)
    HW = Hd * Wd
    base = rng.standard_normal((C, HW))
    q = np.clip(np.rint((base[None] + 0.5 * rng.standard_normal((n_frames, C, HW))) * 3.0), -127, 127).astype(np.int8)
    labels = np.empty((n_frames, d, HW), np.float32)
    labels[0] = first_labels(label_image(H, W, d, 0, seed), d).reshape(d, HW)
    for k in range(1, n_frames):
        yy, xx = np.minimum(np.arange(Hd) * 8 + 4, H - 1), np.minimum(np.arange(Wd) * 8 + 4, W - 1)
        labels[k] = onehot(label_image(H, W, d, k, seed)[yy][:, xx].reshape(-1), d)
    return q, np.float32(scale * 0.33 * C ** -0.25), labels


def features(q, mult):
    return np.asarray(q).astype(np.float32) * np.float32(mult)


def rel_err(pred, pred64):
    """max |pred - pred64| / max_c |pred64[:, q]| over all entries."""
    col = np.abs(pred64).max(0, keepdims=True)
    return float((np.abs(np.asarray(pred, np.float64) - pred64) / col).max())


def decisions_ok(arg, pred64, tol):
    """(ok, n_left_out): arg equals argmax_c pred64 wherever the top two classes differ by at least 2 tol of the column maximum."""
    srt = np.sort(pred64, 0)
    margin = (srt[-1] - srt[-2]) / np.abs(pred64).max(0)
    clear = margin >= 2.0 * tol
    return bool(np.all(np.asarray(arg).reshape(-1)[clear] == np.argmax(pred64, 0)[clear])), int(np.count_nonzero(~clear))


def check(pred, pred64, tol, arg=None):
    """The two rules a result is held to: the error bar, and the decisions with at most 2 % of the positions left out."""
    err = rel_err(pred, pred64)
    ok, out = decisions_ok(np.argmax(pred, 0) if arg is None else arg, pred64, tol)
    return err, err <= tol and ok and out <= 0.02 * pred64.shape[1]


def load_golden():
    return np.load(GOLDEN)


def reference_dir():
    return os.environ.get("BTBA_REFERENCE_DIR", "/root/reference")


def reference_module():
    """The reference's lib/predict.py loaded by path (as the package `lib`, for its relative import) under the two shims it needs
    on a CPU torch -- np.int and an identity Tensor.cuda -- or None where the checkout does not exist."""
    root = os.path.join(reference_dir(), "transductive-vos.pytorch")
    if not os.path.exists(os.path.join(root, "lib", "predict.py")):
        return None
    import importlib.util
    import sys
    import types
    import torch
    if not hasattr(np, "int"):
        np.int = int
    torch.Tensor.cuda = lambda self, *a, **k: self
    pkg = types.ModuleType("btba_vos_reference_lib")
    pkg.__path__ = [os.path.join(root, "lib")]
    sys.modules[pkg.__name__] = pkg
    utils = types.ModuleType(pkg.__name__ + ".utils")       # lib/utils.py imports more than is installed; predict needs only the name
    utils.idx2onehot = None
    sys.modules[utils.__name__] = utils
    spec = importlib.util.spec_from_file_location(pkg.__name__ + ".predict", os.path.join(root, "lib", "predict.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod
