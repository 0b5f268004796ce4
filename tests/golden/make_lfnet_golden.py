"""Writes tests/golden/lfnet/lfnet_reference.npz: inputs and the reference's own results for them.

    python tests/golden/make_lfnet_golden.py          (needs the reference checkout: BTBA_REFERENCE_DIR, see tests/lfnet_ref.py)

The reference's lf-net-release/inference.py, det_tools.py and spatial_transformer.py are loaded by path under stand-in modules of
this project's own writing: an empty `cv2`, a `utils` with the one name inference.py imports, and an eager `tensorflow` on numpy
fp32 (below) that covers the ops those functions use.  build_multi_scale_deep_detector_3DNMS and build_patch_extraction are then
run as run_server.py builds them, with a stand-in detector object that hands back stored score maps, ori_maps, scale_factors and
pad_size.  So the order of operations, the masks, the borders and the tie handling are the reference's own text, and what each op
means is the stand-in's: COMPOSITION FROM THE REFERENCE, OP SEMANTICS RESTATED, UNVERIFIED AGAINST A TENSORFLOW RUN
(INTEGRATION.md has a TF1 snippet that prints values stored here).  Only inputs and results are stored:
  per group of lfnet_ref.GROUPS and case   score maps, photo and ori_maps as int8 levels (one fp32 multiplier per kind and group);
                                           the reference's fp32 max_heatmaps, scale_maps, keypoints (x, y) in its order, refined
                                           kpts, kpts_scale, kpts_ori and patches
  tol_<group>_{heat,scale,kpts,patch}      4 x err_ref, err_ref = the largest difference between the reference's fp32 result and the
                                           fp64 restatement over the group's cases (lfnet_ref.errors)
A seed is taken only if every peak and top-k decision of the case has an fp64 margin above its heat bar, the share of patch
samples on the crop's discontinuity is at most 0.5 %, and the restatement's stage B on the reference's heat map gives the
reference's keypoints; the file is written only if the reference's own fp32 result is inside the bars."""
import contextlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lfnet_ref as R  # noqa: E402
from ref_loader import load_under_stand_ins  # noqa: E402

F32 = np.float32


class Shape(tuple):
    """TensorShape: a tuple with as_list() and ndims."""
    ndims = property(len)

    def as_list(self):
        return list(self)


class T(np.ndarray):
    """An eager tensor: a numpy array with the three shape methods the reference calls."""

    def get_shape(self):
        return Shape(self.shape)

    def set_shape(self, shape):
        pass


def t(x, dtype=None):
    return np.asarray(x, dtype=dtype).view(T)


def _axis(a):
    return tuple(a) if isinstance(a, (list, tuple)) else a


def _shape(s):
    return tuple(int(v) for v in np.asarray(s).reshape(-1))


def _same_pad(x, k, value):
    """[B, D, H, W] padded by k // 2 in H and W."""
    h = k // 2
    return np.pad(x, [(0, 0), (0, 0), (h, h), (h, h)], constant_values=value)


def _pool3d(x, ksize, strides, padding):
    """max_pool3d of [B, D, H, W, 1] with a window of all D planes (stride D) and k x k in space, stride 1, SAME."""
    B, D, H, W, C = x.shape
    assert padding == "SAME" and C == 1 and ksize[1] == D == strides[1] and ksize[2] == ksize[3] and list(strides[2:]) == [1, 1, 1]
    k = ksize[2]
    p = _same_pad(np.asarray(x)[..., 0], k, -np.inf)
    out = np.full((B, H, W), -np.inf, F32)
    for d in range(D):
        for dy in range(k):
            for dx in range(k):
                out = np.maximum(out, p[:, d, dy:dy + H, dx:dx + W])
    return t(out[:, None, :, :, None])


def _conv3d(x, filt, strides, padding):
    """conv3d of [B, D, H, W, 1] with a [D, k, k, 1, 1] filter, stride D over the planes and 1 in space, SAME, summed in fp32."""
    B, D, H, W, C = x.shape
    assert padding == "SAME" and C == 1 and filt.shape[0] == D == strides[1] and filt.shape[1] == filt.shape[2] and filt.shape[3:] == (1, 1)
    k = filt.shape[1]
    p = _same_pad(np.asarray(x)[..., 0], k, 0.0)
    out = np.zeros((B, H, W), F32)
    for d in range(D):
        for dy in range(k):
            for dx in range(k):
                out = (out + p[:, d, dy:dy + H, dx:dx + W] * F32(filt[d, dy, dx, 0, 0])).astype(F32)
    return t(out[:, None, :, :, None])


def _resize_images(images, size):
    """TF1 resize_images: bilinear, align_corners False, no half-pixel centres, in fp32."""
    H, W = int(size[0]), int(size[1])
    x = np.asarray(images, F32)

    def taps(n_in, n_out):
        scale = F32(n_in) / F32(n_out)
        src = (np.arange(n_out, dtype=F32) * scale).astype(F32)
        lo = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        return lo, np.minimum(lo + 1, n_in - 1), (src - lo.astype(F32)).astype(F32)
    ya, yb, fy = taps(x.shape[1], H)
    xa, xb, fx = taps(x.shape[2], W)
    fx, fy = fx[None, None, :, None], fy[None, :, None, None]
    tl, tr, bl, br = x[:, ya][:, :, xa], x[:, ya][:, :, xb], x[:, yb][:, :, xa], x[:, yb][:, :, xb]
    top = (tl + (tr - tl) * fx).astype(F32)
    bot = (bl + (br - bl) * fx).astype(F32)
    return t((top + (bot - top) * fy).astype(F32))


def _moments(x, axes, keep_dims=False):
    x = np.asarray(x, F32)
    mean = x.mean(axis=_axis(axes), keepdims=True, dtype=F32)
    var = ((x - mean) ** 2).mean(axis=_axis(axes), keepdims=True, dtype=F32)
    if not keep_dims:
        mean, var = mean.squeeze(_axis(axes)), var.squeeze(_axis(axes))
    return t(mean), t(var)


def _batch_normalization(x, mean, variance, offset, scale, variance_epsilon):
    assert offset is None and scale is None
    inv = (F32(1.0) / np.sqrt(np.asarray(variance, F32) + F32(variance_epsilon))).astype(F32)
    return t((np.asarray(x, F32) * inv + (-np.asarray(mean, F32) * inv)).astype(F32))


def _top_k(x, k, sorted=True):
    """Largest first; equal values in index order."""
    x = np.asarray(x)
    idx = np.argsort(-x.astype(np.float64), axis=-1, kind="stable")[..., :k]
    return t(np.take_along_axis(x, idx, -1)), t(idx.astype(np.int32))


def _where(cond, x=None, y=None):
    if x is None:
        return t(np.argwhere(np.asarray(cond)).astype(np.int64))
    return t(np.where(np.asarray(cond), x, y))


def _slice(x, begin, size):
    return x[tuple(slice(b, None if s == -1 else b + s) for b, s in zip(begin, size))]


def _sparse_to_dense(indices, shape, value, default, validate_indices=True):
    out = np.full(_shape(shape), default, np.int32)
    out[np.asarray(indices)] = value
    return t(out)


def _gather_nd(params, indices):
    idx = np.asarray(indices)
    return t(np.asarray(params)[tuple(idx[:, j] for j in range(idx.shape[1]))])


def _linspace(start, stop, num):
    step = (F32(stop) - F32(start)) / F32(num - 1)
    return t((F32(start) + np.arange(num, dtype=F32) * step).astype(F32))


def _cast(x, dtype):
    return t(np.asarray(x).astype(dtype))


def make_tensorflow():
    tf = types.ModuleType("tensorflow")
    tf.float32, tf.int32, tf.int64, tf.bool = np.dtype("float32"), np.dtype("int32"), np.dtype("int64"), np.dtype("bool")
    tf.name_scope = lambda *a, **k: contextlib.nullcontext()
    tf.shape = lambda x: _shape(np.shape(x))
    tf.constant = lambda v, dtype=None, shape=None: t(np.asarray(v, dtype=dtype).reshape(shape) if shape is not None else np.asarray(v, dtype=dtype))
    tf.concat = lambda values=None, axis=None, **k: t(np.concatenate([np.asarray(v) for v in values], axis=axis))
    tf.stack = lambda values, axis=0: t(np.stack([np.asarray(v) for v in values], axis=axis))
    tf.transpose = lambda a, perm=None: t(np.transpose(a, perm))
    tf.reshape = lambda x, shape: t(np.reshape(np.asarray(x), _shape(shape)))
    tf.tile = lambda x, m: t(np.tile(np.asarray(x), _shape(m)))
    tf.expand_dims = lambda x, axis: t(np.expand_dims(np.asarray(x), axis))
    tf.split = lambda x, n, axis=0: [t(v) for v in np.split(np.asarray(x), n, axis=axis)]
    tf.slice = lambda x, begin, size: t(_slice(np.asarray(x), begin, size))
    tf.pad = lambda x, paddings, mode="CONSTANT": t(np.pad(np.asarray(x), [tuple(int(v) for v in p) for p in paddings]))
    tf.ones = lambda shape, dtype=np.float32: t(np.ones(_shape(shape), dtype))
    tf.zeros = lambda shape, dtype=np.float32: t(np.zeros(_shape(shape), dtype))
    tf.ones_like = lambda x: t(np.ones_like(np.asarray(x)))
    tf.zeros_like = lambda x: t(np.zeros_like(np.asarray(x)))
    tf.eye = lambda n, m=None, dtype=np.float32: t(np.eye(n, m, dtype=dtype))
    tf.range = lambda *a, dtype=np.int32: t(np.arange(*a, dtype=dtype))
    tf.linspace = _linspace
    tf.identity = lambda x: x
    tf.stop_gradient = lambda x: x
    tf.cast = _cast
    tf.to_float = lambda x: _cast(x, F32)
    tf.exp = lambda x: t(np.exp(np.asarray(x, F32)).astype(F32))
    tf.floor = lambda x: t(np.floor(x))
    tf.mod = lambda a, b: t(np.mod(a, b))
    tf.less = lambda a, b: t(np.less(a, b))
    tf.greater = lambda a, b: t(np.greater(a, b))
    tf.greater_equal = lambda a, b: t(np.greater_equal(a, b))
    tf.logical_and = lambda a, b: t(np.logical_and(a, b))
    tf.clip_by_value = lambda x, lo, hi: t(np.clip(x, lo, hi))
    tf.where = _where
    tf.gather = lambda params, indices: t(np.asarray(params)[np.asarray(indices)])
    tf.gather_nd = _gather_nd
    tf.matmul = lambda a, b: t(np.matmul(np.asarray(a), np.asarray(b)))
    tf.add_n = lambda xs: t(sum(xs[1:], xs[0]))
    tf.reduce_max = lambda x, axis=None, keep_dims=False: t(np.max(np.asarray(x), axis=_axis(axis), keepdims=keep_dims))
    tf.reduce_sum = lambda x, axis=None, keep_dims=False: t(np.sum(np.asarray(x), axis=_axis(axis), keepdims=keep_dims, dtype=np.asarray(x).dtype))
    tf.reduce_mean = lambda x, axis=None, keep_dims=False: t(np.mean(np.asarray(x), axis=_axis(axis), keepdims=keep_dims, dtype=np.asarray(x).dtype))
    tf.sparse_to_dense = _sparse_to_dense
    tf.nn = types.SimpleNamespace(max_pool3d=_pool3d, conv3d=_conv3d, moments=_moments, batch_normalization=_batch_normalization, top_k=_top_k)
    tf.image = types.SimpleNamespace(resize_images=_resize_images)
    return tf


def reference_modules():
    """(inference, det_tools) of the reference loaded under the stand-ins, or None where the checkout does not exist."""
    root = os.path.join(R.reference_dir(), "lf-net-release")
    if not os.path.exists(os.path.join(root, "inference.py")):
        return None
    utils = types.ModuleType("utils")
    utils.embed_breakpoint = lambda *a, **k: None
    mods = load_under_stand_ins(root, [(name, name + ".py") for name in ("spatial_transformer", "det_tools", "inference")],
                                dict(tensorflow=make_tensorflow(), cv2=types.ModuleType("cv2"), utils=utils))
    return mods["inference"], mods["det_tools"]


class StoredDetector:
    """What build_multi_scale_deep_detector_3DNMS asks of a detector: build_model -> (score maps [B, h, w, 1] per scale, endpoints)."""

    def __init__(self, score_maps, ori, scale_factors, pad_size):
        self.score_maps, self.ori, self.scale_factors, self.pad_size = score_maps, ori, scale_factors, pad_size

    def build_model(self, photos, reuse=False):
        maps = [t(m[None, :, :, None].astype(F32)) for m in self.score_maps]
        return maps, dict(scale_factors=[float(s) for s in self.scale_factors], pad_size=int(self.pad_size), ori_maps=t(self.ori[None].astype(F32)))


def run_reference(inference, maps, photo, ori, scale_factors, prm):
    cfg = types.SimpleNamespace(soft_scale=True, desc_inputs="photos", **{k: (bool(v) if k in ("soft_kpts", "do_softmax_kp_refine") else v)
                                                                          for k, v in prm.items() if k != "pad_size"})
    photos = t(photo[None, :, :, None].astype(F32))
    heat, ep = inference.build_multi_scale_deep_detector_3DNMS(cfg, StoredDetector(maps, ori, scale_factors, prm["pad_size"]), photos)
    patches = inference.build_patch_extraction(cfg, ep, photos)
    top = np.argwhere(np.asarray(ep["top_ks"])[0, :, :, 0] > 0)
    kxy = np.stack([top[:, 1], top[:, 0]], -1).astype(np.int32)
    assert int(np.asarray(ep["num_kpts"])[0]) == len(kxy)
    return dict(heat=np.asarray(heat, F32)[0, :, :, 0], scale=np.asarray(ep["scale_maps"], F32)[0], kxy=kxy, kpts=np.asarray(ep["kpts"], F32),
                kscale=np.asarray(ep["kpts_scale"], F32), kori=np.asarray(ep["kpts_ori"], F32), patches=np.asarray(patches, F32)[..., 0])


def main():
    mods = reference_modules()
    if mods is None:
        raise SystemExit(f"no reference checkout at {R.reference_dir()}")
    inference, _ = mods
    out = {}
    for g, (name, H, W, sf, over, n_cases) in enumerate(R.GROUPS):
        prm = R.params(**over)
        cases, seed = [], 20270 + 1000 * g
        while len(cases) < n_cases:
            seed += 1
            assert seed < 20270 + 1000 * g + 400, f"{name}: no seed whose decisions all have a margin"
            q, qm, pq, pm, oq, om = R.make_inputs(seed, H, W, sf)
            maps, photo, ori = [R.levels(m, qm) for m in q], R.levels(pq, pm), R.levels(oq, om)
            ref = run_reference(inference, maps, photo, ori, sf, prm)
            h64, s64 = R.heatmaps(maps, sf, H, W, prm, np.float64)
            kp64, _, _, pt64, edge = R.crops(photo, ori, h64, s64, ref["kxy"], prm, np.float64)
            err = R.errors(ref["heat"], ref["scale"], ref["kpts"], ref["patches"], h64, s64, kp64, pt64, edge, sf, photo.max() - photo.min())
            cases.append(dict(seed=seed, q=q, pq=pq, oq=oq, ref=ref, err=err, h64=h64, edge=edge, mult=(qm, pm, om)))
            # the margin is judged against the bar the group ends up with; a case that fails it below is dropped and replaced
            tol_heat = 4.0 * max(c["err"]["heat"] for c in cases)
            bad = [c for c in cases if R.decision_margin(c["h64"], prm) <= 2.0 * tol_heat or c["edge"].mean() > R.EDGE_SHARE or
                   not np.array_equal(R.select(c["ref"]["heat"], prm), c["ref"]["kxy"]) or len(c["ref"]["kxy"]) == 0]
            cases = [c for c in cases if not any(c is b for b in bad)]
        tol = {k: 4.0 * max(c["err"][k] for c in cases) for k in ("heat", "scale", "kpts", "patch")}
        for i, c in enumerate(cases):
            assert all(c["err"][k] <= tol[k] for k in tol), (name, i, c["err"], tol)
            assert np.array_equal(R.select(c["h64"].astype(F32), prm), c["ref"]["kxy"]), (name, i, "fp64 heat decides differently")
            for s, m in enumerate(c["q"]):
                out[f"{name}_{i}_score{s}"] = m
            out[f"{name}_{i}_photo"], out[f"{name}_{i}_ori"] = c["pq"], c["oq"]
            for k, v in c["ref"].items():
                out[f"{name}_{i}_ref_{k}"] = v
            print(f"{name} case {i}: seed {c['seed']}, {len(c['ref']['kxy'])} keypoints, margin {R.decision_margin(c['h64'], prm):.3e}, "
                  f"edge share {c['edge'].mean():.4f}, err " + ", ".join(f"{k} {v:.3e}" for k, v in c["err"].items()))
        out[f"{name}_score_mult"], out[f"{name}_photo_mult"], out[f"{name}_ori_mult"] = cases[0]["mult"]
        for k, v in tol.items():
            out[f"tol_{name}_{k}"] = np.float64(v)
        print(f"{name}: tol " + ", ".join(f"{k} {v:.3e}" for k, v in tol.items()))
    os.makedirs(os.path.dirname(R.GOLDEN), exist_ok=True)
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
