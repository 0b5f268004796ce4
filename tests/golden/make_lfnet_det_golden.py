"""Writes tests/golden/lfnet_det/lfnet_det_reference.npz: inputs and the reference's own results for them.

    python tests/golden/make_lfnet_det_golden.py     (needs the reference checkout: BTBA_REFERENCE_DIR, see tests/lfnet_ref.py)

The reference's lf-net-release/models/mso_resnet_detector.py, common/tf_layer_utils.py and common/tf_train_utils.py are loaded by
path under the stand-in eager `tensorflow` on numpy fp32 of make_lfnet_desc_golden.py, extended here by what the detector uses:
nn.conv2d with stride 1 and SAME, image.resize_images (TF1: bilinear, no half-pixel centres), shape / to_float / cast / stack /
identity / constant (the map-size arithmetic runs in fp32 as TensorFlow runs it on a float32 tensor), nn.l2_normalize(dim=-1),
get_collection, GraphKeys and no-op summaries.  Convolutions accumulate in (ky, kx, c_in) order in fp32.  The net is then built
as mso_resnet_detector.Model.build_model builds it.  So the layers, their order, their names, where the norms and activations
sit, the scale factors, the map sizes and pad_size are the reference's own text, and what each op means is the stand-in's:
COMPOSITION FROM THE REFERENCE, OP SEMANTICS RESTATED, UNVERIFIED AGAINST A TENSORFLOW RUN (INTEGRATION.md has a TF1 snippet that
prints values stored here).  Only inputs and results are stored:
  <group>/ConvOnlyResNet/...   weights and batch-norm arrays as int8 levels, <key>@mult their fp32 multiplier
  <group>/photos               int8 levels of 1 / 127
  <group>/ref_score_<j>, <group>/ref_ori     the reference's fp32 score maps and unit orientation map
  <group>/scale_factors, <group>/pad_size, <group>/map_sizes    what the reference run reported
  tol_<group>                  4 x the largest error of the reference's fp32 result against the fp64 restatement over the group
                               (lfnet_det_ref.error: per score map relative to the map's largest value; absolute on the unit orientation
                               over the pixels whose fp64 raw norm is at least 0.05 x the frame's largest)
The file is written only if the restatement in fp32 mode is inside the bars and at most 1 % of any frame's pixels are left out of
the orientation comparison."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lfnet_det_ref as R  # noqa: E402
import lfnet_ref  # noqa: E402
import make_lfnet_desc_golden as D  # noqa: E402
from ref_loader import load_under_stand_ins  # noqa: E402

F32 = np.float32
t = D.t


class Scalar32:
    """A float32 scalar tensor: arithmetic with Python or numpy numbers converts them to fp32 first, as TensorFlow converts a
    constant to the tensor's dtype, and rounds every result to fp32."""

    def __init__(self, v):
        self.v = F32(v)

    def __mul__(self, o):
        return Scalar32(self.v * F32(o))

    def __add__(self, o):
        return Scalar32(self.v + F32(o))

    __rmul__, __radd__ = __mul__, __add__


def _conv2d(inputs, W, strides, padding="SAME", data_format="NHWC"):
    """Stride-1 SAME: k // 2 zeros on every side."""
    assert padding == "SAME" and data_format == "NHWC" and list(strides) == [1, 1, 1, 1]
    x, w = np.asarray(inputs, F32), np.asarray(W, F32)
    k = w.shape[0]
    assert w.shape[1] == k and k % 2 == 1 and w.shape[2] == x.shape[3]
    H, Wd = x.shape[1:3]
    xp = np.pad(x, [(0, 0), (k // 2, k // 2), (k // 2, k // 2), (0, 0)])
    out = np.zeros((x.shape[0], H, Wd, w.shape[3]), F32)
    for ky in range(k):
        for kx in range(k):
            for c in range(x.shape[3]):
                out = (out + (xp[:, ky:ky + H, kx:kx + Wd, c, None] * w[ky, kx, c]).astype(F32)).astype(F32)
    return t(out)


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
    top = (tl + ((tr - tl).astype(F32) * fx).astype(F32)).astype(F32)
    bot = (bl + ((br - bl).astype(F32) * fx).astype(F32)).astype(F32)
    return t((top + ((bot - top).astype(F32) * fy).astype(F32)).astype(F32))


def _l2_normalize(x, dim=None, axis=None, epsilon=1e-12):
    assert (dim if dim is not None else axis) == -1
    x = np.asarray(x, F32)
    ss = np.zeros(x.shape[:-1] + (1,), F32)
    for k in range(x.shape[-1]):
        ss = (ss + (x[..., k, None] * x[..., k, None]).astype(F32)).astype(F32)
    return t(x * (F32(1.0) / np.sqrt(np.maximum(ss, F32(epsilon)))).astype(F32))


def _cast(x, dtype):
    assert dtype == "int32" and isinstance(x, Scalar32)
    return int(np.int32(x.v))                              # truncation


def make_tensorflow(store):
    tf = D.make_tensorflow(store)
    tf.int32 = "int32"
    tf.identity = lambda x, name=None: x
    tf.constant = lambda v, dtype=None: np.asarray(v)
    tf.shape = lambda x: tuple(int(s) for s in x.shape)
    tf.to_float = Scalar32
    tf.cast = _cast
    tf.stack = list
    tf.image = types.SimpleNamespace(resize_images=_resize_images)
    tf.nn.conv2d = _conv2d
    tf.nn.l2_normalize = _l2_normalize
    return tf


def reference_modules(store):
    """(mso_resnet_detector, tf_train_utils) of the reference loaded under the stand-ins, or None where the checkout does not exist."""
    root = os.path.join(lfnet_ref.reference_dir(), "lf-net-release")
    if not os.path.exists(os.path.join(root, "models", "mso_resnet_detector.py")):
        return None
    common = types.ModuleType("common")
    common.__path__ = []
    mods = load_under_stand_ins(root, D.REFERENCE_FILES + (("mso_resnet_detector", "models/mso_resnet_detector.py"),),
                                dict(tensorflow=make_tensorflow(store), common=common))
    return mods["mso_resnet_detector"], mods["common.tf_train_utils"]


def run_reference(weights, cfg, perform_bn, use_bias, photos):
    """(score maps, unit orientation, scale factors, pad_size) of Model.build_model."""
    store = D.Store(weights)
    mods = reference_modules(store)
    if mods is None:
        raise SystemExit(f"no reference checkout at {lfnet_ref.reference_dir()}")
    detector, _ = mods
    assert abs(cfg["bn_eps"] - 1e-5) < 1e-12               # tf_batch_norm_act's constant: not a parameter of the reference
    config = types.SimpleNamespace(activ_fn="relu" if cfg["activation"] == 0 else "leaky_relu", leaky_alpha=cfg["leaky_alpha"],
                                   conv_ksize=cfg["ksize"], use_bias=use_bias, perform_bn=perform_bn, net_min_scale=cfg["min_scale"],
                                   net_max_scale=cfg["max_scale"], net_num_scales=cfg["num_scales"], net_block=cfg["blocks"],
                                   net_channel=cfg["channels"])
    logits, ep = detector.Model(config, False).build_model(t(photos[..., None]), reuse=False, name=R.SCOPE)
    assert sorted(store.asked) == sorted(weights), "the model did not read every stored variable exactly once"
    return ([np.asarray(m, F32)[..., 0] for m in logits], np.asarray(ep["ori_maps"], F32), np.asarray(ep["scale_factors"], np.float64),
            int(ep["pad_size"]))


def main():
    out = {}
    for g, (name, over, (perform_bn, use_bias), (n, H, W), big_beta) in enumerate(R.GROUPS):
        cfg = R.config(**over)
        q = R.make_model(R.MODEL_SEED + g, cfg, perform_bn, use_bias, big_beta)
        pq, pm = R.make_photos(R.PHOTO_SEED + g, n, H, W)
        weights, photos = R.model_weights(q), R.levels(pq, pm)
        ref_maps, ref_ori, ref_sf, ref_pad = run_reference(weights, cfg, perform_bn, use_bias, photos)
        assert np.array_equal(ref_sf, np.asarray(cfg["scale_factors"])) and ref_pad == R.pad_size(cfg)
        sizes = [m.shape[1:] for m in ref_maps]
        assert sizes == R.map_sizes(cfg, H, W), (sizes, R.map_sizes(cfg, H, W))
        m64, r64, u64 = R.forward(weights, cfg, photos, np.float64)
        m32, r32, u32 = R.forward(weights, cfg, photos, np.float32)
        assert u32.dtype == np.float32 and all(m.dtype == np.float32 for m in m32)
        e_ref, e_32 = R.error(ref_maps, ref_ori, m64, r64, u64), R.error(m32, u32, m64, r64, u64)
        tol = 4.0 * e_ref["worst"]
        print(f"group {name}: reference vs fp64 score {e_ref['score']:.3e} ori {e_ref['ori']:.3e}, restatement fp32 vs fp64 score {e_32['score']:.3e} "
              f"ori {e_32['ori']:.3e}, tol {tol:.3e}, left out {100 * e_ref['left_out']:.2f} %, |score| max {max(np.abs(m).max() for m in m64):.3f}, "
              f"map sizes {sizes}, pad_size {ref_pad}")
        assert e_32["worst"] <= tol, (name, e_32, tol)
        assert e_ref["left_out"] <= R.ORI_CAP, (name, e_ref["left_out"])
        assert e_ref["norm"] < 1e-6 and e_32["norm"] < 1e-6
        if big_beta:                                        # the wrong padding rule must be far outside the bar
            wrong = R.error(*R.forward(weights, cfg, photos, np.float64, pad_before_bn=True)[::2], m64, r64, u64)
            print(f"          padding before the batch norm: score {wrong['score']:.3e}, ori {wrong['ori']:.3e}")
            assert wrong["worst"] > 1e3 * tol
        for k, (lv, mult) in q.items():
            out[f"{name}/{k}"], out[f"{name}/{k}@mult"] = lv, mult
        out[f"{name}/photos"], out[f"{name}/photos@mult"] = pq, pm
        for j, m in enumerate(ref_maps):
            out[f"{name}/ref_score_{j}"] = m
        out[f"{name}/ref_ori"] = ref_ori
        out[f"{name}/scale_factors"], out[f"{name}/pad_size"] = ref_sf, np.int32(ref_pad)
        out[f"{name}/map_sizes"] = np.asarray(sizes, np.int32)
        out[f"tol_{name}"] = np.float64(tol)
    os.makedirs(os.path.dirname(R.GOLDEN), exist_ok=True)
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
