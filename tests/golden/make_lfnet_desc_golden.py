"""Writes tests/golden/lfnet_desc/lfnet_desc_reference.npz: inputs and the reference's own results for them.

    python tests/golden/make_lfnet_desc_golden.py     (needs the reference checkout: BTBA_REFERENCE_DIR, see tests/lfnet_ref.py)

The reference's lf-net-release/models/simple_desc.py, common/tf_layer_utils.py and common/tf_train_utils.py are loaded by path
under stand-in modules of this project's own writing: a `det_tools` with the one name simple_desc.py imports, and an eager
`tensorflow` on numpy fp32 (below) that covers what get_model uses: variable scopes with get_variable served from the stored
weights, nn.conv2d with TensorFlow's SAME rule, bias_add, layers.batch_normalization in inference, layers.flatten, matmul,
nn.l2_normalize, relu and leaky relu, no-op summaries.  Convolutions, matrix products and the sum of squares accumulate in k order
in fp32.  get_model is then called as Model.build_model calls it.  So the layers, their order, their names, the flatten and what
is normalised are the reference's own text, and what each op means is the stand-in's: COMPOSITION FROM THE REFERENCE, OP SEMANTICS
RESTATED, UNVERIFIED AGAINST A TENSORFLOW RUN (INTEGRATION.md has a TF1 snippet that prints values stored here).  Only inputs and
results are stored:
  <group>/SimpleDesc/...   weights and batch-norm arrays as int8 levels, <key>@mult their fp32 multiplier
  <group>/patches          int8 levels of 1 / 127
  <group>/ref_desc, <group>/ref_raw    the reference's fp32 norm_feats and raw_feats
  tol_<group>              4 x the largest difference between the reference's fp32 result and the fp64 restatement over the group
                           (lfnet_desc_ref.error: absolute on unit-norm descriptors, relative to the case's largest |raw| without norm)
Every op is continuous, so no case is left out; the file is written only if the restatement in fp32 mode is inside the bars.
Two places where a group is not get_model's text as it stands: get_model asks for 512 outputs of fc1 whatever the configuration, and
the store hands out the stored, narrower array (Store.get_variable); and get_model switches batch norm and biases for all layers at
once, so the group without them (c) has neither in any layer."""
import contextlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lfnet_desc_ref as R  # noqa: E402
import lfnet_ref  # noqa: E402
from ref_loader import load_under_stand_ins  # noqa: E402

F32 = np.float32
REFERENCE_FILES = (("common.tf_layer_utils", "common/tf_layer_utils.py"), ("common.tf_train_utils", "common/tf_train_utils.py"))


class Dim(int):
    value = property(int)


class Shape(tuple):
    ndims = property(len)

    def as_list(self):
        return list(self)


class T(np.ndarray):
    def get_shape(self):
        return Shape(Dim(s) for s in self.shape)


def t(x):
    return np.asarray(x, F32).view(T)


def _conv2d(inputs, W, strides, padding="SAME", data_format="NHWC"):
    """Stride-2 SAME: out = ceil(in / 2), total = max((out - 1) * 2 + k - in, 0), before = total // 2, the rest after."""
    assert padding == "SAME" and data_format == "NHWC" and list(strides) == [1, 2, 2, 1]
    x, w = np.asarray(inputs, F32), np.asarray(W, F32)
    k = w.shape[0]
    assert w.shape[1] == k and w.shape[2] == x.shape[3]

    def pads(n):
        out = -(-n // 2)
        total = max((out - 1) * 2 + k - n, 0)
        return out, total // 2, total - total // 2
    (Ho, hb, ha), (Wo, wb, wa) = pads(x.shape[1]), pads(x.shape[2])
    xp = np.pad(x, [(0, 0), (hb, ha), (wb, wa), (0, 0)])
    out = np.zeros((x.shape[0], Ho, Wo, w.shape[3]), F32)
    for ky in range(k):
        for kx in range(k):
            for c in range(x.shape[3]):
                out = (out + (xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, c, None] * w[ky, kx, c]).astype(F32)).astype(F32)
    return t(out)


def _matmul(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    out = np.zeros((a.shape[0], b.shape[1]), F32)
    for k in range(a.shape[1]):
        out = (out + (a[:, k, None] * b[k]).astype(F32)).astype(F32)
    return t(out)


def _l2_normalize(x, dim=None, axis=None, epsilon=1e-12):
    assert (dim if dim is not None else axis) == 1
    x = np.asarray(x, F32)
    ss = np.zeros((x.shape[0], 1), F32)
    for k in range(x.shape[1]):
        ss = (ss + (x[:, k, None] * x[:, k, None]).astype(F32)).astype(F32)
    return t(x * (F32(1.0) / np.sqrt(np.maximum(ss, F32(epsilon)))).astype(F32))


class Store:
    """The variable store: scopes nest by name, get_variable hands out the stored array of the full name."""

    def __init__(self, variables):
        self.variables, self.scope, self.asked = variables, [], []

    @contextlib.contextmanager
    def variable_scope(self, name, reuse=None):
        self.scope.append(name)
        try:
            yield types.SimpleNamespace(name="/".join(self.scope))
        finally:
            self.scope.pop()

    def get_variable(self, name, shape=None, initializer=None, dtype=F32):
        full = "/".join(self.scope + [name])
        v = self.variables[full]                           # KeyError: the model asks for a variable that was not stored
        # get_model asks for 512 outputs of fc1 whatever the configuration; the stored groups are narrower (the file has to stay
        # small), so the width is the stored array's: the one place where a group departs from the reference's text
        assert shape is None or tuple(shape)[:-1] == v.shape[:-1], (full, shape, v.shape)
        assert shape is None or tuple(shape) == v.shape or full in (R.SCOPE + "/fc1/weights", R.SCOPE + "/fc1/biases"), (full, shape, v.shape)
        self.asked.append(full)
        return t(v)

    def batch_normalization(self, inputs, axis=-1, momentum=0.99, epsilon=1e-3, center=True, scale=True, training=False, trainable=True,
                            fused=None, name=None):
        """Inference: (x - moving_mean) * (gamma * rsqrt(moving_variance + epsilon)) + beta, every step in fp32."""
        assert training is False and axis == -1 and center and scale
        with self.variable_scope(name):
            gamma, beta = self.get_variable("gamma"), self.get_variable("beta")
            mean, var = self.get_variable("moving_mean"), self.get_variable("moving_variance")
        inv = ((F32(1.0) / np.sqrt((np.asarray(var) + F32(epsilon)).astype(F32))).astype(F32) * np.asarray(gamma)).astype(F32)
        return t(((np.asarray(inputs, F32) - np.asarray(mean)).astype(F32) * inv).astype(F32) + np.asarray(beta))


def make_tensorflow(store):
    tf = types.ModuleType("tensorflow")
    tf.float32 = np.dtype("float32")
    tf.variable_scope = store.variable_scope
    tf.get_variable = store.get_variable
    tf.zeros_initializer = lambda *a, **k: None
    tf.ones_initializer = lambda *a, **k: None
    tf.variance_scaling_initializer = lambda *a, **k: None
    tf.contrib = types.SimpleNamespace(layers=types.SimpleNamespace(xavier_initializer=lambda *a, **k: None))
    tf.summary = types.SimpleNamespace(histogram=lambda *a, **k: None, scalar=lambda *a, **k: None)
    tf.GraphKeys = types.SimpleNamespace(TRAINABLE_VARIABLES="trainable_variables")
    tf.get_collection = lambda *a, **k: []
    tf.matmul = _matmul
    tf.nn = types.SimpleNamespace(
        conv2d=_conv2d,
        bias_add=lambda x, b, data_format=None: t(np.asarray(x, F32) + np.asarray(b, F32)),
        relu=lambda x, name=None: t(np.maximum(np.asarray(x, F32), F32(0.0))),
        leaky_relu=lambda x, alpha=0.2, name=None: t(np.maximum(np.asarray(x, F32), (np.asarray(x, F32) * F32(alpha)).astype(F32))),
        l2_normalize=_l2_normalize)
    tf.layers = types.SimpleNamespace(batch_normalization=store.batch_normalization,
                                      flatten=lambda x: t(np.ascontiguousarray(x).reshape(x.shape[0], -1)))
    return tf


def reference_modules(store):
    """(simple_desc, tf_train_utils) of the reference loaded under the stand-ins, or None where the checkout does not exist."""
    root = os.path.join(lfnet_ref.reference_dir(), "lf-net-release")
    if not os.path.exists(os.path.join(root, "models", "simple_desc.py")):
        return None
    det_tools = types.ModuleType("det_tools")

    def instance_normalization(*a, **k):
        raise NotImplementedError("feat_norm='inst' is not covered")
    det_tools.instance_normalization = instance_normalization
    common = types.ModuleType("common")
    common.__path__ = []
    mods = load_under_stand_ins(root, REFERENCE_FILES + (("simple_desc", "models/simple_desc.py"),),
                                dict(tensorflow=make_tensorflow(store), det_tools=det_tools, common=common))
    return mods["simple_desc"], mods["common.tf_train_utils"]


def run_reference(weights, cfg, perform_bn, use_bias, patches):
    """norm_feats and raw_feats of get_model, called as simple_desc.Model.build_model calls it."""
    store = Store(weights)
    mods = reference_modules(store)
    if mods is None:
        raise SystemExit(f"no reference checkout at {lfnet_ref.reference_dir()}")
    simple_desc, train_utils = mods
    act = train_utils.get_activation_fn("relu" if cfg["activation"] == 0 else "leaky_relu", alpha=cfg["leaky_alpha"])
    assert abs(cfg["bn_eps"] - 1e-5) < 1e-12               # tf_batch_norm_act's constant: not a parameter of the reference
    feats, ep = simple_desc.get_model(t(patches[..., None]), False, out_dim=cfg["out_dim"], init_num_channels=cfg["channels"],
                                      num_conv_layers=cfg["depth"], conv_ksize=3, activation_fn=act, perform_bn=perform_bn,
                                      use_bias=use_bias, feat_norm="l2norm" if cfg["norm"] == 0 else "non", reuse=False, name=R.SCOPE)
    assert sorted(store.asked) == sorted(weights), "the model did not read every stored variable exactly once"
    return np.asarray(feats, F32), np.asarray(ep["raw_feats"], F32)


def main():
    out = {}
    for g, (name, over, (perform_bn, use_bias), m) in enumerate(R.GROUPS):
        cfg = R.config(**over)
        q = R.make_model(R.MODEL_SEED + g, cfg, perform_bn, use_bias)
        pq, pm = R.make_patches(R.PATCH_SEED + g, m, cfg["patch_size"])
        weights, patches = R.model_weights(q), R.levels(pq, pm)
        ref_desc, ref_raw = run_reference(weights, cfg, perform_bn, use_bias, patches)
        d64, r64 = R.forward(weights, cfg, patches, np.float64)
        d32, r32 = R.forward(weights, cfg, patches, np.float32)
        assert d32.dtype == np.float32
        err_ref = max(R.error(ref_desc[i:i + 1], ref_raw[i:i + 1], d64[i:i + 1], r64[i:i + 1], cfg) for i in range(m))
        err_32 = max(R.error(d32[i:i + 1], r32[i:i + 1], d64[i:i + 1], r64[i:i + 1], cfg) for i in range(m))
        tol = 4.0 * err_ref
        print(f"group {name}: reference vs fp64 {err_ref:.3e}, restatement fp32 vs fp64 {err_32:.3e}, tol {tol:.3e}, "
              f"|raw| max {np.abs(r64).max():.3f}, live outputs {np.mean(np.abs(r64) > 0):.2f}")
        assert err_32 <= tol, (name, err_32, tol)
        assert np.abs(r64).max() > 1e-3 and np.mean(np.abs(d64) > 1e-4) > 0.5, "a layer has collapsed"
        for k, (lv, mult) in q.items():
            out[f"{name}/{k}"], out[f"{name}/{k}@mult"] = lv, mult
        out[f"{name}/patches"], out[f"{name}/patches@mult"] = pq, pm
        out[f"{name}/ref_desc"], out[f"{name}/ref_raw"] = ref_desc, ref_raw
        out[f"tol_{name}"] = np.float64(tol)
    os.makedirs(os.path.dirname(R.GOLDEN), exist_ok=True)
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
