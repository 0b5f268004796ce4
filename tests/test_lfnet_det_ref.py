"""The detector net (btba_lfnet_det_*, btba_lfnet_scores) on the CPU: the numpy restatement (tests/lfnet_det_ref.py) against the
reference's own numbers (tests/golden/lfnet_det/lfnet_det_reference.npz, made under the stand-in ops of
tests/golden/make_lfnet_det_golden.py) within the stored bars, the padding rule, pad_size, the map sizes and the scale factors
through the library's host helpers, the BTBA_EINVAL of model creation that is decided before any GPU work, from_npz's missing-name
error and the struct sizes.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import lfnet_det_ref as R
from bundletrack_amd import _lib, lfnet_det


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _stored(golden, name, cfg):
    return [golden[f"{name}/ref_score_{j}"] for j in range(cfg["num_scales"])], golden[f"{name}/ref_ori"]


def test_restatement_meets_the_reference_under_the_stored_bars(golden):
    for name, over, _, (n, H, W), _ in R.GROUPS:
        cfg = R.config(**over)
        weights, photos = R.group_model(golden, name)
        assert photos.shape == (n, H, W)
        ref_maps, ref_ori = _stored(golden, name, cfg)
        m64, r64, u64 = R.forward(weights, cfg, photos, np.float64)
        m32, r32, u32 = R.forward(weights, cfg, photos, np.float32)
        assert u32.dtype == np.float32 and all(m.dtype == np.float32 for m in m32)
        tol = float(golden[f"tol_{name}"])
        assert 1e-8 < tol < 1e-4                            # the bars are those of fp32 rounding
        e_ref = R.error(ref_maps, ref_ori, m64, r64, u64)
        e_32 = R.error(m32, u32, m64, r64, u64)
        e_32_ref = R.error(m32, u32, [np.asarray(m, np.float64) for m in ref_maps], r64, np.asarray(ref_ori, np.float64))
        print(name, "reference vs fp64", e_ref, "restatement fp32 vs fp64", e_32, "restatement fp32 vs reference", e_32_ref, "tol", tol)
        assert e_ref["worst"] <= tol / 4                    # fp64 against the stored results
        assert e_32["worst"] <= tol and e_32_ref["worst"] <= tol
        for e in (e_ref, e_32):
            assert e["left_out"] <= R.ORI_CAP and e["norm"] < 1e-6
        assert np.abs(np.sqrt((u64 ** 2).sum(-1)) - 1.0).max() < 1e-12


def test_the_seeds_reproduce_the_stored_levels(golden):
    for g, (name, over, (perform_bn, use_bias), (n, H, W), big_beta) in enumerate(R.GROUPS):
        q = dict(R.make_model(R.MODEL_SEED + g, R.config(**over), perform_bn, use_bias, big_beta), photos=R.make_photos(R.PHOTO_SEED + g, n, H, W))
        stored = {k for k in golden.files if k.startswith(f"{name}/{R.SCOPE}/") and not k.endswith("@mult")} | {f"{name}/photos"}
        assert stored == {f"{name}/{k}" for k in q}
        for k, (lv, mult) in q.items():
            got, got_mult = golden[f"{name}/{k}"], golden[f"{name}/{k}@mult"]
            assert got.dtype == np.int8 and got_mult.dtype == np.float32 and np.array_equal(got, lv) and got_mult == mult, (name, k)


def test_pad_size_map_sizes_and_scale_factors_are_the_reference_runs(golden):
    for name, over, _, (n, H, W), _ in R.GROUPS:
        cfg = R.config(**over)
        assert int(golden[f"{name}/pad_size"]) == R.pad_size(cfg)
        assert [tuple(s) for s in golden[f"{name}/map_sizes"]] == R.map_sizes(cfg, H, W)
        assert np.array_equal(golden[f"{name}/scale_factors"], np.asarray(cfg["scale_factors"]))
        for j, (h, w) in enumerate(R.map_sizes(cfg, H, W)):
            assert golden[f"{name}/ref_score_{j}"].shape == (n, h, w)
        assert golden[f"{name}/ref_ori"].shape == (n, H, W, 2)
    assert R.pad_size(R.config()) == 16 and R.map_sizes(R.config(**R.GROUPS[2][1]), 24, 20) == [(24, 20), (48, 40)]


def test_zeros_pad_after_batch_norm_and_activation(golden):
    """Group b's pre-bn betas are 0.5 .. 1 in size: zeros put in before the norm become act(shift) at the border."""
    name, over, _, _, big_beta = R.GROUPS[1]
    assert big_beta
    cfg = R.config(**over)
    weights, photos = R.group_model(golden, name)
    for i in (1, 2):
        assert np.abs(weights[f"ConvOnlyResNet/block-{i}/pre-bn/beta"]).min() >= 0.5
    assert np.abs(weights["ConvOnlyResNet/fin-bn/beta"]).min() >= 0.5
    m64, r64, u64 = R.forward(weights, cfg, photos)
    wm, _, wu = R.forward(weights, cfg, photos, pad_before_bn=True)
    tol = float(golden[f"tol_{name}"])
    wrong = R.error(wm, wu, m64, r64, u64)
    print("padding before the norm:", wrong, "tol", tol)
    assert wrong["score"] > 1e3 * tol and wrong["ori"] > 1e3 * tol
    # SAME's zeros by hand: a 3 x 3 image of ones under a 3 x 3 filter of ones counts the taps inside the image
    x = np.ones((1, 3, 3, 1))
    assert R.conv(x, np.ones((3, 3, 1, 1)), np.float64)[0, :, :, 0].tolist() == [[4, 6, 4], [6, 9, 6], [4, 6, 4]]
    assert R.conv(x, np.ones((3, 3, 1, 1)), np.float32)[0, :, :, 0].tolist() == [[4, 6, 4], [6, 9, 6], [4, 6, 4]]


def test_resize_is_tf1s():
    """No half-pixel centres: src = dst * (in / out); 2 -> 4 gives taps 0, 0.5, 1, 1.5 with the upper tap clamped."""
    x = np.array([0.0, 10.0]).reshape(1, 1, 2, 1)
    assert R.resize(x, 1, 4, np.float64)[0, 0, :, 0].tolist() == [0.0, 5.0, 10.0, 10.0]
    assert R.resize(x, 1, 4, np.float32)[0, 0, :, 0].tolist() == [0.0, 5.0, 10.0, 10.0]
    assert R.resize(x, 1, 1, np.float64)[0, 0, :, 0].tolist() == [0.0]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

NEW = ("btba_lfnet_det_config_default", "btba_lfnet_det_scales", "btba_lfnet_det_model_create", "btba_lfnet_det_model_destroy",
       "btba_lfnet_det_map_size", "btba_lfnet_det_map_sizes", "btba_lfnet_det_pad_size", "btba_lfnet_scores")


def test_symbols_struct_sizes_and_defaults():
    assert set(NEW) <= set(_lib.declared_symbols()) and set(NEW) <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name)
    assert L.btba_version() == 105
    assert C.sizeof(_lib.LfnetDetConfig) == 160 and C.sizeof(_lib.LfnetDetBlock) == 3 * 48
    assert C.sizeof(_lib.LfnetDetWeights) == 48 * (1 + 3 * 8 + 1 + 16 + 1)
    txt = open(_lib.HEADER).read()
    body = re.search(r"typedef struct btba_lfnet_det_config \{(.*?)\} btba_lfnet_det_config;", txt, re.S).group(1)
    fields = re.findall(r"^\s*(?:int32_t|float|double)\s+(\w+)", body, re.M)
    assert fields == [f[0] for f in _lib.LfnetDetConfig._fields_]
    for struct, cls in (("btba_lfnet_det_block", _lib.LfnetDetBlock), ("btba_lfnet_det_weights", _lib.LfnetDetWeights)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, re.S).group(1)
        assert re.findall(r"^\s*btba_lfnet_de\w+\s+(\w+)", body, re.M) == [f[0] for f in cls._fields_]
    assert int(re.search(r"#define BTBA_LFNET_DET_MAX_BLOCKS (\d+)", txt).group(1)) == lfnet_det.MAX_BLOCKS == len(_lib.LfnetDetWeights().block)
    assert int(re.search(r"#define BTBA_LFNET_MAX_SCALES (\d+)", txt).group(1)) == lfnet_det.MAX_SCALES == len(_lib.LfnetDetWeights().score_conv)
    assert re.search(r"#define BTBA_LFNET_DET_PASS_PIXELS \(1 << 20\)", txt)
    c = _lib.lfnet_det_config()
    assert (c.channels, c.ksize, c.blocks, c.num_scales, c.activation) == (16, 5, 3, 5, 1)
    assert c.leaky_alpha == np.float32(0.2) and c.bn_eps == np.float32(1e-5)
    want = R.scales(2.0 ** -0.5, 2.0 ** 0.5, 5)
    got = np.array([c.scale_factors[j] for j in range(5)])
    assert np.abs(got - want).max() <= np.spacing(want).max() and got[0] > got[4] and got[2] == 1.0
    L.btba_lfnet_det_config_default(None)                   # a NULL is ignored
    assert L.btba_lfnet_det_pad_size(None) == -1
    c2 = _lib.lfnet_det_config(scale_factors=[1.0, 0.5])
    assert c2.num_scales == 2 and c2.scale_factors[1] == 0.5


def test_scales_within_one_ulp_of_numpys():
    for lo, hi, n in ((2.0 ** -0.5, 2.0 ** 0.5, 5), (1.0 / 8.0, 1.0, 9), (0.3, 2.0, 1)):
        got, want = lfnet_det.detector_scales(lo, hi, n), R.scales(lo, hi, n)
        print(lo, hi, n, got, "ulps", np.abs(got - want) / np.spacing(want))
        assert got.shape == want.shape and (np.abs(got - want) <= np.spacing(want)).all()
    assert lfnet_det.detector_scales(0.3, 2.0, 1).tolist() == [1.0]
    L = _lib.lib()
    out = np.zeros(16)
    for bad in ((0.0, 1.0, 3), (-1.0, 1.0, 3), (1.0, float("nan"), 3), (1.0, float("inf"), 3), (0.5, 1.0, 0), (0.5, 1.0, 17)):
        assert L.btba_lfnet_det_scales(bad[0], bad[1], bad[2], out.ctypes.data) == _lib.BTBA_EINVAL, bad
    assert L.btba_lfnet_det_scales(0.5, 1.0, 3, None) == _lib.BTBA_EINVAL


def test_map_sizes_equal_the_fp32_expression():
    L = _lib.lib()
    sf = R.scales(2.0 ** -0.5, 2.0 ** 0.5, 5)
    for H in range(1, 1025):
        for s in sf:
            want = int(np.float32(np.float32(H) * np.float32(1.0 / s)) + np.float32(0.5))
            assert L.btba_lfnet_det_map_size(float(s), H) == want == R.map_size(s, H), (H, s)
    assert L.btba_lfnet_det_map_size(1.0, 0) == -1 and L.btba_lfnet_det_map_size(0.0, 5) == -1 and L.btba_lfnet_det_map_size(float("nan"), 5) == -1
    assert L.btba_lfnet_det_map_sizes(None, 5, 5, np.zeros(16, np.int32).ctypes.data, np.zeros(16, np.int32).ctypes.data) == _lib.BTBA_EINVAL


def host_weights(cfg, seed=3, drop=(), perform_bn=True, use_bias=True):
    """An LfnetDetWeights over seeded host arrays for cfg (a dict), and the arrays themselves (to keep alive and to damage)."""
    w = R.model_weights(R.make_model(seed, cfg, perform_bn, use_bias))
    for name in drop:
        del w[name]
    return fill_weights(w, cfg), w


def fill_weights(w, cfg):
    W = _lib.LfnetDetWeights()
    S = "ConvOnlyResNet"

    def put(dst, scope, fields):
        for f in fields:
            if f"{S}/{scope}/{f}" in w:
                setattr(dst, f, w[f"{S}/{scope}/{f}"].ctypes.data)
    put(W.init_conv, "init_conv", ("weights", "biases"))
    for i in range(cfg["blocks"]):
        b = W.block[i]
        put(b.pre_bn, f"block-{i + 1}/pre-bn", R._BN)
        put(b.conv1, f"block-{i + 1}/conv1", ("weights", "biases"))
        put(b.conv1, f"block-{i + 1}/mid-bn", R._BN)
        put(b.conv2, f"block-{i + 1}/conv2", ("weights", "biases"))
    put(W.fin_bn, "fin-bn", R._BN)
    for j in range(cfg["num_scales"]):
        put(W.score_conv[j], f"score_conv_{j}", ("weights", "biases"))
    put(W.ori_conv, "ori_conv", ("weights", "biases"))
    return W


SMALL = dict(channels=16, ksize=3, blocks=2, num_scales=2)


def create_rejections(ws_handle):
    """Every BTBA_EINVAL of btba_lfnet_det_model_create; ws_handle may be a fake that is never dereferenced."""
    L = _lib.lib()
    E = _lib.BTBA_EINVAL
    cfg0 = R.config(**SMALL)
    W0, keep0 = host_weights(cfg0)
    c0 = _lib.lfnet_det_config(**R.lib_config(cfg0))
    h = C.c_void_p()
    assert L.btba_lfnet_det_model_create(None, C.byref(c0), C.byref(W0), C.byref(h)) == E
    assert L.btba_lfnet_det_model_create(ws_handle, None, C.byref(W0), C.byref(h)) == E
    assert L.btba_lfnet_det_model_create(ws_handle, C.byref(c0), None, C.byref(h)) == E
    assert L.btba_lfnet_det_model_create(ws_handle, C.byref(c0), C.byref(W0), None) == E

    def create(W, **over):
        c = _lib.lfnet_det_config(**dict(R.lib_config(cfg0), **over))
        h = C.c_void_p(7)
        rc = L.btba_lfnet_det_model_create(ws_handle, C.byref(c), C.byref(W), C.byref(h))
        assert h.value is None                              # the handle is cleared on failure
        return rc

    bad = [dict(channels=0), dict(channels=8), dict(channels=24), dict(channels=80), dict(ksize=1), dict(ksize=4), dict(ksize=7), dict(blocks=0),
           dict(blocks=9), dict(activation=-1), dict(activation=2), dict(bn_eps=float("nan")), dict(bn_eps=-1e-3), dict(bn_eps=float("inf")),
           dict(leaky_alpha=float("nan")), dict(leaky_alpha=float("inf")), dict(scale_factors=[1.0, 0.0]), dict(scale_factors=[-1.0, 1.0]),
           dict(scale_factors=[float("nan"), 1.0]), dict(scale_factors=[1.0, float("inf")])]
    for over in bad:
        assert create(W0, **over) == E, over
    for ns in (0, 17):
        c = _lib.lfnet_det_config(**R.lib_config(cfg0))
        c.num_scales = ns
        h = C.c_void_p(7)
        assert L.btba_lfnet_det_model_create(ws_handle, C.byref(c), C.byref(W0), C.byref(h)) == E and h.value is None
    # the arrays
    for layer in ("init_conv", "block-1/conv1", "block-2/conv2", "score_conv_1", "ori_conv"):
        W, keep = host_weights(cfg0, drop=(f"ConvOnlyResNet/{layer}/weights",))
        assert create(W) == E, layer
    for drop in ("block-1/pre-bn/moving_mean", "block-2/mid-bn/moving_variance", "fin-bn/moving_mean"):
        W, keep = host_weights(cfg0, drop=("ConvOnlyResNet/" + drop,))
        assert create(W) == E, drop                         # only one of the two moving arrays
    for name in ("init_conv/weights", "init_conv/biases", "block-1/pre-bn/gamma", "block-1/conv1/weights", "block-1/mid-bn/beta",
                 "block-2/conv2/biases", "block-2/pre-bn/moving_mean", "fin-bn/moving_variance", "score_conv_0/weights", "score_conv_1/biases",
                 "ori_conv/weights", "ori_conv/biases"):
        for poison in (np.nan, np.inf, -np.inf):
            W, keep = host_weights(cfg0)
            keep["ConvOnlyResNet/" + name].reshape(-1)[-1] = poison
            assert create(W) == E, (name, poison)
    W, keep = host_weights(cfg0)
    keep["ConvOnlyResNet/block-2/pre-bn/moving_variance"][3] = -1.0      # variance + eps <= 0
    assert create(W) == E
    W, keep = host_weights(cfg0)
    keep["ConvOnlyResNet/fin-bn/moving_variance"][3] = 0.0
    assert create(W, bn_eps=0.0) == E


def test_create_rejects_bad_arguments_before_any_gpu_work():
    create_rejections(C.c_void_p(1))                        # never dereferenced: every case fails validation first


def test_from_npz_lists_what_it_expected(tmp_path):
    cfg = R.config(**SMALL)
    w = R.model_weights(R.make_model(1, cfg))
    names = lfnet_det.expected_names(2, 2)
    assert names == sorted(w, key=names.index) and len(names) == len(w)
    del w["ConvOnlyResNet/block-2/mid-bn/moving_mean"]
    path = str(tmp_path / "det.npz")
    np.savez(path, **w)
    with pytest.raises(KeyError) as e:
        lfnet_det.LfnetScoreNet.from_npz(None, path)
    msg = str(e.value)
    assert "missing ['ConvOnlyResNet/block-2/mid-bn/moving_mean']" in msg
    for name in names:
        assert name in msg
    plain = lfnet_det.expected_names(1, 1, perform_bn=False, use_bias=False)
    assert plain == ["ConvOnlyResNet/init_conv/weights", "ConvOnlyResNet/block-1/conv1/weights", "ConvOnlyResNet/block-1/conv2/weights",
                     "ConvOnlyResNet/score_conv_0/weights", "ConvOnlyResNet/ori_conv/weights", "ConvOnlyResNet/ori_conv/biases"]
    full = R.model_weights(R.make_model(1, cfg))
    c = lfnet_det.config_from_weights(full, activation=0)
    assert (c.channels, c.ksize, c.blocks, c.num_scales, c.activation) == (16, 3, 2, 2, 0)
    assert c.scale_factors[0] == pytest.approx(2.0 ** 0.5) and c.scale_factors[1] == pytest.approx(2.0 ** -0.5)
