"""The descriptor net (btba_lfnet_desc_*, btba_lfnet_descriptors) on the CPU: the numpy restatement (tests/lfnet_desc_ref.py) against
the reference's own numbers (tests/golden/lfnet_desc/lfnet_desc_reference.npz, made under the stand-in ops of
tests/golden/make_lfnet_desc_golden.py) within the stored bars, TensorFlow's SAME rule and the flatten order by hand, every
BTBA_EINVAL that is decided before any GPU work, from_npz's missing-name error and the struct sizes.  No GPU."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import lfnet_desc_ref as R
import lfnet_net_ref
from bundletrack_amd import _lib, lfnet_desc


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def test_fp64_restatement_meets_the_reference_under_the_stored_bars(golden):
    n = 0
    for name, over, _, m in R.GROUPS:
        cfg = R.config(**over)
        weights, patches = R.group_model(golden, name)
        assert patches.shape == (m, cfg["patch_size"], cfg["patch_size"])
        d64, r64 = R.forward(weights, cfg, patches, np.float64)
        d32, r32 = R.forward(weights, cfg, patches, np.float32)
        assert d32.dtype == np.float32
        tol = float(golden[f"tol_{name}"])
        assert 1e-8 < tol < 1e-5                            # the bars are those of fp32 rounding
        for i in range(m):
            s = slice(i, i + 1)
            e_ref = R.error(golden[f"{name}/ref_desc"][s], golden[f"{name}/ref_raw"][s], d64[s], r64[s], cfg)
            e_32 = R.error(d32[s], r32[s], d64[s], r64[s], cfg)
            print(name, i, "reference", e_ref, "restatement fp32", e_32, "tol", tol)
            assert e_ref <= tol and e_32 <= tol, (name, i, e_ref, e_32, tol)
            n += 1
        if cfg["norm"] == 0:
            assert np.abs(np.linalg.norm(d64, axis=1) - 1.0).max() < 1e-12
        else:
            assert np.array_equal(d64, r64)
    assert n == 15


def test_the_seeds_reproduce_the_stored_levels(golden):
    for g, (name, over, (perform_bn, use_bias), m) in enumerate(R.GROUPS):
        cfg = R.config(**over)
        q = dict(R.make_model(R.MODEL_SEED + g, cfg, perform_bn, use_bias), patches=R.make_patches(R.PATCH_SEED + g, m, cfg["patch_size"]))
        stored = {k for k in golden.files if k.startswith(f"{name}/{R.SCOPE}/") and not k.endswith("@mult")} | {f"{name}/patches"}
        assert stored == {f"{name}/{k}" for k in q}
        for k, (lv, mult) in q.items():
            got, got_mult = golden[f"{name}/{k}"], golden[f"{name}/{k}@mult"]
            assert got.dtype == np.int8 and got_mult.dtype == np.float32 and np.array_equal(got, lv) and got_mult == mult, (name, k)


def test_a_wrong_padding_rule_or_flatten_order_is_far_outside_the_bars(golden):
    name, over, _, _ = R.GROUPS[0]
    cfg = R.config(**over)
    weights, patches = R.group_model(golden, name)
    d64, r64 = R.forward(weights, cfg, patches)
    tol = float(golden[f"tol_{name}"])
    # symmetric padding (what torch's padding=1 does): every window moves by one pixel
    assert R.error(*R.forward(weights, cfg, np.roll(patches, (1, 1), (1, 2))), d64, r64, cfg) > 1e3 * tol
    # flatten in (c, h, w) order: fc1's rows permuted
    side, c = cfg["patch_size"] >> cfg["depth"], cfg["channels"] << (cfg["depth"] - 1)
    wrong = dict(weights)
    wrong["SimpleDesc/fc1/weights"] = weights["SimpleDesc/fc1/weights"].reshape(side, side, c, -1).transpose(2, 0, 1, 3).reshape(side * side * c, -1)
    assert R.error(*R.forward(wrong, cfg, patches), d64, r64, cfg) > 1e3 * tol


def test_same_rule_pads_after_not_before():
    assert R.same_pads(4) == (2, 0, 1) and R.same_pads(32) == (16, 0, 1) and R.same_pads(5) == (3, 1, 1) and R.same_pads(1) == (1, 1, 1)
    # hand-computed 4 x 4: x = 1 .. 16 in raster order, all-ones 3 x 3 filter.  Windows start at rows / columns 0 and 2 and run one
    # past the edge: (0,0) = rows 0-2 x cols 0-2 = 1+2+3+5+6+7+9+10+11 = 54, (0,1) = cols 2-3 = 3+4+7+8+11+12 = 45,
    # (1,0) = rows 2-3 x cols 0-2 = 9+10+11+13+14+15 = 72, (1,1) = 11+12+15+16 = 54
    x = np.arange(1.0, 17.0).reshape(1, 4, 4, 1)
    out = R.conv(x, np.ones((3, 3, 1, 1)), np.float64)
    assert np.array_equal(out[0, :, :, 0], [[54.0, 45.0], [72.0, 54.0]])
    assert np.array_equal(R.conv(x, np.ones((3, 3, 1, 1)), np.float32)[0, :, :, 0], [[54.0, 45.0], [72.0, 54.0]])
    # with a "before" pad the top-left window would be rows -1 .. 1: 1+2+5+6 = 14
    assert out[0, 0, 0, 0] != 14.0
    # an impulse in the last row / column reaches the output through the filter's first taps of the last window only
    w = np.arange(1.0, 10.0).reshape(3, 3, 1, 1)
    for (iy, ix), want in (((3, 3), {(1, 1): w[1, 1]}), ((3, 0), {(1, 0): w[1, 0]}), ((0, 3), {(0, 1): w[0, 1]}),
                           ((0, 0), {(0, 0): w[0, 0]}), ((2, 2), {(0, 0): w[2, 2], (0, 1): w[2, 0], (1, 0): w[0, 2], (1, 1): w[0, 0]})):
        imp = np.zeros((1, 4, 4, 1))
        imp[0, iy, ix, 0] = 1.0
        got = R.conv(imp, w, np.float64)[0, :, :, 0]
        exp = np.zeros((2, 2))
        for k, v in want.items():
            exp[k] = v[0, 0]
        assert np.array_equal(got, exp), (iy, ix)
    # an odd size pads one before: the impulse at (0, 0) is then the window's centre tap
    imp = np.zeros((1, 5, 5, 1))
    imp[0, 0, 0, 0] = 1.0
    assert R.conv(imp, w, np.float64)[0, 0, 0, 0] == w[1, 1, 0, 0]


def test_flatten_is_h_w_c():
    x = np.arange(2 * 2 * 3 * 4).reshape(2, 2, 3, 4)
    f = R.flatten(x)
    assert f.shape == (2, 24) and f[1, (1 * 3 + 2) * 4 + 3] == x[1, 1, 2, 3] and np.array_equal(f[0, :4], x[0, 0, 0])


def test_l2_normalize_floor():
    raw = np.array([[3.0, 4.0], [0.0, 0.0], [1e-8, 0.0]])
    out = R.l2_normalize(raw, np.float64)
    assert np.allclose(out[0], [0.6, 0.8]) and np.array_equal(out[1], [0.0, 0.0]) and out[2, 0] == pytest.approx(1e-8 / 1e-6)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

NEW = ("btba_lfnet_desc_config_default", "btba_lfnet_desc_model_create", "btba_lfnet_desc_model_destroy", "btba_lfnet_descriptors")


def test_symbols_struct_sizes_and_defaults():
    assert set(NEW) <= set(_lib.declared_symbols()) and set(NEW) <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name)
    assert L.btba_version() == 105
    assert C.sizeof(_lib.LfnetDescConfig) == 36 and C.sizeof(_lib.LfnetDescLayer) == 48 and C.sizeof(_lib.LfnetDescWeights) == 6 * 48
    txt = open(_lib.HEADER).read()
    body = re.search(r"typedef struct btba_lfnet_desc_config \{(.*?)\} btba_lfnet_desc_config;", txt, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|float)\s+(\w+);", body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in _lib.LfnetDescConfig._fields_]
    assert [{"int32_t": C.c_int32, "float": C.c_float}[f[0]] for f in fields] == [f[1] for f in _lib.LfnetDescConfig._fields_]
    body = re.search(r"typedef struct btba_lfnet_desc_layer \{(.*?)\} btba_lfnet_desc_layer;", txt, re.S).group(1)
    assert re.findall(r"\*(\w+)", body) == [f[0] for f in _lib.LfnetDescLayer._fields_]
    assert int(re.search(r"#define BTBA_LFNET_DESC_MAX_DEPTH (\d+)", txt).group(1)) == lfnet_desc.MAX_DEPTH == len(_lib.LfnetDescWeights().conv)
    c = _lib.lfnet_desc_config()
    assert (c.patch_size, c.depth, c.channels, c.fc_dim, c.out_dim, c.activation, c.norm) == (32, 3, 64, 512, 256, 0, 0)
    assert c.leaky_alpha == np.float32(0.2) and c.bn_eps == np.float32(1e-5)
    L.btba_lfnet_desc_config_default(None)                  # a NULL is ignored


def _host_weights(cfg, seed=3, drop=()):
    """An LfnetDescWeights over seeded host arrays for cfg (a dict), the arrays themselves (to keep alive and to damage)."""
    w = R.model_weights(R.make_model(seed, cfg))
    for name in drop:
        del w[name]
    W = _lib.LfnetDescWeights()
    for i, (layer, bn) in enumerate(R.layer_scopes(cfg["depth"])):
        dst = W.conv[i] if i < cfg["depth"] else (W.fc1 if layer == "fc1" else W.fc2)
        for field, name in [("weights", f"SimpleDesc/{layer}/weights"), ("biases", f"SimpleDesc/{layer}/biases")] + \
                           ([(k, f"SimpleDesc/{bn}/{k}") for k in ("gamma", "beta", "moving_mean", "moving_variance")] if bn else []):
            if name in w:
                setattr(dst, field, w[name].ctypes.data)
    return W, w


SMALL = dict(patch_size=16, depth=2, channels=16, fc_dim=32, out_dim=16)


def test_create_rejects_bad_arguments_before_any_gpu_work():
    L = _lib.lib()
    fake = C.c_void_p(1)                                    # never dereferenced: every case fails validation first
    E = _lib.BTBA_EINVAL

    def create(ws=fake, cfg=None, W=None, out=True, **over):
        cfg = R.config(**dict(SMALL, **over)) if cfg is None else cfg
        Wd, keep = _host_weights(cfg) if W is None else (W, None)
        c = _lib.lfnet_desc_config(**cfg)
        h = C.c_void_p(7)
        rc = L.btba_lfnet_desc_model_create(ws, C.byref(c), C.byref(Wd), C.byref(h) if out else None)
        assert not out or h.value is None                   # the handle is cleared on failure
        return rc

    cfg0 = R.config(**SMALL)
    W0, keep0 = _host_weights(cfg0)
    c0 = _lib.lfnet_desc_config(**cfg0)
    h = C.c_void_p()
    assert L.btba_lfnet_desc_model_create(None, C.byref(c0), C.byref(W0), C.byref(h)) == E
    assert L.btba_lfnet_desc_model_create(fake, None, C.byref(W0), C.byref(h)) == E
    assert L.btba_lfnet_desc_model_create(fake, C.byref(c0), None, C.byref(h)) == E
    assert L.btba_lfnet_desc_model_create(fake, C.byref(c0), C.byref(W0), None) == E
    # the configuration: every field's range (the weights pointers are valid for the SMALL shape; a rejected configuration is
    # rejected before any array is read)
    bad = [dict(patch_size=4), dict(patch_size=68), dict(patch_size=72), dict(patch_size=18), dict(patch_size=24, depth=4), dict(depth=0), dict(depth=5),
           dict(channels=0), dict(channels=8), dict(channels=24), dict(channels=144), dict(fc_dim=0), dict(fc_dim=40), dict(fc_dim=1040),
           dict(out_dim=0), dict(out_dim=8), dict(out_dim=24), dict(out_dim=528), dict(activation=-1), dict(activation=2), dict(norm=-1), dict(norm=2),
           dict(bn_eps=float("nan")), dict(bn_eps=-1e-3), dict(bn_eps=float("inf")), dict(leaky_alpha=float("nan")),
           dict(patch_size=64, depth=1, channels=128)]      # flatten 32 * 32 * 128 > 16384
    for over in bad:
        c = _lib.lfnet_desc_config(**dict(cfg0, **over))
        h = C.c_void_p(7)
        assert L.btba_lfnet_desc_model_create(fake, C.byref(c), C.byref(W0), C.byref(h)) == E and h.value is None, over
    # the arrays
    for layer in ("conv1", "conv2", "fc1", "fc2"):
        W, keep = _host_weights(cfg0, drop=(f"SimpleDesc/{layer}/weights",))
        assert create(W=W) == E, layer
    for drop in ("SimpleDesc/bn1/moving_mean", "SimpleDesc/bn2/moving_variance", "SimpleDesc/fc-bn1/moving_mean"):
        W, keep = _host_weights(cfg0, drop=(drop,))
        assert create(W=W) == E, drop                       # only one of the two moving arrays
    for name in ("SimpleDesc/conv1/weights", "SimpleDesc/conv2/biases", "SimpleDesc/bn1/gamma", "SimpleDesc/bn2/beta", "SimpleDesc/fc-bn1/moving_mean",
                 "SimpleDesc/bn1/moving_variance", "SimpleDesc/fc1/weights", "SimpleDesc/fc2/weights", "SimpleDesc/fc2/biases"):
        for poison in (np.nan, np.inf, -np.inf):
            W, keep = _host_weights(cfg0)
            keep[name].reshape(-1)[-1] = poison
            assert create(W=W) == E, (name, poison)
    W, keep = _host_weights(cfg0)
    keep["SimpleDesc/bn2/moving_variance"][3] = -1.0        # variance + eps <= 0
    assert create(W=W) == E
    W, keep = _host_weights(cfg0)
    keep["SimpleDesc/bn2/moving_variance"][3] = 0.0
    assert create(W=W, bn_eps=0.0) == E


def test_weights_layer_verdicts_and_fold_bits_under_sanitizers(tmp_path):
    """bundletrack_amd/csrc/btba_lfnet_weights.hpp alone, in tests/cpp/lfnet_weights_host.cpp built with AddressSanitizer and
    UBSan: the verdicts of lfnet_conv_ok and lfnet_bn_ok are the rules of include/btba.h, lfnet_fold's bits are float32 of
    lfnet_net_ref.fold, and the sanitizers report nothing (the arrays are heap blocks of exactly N, or K * N, floats)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "lfnet_weights_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "lfnet_weights_host.cpp"), "-o", exe])
    names = ("weights", "biases") + lfnet_net_ref.BN
    K = 9
    cases = []                                              # (N, eps, {array name: float32 array})

    def arrays(N, have, seed):
        rs = np.random.default_rng(seed)
        a = dict(weights=rs.standard_normal(K * N), biases=rs.standard_normal(N), gamma=rs.uniform(0.5, 1.5, N), beta=rs.standard_normal(N),
                 moving_mean=rs.standard_normal(N), moving_variance=rs.uniform(0.5, 2.0, N))
        return {k: v.astype(np.float32) for k, v in a.items() if k in have}

    bn_sets = (lfnet_net_ref.BN, ("moving_mean", "moving_variance"), ())
    for N, bn, bias in itertools.product((16, 2), bn_sets, (True, False)):
        have = ("weights",) + (("biases",) if bias else ()) + tuple(bn)
        cases.append((N, 1e-5, arrays(N, have, len(cases))))
        for name in have:                                   # one NaN in the last element of each array in turn
            a = arrays(N, have, len(cases))
            a[name][-1] = np.nan
            cases.append((N, 1e-5, a))
    for N in (16, 2):
        a = arrays(N, names, len(cases))
        a["moving_variance"][-1] = 0.0                      # variance + eps == 0, with and without an eps
        cases.append((N, 0.0, a))
        a = arrays(N, names, len(cases))
        a["moving_variance"][-1] = -np.float32(1e-5)
        cases.append((N, 1e-5, a))
        for only in ("moving_mean", "moving_variance"):     # one moving array without the other
            cases.append((N, 1e-5, arrays(N, ("weights", "biases", "gamma", "beta", only), len(cases))))
        cases.append((N, 1e-5, arrays(N, names[1:], len(cases))))      # no weights
    assert len(cases) == 2 * (27 + 5)                      # per size: 6 layouts and a NaN per array of each, 5 refusals more

    bits = lambda a: " ".join(f"{b:08x}" for b in np.asarray(a, np.float32).reshape(-1).view(np.uint32))
    text = "".join(f"{K} {N} {bits(eps)} " + " ".join(str(int(k in a)) for k in names) + " " + " ".join(bits(a[k]) for k in names if k in a) + "\n"
                   for N, eps, a in cases)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    n_ok = 0
    for (N, eps, a), line in zip(cases, lines):
        finite = lambda k: bool(np.isfinite(a[k]).all())
        conv_ok = "weights" in a and finite("weights") and ("biases" not in a or finite("biases"))
        bn_ok = ("moving_mean" in a) == ("moving_variance" in a)
        if bn_ok and "moving_mean" in a:
            bn_ok = all(finite(k) for k in lfnet_net_ref.BN if k in a) and \
                bool((a["moving_variance"].astype(np.float64) + np.float64(np.float32(eps)) > 0.0).all())
        words = line.split()
        assert (int(words[0]), int(words[1])) == (int(conv_ok), int(bn_ok)), (N, eps, sorted(a), line[:40])
        if not bn_ok:
            assert len(words) == 2
            continue
        got = np.array([int(w, 16) for w in words[2:]], np.uint32).view(np.float32).reshape(2, N)
        w = {f"S/bn/{k}": a[k] for k in lfnet_net_ref.BN if k in a}
        want = np.stack(lfnet_net_ref.fold(w, "S", "bn", N, eps, a.get("biases"))).astype(np.float32)
        np.testing.assert_array_equal(got, want)           # NaN (a refused bias) equals NaN
        if conv_ok:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, eps, sorted(a))
            n_ok += 1
    assert n_ok == 2 * 3 * 2                                # every accepted layout at both sizes


def test_descriptors_rejects_bad_arguments_before_any_gpu_work():
    L = _lib.lib()
    fake, model, E = C.c_void_p(1), C.c_void_p(1), _lib.BTBA_EINVAL
    p, d, k = C.c_void_p(1 << 12), C.c_void_p(1 << 13), C.c_void_p(1 << 14)
    call = L.btba_lfnet_descriptors
    assert call(None, model, 1, 5, p, k, d) == E and call(fake, None, 1, 5, p, k, d) == E
    assert call(fake, model, -1, 5, p, k, d) == E and call(fake, model, 1, -5, p, k, d) == E
    assert call(fake, model, 1, 2049, p, k, d) == E and call(fake, model, 1 << 20, 2048, p, k, d) == E
    assert call(fake, model, 0, 5, p, k, d) == _lib.BTBA_OK and call(fake, model, 3, 0, None, None, None) == _lib.BTBA_OK      # nothing to do
    assert call(fake, model, 1, 5, None, k, d) == E and call(fake, model, 1, 5, p, k, None) == E
    assert call(fake, model, 1, 5, C.c_void_p((1 << 12) + 2), k, d) == E and call(fake, model, 1, 5, p, k, C.c_void_p((1 << 13) + 1)) == E
    assert call(fake, model, 1, 5, p, C.c_void_p((1 << 14) + 2), d) == E


def test_from_npz_lists_what_it_expected(tmp_path):
    cfg = R.config(**SMALL)
    w = R.model_weights(R.make_model(1, cfg))
    del w["SimpleDesc/bn2/moving_mean"]
    path = str(tmp_path / "desc.npz")
    np.savez(path, **w)
    with pytest.raises(KeyError) as e:
        lfnet_desc.LfnetDescriptor.from_npz(None, path)
    msg = str(e.value)
    assert "missing ['SimpleDesc/bn2/moving_mean']" in msg
    for name in lfnet_desc.expected_names(2):
        assert name in msg
    assert lfnet_desc.expected_names(2) == sorted(R.make_model(1, cfg), key=lfnet_desc.expected_names(2).index)
    assert "SimpleDesc/fc-bn1/gamma" in lfnet_desc.expected_names(3) and "SimpleDesc/conv3/biases" in lfnet_desc.expected_names(3)
    assert "SimpleDesc/conv1/biases" not in lfnet_desc.expected_names(1, use_bias=False) and len(lfnet_desc.expected_names(3, False, False)) == 5
    full = R.model_weights(R.make_model(1, cfg))
    c = lfnet_desc.config_from_weights(full, norm=1)
    assert (c.patch_size, c.depth, c.channels, c.fc_dim, c.out_dim, c.norm) == (16, 2, 16, 32, 16, 1)
