"""btba_vos_features on the MI355X: the stored groups against the fp64 restatement under the stored bars
(tests/golden/vos_net/vos_net_reference.npz, tests/vos_net_ref.py), the tile and stride edges and resnet50 under bars computed from the
restatement's own fp32 error, bit-exactness across calls, batches and passes, loading, every BTBA_EINVAL, the net as Bundler's
segmenter, the C++ host.  One module-scoped workspace.  All figures are printed before they are asserted."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib, vos, vos_net

import vos_net_ref as R


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(net, photos):
    return _np(net.features(_t(photos)))


@pytest.fixture(scope="module")
def model_b(ws, golden):
    """Group b's model: Bottleneck, one block per layer."""
    G = R.group(golden, 1)
    net = vos_net.VosBackbone(ws, G["weights"], G["cfg"])
    G["net"] = net
    yield G
    net.close()


def _check(what, got, weights, cfg, photos, tol=None):
    """Device results against fp64 under `tol`, or under 4 x the restatement's own fp32 error where tol is None."""
    n, _, H, W = photos.shape
    y64 = R.forward(weights, cfg, photos, np.float64)
    if tol is None:
        e32 = R.error(R.forward(weights, cfg, photos, np.float32), y64)
        tol = 4.0 * e32
        print(f"{what}: restatement fp32 vs fp64 {e32:.3e}")
        assert 1e-8 < tol < 1e-4
    assert got.shape == (n, 256, -(-H // 8), -(-W // 8)) and got.dtype == np.float32
    assert np.isfinite(got).all()
    e = R.error(got, y64)
    print(f"{what}: device vs fp64 {e:.3e}, bar {tol:.3e}")
    assert e <= tol


@pytest.mark.parametrize("g", [0, 1, 2])
def test_stored_groups_against_fp64_under_the_stored_bars(ws, golden, g):
    G = R.group(golden, g)
    net = vos_net.VosBackbone(ws, G["weights"], G["cfg"])
    got = _run(net, G["photos"])
    net.close()
    print(f"group {G['name']}: reference fp32 vs fp64 {float(golden[G['name'] + '/err_ref32']):.3e}, fp32 chain {float(golden[G['name'] + '/err_chain32']):.3e}")
    _check(f"group {G['name']}", got, G["weights"], G["cfg"], G["photos"], G["tol"])


@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (1, 7, 9), (1, 8, 8), (1, 9, 17), (1, 16, 16), (1, 64, 72), (1, 65, 63), (3, 33, 47)])
def test_tile_and_stride_edges(model_b, n, H, W):
    """3 frames of 33 x 47 are 90 rows at the last stage: an M tile of 64 straddles two frames."""
    b = model_b
    photos = R.levels(*R.make_photos(100 * H + W, n, H, W))
    _check(f"{n} x {H} x {W}", _run(b["net"], photos), b["weights"], b["cfg"], photos)


def test_resnet50_under_the_restatements_own_fp32_error(ws):
    cfg = R.config()
    assert (cfg["block"], cfg["layers"]) == (1, [3, 4, 6, 3])
    weights = R.model_weights(R.make_model(7, cfg))
    net = vos_net.VosBackbone(ws, weights)                  # block kind and depths read off the names
    assert (int(net.config.block), list(net.config.layers)) == (1, [3, 4, 6, 3])
    photos = R.levels(*R.make_photos(8, 2, 96, 128))
    got = _run(net, photos)
    net.close()
    _check("resnet50, 2 x 96 x 128", got, weights, cfg, photos)


def test_same_frame_same_bits_whatever_the_call_and_the_batch(model_b):
    b = model_b
    one = b["photos"][1:2]
    y1, y2 = _run(b["net"], one), _run(b["net"], one)
    assert np.array_equal(_bits(y1), _bits(y2))                                   # two calls
    three = np.stack([b["photos"][0], R.levels(*R.make_photos(5, 1, 33, 47))[0], b["photos"][1]])
    y3 = _run(b["net"], three)
    assert np.array_equal(_bits(y3[2]), _bits(y1[0]))                             # frame 2 of 3
    assert not np.array_equal(y3[0], y3[2])


def test_same_bits_across_passes(model_b):
    """One more frame than a pass holds: the last frame is worked in a pass of its own and is the same bits as in a single pass."""
    txt = open(_lib.HEADER).read()
    pass_pixels = 1 << int(re.search(r"#define BTBA_VOS_NET_PASS_PIXELS \(1 << (\d+)\)", txt).group(1))
    n = pass_pixels // (32 * 32) + 1
    three = R.levels(*R.make_photos(9, 3, 32, 32))
    idx = (np.arange(n) * 2) % 3                            # the last frame (index n - 1 = 1024 -> photo 2) follows photos 0 and 1 in the first pass
    assert n * 32 * 32 > pass_pixels >= (n - 1) * 32 * 32 and idx[-1] == 2
    many = _run(model_b["net"], three[idx])
    single = _run(model_b["net"], three)
    assert many.shape == (n, 256, 4, 4)
    assert np.array_equal(_bits(many), _bits(single[idx]))
    assert not np.array_equal(single[0], single[2])


def test_loading(ws, model_b, tmp_path):
    import torch
    b = model_b
    photo = _t(b["photos"])
    want = _bits(_np(b["net"].features(photo)))
    tracked = {k: np.array(3, np.int64) for k in b["keys"] if k.endswith("num_batches_tracked")}
    assert len(tracked) > 0
    sd = dict(b["weights"], **tracked)
    variants = dict(module={"module." + k: v for k, v in sd.items()}, tracked=sd,
                    tensors={k: torch.from_numpy(v) for k, v in b["weights"].items()})
    for what, state in variants.items():
        net = vos_net.VosBackbone(ws, state)                # the configuration is read off the names
        assert np.array_equal(_bits(_np(net.features(photo))), want), what
        net.close()
    path = str(tmp_path / "backbone.npz")
    np.savez(path, **sd)
    net = vos_net.VosBackbone.from_npz(ws, path)
    assert np.array_equal(_bits(_np(net.features(photo))), want)
    net.close()
    ckpt = str(tmp_path / "checkpoint.pth.tar")
    torch.save({"epoch": 1, "state_dict": {"module." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, ckpt)
    net = vos_net.VosBackbone.from_checkpoint(ws, ckpt)
    assert np.array_equal(_bits(_np(net.features(photo))), want)
    net.close()
    # one array removed is an error that lists every expected name
    w = dict(b["weights"])
    del w["backbone.5.0.downsample.1.running_var"]
    with pytest.raises(KeyError) as e:
        vos_net.VosBackbone(ws, w)
    assert "missing ['backbone.5.0.downsample.1.running_var']" in str(e.value)
    for name in vos_net.expected_names(b["cfg"]):
        assert name in str(e.value)
    with pytest.raises(ValueError):
        vos_net.VosBackbone(ws, dict(b["weights"], **{"bn256.bias": np.zeros(255, np.float32)}))


@pytest.mark.parametrize("g", [0, 1, 2])
def test_config_from_state_dict(golden, g):
    name, over, _ = R.GROUPS[g]
    cfg = vos_net.config_from_state_dict({str(k): None for k in golden[f"{name}/keys"]})
    assert (int(cfg.block), list(cfg.layers)) == (over["block"], over["layers"])


def _records(weights, cfg):
    """(records, keep-alive list) of btba_vos_net_layer in forward order."""
    table = vos_net.layer_table(cfg)
    keep = {k: np.ascontiguousarray(v, np.float32) for k, v in weights.items()}
    rec = (_lib.VosNetLayer * len(table))()
    for r, (conv, bn, _, _, _) in zip(rec, table):
        r.weight = keep[f"{conv}.weight"].ctypes.data
        r.bn_weight, r.bn_bias = keep[f"{bn}.weight"].ctypes.data, keep[f"{bn}.bias"].ctypes.data
        r.running_mean, r.running_var = keep[f"{bn}.running_mean"].ctypes.data, keep[f"{bn}.running_var"].ctypes.data
    return rec, keep


def test_empty_calls_and_every_einval(ws, model_b):
    import torch
    from bundletrack_amd.optimizer import Workspace
    b = model_b
    net, L, E = b["net"], _lib.lib(), _lib.BTBA_EINVAL
    assert tuple(net.features(torch.empty((0, 3, 33, 47), dtype=torch.float32, device="cuda")).shape) == (0, 256, 5, 6)
    assert L.btba_vos_features(ws.handle, net.handle, 0, 33, 47, None, None) == _lib.BTBA_OK
    photo = _t(b["photos"])
    out = net.features(photo)
    want = _bits(_np(out))
    call = L.btba_vos_features
    args = lambda **kw: [kw.get(k, v) for k, v in (("ws", ws.handle), ("model", net.handle), ("n", 2), ("H", 33), ("W", 47), ("rgb", photo.data_ptr()),
                                                   ("out", out.data_ptr()))]
    other = Workspace()
    for bad in (dict(ws=None), dict(model=None), dict(n=-1), dict(rgb=None), dict(out=None), dict(H=0), dict(W=0), dict(H=4097), dict(W=4097),
                dict(rgb=photo.data_ptr() + 4), dict(out=out.data_ptr() + 8), dict(ws=other.handle)):
        assert call(*args(**bad)) == E, bad
        out.fill_(7.0)
        assert call(*args()) == _lib.BTBA_OK                # a good call after every refusal
        assert np.array_equal(_bits(_np(out)), want), bad
    # create
    cfg = _lib.vos_net_config(**b["cfg"])
    rec, keep = _records(b["weights"], b["cfg"])
    n_layers = len(rec)
    h = C.c_void_p()
    create = lambda c=cfg, r=rec, n=n_layers, w=ws.handle, o=C.byref(h): L.btba_vos_net_model_create(w, C.byref(c) if c is not None else None,
                                                                                                      C.cast(r, C.c_void_p) if r is not None else None, n, o)
    assert create(w=None) == E and create(c=None) == E and create(r=None) == E and create(o=None) == E
    assert create(n=n_layers - 1) == E and create(n=n_layers + 1) == E and create(n=0) == E
    for over in (dict(block=2), dict(layers=[1, 1, 1, 0]), dict(layers=[65, 1, 1, 1]), dict(bn_eps=-1.0), dict(bn_eps=float("nan"))):
        assert create(c=_lib.vos_net_config(**dict(b["cfg"], **over))) == E, over
    assert create(c=_lib.vos_net_config(block=0, layers=[1, 1, 1, 1])) == E      # the basic net of these depths has another count
    for field in ("weight", "bn_weight", "bn_bias", "running_mean", "running_var"):
        r2, _ = _records(b["weights"], b["cfg"])
        setattr(r2[3], field, None)                         # a missing array
        assert create(r=r2) == E, field
    for name, value in (("backbone.6.0.conv2.weight", np.nan), ("adjust_dim.weight", np.inf), ("bn256.bias", np.nan),
                        ("backbone.1.running_var", np.float32(-1e-5)), ("backbone.4.0.bn3.running_var", -1.0)):
        w2 = dict(b["weights"])
        w2[name] = w2[name].copy()
        w2[name].ravel()[-1] = value
        r2, keep2 = _records(w2, b["cfg"])
        assert create(r=r2) == E, name
    assert h.value is None
    assert create() == _lib.BTBA_OK and h.value
    out.fill_(7.0)
    assert call(ws.handle, h, 2, 33, 47, photo.data_ptr(), out.data_ptr()) == _lib.BTBA_OK
    assert np.array_equal(_bits(_np(out)), want)
    L.btba_vos_net_model_destroy(h)
    L.btba_vos_net_model_destroy(None)
    torch.cuda.synchronize()
    other.close()
    with pytest.raises(ValueError):
        net.features(_t(np.zeros((1, 1, 33, 47), np.float32)))


def test_backbone_as_the_bundlers_segmenter(ws, model_b):
    """Bundler(segmenter=VosBackbone, mask_propagator=...) on a 3-frame 64 x 64 clip: the features and masks are those of
    normalize_inputs -> features -> MaskPropagator.start / step by hand, bit for bit."""
    import torch
    from bundletrack_amd import synthetic as S
    from bundletrack_amd.bundler import Bundler, FrameRef
    from bundletrack_amd.optimizer import OptimizerGpu, depth_to_normals, process_depth
    n, H, W = 3, 64, 64
    K = np.array([[120.0, 0.0, 32.0], [0.0, 160.0, 32.0], [0.0, 0.0, 1.0]])
    seq = S.SyntheticSequence(n_frames=n, seed=S.config_seed(1), background=True, H=H, W=W, K=K)
    net = model_b["net"]
    masks0 = [S.make_mask(seq.poses_gt[k], seq.K, H, W, seed=k) for k in range(n)]
    assert all((m > 0).sum() > 100 for m in masks0)
    bgrs = [np.where((masks0[k] > 0)[..., None], np.array([30, 60, 220], np.uint8), np.array([200, 120, 40], np.uint8)).astype(np.uint8) for k in range(n)]
    first = _t((masks0[0] > 0).astype(np.uint8) * 255)

    mp_hand = vos.MaskPropagator(ws, 2, H, W)
    hand_masks, hand_feats = [], []
    for k in range(n):
        feats = net.features(vos.normalize_inputs(ws, [_t(bgrs[k])]))
        assert tuple(feats.shape) == (1, 256, 8, 8)
        hand_feats.append(_np(feats)[0])
        if k == 0:
            mp_hand.start(first, feats[0])
        else:
            hand_masks.append(_np(mp_hand.step(feats[0])))

    mp = vos.MaskPropagator(ws, 2, H, W)
    bundler = Bundler(OptimizerGpu(workspace=ws), S.SyntheticFeatureManager(seq, corr_per_pair=300), seq.K, H, W, window_size=5, max_BA_frames=5,
                      segmenter=net, mask_propagator=mp)
    for k in range(n):
        fr = FrameRef(id=0, pose_in_model=seq.poses_gt[0].astype(np.float32), n_keypts=300)
        fr.depth_gpu = process_depth(ws, _t(seq.render(k)[0]))
        fr.normal_gpu = depth_to_normals(ws, fr.depth_gpu, seq.K)
        fr.bgr_gpu = _t(bgrs[k])
        if k == 0:
            fr.mask_gpu = first.clone()
        bundler.fm.register(fr, k)
        bundler.process_new_frame(fr)
        assert fr.mask_gpu is not None
        if k > 0:
            assert np.array_equal(_np(fr.mask_gpu), hand_masks[k - 1]), k
        assert np.array_equal(_bits(_np(mp.history(k)[0]).reshape(256, 8, 8)), _bits(hand_feats[k])), k
    assert mp.n_frames == n
    print("foreground pixels of the propagated masks:", [int((m > 0).sum()) for m in hand_masks])


@pytest.mark.parametrize("via_segmenter", [0, 1])
def test_cpp_host_equals_python(ws, model_b, via_segmenter):
    import torch
    _lib.build_host_cpp()                                   # a no-op after build()
    drv = C.CDLL(_lib.VOS_NET_DRIVER)
    drv.vos_net_driver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    b = model_b
    H, W = (32, 40) if via_segmenter else (33, 47)          # frame by frame, every frame's planes must start on 16 bytes
    photo = _t(R.levels(*R.make_photos(21, 2, H, W)))
    want = _np(b["net"].features(photo))
    rec, keep = _records(b["weights"], b["cfg"])
    cfg = _lib.vos_net_config(**b["cfg"])
    out = torch.full(want.shape, 7.0, dtype=torch.float32, device="cuda")
    rc = drv.vos_net_driver(ws.handle, C.addressof(cfg), C.addressof(rec), len(rec), 2, H, W, photo.data_ptr(), out.data_ptr(), via_segmenter)
    assert rc == 0
    assert np.array_equal(_bits(_np(out)), _bits(want))
    assert drv.vos_net_driver(ws.handle, C.addressof(cfg), C.addressof(rec), len(rec) - 1, 2, H, W, photo.data_ptr(), out.data_ptr(), via_segmenter) == _lib.BTBA_EINVAL
