"""btba_lfnet_scores on the MI355X: the stored groups against the fp64 restatement under the stored bars
(tests/golden/lfnet_det/lfnet_det_reference.npz, tests/lfnet_det_ref.py), the tile and halo edges and the release shape under bars
computed from the restatement's own fp32 error, bit-exactness across calls, batches and passes, the net inside LfnetDetector with
the descriptor net, every BTBA_EINVAL, the C++ host.  One module-scoped workspace.  All figures are printed before they are asserted."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib, lfnet, lfnet_desc, lfnet_det

import lfnet_desc_ref as RD
import lfnet_det_ref as R
from test_lfnet_det_ref import create_rejections, fill_weights


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


def _group(golden, g):
    name, over, _, shape, _ = R.GROUPS[g]
    cfg = R.config(**over)
    weights, photos = R.group_model(golden, name)
    return name, cfg, weights, photos, float(golden[f"tol_{name}"])


def _net(ws, weights, cfg):
    return lfnet_det.LfnetScoreNet(ws, weights, R.lib_config(cfg))


def _run(net, photos):
    maps, ori = net.scores(_t(photos))
    return [_np(m) for m in maps], _np(ori)


@pytest.fixture(scope="module")
def model_b(ws, golden):
    """Group b's model (C 16, k 5, 2 blocks, 3 scales, leaky relu, large betas)."""
    name, cfg, weights, photos, tol = _group(golden, 1)
    net = _net(ws, weights, cfg)
    yield dict(cfg=cfg, net=net, weights=weights, photos=photos, tol=tol)
    net.close()


@pytest.fixture(scope="module")
def release(ws):
    """The release shape with seeded weights and one 96 x 112 photo."""
    cfg = R.config()
    weights = R.model_weights(R.make_model(7, cfg))
    photo = R.levels(*R.make_photos(8, 1, 96, 112))
    net = lfnet_det.LfnetScoreNet(ws, weights)              # the default configuration is the release net
    yield dict(cfg=cfg, net=net, weights=weights, photo=photo)
    net.close()


def _check(what, maps, ori, weights, cfg, photos, tol=None):
    """Device results against fp64 under `tol`, or under 4 x the restatement's own fp32 error where tol is None."""
    m64, r64, u64 = R.forward(weights, cfg, photos, np.float64)
    e = R.error(maps, ori, m64, r64, u64)
    if tol is None:
        m32, _, u32 = R.forward(weights, cfg, photos, np.float32)
        e32 = R.error(m32, u32, m64, r64, u64)
        tol = 4.0 * e32["worst"]
        print(f"{what}: restatement fp32 vs fp64 score {e32['score']:.3e} ori {e32['ori']:.3e}")
        assert 1e-8 < tol < 1e-4
    print(f"{what}: device vs fp64 score {e['score']:.3e} ori {e['ori']:.3e}, bar {tol:.3e}, left out {100 * e['left_out']:.2f} %, "
          f"| |ori| - 1 | {e['norm']:.2e}")
    assert [m.shape[1:] for m in maps] == R.map_sizes(cfg, photos.shape[1], photos.shape[2])
    assert all(np.isfinite(m).all() for m in maps) and np.isfinite(ori).all()
    assert e["left_out"] <= R.ORI_CAP and e["norm"] < 1e-6
    assert e["worst"] <= tol


@pytest.mark.parametrize("g", [0, 1, 2])
def test_stored_groups_against_fp64_under_the_stored_bars(ws, golden, g):
    name, cfg, weights, photos, tol = _group(golden, g)
    net = _net(ws, weights, cfg)
    maps, ori = _run(net, photos)
    assert net.pad_size == int(golden[f"{name}/pad_size"]) == R.pad_size(cfg)
    assert np.array_equal(net.scale_factors, golden[f"{name}/scale_factors"])
    net.close()
    ref = R.error([golden[f"{name}/ref_score_{j}"] for j in range(cfg["num_scales"])], golden[f"{name}/ref_ori"], *R.forward(weights, cfg, photos))
    print(f"group {name}: reference vs fp64 score {ref['score']:.3e} ori {ref['ori']:.3e}")
    _check(f"group {name}", maps, ori, weights, cfg, photos, tol)


@pytest.mark.parametrize("H,W", [(1, 1), (4, 7), (16, 16), (17, 33), (40, 52), (65, 63)])
def test_tile_and_halo_edges(model_b, H, W):
    b = model_b
    photos = R.levels(*R.make_photos(100 * H + W, 1, H, W))
    maps, ori = _run(b["net"], photos)
    _check(f"{H} x {W}", maps, ori, b["weights"], b["cfg"], photos)


def test_release_shape_under_the_restatements_own_fp32_error(release):
    r = release
    cfg = r["cfg"]
    assert (cfg["channels"], cfg["ksize"], cfg["blocks"], cfg["num_scales"]) == (16, 5, 3, 5)
    assert r["net"].pad_size == 16
    mh, mw = r["net"].map_sizes(96, 112)
    want = [(int(np.float32(np.float32(96) * np.float32(1.0 / s)) + np.float32(0.5)), int(np.float32(np.float32(112) * np.float32(1.0 / s)) + np.float32(0.5)))
            for s in R.scales(2.0 ** -0.5, 2.0 ** 0.5, 5)]
    assert list(zip(mh.tolist(), mw.tolist())) == want == [(68, 79), (81, 94), (96, 112), (114, 133), (136, 158)]
    sf = R.scales(2.0 ** -0.5, 2.0 ** 0.5, 5)
    for H in range(1, 1025):                                # host only
        mh, mw = r["net"].map_sizes(H, 1025 - H)
        assert mh.tolist() == [R.map_size(s, H) for s in sf] and mw.tolist() == [R.map_size(s, 1025 - H) for s in sf]
    maps, ori = _run(r["net"], r["photo"])
    _check("release shape, 96 x 112", maps, ori, r["weights"], cfg, r["photo"])


def test_same_frame_same_bits_whatever_the_call_and_the_batch(model_b):
    b = model_b
    one = b["photos"][1:2]
    m1, o1 = _run(b["net"], one)
    m2, o2 = _run(b["net"], one)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(m1, m2)) and np.array_equal(_bits(o1), _bits(o2))      # two calls
    three = np.stack([b["photos"][0], R.levels(*R.make_photos(5, 1, 33, 47))[0], b["photos"][1]])
    m3, o3 = _run(b["net"], three)
    assert all(np.array_equal(_bits(x[2]), _bits(y[0])) for x, y in zip(m3, m1)) and np.array_equal(_bits(o3[2]), _bits(o1[0]))      # frame 2 of 3


def test_same_bits_across_passes(ws, golden):
    """One more frame than a pass holds: the last frame is worked in a pass of its own and is the same bits as alone."""
    txt = open(_lib.HEADER).read()
    pass_pixels = 1 << int(re.search(r"#define BTBA_LFNET_DET_PASS_PIXELS \(1 << (\d+)\)", txt).group(1))
    n = pass_pixels // (128 * 128) + 1
    name, cfg, weights, _, _ = _group(golden, 0)
    net = _net(ws, weights, cfg)
    three = R.levels(*R.make_photos(9, 3, 128, 128))
    idx = (np.arange(n) * 2) % 3                            # the last frame (index n - 1 = 64 -> photo 2) follows photos 0 and 1 in the first pass
    m, o = _run(net, three[idx])
    ma, oa = _run(net, three)
    net.close()
    assert np.array_equal(_bits(m[0]), _bits(ma[0][idx])) and np.array_equal(_bits(o), _bits(oa[idx]))
    assert not np.array_equal(ma[0][0], ma[0][1])


def test_from_models_is_the_three_stages_by_hand(ws, release):
    import torch
    dcfg = RD.config(**RD.GROUPS[2][1])                     # P = 32, the keypoint head's patch size
    desc = lfnet_desc.LfnetDescriptor(ws, RD.group_model(RD.load_golden(), "c")[0], dcfg)
    net = release["net"]
    det = lfnet.LfnetDetector.from_models(ws, net, desc, dict(top_k=64, pad_size=3))
    assert det.params.pad_size == net.pad_size == 16 and det.scale_factors == net.scale_factors and det.params.top_k == 64
    gray = _t(release["photo"][:, None])                    # [1, 1, 96, 112]
    kpts, d = det(None, gray)
    m = int(det.last["n_kpts_host"][0])
    print("keypoints:", m)
    assert 0 < m <= 64 and tuple(kpts.shape) == (m, 2) and tuple(d.shape) == (m, dcfg["out_dim"])
    maps, ori = net.scores(gray)
    r = lfnet.lfnet_keypoints(ws, maps, net.scale_factors, gray, ori, _lib.lfnet_params(top_k=64, pad_size=16))
    assert int(r["n_kpts_host"][0]) == m
    hand = desc(r["patches"][0, :m].reshape(m, 1, 32, 32))
    assert np.array_equal(_bits(_np(kpts)), _bits(_np(r["kpts"][0, :m]))) and np.array_equal(_bits(_np(d)), _bits(_np(hand)))
    assert np.abs(np.linalg.norm(_np(d).astype(np.float64), axis=1) - 1.0).max() < 1e-6
    desc.close()


def test_empty_calls_and_every_einval(ws, model_b, tmp_path):
    import torch
    from bundletrack_amd.optimizer import Workspace
    b = model_b
    net, L, E = b["net"], _lib.lib(), _lib.BTBA_EINVAL
    maps, ori = net.scores(torch.empty((0, 1, 33, 47), dtype=torch.float32, device="cuda"))
    assert [tuple(m.shape) for m in maps] == [(0, 23, 33), (0, 33, 47), (0, 47, 66)] and tuple(ori.shape) == (0, 33, 47, 2)
    assert L.btba_lfnet_scores(ws.handle, net.handle, 0, 33, 47, None, None, None) == _lib.BTBA_OK
    create_rejections(ws.handle)
    photo = _t(b["photos"])
    maps, ori = net.scores(photo)
    table = (C.c_void_p * 3)(*[m.data_ptr() for m in maps])
    tp = C.cast(table, C.c_void_p)
    call = L.btba_lfnet_scores
    args = lambda **kw: [kw.get(k, v) for k, v in (("ws", ws.handle), ("model", net.handle), ("n", 2), ("H", 33), ("W", 47), ("photo", photo.data_ptr()),
                                                   ("table", tp), ("ori", ori.data_ptr()))]
    assert call(*args()) == _lib.BTBA_OK
    for bad in (dict(ws=None), dict(model=None), dict(n=-1), dict(photo=None), dict(table=None), dict(ori=None), dict(H=0), dict(W=0), dict(H=8193),
                dict(W=8193), dict(H=6000), dict(W=6000),        # a map of 8485 > BTBA_LFNET_MAX_SIZE at scale 1 / sqrt(2)
                dict(photo=photo.data_ptr() + 2), dict(ori=ori.data_ptr() + 1)):
        assert call(*args(**bad)) == E, bad
    for j in range(3):
        for v in (None, maps[j].data_ptr() + 2):
            t2 = (C.c_void_p * 3)(*[m.data_ptr() for m in maps])
            t2[j] = v
            assert call(*args(table=C.cast(t2, C.c_void_p))) == E, (j, v)
    other = Workspace()
    assert call(*args(ws=other.handle)) == E                # a model of another workspace
    assert call(*args()) == _lib.BTBA_OK
    torch.cuda.synchronize()
    other.close()
    with pytest.raises(ValueError):
        net.scores(_t(np.zeros((1, 2, 33, 47), np.float32)))
    # from_npz: the full set gives the same bits; one array removed is an error that lists the expected names
    path = str(tmp_path / "det.npz")
    np.savez(path, **b["weights"])
    cfg = b["cfg"]
    again = lfnet_det.LfnetScoreNet.from_npz(ws, path, scale_factors=cfg["scale_factors"], activation=1)
    assert (again.config.channels, again.config.ksize, again.config.blocks, again.config.num_scales) == (16, 5, 2, 3)
    m2, o2 = again.scores(photo)
    assert all(np.array_equal(_bits(_np(x)), _bits(_np(y))) for x, y in zip(m2, maps)) and np.array_equal(_bits(_np(o2)), _bits(_np(ori)))
    again.close()
    w = dict(b["weights"])
    del w["ConvOnlyResNet/fin-bn/gamma"]
    np.savez(path, **w)
    with pytest.raises(KeyError) as e:
        lfnet_det.LfnetScoreNet.from_npz(ws, path)
    assert "missing ['ConvOnlyResNet/fin-bn/gamma']" in str(e.value)
    for name in lfnet_det.expected_names(2, 3):
        assert name in str(e.value)


class _HeadBuffers(C.Structure):
    """btba::LfnetBuffers (bundletrack_amd/cpp/btba_host.hpp)."""
    _fields_ = [(n, C.c_void_p) for n in ("max_heatmaps", "max_scales", "kpts_xy", "n_kpts", "kpts", "kpts_scale", "kpts_ori", "patches")]


@pytest.mark.parametrize("via_score_net", [0, 1])
def test_cpp_host_equals_python(ws, model_b, via_score_net):
    import torch
    _lib.build_host_cpp()                                   # a no-op after build()
    drv = C.CDLL(_lib.LFNET_DET_DRIVER)
    drv.lfnet_det_driver.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
    b = model_b
    cfg, net = b["cfg"], b["net"]
    n, H, W = (1, 48, 48) if via_score_net else (2, 33, 47)
    photos = R.levels(*R.make_photos(21, n, H, W))
    photo = _t(photos)
    want_maps, want_ori = net.scores(photo)
    keep = {k: np.ascontiguousarray(v, np.float32) for k, v in b["weights"].items()}
    Wt = fill_weights(keep, cfg)
    c = _lib.lfnet_det_config(**R.lib_config(cfg))
    maps = [torch.full_like(m, 7.0) for m in want_maps]
    ori = torch.full_like(want_ori, 7.0)
    table = (C.c_void_p * 3)(*[m.data_ptr() for m in maps])
    if via_score_net:
        p = _lib.lfnet_params(top_k=32, pad_size=1)
        want = lfnet.lfnet_keypoints(ws, want_maps, net.scale_factors, photo, want_ori, _lib.lfnet_params(top_k=32, pad_size=net.pad_size))
        got = {k: torch.zeros_like(want[k]) for k in ("max_heatmaps", "max_scales", "kpts_xy", "n_kpts", "kpts", "kpts_scale", "kpts_ori", "patches")}
        head = _HeadBuffers(*[got[k].data_ptr() for k, _ in _HeadBuffers._fields_])
        m = C.c_int(-1)
        rc = drv.lfnet_det_driver(ws.handle, C.addressof(c), C.addressof(Wt), 1, H, W, photo.data_ptr(), C.cast(table, C.c_void_p), ori.data_ptr(), 1,
                                  C.addressof(p), C.addressof(head), C.addressof(m))
        assert rc == 0
        print("keypoints through the C++ detector:", m.value)
        assert m.value == int(want["n_kpts_host"][0])
        for k in got:
            assert np.array_equal(_np(got[k]).view(np.uint32), _np(want[k]).view(np.uint32)), k
    else:
        rc = drv.lfnet_det_driver(ws.handle, C.addressof(c), C.addressof(Wt), n, H, W, photo.data_ptr(), C.cast(table, C.c_void_p), ori.data_ptr(), 0,
                                  None, None, None)
        assert rc == 0
    assert all(np.array_equal(_bits(_np(x)), _bits(_np(y))) for x, y in zip(maps, want_maps)) and np.array_equal(_bits(_np(ori)), _bits(_np(want_ori)))
    c.channels = 24
    assert drv.lfnet_det_driver(ws.handle, C.addressof(c), C.addressof(Wt), n, H, W, photo.data_ptr(), C.cast(table, C.c_void_p), ori.data_ptr(), 0,
                                None, None, None) == _lib.BTBA_EINVAL
