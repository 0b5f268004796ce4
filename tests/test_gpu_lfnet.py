"""btba_lfnet_* on the MI355X: stage A against the fp64 restatement under the measured bars (tests/golden/lfnet/lfnet_reference.npz,
tests/lfnet_ref.py) at the stored groups and at fresh shapes, its repeatability and batch independence; stage B exactly equal to
the restatement on the device's own heat maps and on made-up ones; stage C against fp64 under the bars; btba_lfnet_keypoints
against the three calls and the stored reference keypoints; the argument checks; LfnetDetector inside a Bundler session; the C++
host.  One module-scoped workspace.  All figures are printed before they are asserted."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib
from bundletrack_amd import lfnet

import lfnet_ref as R


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


def _stack(frames_maps):
    """per-frame lists of [h_s, w_s] -> per-scale CUDA tensors [n, h_s, w_s]"""
    return [_t(np.stack([fm[s] for fm in frames_maps]).astype(np.float32)) for s in range(len(frames_maps[0]))]


def _heat(ws, frames_maps, sf, H, W, prm):
    heat, scl = lfnet.lfnet_heatmaps(ws, _stack(frames_maps), sf, H, W, dict(prm))
    return _np(heat), _np(scl)


def _group(golden, g):
    name, H, W, sf, over, n_cases = R.GROUPS[g]
    prm = R.params(**over)
    tol = {k: float(golden[f"tol_{name}_{k}"]) for k in ("heat", "scale", "kpts", "patch")}
    cases = [R.group_inputs(golden, name, i, sf) for i in range(n_cases)]
    return name, H, W, sf, prm, tol, cases


def _hold_heat(what, heat, scl, maps, sf, H, W, prm, tol):
    h64, s64 = R.heatmaps(maps, sf, H, W, prm, np.float64)
    sr = max(max(sf) - min(sf), 1.0)
    eh, es = np.abs(heat - h64).max(), np.abs(scl - s64).max() / sr
    print(f"{what}: heat err {eh:.3e} (tol {tol['heat']:.3e}), scale err {es:.3e} (tol {tol['scale']:.3e})")
    assert np.isfinite(heat).all() and np.isfinite(scl).all()
    assert not heat[~R.frame_mask(H, W, prm["pad_size"])].any()
    assert eh <= tol["heat"] and es <= tol["scale"], (what, eh, es, tol)
    return h64, s64


@pytest.mark.parametrize("g", [0, 1, 2])
def test_stage_a_stored_groups_against_fp64(ws, golden, g):
    name, H, W, sf, prm, tol, cases = _group(golden, g)
    heat, scl = _heat(ws, [c[0] for c in cases], sf, H, W, prm)
    for i, (maps, _, _) in enumerate(cases):
        _hold_heat(f"{name} case {i}", heat[i], scl[i], maps, sf, H, W, prm, tol)


# fresh seeds: the window larger than the image; S = 2 at a size that is no tile multiple; S = 16 with k = 31 (the small tile).  The
# bars are the stored ones of the first group: the error is that of the fp32 roundings of one pixel's window, scaled by the heat
# values, and neither grows with the shape
FRESH = [("9x9_k15", 9, 9, (1.0, 0.8), dict(sm_ksize=15, pad_size=2, crop_radius=2), 0),
         ("33x47_s2", 33, 47, (R.SQRT2, 1.0 / R.SQRT2), dict(pad_size=5, crop_radius=5), 0),
         ("16x16_s16_k31", 16, 16, tuple(2.0 ** (0.5 - j / 15.0) for j in range(16)), dict(sm_ksize=31, pad_size=3, crop_radius=3), 0)]


@pytest.mark.parametrize("case", FRESH, ids=[c[0] for c in FRESH])
def test_stage_a_fresh_shapes_against_fp64(ws, golden, case):
    what, H, W, sf, over, g = case
    prm = R.params(**over)
    tol = {k: float(golden[f"tol_{R.GROUPS[g][0]}_{k}"]) for k in ("heat", "scale")}
    maps = [R.levels(m, 1.0 / 32.0) for m in R.make_inputs(777 + H, H, W, sf)[0]]
    heat, scl = _heat(ws, [maps], sf, H, W, prm)
    _hold_heat(what, heat[0], scl[0], maps, sf, H, W, prm, tol)


def test_stage_a_constant_map_has_variance_zero(ws, golden):
    H, W, sf = 24, 24, (1.25, 1.0)
    prm = R.params(pad_size=3, crop_radius=3)
    maps = [np.full(sz, 0.75, np.float32) for sz in R.map_sizes(H, W, sf)]
    heat, scl = _heat(ws, [maps], sf, H, W, prm)
    tol = {k: float(golden[f"tol_{R.GROUPS[0][0]}_{k}"]) for k in ("heat", "scale")}
    _hold_heat("constant", heat[0], scl[0], maps, sf, H, W, prm, tol)


def test_stage_a_batch_equals_single_frames_and_repeats(ws, golden):
    name, H, W, sf, prm, tol, cases = _group(golden, 0)
    third = [R.levels(m, 1.0 / 32.0) for m in R.make_inputs(5, H, W, sf)[0]]
    frames = [cases[0][0], cases[1][0], third]
    heat, scl = _heat(ws, frames, sf, H, W, prm)
    heat2, scl2 = _heat(ws, frames, sf, H, W, prm)
    assert np.array_equal(heat.view(np.uint32), heat2.view(np.uint32)) and np.array_equal(scl.view(np.uint32), scl2.view(np.uint32))
    for i, fm in enumerate(frames):
        h1, s1 = _heat(ws, [fm], sf, H, W, prm)
        assert np.array_equal(h1[0].view(np.uint32), heat[i].view(np.uint32)) and np.array_equal(s1[0].view(np.uint32), scl[i].view(np.uint32))


def _select(ws, heat, prm):
    kxy, cnt = lfnet.lfnet_select(ws, _t(np.asarray(heat, np.float32)), dict(prm))
    kxy, cnt = _np(kxy), _np(cnt)
    for f in range(len(cnt)):
        assert not kxy[f, cnt[f]:].any()
    return [kxy[f, :cnt[f]] for f in range(len(cnt))]


@pytest.mark.parametrize("g", [0, 1, 2])
def test_stage_b_on_the_devices_own_heat_maps(ws, golden, g):
    name, H, W, sf, prm, tol, cases = _group(golden, g)
    heat, _ = _heat(ws, [c[0] for c in cases], sf, H, W, prm)
    got = _select(ws, heat, prm)
    for i in range(len(cases)):
        assert np.array_equal(got[i], R.select(heat[i], prm)), (name, i)
        assert len(got[i]) > 0


def _made_up(H, W):
    rs = np.random.default_rng(H * W)
    one = np.zeros((H, W), np.float32)
    one[H // 2, W // 2 + 1] = 0.5
    plateau = np.zeros((H, W), np.float32)
    plateau[3:H - 3, 3:W - 3] = 0.25
    plateau[H // 2, 3:W - 3] = 0.5                                     # a ridge of equal neighbours: no peak either
    grid = np.zeros((H, W), np.float32)
    grid[3:H - 3:3, 3:W - 3:3] = 1.0                                   # many equal peaks
    noise = rs.random((H, W), dtype=np.float32)
    levels4 = rs.integers(0, 4, (H, W)).astype(np.float32)             # repeated values everywhere
    signed = rs.normal(size=(H, W)).astype(np.float32)
    return dict(zeros=np.zeros((H, W), np.float32), one=one, plateau=plateau, grid=grid, noise=noise, levels4=levels4, signed=signed)


@pytest.mark.parametrize("H,W", [(12, 12), (40, 52), (64, 64)])
def test_stage_b_made_up_maps_exactly(ws, H, W):
    maps = _made_up(H, W)
    n_grid = int((maps["grid"] > 0).sum())
    configs = [dict(pad_size=2, crop_radius=2, nms_ksize=3, top_k=n_grid // 2),          # top_k below the number of equal peaks
               dict(pad_size=2, crop_radius=2, nms_ksize=5, top_k=1),
               dict(pad_size=2, crop_radius=2, nms_ksize=3, top_k=2048),                  # above the peak count (and above H W at 12 x 12)
               dict(pad_size=1, crop_radius=4, nms_ksize=3, top_k=H * W // 3),            # the fill case: pad_size < crop_radius
               dict(pad_size=0, crop_radius=3, nms_ksize=3, top_k=min(H * W - 7, 2048), nms_thresh=-0.5),
               dict(pad_size=2, crop_radius=2, nms_ksize=1, top_k=50, nms_thresh=0.3)]
    for over in configs:
        prm = R.params(**over)
        got = _select(ws, np.stack(list(maps.values())), prm)           # all maps as the frames of one call
        for (what, m), kxy in zip(maps.items(), got):
            want = R.select(m, prm)
            assert np.array_equal(kxy, want), (what, over, len(kxy), len(want))
    prm = R.params(pad_size=2, crop_radius=2, nms_ksize=3, top_k=n_grid // 2)
    got = _select(ws, maps["grid"][None], prm)[0]
    assert len(got) == n_grid // 2 and len(_select(ws, maps["zeros"][None], prm)[0]) == 0 and len(_select(ws, maps["plateau"][None], prm)[0]) == 0
    flat = got[:, 1] * W + got[:, 0]
    all_peaks = np.flatnonzero(maps["grid"].reshape(-1) > 0)
    assert np.array_equal(flat, all_peaks[:n_grid // 2])                # the lower indices win
    assert np.array_equal(_select(ws, maps["one"][None], prm)[0], [[W // 2 + 1, H // 2]])


def test_stage_b_2048_peaks(ws):
    heat = np.zeros((128, 128), np.float32)
    vals = np.random.default_rng(3).permutation(62 * 62).astype(np.float32) + 1.0
    heat[2:126:2, 2:126:2] = vals.reshape(62, 62)                       # 3 844 isolated peaks, all different
    prm = R.params(pad_size=2, crop_radius=2, nms_ksize=3, top_k=2048)
    got = _select(ws, heat[None], prm)[0]
    assert len(got) == 2048 and np.array_equal(got, R.select(heat, prm))
    heat[heat > 0] = 1.0                                                # all equal: the first 2 048 in raster order
    got = _select(ws, heat[None], prm)[0]
    assert len(got) == 2048 and np.array_equal(got, R.select(heat, prm))


def _crops(ws, photo, ori, heat, scl, kxy_list, prm):
    K = int(prm["top_k"])
    n = len(kxy_list)
    kxy = np.zeros((n, K, 2), np.int32)
    for f, k in enumerate(kxy_list):
        kxy[f, :len(k)] = k
    cnt = np.array([len(k) for k in kxy_list], np.int32)
    out = lfnet.lfnet_crops(ws, _t(photo), _t(ori), _t(heat), _t(scl), _t(kxy), _t(cnt), dict(prm))
    return [_np(o) for o in out]


def _hold_crops(what, got, f, m, photo, ori, h64, s64, kxy, prm, tol, sf):
    kp, ksc, kor, pt = (o[f] for o in got)
    kp64, ksc64, kor64, pt64, edge = R.crops(photo, ori, h64, s64, kxy, prm, np.float64)
    assert not kp[m:].any() and not ksc[m:].any() and not kor[m:].any() and not pt[m:].any()          # slots past n_kpts are zero
    rng = float(photo.max() - photo.min())
    ek = np.abs(kp[:m] - kp64).max()
    ep = np.abs(pt[:m] - pt64)[~edge].max() / rng
    es = np.abs(ksc[:m] - ksc64).max() / max(max(sf) - min(sf), 1.0)
    print(f"{what}: kpts err {ek:.3e} (tol {tol['kpts']:.3e}), patch err {ep:.3e} (tol {tol['patch']:.3e}), scale err {es:.3e}, "
          f"edge share {edge.mean():.4f}")
    assert edge.mean() <= R.EDGE_SHARE
    assert np.isfinite(pt).all() and ek <= tol["kpts"] and ep <= tol["patch"] and es <= tol["scale"], (what, ek, ep, es, tol)
    assert np.array_equal(kor[:m], ori[kxy[:, 1], kxy[:, 0]])


@pytest.mark.parametrize("g", [0, 1, 2])
def test_stage_c_stored_keypoints_against_fp64(ws, golden, g):
    name, H, W, sf, prm, tol, cases = _group(golden, g)
    heat, scl = _heat(ws, [c[0] for c in cases], sf, H, W, prm)
    kxys = [golden[f"{name}_{i}_ref_kxy"] for i in range(len(cases))]
    got = _crops(ws, np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]), heat, scl, kxys, prm)
    for i, (maps, photo, ori) in enumerate(cases):
        h64, s64 = R.heatmaps(maps, sf, H, W, prm, np.float64)
        _hold_crops(f"{name} case {i}", got, i, len(kxys[i]), photo, ori, h64, s64, kxys[i], prm, tol, sf)


def test_stage_c_made_up_keypoints_at_the_borders(ws, golden):
    """Keypoints at distance crop_radius from each border with scale 1/sqrt2, 1, sqrt2 and orientations 0, 45, 90, 180 degrees: the
    patch leaves the image on every side.  The heat and scale maps are handed over as they are (stage C takes any), so fp64 reads
    the same values; the bars are the stored ones of the 40 x 52 group."""
    name, H, W, sf, prm, tol, cases = _group(golden, 0)
    _, photo, _ = cases[0]
    r = prm["crop_radius"]
    pts = [(r, r), (W - 1 - r, r), (r, H - 1 - r), (W - 1 - r, H - 1 - r), (W // 2, r), (r, H // 2), (W - 1 - r, H // 2), (W // 2, H - 1 - r),
           (W // 2 - 3, H // 2 + 1), (W // 2 + 4, H // 2 - 2), (r + 1, r + 2), (W - 2 - r, H - 3 - r)]
    pts = sorted(pts, key=lambda p: (p[1], p[0]))
    scl = np.ones((H, W), np.float32)
    ori = np.zeros((H, W, 2), np.float32)
    ori[..., 0] = 1.0
    for j, (x, y) in enumerate(pts):
        scl[y, x] = np.float32((1.0 / R.SQRT2, 1.0, R.SQRT2)[j % 3])
        a = np.deg2rad((0.0, 45.0, 90.0, 180.0)[j % 4])
        ori[y, x] = (np.float32(np.cos(a)), np.float32(np.sin(a)))
    heat = (np.random.default_rng(8).random((H, W), dtype=np.float32) * R.frame_mask(H, W, prm["pad_size"])).astype(np.float32)
    kxy = np.asarray(pts, np.int32)
    # sample points that fall on the discontinuity by construction (integer keypoint, scale 1, no rotation) move off it with the
    # soft refinement; the share left is asserted in _hold_crops
    got = _crops(ws, photo[None], ori[None], heat[None], scl[None], [kxy], prm)
    _hold_crops("borders", got, 0, len(kxy), photo, ori, heat.astype(np.float64), scl.astype(np.float64), kxy, prm, tol, sf)
    hard = R.params(**dict(prm, soft_kpts=0))
    got = _crops(ws, photo[None], ori[None], heat[None], scl[None], [kxy], hard)
    assert np.array_equal(got[0][0, :len(kxy)], kxy.astype(np.float32))          # soft_kpts = 0: the integer keypoints as floats


def _keypoints(ws, cases, sf, prm):
    r = lfnet.lfnet_keypoints(ws, _stack([c[0] for c in cases]), sf, _t(np.stack([c[1] for c in cases])), _t(np.stack([c[2] for c in cases])), dict(prm))
    return {k: (_np(v) if k != "n_kpts_host" else v) for k, v in r.items()}


@pytest.mark.parametrize("g", [0, 1, 2])
def test_keypoints_equals_the_three_stages_and_the_reference(ws, golden, g):
    import torch
    name, H, W, sf, prm, tol, cases = _group(golden, g)
    r = _keypoints(ws, cases, sf, prm)
    heat, scl = lfnet.lfnet_heatmaps(ws, _stack([c[0] for c in cases]), sf, H, W, dict(prm))
    kxy, cnt = lfnet.lfnet_select(ws, heat, dict(prm))
    kp, ksc, kor, pt = lfnet.lfnet_crops(ws, _t(np.stack([c[1] for c in cases])), _t(np.stack([c[2] for c in cases])), heat, scl, kxy, cnt, dict(prm))
    torch.cuda.synchronize()
    for key, t in (("max_heatmaps", heat), ("max_scales", scl), ("kpts_xy", kxy), ("n_kpts", cnt), ("kpts", kp), ("kpts_scale", ksc),
                   ("kpts_ori", kor), ("patches", pt)):
        a, b = r[key], t.cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), key
    assert np.array_equal(r["n_kpts_host"], r["n_kpts"])
    for i in range(len(cases)):
        want = golden[f"{name}_{i}_ref_kxy"]
        m = int(r["n_kpts_host"][i])
        assert m == len(want) and np.array_equal(r["kpts_xy"][i, :m], want), (name, i)
        ek = np.abs(r["kpts"][i, :m] - golden[f"{name}_{i}_ref_kpts"]).max()
        print(f"{name} case {i}: {m} keypoints, refined against the stored reference {ek:.3e}")
        assert ek <= 2.0 * tol["kpts"]                                  # both within tol of fp64


def test_every_einval_case(ws):
    import torch
    L = _lib.lib()
    H = W = 40
    sf = np.array([1.0, 0.8], np.float32)
    mh, mw = np.array([40, 50], np.int32), np.array([40, 50], np.int32)
    maps = [torch.zeros((1, 40, 40), device="cuda"), torch.zeros((1, 50, 50), device="cuda")]
    photo, ori = torch.zeros((1, H, W), device="cuda"), torch.zeros((1, H, W, 2), device="cuda")
    heat, scl = torch.zeros((1, H, W), device="cuda"), torch.zeros((1, H, W), device="cuda")
    K = 16
    kxy, cnt = torch.zeros((1, K, 2), dtype=torch.int32, device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    kp, ksc, kor = torch.zeros((1, K, 2), device="cuda"), torch.zeros((1, K), device="cuda"), torch.zeros((1, K, 2), device="cuda")
    pt = torch.zeros((1, K, 32, 32), device="cuda")
    table = (C.c_void_p * 2)(*[m.data_ptr() for m in maps])
    good = _lib.lfnet_params(top_k=K, pad_size=4, crop_radius=4)

    def heatmaps(p=good, ws_=ws.handle, n=1, H_=H, W_=W, S=2, tab=table, mh_=mh, mw_=mw, sf_=sf, a=heat.data_ptr(), b=scl.data_ptr()):
        return L.btba_lfnet_heatmaps(ws_, C.byref(p) if p is not None else None, n, H_, W_, S, C.cast(tab, C.c_void_p) if tab is not None else None,
                                     mh_.ctypes.data if mh_ is not None else None, mw_.ctypes.data if mw_ is not None else None,
                                     sf_.ctypes.data if sf_ is not None else None, a, b)

    def select(p=good, ws_=ws.handle, n=1, H_=H, W_=W, a=heat.data_ptr(), b=kxy.data_ptr(), c=cnt.data_ptr()):
        return L.btba_lfnet_select(ws_, C.byref(p) if p is not None else None, n, H_, W_, a, b, c)

    ptrs = [photo, ori, heat, scl, kxy, cnt, kp, ksc, kor, pt]

    def crops(p=good, ws_=ws.handle, n=1, H_=H, W_=W, null=None):
        args = [None if j == null else t.data_ptr() for j, t in enumerate(ptrs)]
        return L.btba_lfnet_crops(ws_, C.byref(p) if p is not None else None, n, H_, W_, *args)

    def keypoints(p=good, ws_=ws.handle, n=1, H_=H, W_=W, S=2, tab=table, null=None):
        order = [photo, ori, heat, scl, kxy, cnt, kp, ksc, kor, pt]
        args = [None if j == null else t.data_ptr() for j, t in enumerate(order)]
        return L.btba_lfnet_keypoints(ws_, C.byref(p) if p is not None else None, n, H_, W_, S, C.cast(tab, C.c_void_p) if tab is not None else None,
                                      mh.ctypes.data, mw.ctypes.data, sf.ctypes.data, *args, None)

    assert heatmaps() == select() == crops() == keypoints() == _lib.BTBA_OK
    torch.cuda.synchronize()
    bad_params = [dict(sm_ksize=14), dict(sm_ksize=33), dict(sm_ksize=0), dict(nms_ksize=4), dict(nms_ksize=33), dict(top_k=0), dict(top_k=2049),
                  dict(pad_size=20), dict(crop_radius=20), dict(pad_size=-1), dict(patch_size=1), dict(patch_size=65), dict(kp_loc_size=1),
                  dict(kp_loc_size=65)]
    for over in bad_params:
        p = _lib.lfnet_params(**dict(dict(top_k=K, pad_size=4, crop_radius=4), **over))
        for call in (heatmaps, select, crops, keypoints):
            assert call(p=p) == _lib.BTBA_EINVAL, (over, call.__name__)
    for call in (heatmaps, select, crops, keypoints):
        for kw in (dict(p=None), dict(ws_=None), dict(n=0), dict(H_=0), dict(W_=0), dict(H_=8193), dict(W_=8193)):
            assert call(**kw) == _lib.BTBA_EINVAL, (kw, call.__name__)
    null_entry = (C.c_void_p * 2)(maps[0].data_ptr(), None)
    for kw in (dict(S=0), dict(S=17), dict(tab=None), dict(tab=null_entry)):
        assert heatmaps(**kw) == _lib.BTBA_EINVAL and keypoints(**kw) == _lib.BTBA_EINVAL, kw
    for kw in (dict(mh_=None), dict(mw_=None), dict(sf_=None), dict(mh_=np.array([40, 0], np.int32)), dict(mw_=np.array([-1, 50], np.int32)),
               dict(a=None), dict(b=None)):
        assert heatmaps(**kw) == _lib.BTBA_EINVAL, kw
    for kw in (dict(a=None), dict(b=None), dict(c=None), dict(a=heat.data_ptr() + 2)):
        assert select(**kw) == _lib.BTBA_EINVAL, kw
    for j in range(len(ptrs)):
        assert crops(null=j) == _lib.BTBA_EINVAL and keypoints(null=j) == _lib.BTBA_EINVAL, j


class _ScoreNet:
    """A fixed-weight conv 'score net': S score maps at int(H / s + 0.5) and a unit orientation map."""

    def __init__(self, scale_factors):
        import torch
        g = torch.Generator().manual_seed(11)
        self.sf = scale_factors
        self.w = torch.randn((3, 1, 5, 5), generator=g).cuda()

    def __call__(self, gray):
        import torch
        F = torch.nn.functional
        H, W = gray.shape[-2:]
        maps = []
        for s in self.sf:
            x = F.interpolate(gray, size=(int(H / s + 0.5), int(W / s + 0.5)), mode="bilinear", align_corners=False)
            maps.append(F.conv2d(x, self.w[:1], padding=2)[:, 0])
        o = F.conv2d(gray, self.w[1:], padding=2)
        o = o / o.norm(dim=1, keepdim=True).clamp_min(1e-6)
        return maps, o.permute(0, 2, 3, 1).contiguous()


class _DescNet:
    def __init__(self, D=24):
        import torch
        self.w = torch.randn((D, 32 * 32), generator=torch.Generator().manual_seed(12)).cuda()

    def __call__(self, patches):
        return patches.reshape(patches.shape[0], -1) @ self.w.T


def test_lfnet_detector_inside_a_bundler_session(ws):
    from bundletrack_amd import synthetic as S
    from bundletrack_amd.bundler import Bundler, FrameRef
    from bundletrack_amd.optimizer import OptimizerGpu
    sf = (R.SQRT2, 2.0 ** 0.25, 1.0, 2.0 ** -0.25, 1.0 / R.SQRT2)
    det = lfnet.LfnetDetector(ws, _ScoreNet(sf), _DescNet(), sf)
    seq = S.SyntheticSequence(n_frames=3, seed=S.config_seed(1), background=True)
    fm = S.SyntheticFeatureManager(seq, corr_per_pair=300)
    bundler = Bundler(OptimizerGpu(workspace=ws), fm, seq.K, seq.H, seq.W, window_size=5, max_BA_frames=5, detector=det)
    for k in range(3):
        depth, normals = seq.render(k)
        fr = FrameRef(id=0, pose_in_model=seq.poses_gt[0].astype(np.float32), n_keypts=0, depth_gpu=_t(depth), normal_gpu=_t(normals),
                      color_gpu=_t(S.make_color(seq.poses_gt[k], seq.K, seq.H, seq.W, seed=k)),
                      mask_gpu=_t(S.make_mask(seq.poses_gt[k], seq.K, seq.H, seq.W, seed=k)))
        fm.register(fr, k)
        bundler.process_new_frame(fr)
        m = int(det.last["n_kpts_host"][0])
        assert fr.status != "FAIL" and 0 < m <= 500
        assert tuple(fr.kpts_gpu.shape) == (m, 2) and tuple(fr.desc_gpu.shape) == (m, 24) and fr.n_keypts == m
        kxy = _np(det.last["kpts_xy"])[0, :m]
        assert np.array_equal(kxy, R.select(_np(det.last["max_heatmaps"])[0], R.params()))
        assert np.isfinite(_np(fr.desc_gpu)).all()


def _lfnet_driver():
    so = _lib.build_driver("lfnet_driver")
    lib = C.CDLL(so)
    lib.lfnet_keypoints_driver.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 8
    lib.lfnet_detector_driver.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 9
    return lib


@pytest.mark.parametrize("via_detector", [0, 1])
def test_cpp_host_equals_python(ws, golden, via_detector):
    import torch
    g = 1 if via_detector else 2                                        # the detector takes one square frame
    name, H, W, sf, prm, tol, cases = _group(golden, g)
    if via_detector:
        cases = cases[:1]
    want = _keypoints(ws, cases, sf, prm)
    drv = _lfnet_driver()
    n, K, P = len(cases), int(prm["top_k"]), int(prm["patch_size"])
    maps = _stack([c[0] for c in cases])
    photo, ori = _t(np.stack([c[1] for c in cases])), _t(np.stack([c[2] for c in cases]))
    f32 = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device="cuda")
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")
    out = [f32(n, H, W), f32(n, H, W), i32(n, K, 2), i32(n), f32(n, K, 2), f32(n, K), f32(n, K, 2), f32(n, K, P, P)]
    table = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
    outs = (C.c_void_p * 8)(*[o.data_ptr() for o in out])
    mh = np.array([m.shape[-2] for m in maps], np.int32)
    mw = np.array([m.shape[-1] for m in maps], np.int32)
    sfa = np.asarray(sf, np.float32)
    if via_detector:
        desc, dim = f32(K, P * P), C.c_int(0)
        rc = drv.lfnet_detector_driver(ws.handle, H, len(sf), K, prm["pad_size"], prm["crop_radius"], C.cast(table, C.c_void_p), mh.ctypes.data,
                                       mw.ctypes.data, sfa.ctypes.data, photo.data_ptr(), ori.data_ptr(), C.cast(outs, C.c_void_p), desc.data_ptr(),
                                       C.addressof(dim))
        assert rc == int(want["n_kpts_host"][0]) and dim.value == P * P
        assert np.array_equal(_np(desc)[:rc].reshape(rc, P, P).view(np.uint32), want["patches"][0, :rc].view(np.uint32))
    else:
        counts = np.zeros(n, np.int32)
        rc = drv.lfnet_keypoints_driver(ws.handle, n, H, W, len(sf), K, prm["pad_size"], prm["crop_radius"], C.cast(table, C.c_void_p), mh.ctypes.data,
                                        mw.ctypes.data, sfa.ctypes.data, photo.data_ptr(), ori.data_ptr(), C.cast(outs, C.c_void_p), counts.ctypes.data)
        assert rc == 0 and np.array_equal(counts, want["n_kpts_host"])
    for key, o in zip(("max_heatmaps", "max_scales", "kpts_xy", "n_kpts", "kpts", "kpts_scale", "kpts_ori", "patches"), out):
        assert np.array_equal(_np(o).view(np.uint32), want[key].view(np.uint32)), key
