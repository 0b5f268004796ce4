"""btba_vos_* on the MI355X: the propagation against the reference's stored results and the fp64 restatement under the measured bars
(tests/golden/vos/vos_reference.npz, tests/vos_ref.py) at every path's shapes, repeatability and batch independence, the one-hot
output, the two interpolations against torch's, the input normalisation, the argument checks, a 30-frame session through
MaskPropagator held step by step against the restatement on its own history, the C++ MaskPropagator, and the Bundler's hook.
One module-scoped workspace."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib
from bundletrack_amd import vos

import vos_ref as V


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


@pytest.fixture(scope="module")
def golden():
    return V.load_golden()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _propagate(ws, items, Hd, Wd, params=None):
    """items: (refs [n, C, HW], labels [n, d, HW], tgt [C, HW], n_dense) in numpy -> [(pred [d, HW], onehot [d, HW])] in numpy."""
    import torch
    refs = [[_t(r) for r in it[0]] for it in items]
    labs = [[_t(l) for l in it[1]] for it in items]
    pred, hot = vos.propagate(ws, refs, labs, [_t(it[2]) for it in items], [it[3] for it in items], Hd, Wd, params)
    torch.cuda.synchronize()
    return [(p.cpu().numpy().reshape(p.shape[0], -1), h.cpu().numpy().reshape(h.shape[0], -1)) for p, h in zip(pred, hot)]


def _hold(pred, hot, p64, tol, what):
    err, ok = V.check(pred, p64, tol, arg=np.argmax(hot, 0))
    print(f"{what}: err {err:.3e} tol {tol:.3e}")
    assert np.isfinite(pred).all() and ok, (what, err, tol)


def _golden_cases(golden, group):
    name, Hd, Wd, H, W, Cn, d, scale, idxs = V.GROUPS[group]
    feats = V.features(golden[f"{name}_q"], golden[f"{name}_mult"])
    labels, tol = golden[f"{name}_labels"], float(golden[f"tol_{name}"])
    for k, f in enumerate(idxs):
        sel, n_dense = V.sample_frames(f)
        yield f, (feats[sel], labels[sel], feats[f], n_dense), Hd, Wd, golden[f"{name}_pred"][k], tol


@pytest.mark.parametrize("group", [0, 1, 2])
def test_propagate_against_the_reference_vectors(ws, golden, group):
    """Every stored case: within the group's measured bar of the fp64 values, decisions equal above the margin; and as close to
    the reference's own fp32 result as two results inside that bar can be.  Group 1 is the large-logit one: finite output."""
    for f, item, Hd, Wd, pred_ref, tol in _golden_cases(golden, group):
        (pred, hot), = _propagate(ws, [item], Hd, Wd)
        p64 = V.predict(*item[:3], item[3], Hd, Wd)
        _hold(pred, hot, p64, tol, f"{V.GROUPS[group][0]} frame_idx {f}")
        assert float((np.abs(pred.astype(np.float64) - pred_ref) / np.abs(p64).max(0, keepdims=True)).max()) <= 2.0 * tol


# Hd, Wd, C, d, n_ref, n_dense, golden group whose bar applies (by C and logit scale: fewer channels round less, so C = 8 is held to the
# C = 24 bar; C = 264, the narrow-tile path above 256 channels, to the C = 256 bar)
FRESH = [(1, 1, 8, 2, 1, 0, 0), (7, 9, 24, 3, 4, 4, 0), (8, 8, 8, 16, 9, 4, 0), (15, 20, 256, 3, 9, 4, 2), (7, 9, 24, 2, 32, 0, 0),
         (8, 8, 24, 16, 32, 32, 0), (7, 9, 8, 2, 1, 1, 0), (7, 9, 264, 2, 4, 2, 2)]


def _fresh(seed, Hd, Wd, Cn, d, n_ref, n_dense):
    q, mult, labels = V.make_history(seed, Hd, Wd, 8 * Hd - (4 if Hd > 1 else 0), 8 * Wd - (4 if Wd > 1 else 0), Cn, d, n_ref + 1)
    feats = V.features(q, mult)
    return feats[:n_ref], labels[:n_ref], feats[n_ref], n_dense


@pytest.mark.parametrize("case", FRESH)
def test_propagate_against_fp64_on_fresh_seeds(ws, golden, case):
    Hd, Wd, Cn, d, n_ref, n_dense, group = case
    tol = float(golden[f"tol_{V.GROUPS[group][0]}"])
    for seed in (101, 102):
        item = _fresh(seed + 7 * n_ref + Cn, Hd, Wd, Cn, d, n_ref, n_dense)
        (pred, hot), = _propagate(ws, [item], Hd, Wd)
        _hold(pred, hot, V.predict(*item[:3], n_dense, Hd, Wd), tol, f"{case} seed {seed}")
        assert np.array_equal(np.argmax(hot, 0), np.argmax(pred, 0)) and np.array_equal(hot.sum(0), np.ones(Hd * Wd, np.float32))


def test_mixed_batch_twice_and_alone(ws, golden):
    """One batch whose items differ in n_ref and n_dense (six items: two launch chunks): each inside the bar, the same bits when the
    call is repeated, and the same bits as each item propagated alone."""
    Hd, Wd, Cn, d = 7, 9, 24, 3
    tol = float(golden[f"tol_{V.GROUPS[0][0]}"])
    items = [_fresh(300 + k, Hd, Wd, Cn, d, n_ref, n_dense) for k, (n_ref, n_dense) in enumerate([(1, 0), (4, 4), (9, 4), (32, 0), (9, 9), (2, 1)])]
    a = _propagate(ws, items, Hd, Wd)
    b = _propagate(ws, items, Hd, Wd)
    for k, (item, (pred, hot)) in enumerate(zip(items, a)):
        _hold(pred, hot, V.predict(*item[:3], item[3], Hd, Wd), tol, f"batch item {k}")
        assert np.array_equal(pred.view(np.uint32), b[k][0].view(np.uint32)) and np.array_equal(hot, b[k][1])
        (p1, h1), = _propagate(ws, [item], Hd, Wd)
        assert np.array_equal(pred.view(np.uint32), p1.view(np.uint32)) and np.array_equal(hot, h1)


def test_parameters_reach_the_kernel(ws, golden):
    """Sigmas and temperature other than the defaults against the fp64 restatement with the same values."""
    Hd, Wd = 7, 9
    tol = float(golden[f"tol_{V.GROUPS[0][0]}"])
    item = _fresh(411, Hd, Wd, 24, 2, 9, 4)
    (pred, hot), = _propagate(ws, [item], Hd, Wd, dict(sigma_dense=3.0, sigma_sparse=5.5, temperature=0.5))
    _hold(pred, hot, V.predict(*item[:3], 4, Hd, Wd, sigma_dense=3.0, sigma_sparse=5.5, temperature=0.5), tol, "sigma 3 / 5.5, temperature 0.5")


@pytest.mark.parametrize("H,W", [(52, 68), (64, 64), (8, 8)])
def test_first_labels_and_masks_against_torch(ws, H, W):
    import torch
    Hd, Wd = V.grid_of(H, W)
    lab = V.label_image(H, W, 3, 1, seed=H)
    down = torch.nn.functional.interpolate(torch.from_numpy(V.onehot(lab, 3))[None], size=(Hd, Wd), mode="bilinear", align_corners=False)[0].numpy()
    got = vos.first_labels(ws, _t(lab), 3).cpu().numpy()
    assert got.shape == down.shape and np.abs(got - down).max() <= 1e-6
    pred = np.random.default_rng(H * W).random((3, Hd, Wd), dtype=np.float32)
    up = torch.nn.functional.interpolate(torch.from_numpy(pred)[None], size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
    cls = vos.masks(ws, _t(pred), H, W).cpu().numpy()
    assert cls.shape == (H, W) and cls.dtype == np.uint8
    ok, left = V.decisions_ok(cls, up.reshape(3, -1).astype(np.float64), 1e-6)
    assert ok and left <= 0.02 * H * W


def test_inputs_against_numpy(ws):
    rng = np.random.default_rng(5)
    H, W, n = 37, 53, 35                                   # two launch chunks
    bgr = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    bgr.reshape(n, -1, 3)[0, :256, :] = np.arange(256)[:, None]          # every byte value
    got = vos.normalize_inputs(ws, [_t(b) for b in bgr]).cpu().numpy()
    want = V.normalize_inputs(bgr)
    assert got.shape == want.shape == (n, 3, H, W)
    assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()


def test_refusals(ws):
    """Every BTBA_EINVAL rule of the four device calls, on real buffers."""
    import torch
    L, h = _lib.lib(), ws.handle
    Hd, Wd, Cn, d = 3, 4, 8, 2
    f = torch.zeros((Cn, Hd * Wd), device="cuda")
    l = torch.zeros((d, Hd * Wd), device="cuda")
    po, ho = torch.zeros((d, Hd * Wd), device="cuda"), torch.zeros((d, Hd * Wd), device="cuda")
    one = (C.c_void_p * 1)

    def call(prm=None, n_items=1, Cn=Cn, d=d, Hd=Hd, Wd=Wd, n_ref=1, n_dense=0, ref=f.data_ptr(), lab=l.data_ptr(), tgt=f.data_ptr(), pred=po.data_ptr(),
             hot=ho.data_ptr(), hws=h, tables=True):
        nr, nd = np.array([n_ref] * 1, np.int32), np.array([n_dense], np.int32)
        k = max(n_ref, 1)
        rt, lt = (C.c_void_p * k)(*[ref] * k), (C.c_void_p * k)(*[lab] * k)
        return L.btba_vos_propagate(hws, C.byref(prm if prm is not None else _lib.vos_params()), n_items, Cn, d, Hd, Wd, nr.ctypes.data, nd.ctypes.data,
                                    rt if tables else None, lt, one(tgt), one(pred), one(hot))

    assert call() == _lib.BTBA_OK
    bad = [dict(hws=None), dict(n_items=0), dict(Cn=12), dict(Cn=0), dict(Cn=520), dict(d=1), dict(d=17), dict(Hd=0), dict(Wd=0), dict(Hd=257, Wd=256),
           dict(n_ref=0), dict(n_ref=33), dict(n_dense=-1), dict(n_dense=2), dict(ref=None), dict(lab=None), dict(tgt=None), dict(pred=None),
           dict(ref=f.data_ptr() + 2), dict(pred=po.data_ptr() + 1), dict(hot=ho.data_ptr() + 2), dict(tables=False),
           dict(prm=_lib.vos_params(sigma_dense=0.0)), dict(prm=_lib.vos_params(sigma_sparse=-2.0)), dict(prm=_lib.vos_params(ref_num=0)),
           dict(prm=_lib.vos_params(temperature=float("inf")))]
    for kw in bad:
        assert call(**kw) == _lib.BTBA_EINVAL, kw
    img = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    out = torch.zeros((16, 2, 2), device="cuda")
    assert L.btba_vos_first_labels(h, 16, 16, 2, img.data_ptr(), out.data_ptr()) == _lib.BTBA_OK
    for args in ((None, 16, 16, 2, img.data_ptr(), out.data_ptr()), (h, 0, 16, 2, img.data_ptr(), out.data_ptr()), (h, 16, 0, 2, img.data_ptr(), out.data_ptr()),
                 (h, 16, 16, 1, img.data_ptr(), out.data_ptr()), (h, 16, 16, 17, img.data_ptr(), out.data_ptr()), (h, 16, 16, 2, None, out.data_ptr()),
                 (h, 16, 16, 2, img.data_ptr(), None), (h, 2056, 2056, 2, img.data_ptr(), out.data_ptr())):
        assert L.btba_vos_first_labels(*args) == _lib.BTBA_EINVAL, args
    assert L.btba_vos_masks(h, 2, 2, 2, 16, 16, out.data_ptr(), img.data_ptr()) == _lib.BTBA_OK
    for args in ((None, 2, 2, 2, 16, 16, out.data_ptr(), img.data_ptr()), (h, 1, 2, 2, 16, 16, out.data_ptr(), img.data_ptr()),
                 (h, 17, 2, 2, 16, 16, out.data_ptr(), img.data_ptr()), (h, 2, 0, 2, 16, 16, out.data_ptr(), img.data_ptr()),
                 (h, 2, 2, 2, 0, 16, out.data_ptr(), img.data_ptr()), (h, 2, 257, 256, 16, 16, out.data_ptr(), img.data_ptr()),
                 (h, 2, 2, 2, 16, 16, None, img.data_ptr()), (h, 2, 2, 2, 16, 16, out.data_ptr(), None)):
        assert L.btba_vos_masks(*args) == _lib.BTBA_EINVAL, args
    bgr = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
    rgb = torch.zeros((1, 3, 4, 4), device="cuda")
    assert L.btba_vos_inputs(h, 1, 4, 4, one(bgr.data_ptr()), rgb.data_ptr()) == _lib.BTBA_OK
    for args in ((None, 1, 4, 4, one(bgr.data_ptr()), rgb.data_ptr()), (h, 0, 4, 4, one(bgr.data_ptr()), rgb.data_ptr()), (h, 1, 0, 4, one(bgr.data_ptr()), rgb.data_ptr()),
                 (h, 1, 4, 4, None, rgb.data_ptr()), (h, 1, 4, 4, one(None), rgb.data_ptr()), (h, 1, 4, 4, one(bgr.data_ptr()), None)):
        assert L.btba_vos_inputs(*args) == _lib.BTBA_EINVAL, args
    torch.cuda.synchronize()


# ---- sessions ---------------------------------------------------------------------------------------------------------------

H_S, W_S, C_S, N_S = 52, 68, 24, 30


def _session_frames(n=N_S, H=H_S, W=W_S, Cn=C_S, seed=9):
    """A blob that drifts over a textured background: per frame the grid features [C, Hd*Wd] -- a fixed random projection of position
    and colour -- and the first frame's 0 / 255 label image."""
    rng = np.random.default_rng(seed)
    Hd, Wd = V.grid_of(H, W)
    proj = rng.standard_normal((Cn, 5)) * 1.2
    gy, gx = np.mgrid[0:Hd, 0:Wd]
    feats = []
    for k in range(n):
        cy, cx = 2.5 + 0.05 * k, 2.0 + 0.15 * k
        blob = ((gy - cy) ** 2 + (gx - cx) ** 2 <= 4.0)
        colour = np.where(blob[None], np.array([0.9, 0.2, 0.1])[:, None, None], np.array([0.1, 0.4, 0.8])[:, None, None]) + 0.05 * rng.standard_normal((3, Hd, Wd))
        x = np.concatenate([gy[None] / Hd, gx[None] / Wd, colour]).reshape(5, -1)
        feats.append((proj @ x).astype(np.float32))
    y, x = np.mgrid[0:H, 0:W]
    label = (((y / 8.0 - 0.5 - 2.5) ** 2 + (x / 8.0 - 0.5 - 2.0) ** 2 <= 4.0) * 255).astype(np.uint8)
    return np.stack(feats), label


def _run_session(ws, feats, label, params=None, d=2):
    """MaskPropagator over the frames; per step (class map, pred, one-hot, the sampled history as the device held it, n_dense)."""
    import torch
    mp = vos.MaskPropagator(ws, d, H_S, W_S, C=feats.shape[1], params=params)
    mp.start(_t(label), _t(feats[0]))
    steps = []
    for f in range(1, feats.shape[0]):
        idx, n_dense = vos.sample_frames(f, mp.params)
        hist = [mp.history(i) for i in idx]
        refs, labs = np.stack([h[0].cpu().numpy() for h in hist]), np.stack([h[1].cpu().numpy() for h in hist])
        cls = mp.step(_t(feats[f]))
        torch.cuda.synchronize()
        steps.append((cls.cpu().numpy(), mp.last_pred.cpu().numpy().reshape(d, -1), mp.history(f)[1].cpu().numpy(), refs, labs, n_dense))
    return mp, steps


@pytest.mark.parametrize("rng", [40, 10])
def test_session_step_by_step(ws, rng):
    """30 frames (across frame_idx 9 -> 10 and 15 -> 16; with range 10 the ring of 15 slots wraps): every step against the fp64
    restatement on the history the device itself held, so no flipped decision compounds.  The bar is measured as the golden file's
    is: 4 x the largest error of the fp32 restatement over the session's steps."""
    feats, label = _session_frames()
    Hd, Wd = V.grid_of(H_S, W_S)
    mp, steps = _run_session(ws, feats, label, dict(range=rng))
    assert mp.values == [0, 255] and mp.slots == rng + 5 and mp.n_frames == N_S
    p64s = [V.predict(refs, labs, feats[f + 1], n_dense, Hd, Wd) for f, (_, _, _, refs, labs, n_dense) in enumerate(steps)]
    tol = 4.0 * max(V.rel_err(V.predict(refs, labs, feats[f + 1], n_dense, Hd, Wd, dtype=np.float32), p64s[f])
                    for f, (_, _, _, refs, labs, n_dense) in enumerate(steps))
    assert 1e-7 < tol < 1e-3
    fg = 0
    for f, (cls, pred, hot, refs, labs, n_dense) in enumerate(steps):
        _hold(pred, hot, p64s[f], tol, f"range {rng} frame_idx {f + 1}")
        assert np.array_equal(np.argmax(hot, 0), np.argmax(pred, 0))
        want, up = V.masks(pred, Hd, Wd, H_S, W_S)
        ok, left = V.decisions_ok(cls, up.reshape(2, -1).astype(np.float64), 1e-6)
        assert ok and left <= 0.02 * H_S * W_S
        fg += int(cls.any())
    assert fg == len(steps)                                  # the blob is tracked in every frame


def _vos_driver():
    so = _lib.build_driver("vos_driver")
    lib = C.CDLL(so)
    lib.vos_session_driver.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 7
    lib.vos_bundler_driver.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 11
    return lib


@pytest.mark.parametrize("via_bundler", [0, 1])
def test_cpp_mask_propagator_equals_python(ws, via_bundler):
    """btba::MaskPropagator on caller-owned buffers, driven directly and through btba::Bundler::processNewFrame's hook (frames that
    bring only their BGR image after the annotated first one), gives the Python MaskPropagator's class maps; the ring of 15 slots wraps."""
    import torch
    drv = _vos_driver()
    feats, label = _session_frames()
    rng, d = 10, 2
    Hd, Wd = V.grid_of(H_S, W_S)
    _, steps = _run_session(ws, feats, label, dict(range=rng))
    small, _ = V.compact_labels(label)                      # the C++ start takes classes 0 .. d-1
    ring_f = torch.zeros((rng + 5, C_S, Hd * Wd), device="cuda")
    ring_l = torch.zeros((rng + 5, d, Hd * Wd), device="cuda")
    pred = torch.zeros((d, Hd * Wd), device="cuda")
    mask = torch.zeros((H_S, W_S), dtype=torch.uint8, device="cuda")
    out = torch.zeros((N_S - 1, H_S, W_S), dtype=torch.uint8, device="cuda")
    fin, lin = _t(feats), _t(small)
    torch.cuda.synchronize()
    args = [ws.handle.value, d, H_S, W_S, C_S, rng, N_S, fin.data_ptr(), lin.data_ptr(), ring_f.data_ptr(), ring_l.data_ptr(), pred.data_ptr(),
            mask.data_ptr(), out.data_ptr()]
    if via_bundler:
        bgr = torch.from_numpy(np.random.default_rng(1).integers(0, 256, size=(N_S, H_S, W_S, 3), dtype=np.uint8)).cuda()
        depth, normal = torch.ones((H_S, W_S), device="cuda"), torch.zeros((H_S, W_S, 4), device="cuda")
        rgb = torch.zeros((3, H_S, W_S), device="cuda")
        rc = drv.vos_bundler_driver(*args, (C.c_void_p * N_S)(*[bgr[k].data_ptr() for k in range(N_S)]), depth.data_ptr(), normal.data_ptr(), rgb.data_ptr())
    else:
        rc = drv.vos_session_driver(*args)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for f, st in enumerate(steps):
        assert np.array_equal(got[f], st[0]), f
    assert np.array_equal(pred.cpu().numpy().view(np.uint32), steps[-1][1].view(np.uint32))
    if via_bundler:
        assert np.array_equal(rgb.cpu().numpy(), V.normalize_inputs(bgr[-1:].cpu().numpy())[0]) or \
            (np.abs(rgb.cpu().numpy() - V.normalize_inputs(bgr[-1:].cpu().numpy())[0]) <= np.spacing(np.abs(V.normalize_inputs(bgr[-1:].cpu().numpy())[0]))).all()


def test_bundler_hook_equals_masks_by_hand(ws, tmp_path):
    """A Bundler with a stub segmenter and a MaskPropagator, fed frames that bring only their images after the annotated first one,
    reaches the poses of the same session fed the propagator's masks through mask_gpu by hand."""
    import torch
    from bundletrack_amd import synthetic as S
    from bundletrack_amd.bundler import Bundler, FrameRef
    from bundletrack_amd.optimizer import OptimizerGpu, depth_to_normals, process_depth
    n, Cn = 4, 8
    seq = S.SyntheticSequence(n_frames=n, seed=S.config_seed(1), background=True)
    H, W = seq.H, seq.W
    gen = torch.Generator().manual_seed(3)
    proj = torch.randn((Cn, 3), generator=gen).cuda()
    masks0 = [S.make_mask(seq.poses_gt[k], seq.K, H, W, seed=k) for k in range(n)]
    bgrs = []
    for k in range(n):
        on = (masks0[k] > 0)[..., None]
        bgrs.append(np.where(on, np.array([30, 60, 220], np.uint8), np.array([200, 120, 40], np.uint8)).astype(np.uint8))

    def segmenter(rgb):                                      # 8 x 8 mean colour, projected: [1, 3, H, W] -> [C, Hd, Wd]
        pooled = torch.nn.functional.avg_pool2d(rgb, 8, ceil_mode=True)[0]
        return torch.einsum("ck,khw->chw", proj, pooled).contiguous()

    def session(by_hand, pose_dir):
        fm = S.SyntheticFeatureManager(seq, corr_per_pair=300)
        mp = vos.MaskPropagator(ws, 2, H, W, C=Cn)
        kw = {} if by_hand else dict(segmenter=segmenter, mask_propagator=mp)
        bundler = Bundler(OptimizerGpu(workspace=ws), fm, seq.K, H, W, window_size=5, max_BA_frames=5, pose_dir=pose_dir, **kw)
        frames = []
        for k in range(n):
            fr = FrameRef(id=0, pose_in_model=seq.poses_gt[0].astype(np.float32), n_keypts=300)
            fr.depth_gpu = process_depth(ws, _t(seq.render(k)[0]))
            fr.normal_gpu = depth_to_normals(ws, fr.depth_gpu, seq.K)
            fr.bgr_gpu = _t(bgrs[k])
            if k == 0:
                fr.mask_gpu = _t((masks0[0] > 0).astype(np.uint8) * 255)
            if by_hand:
                feats = segmenter(vos.normalize_inputs(ws, [fr.bgr_gpu]))
                if k == 0:
                    mp.start(fr.mask_gpu, feats)
                else:
                    fr.mask_gpu = mp.step(feats)
                fr.bgr_gpu = None
            fm.register(fr, k)
            bundler.process_new_frame(fr)
            assert fr.status != "FAIL" and fr.mask_gpu is not None and bool(fr.mask_gpu.any())
            frames.append(fr)
        assert bundler.n_ba_calls == n - 1 and mp.n_frames == n
        return frames

    a = session(True, str(tmp_path / "a"))
    b = session(False, str(tmp_path / "b"))
    for fa, fb in zip(a, b):
        assert np.array_equal(fa.mask_gpu.cpu().numpy(), fb.mask_gpu.cpu().numpy())
        assert np.array_equal(fa.pose_in_model, fb.pose_in_model)
