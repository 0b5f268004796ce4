"""btba_apply_masks on the MI355X: exact equality with the CPU restatement (tests/mask_ref.py) of the final mask, depth,
normals, colour and ROI in both modes, on synthetic silhouettes and on the edge cases of labelling, tie rule, hull and dilation;
a batch of mixed frames across two launch chunks; determinism; the asynchronous form; bit-identity inside the mask; the
depth -> normals -> mask -> matching chain; the Python Bundler's ROI gate; and the C++ host layer.  One module-scoped workspace,
one C++ driver library loaded in-process (no child processes)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S

import mask_ref as R


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _maps(H, W, seed):
    """Random depth / normals / colour whose bits must survive inside the mask (NaN payloads and -0 included)."""
    rng = np.random.default_rng(seed)
    depth = rng.integers(0, 2**32, size=(H, W), dtype=np.uint32).view(np.float32)
    normal = rng.integers(0, 2**32, size=(H, W, 4), dtype=np.uint32).view(np.float32)
    color = rng.integers(1, 256, size=(H, W, 4), dtype=np.uint8)
    return depth, normal, color


def _run(ws, masks, maps, *, hull, d, color_none=(), want_roi=True):
    """btba_apply_masks through bundletrack_amd.segmentation on FrameRefs; returns the host copies."""
    import torch
    from bundletrack_amd.bundler import FrameRef
    from bundletrack_amd.segmentation import apply_masks
    frames = []
    for k, (m, (dep, nrm, col)) in enumerate(zip(masks, maps)):
        frames.append(FrameRef(id=k, pose_in_model=np.eye(4, dtype=np.float32), depth_gpu=_t(dep), normal_gpu=_t(nrm),
                               color_gpu=None if k in color_none else _t(col), mask_gpu=_t(m)))
    roi = apply_masks(ws, frames, largest_component_hull=hull, dilate=d, want_roi=want_roi)
    torch.cuda.synchronize()
    out = [(f.fg_mask_gpu.cpu().numpy(), f.depth_gpu.cpu().numpy(), f.normal_gpu.cpu().numpy(),
            None if f.color_gpu is None else f.color_gpu.cpu().numpy()) for f in frames]
    return out, roi, frames


def _check(ws, masks, *, hull, d, seed=0, color_none=()):
    maps = [_maps(m.shape[0], m.shape[1], seed + k) for k, m in enumerate(masks)]
    got, roi, _ = _run(ws, masks, maps, hull=hull, d=d, color_none=color_none)
    for k, (m, (dep, nrm, col)) in enumerate(zip(masks, maps)):
        M, rd, rn, rc, rroi = R.restate(m, dep, nrm, None if k in color_none else col, hull=hull, d=d)
        gM, gd, gn, gc = got[k]
        assert np.array_equal(gM, M), (k, int((gM != M).sum()))
        assert gd.tobytes() == rd.tobytes() and gn.tobytes() == rn.tobytes()
        assert (gc is None) == (rc is None) and (gc is None or gc.tobytes() == rc.tobytes())
        assert roi[k].tobytes() == rroi.tobytes(), (k, roi[k], rroi)
    return got, roi


def _silhouette(seed, **kw):
    pb = S.make_problem(2, 10, seed=seed, background=True)
    return S.make_mask(pb.poses_gt[1], pb.K, pb.H, pb.W, seed=seed, **kw)


def _small_cases():
    c = {}
    tie = np.zeros((40, 50), np.uint8)
    tie[25:30, 3:8] = 1                                      # same size, later in raster order
    tie[5:10, 40:45] = 7                                     # the first: wins the tie
    c["tie"] = tie
    diag = np.zeros((30, 30), np.uint8)
    for k in range(12):
        diag[2 + k, 2 + k] = 255                             # 8-connected diagonal: 12 pixels, one component
    diag[20:23, 20:23] = 255                                 # 9 pixels: largest only if the diagonal fell apart (4-connectivity)
    c["diag8"] = diag
    sp = np.zeros((63, 67), np.uint8)
    y, x, dr, n = 31, 33, 0, 1
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    while 0 <= y < 63 and 0 <= x < 67:
        for _ in range(2):
            for _ in range(n):
                if 0 <= y < 63 and 0 <= x < 67:
                    sp[y, x] = 1
                y, x = y + steps[dr][0], x + steps[dr][1]
            dr = (dr + 1) % 4
        n += 2
    c["spiral"] = sp
    comb = np.zeros((50, 70), np.uint8)
    comb[49, :] = 1
    comb[:, ::2] = 1
    c["comb"] = comb
    border = np.zeros((33, 35), np.uint8)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = 1
    border[16, 17] = 1
    c["border"] = border
    c["empty"] = np.zeros((20, 24), np.uint8)
    c["full"] = np.full((21, 19), 3, np.uint8)
    px = np.zeros((15, 17), np.uint8)
    px[7, 9] = 1
    c["pixel"] = px
    col = np.zeros((30, 30), np.uint8)
    col[[3, 4, 5, 6, 7, 8], [4, 5, 6, 7, 8, 9]] = 1
    col[20, 2:28] = 1                                        # a longer collinear component wins: a horizontal segment
    c["collinear"] = col
    rng = np.random.default_rng(9)
    c["odd_479x641"] = ((rng.random((479, 641)) < 0.02) * 255).astype(np.uint8) | np.pad(np.ones((100, 150), np.uint8), ((200, 179), (300, 191)))
    c["odd_7x3"] = np.array([[0, 1, 0], [0, 0, 0], [1, 1, 0], [0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, 0]], np.uint8)
    c["odd_1x1"] = np.ones((1, 1), np.uint8)
    c["odd_1x1_empty"] = np.zeros((1, 1), np.uint8)
    c["tall_2000x3"] = (np.random.default_rng(3).random((2000, 3)) < 0.6).astype(np.uint8)      # hull stack in global memory
    return c


SMALL = _small_cases()


@pytest.mark.parametrize("hull", [False, True])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_bit_exact_edge_cases(ws, name, hull):
    _check(ws, [SMALL[name]], hull=hull, d=5, seed=len(name))


@pytest.mark.parametrize("hull", [False, True])
@pytest.mark.parametrize("blobs", [False, True])
def test_bit_exact_synthetic_silhouettes(ws, hull, blobs):
    kw = dict(n_blobs=5, n_holes=6, bridge=True) if blobs else {}
    m = _silhouette(11, **kw)
    got, roi = _check(ws, [m], hull=hull, d=5)
    assert got[0][0].sum() > 5000 and roi[0][1] - roi[0][0] > 50


@pytest.mark.parametrize("hull", [False, True])
@pytest.mark.parametrize("d", [1, 3, 5, 15])
def test_bit_exact_dilation_sizes(ws, d, hull):
    _check(ws, [_silhouette(12, n_blobs=3, bridge=True)], hull=hull, d=d)
    _check(ws, [SMALL["comb"]], hull=hull, d=d)
    _check(ws, [SMALL["odd_7x3"]], hull=hull, d=d)


def _batch_masks(n, H=480, W=640):
    """n frames of 480 x 640 mixing silhouettes and every small case pasted at a varying place."""
    out, names = [], sorted(k for k in SMALL if SMALL[k].shape[0] <= H and SMALL[k].shape[1] <= W)
    for k in range(n):
        if k % 3 == 0:
            out.append(_silhouette(20 + k, n_blobs=k % 5, n_holes=k % 4, bridge=k % 2 == 0))
            continue
        m = np.zeros((H, W), np.uint8)
        s = SMALL[names[k % len(names)]]
        y0, x0 = (k * 37) % (H - s.shape[0] + 1), (k * 101) % (W - s.shape[1] + 1)
        if k % 7 == 1:
            y0, x0 = H - s.shape[0], W - s.shape[1]          # touching the bottom-right border
        m[y0:y0 + s.shape[0], x0:x0 + s.shape[1]] = s
        out.append(m)
    return out


@pytest.mark.parametrize("hull", [False, True])
def test_bit_exact_batch_across_chunks(ws, hull):
    masks = _batch_masks(34)                                 # 32 frames per launch: two chunks
    _check(ws, masks, hull=hull, d=5, seed=100, color_none=(1, 5, 32))


@pytest.mark.parametrize("hull", [False, True])
def test_repeatable_and_async_form_equal(ws, hull):
    masks = _batch_masks(6)
    maps = [_maps(480, 640, 200 + k) for k in range(6)]
    a, roi_a, _ = _run(ws, masks, maps, hull=hull, d=5)
    b, roi_b, _ = _run(ws, masks, maps, hull=hull, d=5)
    c, roi_c, _ = _run(ws, masks, maps, hull=hull, d=5, want_roi=False)       # roi_out = NULL: asynchronous, then a sync
    assert roi_c is None and roi_a.tobytes() == roi_b.tobytes()
    for x, y, z in zip(a, b, c):
        for p, q, r in zip(x, y, z):
            assert p.tobytes() == q.tobytes() == r.tobytes()


def test_inside_the_mask_maps_are_untouched(ws):
    m = _silhouette(31, n_blobs=2)
    maps = [_maps(480, 640, 31)]
    got, _, _ = _run(ws, [m], maps, hull=True, d=5)
    M, dep, nrm, col = got[0]
    inside = M == 1
    assert inside.sum() > 5000
    assert dep[inside].tobytes() == maps[0][0][inside].tobytes()
    assert nrm[inside].tobytes() == maps[0][1][inside].tobytes()
    assert col[inside].tobytes() == maps[0][2][inside].tobytes()
    assert not dep[~inside].view(np.uint32).any() and not nrm[~inside].view(np.uint32).any() and not col[~inside].any()


def test_rejects_bad_arguments_on_a_workspace(ws):
    import torch
    from bundletrack_amd.bundler import FrameRef
    from bundletrack_amd.segmentation import apply_masks
    f = FrameRef(id=0, pose_in_model=np.eye(4, dtype=np.float32), depth_gpu=torch.zeros((8, 8), device="cuda"),
                 normal_gpu=torch.zeros((8, 8, 4), device="cuda"), mask_gpu=torch.ones((8, 8), dtype=torch.uint8, device="cuda"))
    for d in (0, 4, 17):
        with pytest.raises(_lib.BtbaError):
            apply_masks(ws, [f], dilate=d)
    apply_masks(ws, [f], dilate=15)
    assert f.roi == (0.0, 7.0, 0.0, 7.0)


def test_depth_normals_mask_match_chain(ws):
    """process_depth -> depth_to_normals -> apply_masks -> match_pairs on background-rendered frames: every match lies on
    the final mask in both frames."""
    import torch
    from bundletrack_amd.bundler import FrameRef
    from bundletrack_amd.matching import match_pairs
    from bundletrack_amd.optimizer import depth_to_normals, process_depth
    from bundletrack_amd.segmentation import apply_masks
    pb = S.make_problem(3, 10, seed=41, background=True)
    kp = S.make_keypoints(pb, 600, 400, D=64, seed=41)
    frames = []
    for k in range(3):
        dep = process_depth(ws, _t(pb.depth[k]))
        nrm = depth_to_normals(ws, dep, pb.K)
        m = S.make_mask(pb.poses_gt[k], pb.K, pb.H, pb.W, seed=k, n_blobs=3)
        frames.append(FrameRef(id=k, pose_in_model=pb.poses_gt[k].astype(np.float32), depth_gpu=dep, normal_gpu=nrm, mask_gpu=_t(m),
                               kpts_gpu=_t(kp.kpts[k].astype(np.float32)), desc_gpu=_t(kp.desc[k].astype(np.float32))))
    apply_masks(ws, frames)
    res = match_pairs(ws, frames, [(1, 0), (2, 1), (2, 0)], K=pb.K, H=pb.H, W=pb.W)
    torch.cuda.synchronize()
    total = 0
    for (a, b), m in zip([(1, 0), (2, 1), (2, 0)], res.per_pair):
        for fi, idx in ((a, m["idx_a"]), (b, m["idx_b"])):
            M = frames[fi].fg_mask_gpu.cpu().numpy()
            kpt = kp.kpts[fi][idx].astype(np.float64)
            u = (np.sign(kpt) * np.floor(np.abs(kpt) + 0.5)).astype(int)
            assert M[u[:, 1], u[:, 0]].all()
        total += len(m)
    assert total > 100


def test_python_bundler_segments_frames_and_fails_a_tiny_roi(ws):
    """A session through Bundler.process_new_frame with mask_gpu set: frames are segmented before use and bundle-adjusted;
    a frame whose mask is a 5 x 5 blob (9 px wide after the 5 x 5 dilation: umax - umin = 8 < 10) comes out FAIL through the
    real ROI, with the reference's plain return (no need_reinit, not in the window)."""
    from bundletrack_amd.bundler import Bundler, FrameRef
    from bundletrack_amd.optimizer import OptimizerGpu
    seq = S.SyntheticSequence(n_frames=5, seed=S.config_seed(1), background=True)
    fm = S.SyntheticFeatureManager(seq, corr_per_pair=300)
    bundler = Bundler(OptimizerGpu(workspace=ws), fm, seq.K, seq.H, seq.W, window_size=5, max_BA_frames=5)
    frames = []
    for k in range(5):
        depth, normals = seq.render(k)
        mask = S.make_mask(seq.poses_gt[k], seq.K, seq.H, seq.W, seed=k)
        if k == 3:
            mask = np.zeros_like(mask)
            mask[100:105, 200:205] = 255
        fr = FrameRef(id=0, pose_in_model=seq.poses_gt[0].astype(np.float32), n_keypts=300, depth_gpu=_t(depth), normal_gpu=_t(normals), mask_gpu=_t(mask))
        fm.register(fr, k)
        bundler.process_new_frame(fr)
        frames.append(fr)
        _, _, _, _, roi = R.restate(mask, depth, normals, None, hull=False, d=5)
        assert np.asarray(fr.roi, np.float32).tobytes() == roi.tobytes()
        if k == 3:
            assert fr.status == "FAIL" and not bundler.need_reinit and fr not in bundler.frames
            assert fr.roi[1] - fr.roi[0] == 8
        else:
            assert fr.status != "FAIL"
            assert not fr.depth_gpu.cpu().numpy()[fr.fg_mask_gpu.cpu().numpy() == 0].any()
    assert bundler.n_ba_calls == 3                                   # frames 1, 2 and 4
    assert [f.id for f in bundler.frames] == [0, 1, 2, 3] and bundler.frames[3] is frames[4]
    assert all(np.isfinite(f.pose_in_model).all() for f in frames)


def _driver():
    so = _lib.build_driver("mask_driver")
    f = C.CDLL(so).mask_driver
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
    return f


@pytest.mark.parametrize("via_bundler", [0, 1])
@pytest.mark.parametrize("hull", [False, True])
def test_cpp_host_layer_equals_python(ws, hull, via_bundler):
    import torch
    masks = _batch_masks(5)
    masks[4] = np.zeros_like(masks[4])
    masks[4][300:305, 100:105] = 1                                    # FAIL by ROI
    maps = [_maps(480, 640, 300 + k) for k in range(5)]
    py, roi_py, _ = _run(ws, masks, maps, hull=hull, d=5)
    dm = [_t(m) for m in masks]
    dd, dn, dc = [_t(x[0]) for x in maps], [_t(x[1]) for x in maps], [_t(x[2]) for x in maps]
    do = [torch.empty((480, 640), dtype=torch.uint8, device="cuda") for _ in masks]
    ptr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    roi = np.zeros((5, 4), np.float32)
    st = np.zeros(5, np.int32)
    rc = _driver()(ws.handle.value, via_bundler, 5, 480, 640, int(hull), 5, ptr(dm), ptr(dd), ptr(dn), ptr(dc), ptr(do), roi.ctypes.data, st.ctypes.data)
    assert rc == 0
    torch.cuda.synchronize()
    assert roi.tobytes() == roi_py.tobytes()
    for k in range(5):
        assert do[k].cpu().numpy().tobytes() == py[k][0].tobytes()
        assert dd[k].cpu().numpy().tobytes() == py[k][1].tobytes() and dn[k].cpu().numpy().tobytes() == py[k][2].tobytes()
        assert dc[k].cpu().numpy().tobytes() == py[k][3].tobytes()
    if via_bundler:
        small = (roi[:, 1] - roi[:, 0] < 10) | (roi[:, 3] - roi[:, 2] < 10)
        assert small[4] and np.array_equal(st == 0, small)             # Frame::FAIL == 0 exactly where the ROI is under 10 px
