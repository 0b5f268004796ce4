"""btba_detector_inputs / btba_detector_keypoints_to_image on the MI355X: exact equality with the CPU restatement
(tests/detector_ref.py) of the BGR bytes and grey floats on small, wide, tall, full-image, border, odd-size, copy and box-average
ROIs; a 40-frame batch across two launch chunks; bit-exact keypoint back-mapping at ragged counts, in place and out of place; the
round trip; determinism and the asynchronous form; the depth -> normals -> mask -> detector input -> stand-in detector ->
back-mapping -> matching chain; the Python Bundler's detector step; and the C++ DetectorFeatureManager.  One module-scoped
workspace, one C++ driver library loaded in-process (no child processes)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S

import detector_ref as R


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _color(H, W, seed):
    if (H, W) == (480, 640):
        pb = S.make_problem(2, 10, seed=seed, background=True)
        return S.make_color(pb.poses_gt[1], pb.K, H, W, seed=seed)
    return np.random.default_rng(seed).integers(0, 256, (H, W, 4), dtype=np.uint8)


def _frames(colors, rois):
    from bundletrack_amd.bundler import FrameRef
    return [FrameRef(id=k, pose_in_model=np.eye(4, dtype=np.float32), color_gpu=_t(c), roi=tuple(float(v) for v in r))
            for k, (c, r) in enumerate(zip(colors, rois))]


def _check(ws, colors, rois, S_=400):
    import torch
    from bundletrack_amd.detection import prepare_detector_inputs
    bgr, gray = prepare_detector_inputs(ws, _frames(colors, rois), out_size=S_)
    torch.cuda.synchronize()
    bgr, gray = bgr.cpu().numpy(), gray.cpu().numpy()
    assert bgr.shape == (len(colors), S_, S_, 3) and gray.shape == (len(colors), 1, S_, S_)
    for k, (c, r) in enumerate(zip(colors, rois)):
        rb, rg = R.inputs(c, r, S_)
        assert np.array_equal(bgr[k], rb), (k, r, int((bgr[k] != rb).sum()))
        assert gray[k, 0].tobytes() == rg.tobytes(), (k, r)
    return bgr, gray


CASES = {
    "10x10": (480, 640, (100, 110, 200, 210), 400),
    "wide": (480, 640, (37, 600, 150, 171), 400),
    "tall": (480, 640, (300, 321, 13, 470), 400),
    "full": (480, 640, (0, 640, 0, 480), 400),
    "full_mask_roi": (480, 640, (0, 639, 0, 479), 400),
    "left": (480, 640, (0, 50, 200, 260), 400),
    "right": (480, 640, (590, 640, 200, 260), 400),
    "top": (480, 640, (300, 360, 0, 45), 400),
    "bottom": (480, 640, (300, 360, 430, 480), 400),
    "odd_image": (37, 53, (3, 50, 1, 36), 400),
    "odd_small_S": (37, 53, (3, 50, 1, 36), 12),
    "S4": (37, 53, (0, 53, 0, 37), 4),
    "upscale_2x": (480, 640, (200, 400, 100, 300), 400),
    "side_eq_S": (480, 640, (100, 500, 40, 440), 400),
    "side_2S": (1000, 1000, (100, 900, 150, 950), 400),
    "side_2S_padded": (1000, 1000, (0, 800, 100, 713), 400),
    "S_not_400": (480, 640, (120, 470, 60, 333), 256),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_exact_inputs(ws, name):
    H, W, roi, S_ = CASES[name]
    _check(ws, [_color(H, W, 11)], [roi], S_)


def _batch(n, seed=5):
    rng = np.random.default_rng(seed)
    colors, rois = [], []
    for k in range(n):
        colors.append(_color(480, 640, k % 6))
        w, h = int(rng.integers(10, 640)), int(rng.integers(10, 480))
        u, v = int(rng.integers(0, 640 - w + 1)), int(rng.integers(0, 480 - h + 1))
        rois.append((u, u + w, v, v + h))
    rois[3] = (0, 400, 0, 400)                                        # side == S
    if n > 37:
        rois[37] = (0, 640, 0, 480)
    return colors, rois


def test_bit_exact_batch_across_chunks(ws):
    colors, rois = _batch(40)
    _check(ws, colors, rois)


def _kpt_case(counts, seed=1):
    rng = np.random.default_rng(seed)
    rois = [(int(u), int(u) + int(w), int(v), int(v) + int(h)) for u, v, w, h in
            zip(rng.integers(0, 300, len(counts)), rng.integers(0, 200, len(counts)), rng.integers(10, 340, len(counts)), rng.integers(10, 280, len(counts)))]
    kp = [rng.uniform(-5, 405, (m, 2)).astype(np.float32) for m in counts]
    return rois, kp


@pytest.mark.parametrize("mode", ["new", "inplace", "given"])
def test_keypoints_bit_exact_ragged_counts(ws, mode):
    import torch
    from bundletrack_amd.detection import keypoints_to_image
    counts = [0, 1, 500, 8192, 37]
    rois, kp = _kpt_case(counts)
    frames = _frames([np.zeros((1, 1, 4), np.uint8)] * len(counts), rois)
    kin = [_t(k) for k in kp]
    out = "inplace" if mode == "inplace" else ([torch.full_like(k, np.nan) for k in kin] if mode == "given" else None)
    res = keypoints_to_image(ws, frames, kin, out=out)
    torch.cuda.synchronize()
    for k, (f, r) in enumerate(zip(frames, rois)):
        assert f.kpts_gpu is res[k] and f.n_keypts == counts[k]
        assert (res[k] is kin[k]) == (mode == "inplace")
        assert res[k].cpu().numpy().tobytes() == R.keypoints_to_image(kp[k], r).tobytes(), (k, r)
        if mode != "inplace":
            assert kin[k].cpu().numpy().tobytes() == kp[k].tobytes()


def test_round_trip_of_projected_keypoints(ws):
    import torch
    from bundletrack_amd.detection import detector_transform, keypoints_to_image
    pb = S.make_problem(2, 10, seed=8, background=True)
    kp = S.make_keypoints(pb, 600, 100, D=32, seed=8)
    true = kp.kpts[1].astype(np.float32)
    roi = (float(np.floor(true[:, 0].min())), float(np.ceil(true[:, 0].max())), float(np.floor(true[:, 1].min())), float(np.ceil(true[:, 1].max())))
    fwd, _ = detector_transform(roi)
    det = (true.astype(np.float64) @ fwd[:2, :2].T.astype(np.float64) + fwd[:2, 2]).astype(np.float32)
    frames = _frames([np.zeros((1, 1, 4), np.uint8)], [roi])
    back = keypoints_to_image(ws, frames, [_t(det)])[0]
    torch.cuda.synchronize()
    assert np.abs(back.cpu().numpy().astype(np.float64) - true).max() < 1e-3


def test_repeatable_and_async_form(ws):
    """Two calls give the same bytes; a raw call whose host ROI array and pointer table are gone before the stream syncs gives
    them too."""
    import gc
    import torch
    from bundletrack_amd.detection import prepare_detector_inputs
    colors, rois = _batch(34, seed=9)
    frames = _frames(colors, rois)
    a = prepare_detector_inputs(ws, frames)
    b = prepare_detector_inputs(ws, frames)
    n = len(frames)
    bgr = torch.empty((n, 400, 400, 3), dtype=torch.uint8, device="cuda")
    gray = torch.empty((n, 1, 400, 400), dtype=torch.float32, device="cuda")
    roi = np.array(rois, np.float32)
    table = (C.c_void_p * n)(*[f.color_gpu.data_ptr() for f in frames])
    rc = _lib.lib().btba_detector_inputs(ws.handle, C.byref(_lib.detector_params()), n, 480, 640, C.cast(table, C.c_void_p), roi.ctypes.data,
                                         bgr.data_ptr(), gray.data_ptr())
    assert rc == 0
    roi[:] = -1.0                                                     # overwritten, then freed, before the work may have run
    del roi, table
    gc.collect()
    torch.cuda.synchronize()
    for x, y in ((a[0], b[0]), (a[1], b[1]), (a[0], bgr), (a[1], gray)):
        assert torch.equal(x, y)
    only_gray = prepare_detector_inputs(ws, frames, want_bgr=False)
    torch.cuda.synchronize()
    assert only_gray[0] is None and torch.equal(only_gray[1], a[1])


def _scene(seed=41, n=3):
    """Background-rendered frames with their masks, colour and planted keypoints (make_keypoints)."""
    pb = S.make_problem(n, 10, seed=seed, background=True)
    kp = S.make_keypoints(pb, 600, 400, D=64, seed=seed)
    masks = [S.make_mask(pb.poses_gt[k], pb.K, pb.H, pb.W, seed=k) for k in range(n)]
    colors = [S.make_color(pb.poses_gt[k], pb.K, pb.H, pb.W, seed=k) for k in range(n)]
    return pb, kp, masks, colors


def _stand_in(fwd_of, kpts_of, desc_of):
    """A torch 'detector': the planted full-resolution keypoints of the current frame through the forward transform."""
    import torch
    state = {"frame": None, "calls": 0, "shapes": []}

    def detector(bgr, gray):
        state["calls"] += 1
        state["shapes"].append((tuple(bgr.shape), tuple(gray.shape), bgr.dtype, gray.dtype))
        k = state["frame"]
        F = torch.from_numpy(fwd_of(k)).to(bgr.device)
        p = torch.from_numpy(kpts_of(k)).to(bgr.device)
        det = torch.stack([p[:, 0] * F[0, 0] + F[0, 2], p[:, 1] * F[1, 1] + F[1, 2]], 1)
        return det, torch.from_numpy(desc_of(k)).to(bgr.device)
    return detector, state


def _round_trip_keeps_pixels(true, roi):
    """The matcher reads keypoints only through roundf: the chain can equal the direct path only if no round trip crosses a half."""
    fwd, _ = R.transform(roi)
    det = np.stack([(true[:, 0] * fwd[0, 0]).astype(np.float32) + fwd[0, 2], (true[:, 1] * fwd[1, 1]).astype(np.float32) + fwd[1, 2]], 1)
    back = R.keypoints_to_image(det.astype(np.float32), roi)
    rnd = lambda x: np.sign(x) * np.floor(np.abs(x.astype(np.float64)) + 0.5)
    return np.array_equal(rnd(back), rnd(true))


def test_depth_normals_mask_inputs_detector_match_chain(ws):
    import torch
    from bundletrack_amd.bundler import FrameRef
    from bundletrack_amd.detection import keypoints_to_image, prepare_detector_inputs
    from bundletrack_amd.matching import match_pairs
    from bundletrack_amd.optimizer import depth_to_normals, process_depth
    from bundletrack_amd.segmentation import apply_masks
    pb, kp, masks, colors = _scene()
    pairs = [(1, 0), (2, 1), (2, 0)]

    def frames():
        out = []
        for k in range(3):
            dep = process_depth(ws, _t(pb.depth[k]))
            nrm = depth_to_normals(ws, dep, pb.K)
            out.append(FrameRef(id=k, pose_in_model=pb.poses_gt[k].astype(np.float32), depth_gpu=dep, normal_gpu=nrm, mask_gpu=_t(masks[k]),
                                color_gpu=_t(colors[k]), desc_gpu=_t(kp.desc[k].astype(np.float32))))
        apply_masks(ws, out)
        return out
    direct = frames()
    for f, k in zip(direct, range(3)):
        f.kpts_gpu = _t(kp.kpts[k].astype(np.float32))
    want = match_pairs(ws, direct, pairs, K=pb.K, H=pb.H, W=pb.W)
    chain = frames()
    fwd = {k: R.transform(chain[k].roi)[0] for k in range(3)}
    detector, state = _stand_in(lambda k: fwd[k], lambda k: kp.kpts[k].astype(np.float32), lambda k: kp.desc[k].astype(np.float32))
    bgr, gray = prepare_detector_inputs(ws, chain)
    dets = []
    for k in range(3):
        state["frame"] = k
        d, _ = detector(bgr[k:k + 1], gray[k:k + 1])
        dets.append(d.contiguous())
        assert _round_trip_keeps_pixels(kp.kpts[k].astype(np.float32), chain[k].roi)
    keypoints_to_image(ws, chain, dets)
    got = match_pairs(ws, chain, pairs, K=pb.K, H=pb.H, W=pb.W)
    torch.cuda.synchronize()
    total = 0
    for a, b in zip(want.per_pair, got.per_pair):
        assert np.array_equal(a["idx_a"], b["idx_a"]) and np.array_equal(a["idx_b"], b["idx_b"])
        assert a["ptA_cam"].tobytes() == b["ptA_cam"].tobytes()
        total += len(a)
    assert total > 100
    for k in range(3):
        rb, rg = R.inputs(chain[k].color_gpu.cpu().numpy(), chain[k].roi)
        assert np.array_equal(bgr[k].cpu().numpy(), rb) and gray[k, 0].cpu().numpy().tobytes() == rg.tobytes()


class _KeypointFM:
    """find_corres on the frames' keypoints (matching.find_corres_by_nn_multi_pair), procrustes as SyntheticFeatureManager's."""

    def __init__(self, ws, K, H, W):
        self.ws, self.K, self.H, self.W = ws, K, H, W
        self.matches, self.inlier_dist, self.forgotten = {}, 0.01, []

    def forget_frame(self, frame):
        self.forgotten.append(frame)
        for key in [k for k in self.matches if frame.id in k]:
            del self.matches[key]

    def find_corres(self, a, b):
        from bundletrack_amd.matching import find_corres_by_nn_multi_pair
        if (a.id, b.id) not in self.matches:
            find_corres_by_nn_multi_pair(self.ws, [(a, b)], self.matches, K=self.K, H=self.H, W=self.W)

    def procrustes_by_correspondence(self, a, b):
        return S.SyntheticFeatureManager.procrustes_by_correspondence(self, a, b)


def _has(seq, x):
    return any(y is x for y in seq)


def _session(ws, use_detector, *, tiny=None, raise_at=None):
    from bundletrack_amd.bundler import Bundler, FrameRef
    from bundletrack_amd.optimizer import OptimizerGpu
    n = 4
    pb, kp, masks, colors = _scene(seed=43, n=n)
    fm = _KeypointFM(ws, pb.K, pb.H, pb.W)
    rois = {}
    detector, state = _stand_in(lambda k: R.transform(rois[k])[0], lambda k: kp.kpts[k].astype(np.float32), lambda k: kp.desc[k].astype(np.float32))

    def det(bgr, gray):
        if state["frame"] == raise_at:
            state["calls"] += 1
            raise RuntimeError("detector failed")
        return detector(bgr, gray)
    bundler = Bundler(OptimizerGpu(workspace=ws), fm, pb.K, pb.H, pb.W, window_size=5, max_BA_frames=5, detector=det if use_detector else None)
    frames = []
    for k in range(n):
        m = masks[k]
        if k == tiny:
            m = np.zeros_like(m)
            m[100:105, 200:205] = 255
        fr = FrameRef(id=0, pose_in_model=pb.poses_gt[0].astype(np.float32), depth_gpu=_t(pb.depth[k]), normal_gpu=_t(pb.normals[k]),
                      color_gpu=_t(colors[k]), mask_gpu=_t(m))
        if not use_detector:
            fr.kpts_gpu, fr.desc_gpu, fr.n_keypts = _t(kp.kpts[k].astype(np.float32)), _t(kp.desc[k].astype(np.float32)), len(kp.kpts[k])
        else:
            from bundletrack_amd.segmentation import apply_masks
            roi = apply_masks(ws, [FrameRef(id=0, pose_in_model=np.eye(4, dtype=np.float32), depth_gpu=_t(pb.depth[k]), normal_gpu=_t(pb.normals[k]),
                                            mask_gpu=_t(m))])[0]
            rois[k] = tuple(float(v) for v in roi)
        state["frame"] = k
        bundler.process_new_frame(fr)
        frames.append(fr)
    return bundler, frames, state, fm, kp


def test_python_bundler_with_detector_equals_direct_keypoints(ws):
    b_det, f_det, state, _, kp = _session(ws, True)
    b_dir, f_dir, _, _, _ = _session(ws, False)
    assert state["calls"] == 4 and all(s == ((1, 400, 400, 3), (1, 1, 400, 400)) for s in [x[:2] for x in state["shapes"]])
    assert b_det.n_ba_calls == b_dir.n_ba_calls == 3
    for a, b, k in zip(f_det, f_dir, range(4)):
        assert a.status == b.status != "FAIL"
        assert a.n_keypts == len(kp.kpts[k]) and a.desc_gpu.shape == b.desc_gpu.shape
        assert np.array_equal(np.asarray(a.pose_in_model), np.asarray(b.pose_in_model)), k


def test_python_bundler_detector_skips_tiny_roi_and_fails_on_exception(ws):
    b, frames, state, fm, _ = _session(ws, True, tiny=2)
    assert state["calls"] == 3                                         # frame 2 (ROI under 10 px) never reaches the detector
    assert frames[2].status == "FAIL" and not _has(b.frames, frames[2]) and not _has(fm.forgotten, frames[2])
    b, frames, state, fm, _ = _session(ws, True, raise_at=1)
    assert state["calls"] == 4
    assert frames[1].status == "FAIL" and _has(fm.forgotten, frames[1]) and not _has(b.frames, frames[1])
    assert b.need_reinit
    assert frames[2].status != "FAIL" and frames[3].status != "FAIL"


def _driver():
    so = _lib.build_driver("detector_driver")
    f = C.CDLL(so).detector_driver
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5
    return f


@pytest.mark.parametrize("via_bundler", [0, 1])
def test_cpp_detector_feature_manager_equals_python(ws, via_bundler):
    import torch
    from bundletrack_amd.detection import keypoints_to_image, prepare_detector_inputs
    colors, rois = _batch(5, seed=13)
    rois[4] = (100, 105, 100, 300)                                     # 5 px wide: FAIL by ROI before the detector
    counts = [300, 0, 8192, 17, 50]
    _, kp = _kpt_case(counts, seed=3)
    D = 8
    frames = _frames(colors, rois)
    py_bgr, py_gray = prepare_detector_inputs(ws, frames[:4])
    py_k = keypoints_to_image(ws, frames[:4], [_t(k) for k in kp[:4]])
    dc = [_t(c) for c in colors]
    dk = [_t(k) if len(k) else torch.zeros((1, 2), device="cuda") for k in kp]
    dd = [torch.zeros((max(m, 1), D), device="cuda") for m in counts]
    bgr = torch.zeros((5, 400, 400, 3), dtype=torch.uint8, device="cuda")
    gray = torch.zeros((5, 400, 400), dtype=torch.float32, device="cuda")
    ptr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    roi = np.array(rois, np.float32)
    n = np.array(counts, np.int32)
    calls, nk, st = np.zeros(1, np.int32), np.zeros(5, np.int32), np.zeros(5, np.int32)
    rc = _driver()(ws.handle.value, via_bundler, 5 if via_bundler else 4, 480, 640, 400, ptr(dc), roi.ctypes.data, ptr(dk), n.ctypes.data, ptr(dd), D,
                   bgr.data_ptr(), gray.data_ptr(), calls.ctypes.data, nk.ctypes.data, st.ctypes.data)
    assert rc == 0
    torch.cuda.synchronize()
    assert calls[0] == 4 and list(nk[:4]) == counts[:4]
    assert torch.equal(bgr[:4], py_bgr) and torch.equal(gray[:4], py_gray[:, 0])
    for k in range(4):
        assert dk[k][:counts[k]].cpu().numpy().tobytes() == py_k[k].cpu().numpy().tobytes()
    if via_bundler:
        assert (st[:4] != 0).all() and st[4] == 0                      # Frame::FAIL == 0 only for the thin ROI
        assert not bgr[4].any()
