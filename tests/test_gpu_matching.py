"""btba_match_pairs on the MI355X: bit-exact against the CPU restatement (tests/cpp/match_host.cpp), consistent with
btba_depth_to_normals, deterministic, equal in both buffer forms, chained into RANSAC, the C++ host layer, and recall of planted
correspondences.  One module-scoped workspace, no subprocesses."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S

from match_ref import HostFrame, restate, scene_frames


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


def _dev(frames):
    """FrameRefs with the frames' data on cuda:0."""
    import torch
    from bundletrack_amd.bundler import FrameRef
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    return [FrameRef(id=f.id, pose_in_model=f.pose, kpts_gpu=t(f.kpts), desc_gpu=t(f.desc), depth_gpu=t(f.depth), normal_gpu=t(f.normal))
            for f in frames]


def _assert_bit_equal(ws, frames, pairs, K, H, W, **kw):
    from bundletrack_amd.matching import match_pairs
    prm = _lib.match_params(**kw)
    ref, pa, pb, n = restate(frames, pairs, prm, K, H, W)
    got = match_pairs(ws, _dev(frames), pairs, prm, K=K, H=H, W=W)
    assert np.array_equal(got.n_out, n)
    for g, r in zip(got.per_pair, ref):
        assert g.tobytes() == r.tobytes()
    T = int(n.sum())
    assert got.ptsA_dev[:T].cpu().numpy().tobytes() == pa.tobytes() and got.ptsB_dev[:T].cpu().numpy().tobytes() == pb.tobytes()
    return got


def _scene(n_frames, n_landmarks, n_distractors, D, seed):
    pb = S.make_problem(n_frames, 10, seed=seed, background=False)
    kp = S.make_keypoints(pb, n_landmarks, n_distractors, D=D, seed=seed)
    return pb, scene_frames(pb, kp)


def _window_pairs(n):
    return [(a, b) for a in range(n) for b in range(a)]


def test_bit_exact_tracker_size(ws):
    pb, frames = _scene(15, 900, 100, 256, 21)
    rng = np.random.default_rng(0)
    for f in frames:                                               # 500 keypoints per frame, as the tracker sees them
        keep = rng.permutation(len(f.kpts))[:500] if len(f.kpts) >= 500 else np.arange(len(f.kpts))
        f.kpts, f.desc = f.kpts[keep], f.desc[keep]
    pairs = [(14, b) for b in range(14)]                           # the new frame against the 14 others
    got = _assert_bit_equal(ws, frames, pairs, pb.K, pb.H, pb.W)
    assert got.n_out.sum() > 14 * 100


def test_bit_exact_ragged_frames(ws):
    pb, frames = _scene(4, 6000, 200, 256, 22)
    for f, n in zip(frames, [0, 1, 3, 4000]):
        f.kpts, f.desc = f.kpts[:n], f.desc[:n]
    _assert_bit_equal(ws, frames, [(3, 2), (3, 1), (3, 0), (2, 1), (1, 0), (2, 3)], pb.K, pb.H, pb.W)


@pytest.mark.parametrize("D", [128, 36])
def test_bit_exact_other_dims(ws, D):
    pb, frames = _scene(5, 500, 80, D, 23 + D)
    _assert_bit_equal(ws, frames, _window_pairs(5), pb.K, pb.H, pb.W)
    _assert_bit_equal(ws, frames, _window_pairs(5), pb.K, pb.H, pb.W, mutual=0, k=3)


def test_bit_exact_batch_of_windows(ws):
    frames, pairs = [], []
    for w in range(8):                                             # 8 windows x 15 frames, every window's 105 pairs in one call
        pb, fr = _scene(15, 150, 30, 64, 100 + w)
        for f in fr:
            f.id += 1000 * w
        pairs += [(len(frames) + a, len(frames) + b) for a, b in _window_pairs(15)]
        frames += fr
    assert len(pairs) == 840
    _assert_bit_equal(ws, frames, pairs, pb.K, pb.H, pb.W)


def test_points_equal_depth_to_normals_xyz(ws):
    import torch
    from bundletrack_amd.matching import match_pairs
    pb, frames = _scene(3, 400, 50, 64, 31)
    dev = _dev(frames)
    res = match_pairs(ws, dev, _window_pairs(3), K=pb.K, H=pb.H, W=pb.W)
    Kf = np.ascontiguousarray(pb.K, np.float32)
    for p, (a, b) in enumerate(_window_pairs(3)):
        m = res.per_pair[p]
        assert len(m) > 50
        for fi, idx, col in ((a, m["idx_a"], "ptA_cam"), (b, m["idx_b"], "ptB_cam")):
            nrm = torch.zeros((pb.H, pb.W, 4), dtype=torch.float32, device="cuda")
            xyz = torch.zeros_like(nrm)
            _lib.check(_lib.lib().btba_depth_to_normals(ws.handle, pb.H, pb.W, Kf.ctypes.data, dev[fi].depth_gpu.data_ptr(), nrm.data_ptr(), xyz.data_ptr()),
                       "btba_depth_to_normals")
            ws.sync()
            kp = frames[fi].kpts[idx].astype(np.float64)
            u = (np.sign(kp) * np.floor(np.abs(kp) + 0.5)).astype(int)
            expect = xyz.cpu().numpy()[u[:, 1], u[:, 0], :3]
            assert expect.tobytes() == np.ascontiguousarray(m[col]).tobytes()


def test_repeatable_and_both_buffer_forms(ws):
    from bundletrack_amd.matching import match_pairs
    pb, frames = _scene(6, 500, 80, 256, 41)
    dev = _dev(frames)
    pairs = _window_pairs(6)
    r1 = match_pairs(ws, dev, pairs, K=pb.K, H=pb.H, W=pb.W)
    r2 = match_pairs(ws, dev, pairs, K=pb.K, H=pb.H, W=pb.W)
    r3 = match_pairs(ws, dev, pairs, K=pb.K, H=pb.H, W=pb.W, device_resident=False)
    T = int(r1.n_out.sum())
    for r in (r2, r3):
        assert np.array_equal(r.n_out, r1.n_out)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(r.per_pair, r1.per_pair))
    assert r2.ptsA_dev[:T].cpu().numpy().tobytes() == r1.ptsA_dev[:T].cpu().numpy().tobytes()
    assert r3.ptsA.tobytes() == r1.ptsA_dev[:T].cpu().numpy().tobytes() and r3.ptsB.tobytes() == r1.ptsB_dev[:T].cpu().numpy().tobytes()


def _ransac_chain(ws, pb, frames):
    """matches -> device-resident RANSAC, and the host chain: find_corres_by_nn_multi_pair -> run_ransac_multi_pair."""
    from bundletrack_amd import ransac
    from bundletrack_amd.matching import find_corres_by_nn_multi_pair, match_pairs
    dev = _dev(frames)
    idx = [(len(frames) - 1, b) for b in range(len(frames) - 1)]
    res = match_pairs(ws, dev, idx, K=pb.K, H=pb.H, W=pb.W)
    n_pts = res.n_out.astype(np.int32)
    ids, n_in, best, _ = ransac.ransac_packed_device(ws, res.ptsA_dev, res.ptsB_dev, n_pts)
    ws.sync()
    ids, n_in = ids.cpu().numpy(), n_in.cpu().numpy()
    matches = {}
    pairs = [(dev[a], dev[b]) for a, b in idx]
    find_corres_by_nn_multi_pair(ws, pairs, matches, K=pb.K, H=pb.H, W=pb.W)
    before = {k: (v[0].copy(), v[1].copy()) for k, v in matches.items()}
    ransac.run_ransac_multi_pair(ws, pairs, matches)
    return res, ids, n_in, n_pts, before, matches, idx, dev


def test_matches_into_device_ransac_equal_host_chain(ws):
    pb, frames = _scene(6, 500, 80, 256, 51)
    res, ids, n_in, n_pts, before, matches, idx, dev = _ransac_chain(ws, pb, frames)
    o = 0
    for p, (a, b) in enumerate(idx):
        key = (dev[a].id, dev[b].id)
        m = res.per_pair[p]
        assert before[key][0].tobytes() == np.ascontiguousarray(m["ptA_cam"]).tobytes()
        keep = ids[o:o + n_in[p]]
        if n_in[p] < 5:
            assert len(matches[key][0]) == 0
        else:
            assert matches[key][0].tobytes() == np.ascontiguousarray(m["ptA_cam"][keep]).tobytes()
        o += int(n_pts[p])


def test_recall_of_planted_correspondences(ws):
    pb = S.make_problem(6, 10, seed=61, background=False)
    kp = S.make_keypoints(pb, 600, 100, D=256, desc_noise=0.02, px_noise=0.1, seed=61)
    frames = scene_frames(pb, kp)
    res, ids, n_in, n_pts, _, _, idx, _ = _ransac_chain(ws, pb, frames)
    planted = found = 0
    o = 0
    for p, (a, b) in enumerate(idx):
        la, lb = kp.landmark[a], kp.landmark[b]
        truth = set(np.intersect1d(la[la >= 0], lb[lb >= 0]).tolist())
        m = res.per_pair[p][ids[o:o + n_in[p]]]
        got = {int(la[x]) for x, y in zip(m["idx_a"], m["idx_b"]) if la[x] >= 0 and la[x] == lb[y]}
        planted += len(truth)
        found += len(truth & got)
        o += int(n_pts[p])
    assert planted > 500
    assert found >= 0.95 * planted, (found, planted)


def _driver():
    so = _lib.build_driver("match_driver")
    f = C.CDLL(so).match_driver
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return f


def test_cpp_find_corres_by_nn_multi_pair_equals_python(ws):
    from bundletrack_amd.matching import find_corres_by_nn_multi_pair
    pb, frames = _scene(5, 500, 80, 256, 71)
    dev = _dev(frames)
    pairs = [(4, b) for b in range(4)] + [(3, 2)]
    matches = {}
    find_corres_by_nn_multi_pair(ws, [(dev[a], dev[b]) for a, b in pairs], matches, K=pb.K, H=pb.H, W=pb.W)
    n = len(dev)
    ptr = lambda attr: (C.c_void_p * n)(*[getattr(f, attr).data_ptr() for f in dev])
    cap = sum(len(frames[a].kpts) + len(frames[b].kpts) for a, b in pairs)
    pa, pb_ = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.float32)
    n_out = np.zeros(len(pairs), np.int32)
    K = np.ascontiguousarray(pb.K, np.float32)
    poses = np.ascontiguousarray(np.stack([f.pose.reshape(16) for f in frames]), np.float32)
    ids = np.array([f.id for f in frames], np.int32)
    nk = np.array([len(f.kpts) for f in frames], np.int32)
    pr = np.ascontiguousarray(np.asarray(pairs, np.int32))
    rc = _driver()(ws.handle.value, n, pb.H, pb.W, K.ctypes.data, 256, ptr("desc_gpu"), ptr("kpts_gpu"), nk.ctypes.data, ptr("depth_gpu"), ptr("normal_gpu"),
                   poses.ctypes.data, ids.ctypes.data, len(pairs), pr.ctypes.data, pa.ctypes.data, pb_.ctypes.data, n_out.ctypes.data)
    assert rc == 0
    o = 0
    for p, (a, b) in enumerate(pairs):
        A, B = matches[(a, b)]
        assert n_out[p] == len(A) > 0
        assert pa[o:o + n_out[p]].tobytes() == A.tobytes() and pb_[o:o + n_out[p]].tobytes() == B.tobytes()
        o += int(n_out[p])


def test_rejects_bad_arguments_on_a_workspace(ws):
    from bundletrack_amd.matching import match_pairs
    pb, frames = _scene(2, 100, 10, 64, 81)
    dev = _dev(frames)
    with pytest.raises(_lib.BtbaError):
        match_pairs(ws, dev, [(0, 0)], K=pb.K, H=pb.H, W=pb.W)
    with pytest.raises(_lib.BtbaError):
        match_pairs(ws, dev, [(0, 1)], _lib.match_params(k=9), K=pb.K, H=pb.H, W=pb.W)


def test_scratch_does_not_grow_over_repeated_calls(ws):
    import torch
    from bundletrack_amd.matching import match_pairs
    pb, frames = _scene(6, 500, 80, 256, 91)
    dev = _dev(frames)
    pairs = _window_pairs(6)
    match_pairs(ws, dev, pairs, K=pb.K, H=pb.H, W=pb.W)
    torch.cuda.synchronize()
    blocks0 = ws.live_blocks()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        match_pairs(ws, dev, pairs, K=pb.K, H=pb.H, W=pb.W)
    torch.cuda.synchronize()
    assert ws.live_blocks() == blocks0
    assert free0 - torch.cuda.mem_get_info()[0] < (64 << 20)
