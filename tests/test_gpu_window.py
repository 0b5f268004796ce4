"""btba_marshal_windows and btba_procrustes_pairs on the MI355X against tests/window_ref.py and bundler.marshal_window: marshalled
EntryJ bytes, pair offsets and the 24-byte layout bit for bit (the chain's output of the scene of tests/test_gpu_corres.py; a
32-window batch with empty pairs, odd first records and untouched tails), fixed-order moments bit for bit, poses inside the Kabsch
bar, identity fallbacks, batch = singles, determinism, the solver on marshalled against host-packed arrays, and two Bundler sessions
(shadowed host path; free-running device path).  One module-scoped workspace, no subprocesses.

Kabsch bar: |d| <= 4 * 2^-24 * max(1, |x|) per pose entry against the restatement's fp64 Kabsch of the same model-frame points (one
fp32 rounding with a 4x margin), on inputs the restatement calls well conditioned.  The host path's own fp32 SVD Kabsch
(bundler.solve_rigid_transform_between_points) is up to 7.5e-7 away from that fp64 optimum on such inputs (measured on the CPU, 14 of
200 planted sets beyond the bar), so the shadow session holds the device pose to the bar against the fp64 Kabsch of the host call's
inputs and prints its distance to the host pose.
Measured on the MI355X: see DESIGN.md 4.7."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S
from bundletrack_amd.bundler import Bundler, FrameRef, marshal_window

import window_ref as WR
from test_gpu_corres import CHAINS, _dev, scene  # noqa: F401  (the scene fixture and its frames on the device)

BAR = 4.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


def _inside_bar(pose, pose64):
    d = np.abs(pose.astype(np.float64) - pose64)
    return float((d / np.maximum(1.0, np.abs(pose64))).max())


def _rigid(rng, angle=0.4, shift=0.2):
    T = np.eye(4)
    T[:3, :3] = S.so3_exp(rng.normal(size=3) * angle)
    T[:3, 3] = rng.normal(scale=shift, size=3)
    return T.astype(np.float32)


def _planted_records(rng, n, noise=0.001):
    """n records of a rigid motion between two camera frames (+ noise), decimetre object at ~0.6 m."""
    a = rng.normal(scale=0.05, size=(n, 3)) + np.array([0.0, 0.0, 0.6])
    M = _rigid(rng, 0.15, 0.03).astype(np.float64)
    b = a @ M[:3, :3].T + M[:3, 3] + rng.normal(scale=noise, size=(n, 3))
    rec = np.zeros(n, _lib.MATCH_DTYPE)
    rec["idx_a"], rec["idx_b"], rec["dist"] = rng.integers(0, 500, n), rng.integers(0, 500, n), rng.random(n)
    rec["ptA_cam"], rec["ptB_cam"] = a, b
    return rec


def _upload(records):
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(np.int32).reshape(-1, 10).copy()).cuda()


def _chain_manager(ws, scene):
    """GpuFeatureManager after the chains a tracker runs on frames 0 .. 5 of the scene."""
    from bundletrack_amd.correspondence import GpuFeatureManager
    pb, kp, frames = scene
    dev = _dev(frames[:6])
    fm = GpuFeatureManager(ws, pb.K, pb.H, pb.W)
    for pairs in CHAINS:
        fm.find_corres_chain([(dev[a], dev[b]) for a, b in pairs])
    return fm, dev


def _window_segments(fm, frames):
    n = len(frames)
    return [fm.device_segments.get((frames[j].id, frames[i].id), (0, 0)) for i in range(n) for j in range(i + 1, n)]


def test_marshalled_chain_output_equals_marshal_window(ws, scene):
    from bundletrack_amd.optimizer import BatchSolver
    from bundletrack_amd.window import marshal_windows, window_layout
    fm, dev = _chain_manager(ws, scene)
    segs = _window_segments(fm, dev)
    counts = np.array([c for _, c in segs], np.int32)
    assert (counts > 0).sum() >= 10 and (counts == 0).any()                       # matched pairs and pairs the chains never ran
    for key, (first, count) in fm.device_segments.items():                        # the pool holds the chain's records
        assert fm.device_records()[first:first + count].cpu().numpy().tobytes() == fm.records[key].tobytes()
    ref = marshal_window(dev, fm.matches, dev[5], 5)
    lay = window_layout(counts[None], 6, 5, 5)
    corr, off, c24 = marshal_windows(ws, fm.device_records(), np.asarray(segs)[None], 6, lay, corr24=True)
    ws.sync()
    assert lay.corr_stride == len(ref.corr) and bool(lay.run_ba[0]) == ref.run_ba and int(lay.n_edges_newframe[0]) == ref.n_edges_newframe
    assert corr.cpu().numpy().tobytes() == ref.corr.tobytes()
    assert np.array_equal(off.cpu().numpy().view(np.uint32), lay.pair_offsets)
    want24 = BatchSolver(workspace=ws).pack_correspondences24(corr, off, lay.max_corr_per_pair, 6)
    ws.sync()
    assert c24.cpu().numpy().tobytes() == want24.cpu().numpy().tobytes()
    fm.close()


def test_batch_of_32_windows_with_empty_pairs(ws):
    import torch
    from bundletrack_amd.optimizer import BatchSolver
    from bundletrack_amd.window import marshal_windows, window_layout
    rng = np.random.default_rng(21)
    n_frames, nw = 6, 32
    P = n_frames * (n_frames - 1) // 2
    n_rec = 40000
    rec = rng.integers(0, 2 ** 32, size=(n_rec, 10), dtype=np.uint64).astype(np.uint32).view(_lib.MATCH_DTYPE).reshape(-1)     # every bit pattern
    sizes = [0, 0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 700]
    segs = np.zeros((nw, P, 2), np.int64)
    for w in range(nw):
        for p in range(P):
            c = 0 if (w == 3 or rng.random() < 0.3) else int(rng.choice(sizes))   # window 3 is empty altogether
            segs[w, p] = (int(rng.integers(0, n_rec - c + 1)), c)
    segs[0, 0] = (n_rec - 513, 513)                                               # ends on the array's last record, odd first record
    segs[1, P - 1] = (1, 700)
    counts = segs[..., 1].astype(np.int32)
    new_idx = rng.integers(0, n_frames, nw)
    lay = window_layout(counts, n_frames, new_idx, 5)
    stride = lay.corr_stride
    assert lay.max_corr_per_pair == 700 and stride == counts.sum(1).max()
    dev = torch.device("cuda")
    corr = torch.full((nw, stride, 32), 0x5B, dtype=torch.uint8, device=dev)
    off = torch.full((nw, P + 1), 0x5B5B5B5B, dtype=torch.int32, device=dev)
    c24 = torch.full((-(-(nw * stride) // 64), 3, 64, 2), 0.0, dtype=torch.float32, device=dev)
    marshal_windows(ws, _upload(rec), segs, n_frames, lay, corr24=True, out=(corr, off, c24))
    ws.sync()
    got, got_off = corr.cpu().numpy(), off.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_off, lay.pair_offsets)
    blocks = []
    for w in range(nw):
        c, o, edges, run = WR.marshal(rec, [tuple(s) for s in segs[w]], n_frames, int(new_idx[w]), 5)
        frames = [FrameRef(id=10 * k, pose_in_model=np.eye(4, dtype=np.float32)) for k in range(n_frames)]
        matches = {(10 * j, 10 * i): (rec["ptA_cam"][f:f + n], rec["ptB_cam"][f:f + n])
                   for (i, j), (f, n) in zip(WR.canonical_pairs(n_frames), segs[w])}
        ref = marshal_window(frames, matches, frames[int(new_idx[w])], 5)
        assert ref.corr.tobytes() == c.tobytes() and np.array_equal(o, got_off[w])
        assert edges == int(lay.n_edges_newframe[w]) == ref.n_edges_newframe and run == bool(lay.run_ba[w]) == ref.run_ba
        assert got[w, :len(c)].tobytes() == c.tobytes(), w
        assert (got[w, len(c):] == 0x5B).all(), w                                 # entries beyond offsets[P] are not written
        blocks.append(c)
    want24 = BatchSolver(workspace=ws).pack_correspondences24(corr, off, lay.max_corr_per_pair, n_frames)
    ws.sync()
    g24 = c24.cpu().numpy().view(np.uint32).reshape(-1)
    assert g24.tobytes() == want24.cpu().numpy().tobytes()
    words, written = WR.pack24(blocks, stride)
    assert np.array_equal(g24[written], words[written]) and not g24[~written].any()
    # without corr24 the EntryJ array is the same
    corr2, off2, none = marshal_windows(ws, _upload(rec), segs, n_frames, lay)
    ws.sync()
    assert none is None and np.array_equal(off2.cpu().numpy().view(np.uint32), got_off)
    for w in range(nw):
        assert corr2[w, :len(blocks[w])].cpu().numpy().tobytes() == blocks[w].tobytes()


def _kabsch_cases(rng):
    """(records, segments, posesA, posesB): well-conditioned planted pairs of many sizes, back to back."""
    sizes = [5, 6, 7, 63, 64, 255, 256, 257, 300, 512, 777, 1000, 2000, 5, 100]
    recs, segs, at = [], [], 0
    for k, n in enumerate(sizes):
        recs.append(_planted_records(rng, n, noise=0.0 if k % 3 == 0 else 0.001))
        segs.append((at, n))
        at += n
    TA = np.stack([_rigid(rng) for _ in sizes])
    TB = np.stack([_rigid(rng) for _ in sizes])
    return np.concatenate(recs), segs, TA, TB


def test_moments_bit_for_bit_and_poses_inside_the_bar(ws):
    from bundletrack_amd.window import procrustes_pairs
    rec, segs, TA, TB = _kabsch_cases(np.random.default_rng(33))
    pose, err, mom = procrustes_pairs(ws, _upload(rec), segs, TA, TB, want_moments=True)
    worst = worst_err = worst_orth = 0.0
    for e, (f, n) in enumerate(segs):
        ref = WR.procrustes(rec[f:f + n], TA[e], TB[e])
        assert ref["well_conditioned"], e
        assert mom[e].tobytes() == ref["moments"].tobytes(), e
        worst = max(worst, _inside_bar(pose[e], ref["pose64"]))
        worst_err = max(worst_err, abs(float(err[e]) - ref["err"]) / max(ref["err"], 1e-7))
        R = pose[e][:3, :3].astype(np.float64)
        worst_orth = max(worst_orth, np.abs(R.T @ R - np.eye(3)).max())
        assert np.linalg.det(R) > 0 and np.array_equal(pose[e][3], [0, 0, 0, 1])
    print(f"kabsch: worst pose difference / max(1, |x|) = {worst:.3e} (bar {BAR:.3e}); err rel {worst_err:.2e}; |R^T R - I| {worst_orth:.2e}")
    assert worst <= BAR
    # R is the fp32 rounding of an fp64 rotation: R^T R - I sums three products of entries each off by <= 2^-24
    assert worst_orth <= 8 * 2.0 ** -24
    # err: the same fp64 sum up to its order and the solver's 1e-13, rounded once to fp32
    assert worst_err <= 4 * 2.0 ** -24
    # the device-resident form gives the same bits
    import torch
    p2, e2, m2 = procrustes_pairs(ws, _upload(rec), segs, torch.from_numpy(TA).cuda(), torch.from_numpy(TB).cuda(), want_moments=True, device_resident=True)
    assert p2.cpu().numpy().tobytes() == pose.tobytes() and e2.cpu().numpy().tobytes() == err.tobytes() and m2.cpu().numpy().tobytes() == mom.tobytes()


def test_chain_pairs_inside_the_bar(ws, scene):
    from bundletrack_amd.window import procrustes_pairs
    fm, dev = _chain_manager(ws, scene)
    keys = [k for k, (_, c) in fm.device_segments.items() if c >= 5]
    by_id = {f.id: f for f in dev}
    segs = [fm.device_segments[k] for k in keys]
    TA = np.stack([by_id[a].pose_in_model for a, _ in keys]).astype(np.float32)
    TB = np.stack([by_id[b].pose_in_model for _, b in keys]).astype(np.float32)
    pose, err, mom = procrustes_pairs(ws, fm.device_records(), segs, TA, TB, want_moments=True)
    worst, n_ok = 0.0, 0
    for e, key in enumerate(keys):
        ref = WR.procrustes(fm.records[key], TA[e], TB[e])
        assert mom[e].tobytes() == ref["moments"].tobytes(), key
        assert ref["well_conditioned"], key
        worst = max(worst, _inside_bar(pose[e], ref["pose64"]))
        n_ok += 1
    print(f"kabsch on {n_ok} chain pairs: worst pose difference {worst:.3e} (bar {BAR:.3e})")
    assert n_ok >= 10 and worst <= BAR
    fm.close()


def test_fallbacks_leave_neighbours_untouched_batch_equals_singles_and_runs_repeat(ws):
    from bundletrack_amd.window import procrustes_pairs
    rng = np.random.default_rng(44)
    rec, segs, TA, TB = _kabsch_cases(rng)
    base, base_err, base_mom = procrustes_pairs(ws, _upload(rec), segs, TA, TB, want_moments=True)
    # spoil pairs 3 (NaN point), 6 (inf point), 9 (non-finite pose) and shorten 1 and 12 to 4 and 0 records
    bad = rec.copy()
    bad["ptA_cam"][segs[3][0] + 2, 1] = np.nan
    bad["ptB_cam"][segs[6][0] + 100, 0] = np.inf
    TA2 = TA.copy()
    TA2[9, 1, 3] = np.nan
    segs2 = list(segs)
    segs2[1], segs2[12] = (segs[1][0], 4), (segs[12][0], 0)
    pose, err, mom = procrustes_pairs(ws, _upload(bad), segs2, TA2, TB, want_moments=True)
    I = np.eye(4, dtype=np.float32)
    for e in range(len(segs)):
        if e in (1, 3, 6, 9, 12):
            assert np.array_equal(pose[e], I) and err[e] == 0.0, e
        else:
            assert pose[e].tobytes() == base[e].tobytes() and err[e] == base_err[e] and mom[e].tobytes() == base_mom[e].tobytes(), e
    assert mom[1][0] == 4 and not mom[1][1:].any() and mom[12][0] == 0
    # a batch of n pairs = n single-pair calls; two runs give the same bits
    dev_rec = _upload(rec)
    for e in range(len(segs)):
        p1, e1, m1 = procrustes_pairs(ws, dev_rec, [segs[e]], TA[e:e + 1], TB[e:e + 1], want_moments=True)
        assert p1[0].tobytes() == base[e].tobytes() and e1[0] == base_err[e] and m1[0].tobytes() == base_mom[e].tobytes(), e
    again, again_err, again_mom = procrustes_pairs(ws, dev_rec, segs, TA, TB, want_moments=True)
    assert again.tobytes() == base.tobytes() and again_err.tobytes() == base_err.tobytes() and again_mom.tobytes() == base_mom.tobytes()
    # rank-deficient input: collinear points give a finite proper rotation, equal points the identity rotation
    line = np.zeros(50, _lib.MATCH_DTYPE)
    line["ptA_cam"] = np.outer(np.linspace(-0.1, 0.1, 50), [1.0, 2.0, -1.0]) + [0.0, 0.0, 0.6]
    line["ptB_cam"] = line["ptA_cam"][:, [1, 2, 0]]
    same = np.zeros(20, _lib.MATCH_DTYPE)
    same["ptA_cam"], same["ptB_cam"] = [0.1, 0.2, 0.6], [0.0, 0.3, 0.5]
    pose, err, _ = procrustes_pairs(ws, _upload(np.concatenate([line, same])), [(0, 50), (50, 20)], np.stack([I, I]), np.stack([I, I]))
    for e in range(2):
        R = pose[e][:3, :3].astype(np.float64)
        assert np.isfinite(pose[e]).all() and np.abs(R.T @ R - np.eye(3)).max() < 1e-6 and np.linalg.det(R) > 0
    assert err[0] < 1e-6                                                          # a maximiser: the line maps onto the line
    assert np.array_equal(pose[1][:3, :3], np.eye(3, dtype=np.float32))
    assert np.allclose(pose[1][:3, 3], np.float32([0.0, 0.3, 0.5]) - np.float32([0.1, 0.2, 0.6]), atol=1e-7)
    assert procrustes_pairs(ws, dev_rec, np.zeros((0, 2), np.int32), np.zeros((0, 4, 4)), np.zeros((0, 4, 4)))[0].shape == (0, 4, 4)


def _zn_window(ws, pb, dev):
    from bundletrack_amd.optimizer import build_cache_zn
    zn, _, _ = build_cache_zn(ws, [f.depth_gpu for f in dev], [f.normal_gpu for f in dev], pb.H, pb.W, pb.K)
    return zn[None]


def test_solve_zn_on_marshalled_equals_host_packed(ws, scene):
    import torch
    from bundletrack_amd.optimizer import BatchSolver
    from bundletrack_amd.window import marshal_windows, window_layout
    pb, kp, frames = scene
    fm, dev = _chain_manager(ws, scene)
    segs = _window_segments(fm, dev)
    lay = window_layout(np.array([c for _, c in segs], np.int32)[None], 6, 5, 5)
    corr, off, _ = marshal_windows(ws, fm.device_records(), np.asarray(segs)[None], 6, lay)
    ref = marshal_window(dev, fm.matches, dev[5], 5)
    h_corr, h_off, h_max = BatchSolver.pack_correspondences([ref.corr], 6)
    assert h_max == lay.max_corr_per_pair and h_corr.shape[1] == corr.shape[1]
    zn = _zn_window(ws, pb, dev)
    solver = BatchSolver(workspace=ws)
    poses0 = np.stack([np.asarray(f.pose_in_model, np.float32) for f in dev])[None]
    poses0[0, 1:, :3, 3] += 0.003                                                 # something to solve
    out = []
    for c, o in ((corr, off), (torch.from_numpy(h_corr.view(np.uint8).reshape(1, -1, 32)).cuda(), torch.from_numpy(h_off.view(np.int32)).cuda())):
        p = torch.from_numpy(poses0.copy()).cuda()
        solver.solve_zn(zn, pb.H, pb.W, pb.K, c, o, h_max, p)
        ws.sync()
        out.append(p.cpu().numpy())
    assert np.isfinite(out[0]).all() and not np.array_equal(out[0], poses0)
    assert out[0].tobytes() == out[1].tobytes()
    fm.close()


def _session_frames(pb, dev, n):
    return [FrameRef(id=0, pose_in_model=np.asarray(pb.poses_gt[0], np.float32) if k == 0 else np.eye(4, dtype=np.float32),
                     kpts_gpu=dev[k].kpts_gpu, desc_gpu=dev[k].desc_gpu, depth_gpu=dev[k].depth_gpu, normal_gpu=dev[k].normal_gpu) for k in range(n)]


def _run_session(ws, scene, n, device_window, hook=None):
    from bundletrack_amd.correspondence import GpuFeatureManager
    from bundletrack_amd.optimizer import OptimizerGpu
    pb, kp, frames = scene
    dev = _dev(frames[:n])
    fm = GpuFeatureManager(ws, pb.K, pb.H, pb.W)
    b = Bundler(OptimizerGpu(workspace=ws), fm, pb.K, pb.H, pb.W, window_size=5, max_BA_frames=5, device_window=device_window)
    if hook is not None:
        hook(b, fm)
    poses, status, windows = [], [], []
    for k, fr in enumerate(_session_frames(pb, dev, n)):
        b.process_new_frame(fr)
        poses.append(np.asarray(fr.pose_in_model, np.float32).copy())
        status.append(fr.status)
        windows.append(b.last_window)
    return b, fm, poses, status, windows


def test_shadow_session(ws, scene):
    """The host-path session of tests/test_gpu_corres.py; at every procrustes and every BA call the device path runs on the same
    inputs."""
    import torch
    from bundletrack_amd.optimizer import BatchSolver
    pb, kp, frames = scene
    seen = {"kabsch": 0, "ba": 0, "worst_init": 0.0, "worst_host": 0.0, "worst_r": 0.0, "worst_t": 0.0}

    def hook(b, fm):
        host_procrustes = fm.procrustes_by_correspondence

        def procrustes(frameA, frameB):
            host = host_procrustes(frameA, frameB)
            got, err = fm.procrustes_by_correspondence_device(frameA, frameB)
            ref = WR.procrustes(fm.records[(frameA.id, frameB.id)], frameA.pose_in_model, frameB.pose_in_model)
            assert ref["well_conditioned"]
            seen["kabsch"] += 1
            seen["worst_init"] = max(seen["worst_init"], _inside_bar(got, ref["pose64"]))
            seen["worst_host"] = max(seen["worst_host"], _inside_bar(got, host.astype(np.float64)))
            assert abs(err - ref["err"]) <= 4 * 2.0 ** -24 * max(ref["err"], 1e-7)
            return host
        fm.procrustes_by_correspondence = procrustes
        host_optimize = b.opt.optimizeFrames

        def optimize(corr, n_match, n_frames, H, W, depths, colors, normals, poses, K, **kw):
            win_frames = b.last_window.frames
            dwin = b.assemble_window_on_device(win_frames)
            assert dwin.run_ba and dwin.corr.tobytes() == np.ascontiguousarray(corr).tobytes()                  # the windows agree bit for bit
            assert np.array_equal(dwin.n_match_per_pair, n_match) and dwin.n_edges_newframe == b.last_window.n_edges_newframe
            assert np.array_equal(dwin.pair_offsets_dev.cpu().numpy()[0].view(np.uint32), np.concatenate([[0], np.cumsum(n_match)]).astype(np.uint32))
            p_dev = torch.from_numpy(np.asarray(poses, np.float32).reshape(1, n_frames, 4, 4).copy()).cuda()
            BatchSolver(workspace=ws).solve_zn(_zn_window(ws, pb, win_frames), H, W, K, dwin.corr_dev, dwin.pair_offsets_dev, dwin.layout.max_corr_per_pair, p_dev)
            ws.sync()
            out = host_optimize(corr, n_match, n_frames, H, W, depths, colors, normals, poses, K, **kw)
            for k in range(n_frames):
                r, t = S.pose_error(p_dev[0, k].cpu().numpy(), np.asarray(poses[k]))
                seen["worst_r"], seen["worst_t"] = max(seen["worst_r"], r), max(seen["worst_t"], t)
            seen["ba"] += 1
            return out
        b.opt.optimizeFrames = optimize

    b, fm, poses, status, _ = _run_session(ws, scene, 6, False, hook)
    print(f"shadow session: {seen['kabsch']} initial poses, worst / max(1, |x|) vs fp64 Kabsch {seen['worst_init']:.3e} (bar {BAR:.3e}), vs the host's fp32 "
          f"Kabsch {seen['worst_host']:.3e}; {seen['ba']} BA calls, solved poses differ by {seen['worst_r']:.3e} rad, {seen['worst_t']:.3e} m")
    assert seen["kabsch"] == 5 and seen["ba"] == b.n_ba_calls == 5
    assert seen["worst_init"] <= BAR
    assert seen["worst_r"] < 1e-4 and seen["worst_t"] < 1e-4
    fm.close()


def test_free_running_device_session_tracks_like_the_host_path(ws, scene):
    pb, kp, frames = scene
    hb, hfm, h_poses, h_status, h_win = _run_session(ws, scene, 6, False)
    db, dfm, d_poses, d_status, d_win = _run_session(ws, scene, 6, True)
    assert d_status == h_status and all(s != "FAIL" for s in d_status)
    assert db.n_ba_calls == hb.n_ba_calls == 5
    worst = (0.0, 0.0)
    for k in range(6):
        r, t = S.pose_error(d_poses[k], pb.poses_gt[k])
        assert r < 0.02 and t < 0.01, (k, r, t)                                   # the bound of the host-path session test
        worst = max(worst, S.pose_error(d_poses[k], h_poses[k]))
    print(f"free-running device session vs host session: poses differ by at most {worst[0]:.3e} rad, {worst[1]:.3e} m")
    for hw, dw in zip(h_win[1:], d_win[1:]):
        assert [f.id for f in hw.frames] == [f.id for f in dw.frames] and hw.run_ba == dw.run_ba
        assert len(hw.n_match_per_pair) == len(dw.n_match_per_pair)               # (match sets may differ once poses differ in the last bits)
    # the switch falls back silently on a feature manager without device records
    seq = S.SyntheticSequence(3, seed=5)
    sfm = S.SyntheticFeatureManager(seq, corr_per_pair=50)
    sb = Bundler(hb.opt, sfm, pb.K, pb.H, pb.W, device_window=True)
    assert not sb._device_records()
    hfm.close()
    dfm.close()
