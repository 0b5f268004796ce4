"""btba_corres_chain and btba_mappoints on the MI355X against tests/corres_ref.py: every pair's records (bit for bit), counts,
stage counts and the FAIL status equal the restatement's, whose NN matches come from tests/match_ref.py and whose RANSAC inliers
come from btba_ransac_pairs_ex on the same points; the map-point state equals the restatement's as track sets.  Also: forget and
slot reuse, a chain of n pairs = n one-pair chains, run-to-run determinism, propagated matches on planted landmarks, a Bundler
session.  One module-scoped workspace, no subprocesses."""
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S

from corres_ref import CorresRef, export_tracks, model_points
from match_ref import restate, scene_frames


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


def _dev(frames):
    import torch
    from bundletrack_amd.bundler import FrameRef
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    return [FrameRef(id=f.id, pose_in_model=f.pose, kpts_gpu=t(f.kpts), desc_gpu=t(f.desc), depth_gpu=t(f.depth), normal_gpu=t(f.normal))
            for f in frames]


@pytest.fixture(scope="module")
def scene():
    """7 frames with ids 0 1 2 3 5 6 7 (a keyframe gap between 3 and 5), ~330 keypoints each (the visible of 650 landmarks + 60
    distractors), duplicate (u, v) keypoints injected.
    Landmark descriptors drift from frame to frame (appearance change): neighbours match directly, distant frames miss landmarks
    that the map points then propagate."""
    pb = S.make_problem(7, 10, seed=31, background=False, rot_step_deg=(4.0, 5.0))
    kp = S.make_keypoints(pb, 650, 60, D=64, seed=31)
    rng = np.random.default_rng(5)
    drift = rng.normal(size=(len(kp.landmarks_model), 64))
    drift /= np.linalg.norm(drift, axis=1, keepdims=True)
    for k in range(len(kp.desc)):
        lm = np.asarray(kp.landmark[k])
        d = kp.desc[k].astype(np.float64)
        d[lm >= 0] += 0.45 * k * drift[lm[lm >= 0]]
        kp.desc[k] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    frames = scene_frames(pb, kp)
    for k, f in enumerate(frames):
        f.id = [0, 1, 2, 3, 5, 6, 7][k]
        n = f.kpts.shape[0]
        src = rng.choice(n, 6, replace=False)
        f.kpts = f.kpts.copy()
        f.kpts[src[3:]] = f.kpts[src[:3]]                      # three keypoints repeat another one's (u, v)
    return pb, kp, frames


# frame indices (A newer); the chains a tracker would run as frames arrive
CHAINS = [[(1, 0)], [(2, 1), (2, 0)], [(3, 2), (3, 0), (3, 1)], [(4, 3), (4, 2), (4, 0)], [(5, 4), (5, 3), (5, 1), (5, 0)]]
AFTER_FORGET = [[(6, 5), (6, 4), (6, 2), (6, 0)]]


class _Ref:
    """The restatement driven like the chain: NN per pair from match_ref, RANSAC per pair from btba_ransac_pairs_ex."""

    def __init__(self, ws, frames, pb, prm):
        self.ws, self.frames, self.pb, self.prm = ws, frames, pb, prm
        self.R, self.status, self.pts = CorresRef(), {}, {}

    def register(self, k):
        self.R.register(k, self.frames[k].kpts)

    def nn(self, a, b):
        recs = restate(self.frames, [(a, b)], self.prm, self.pb.K, self.pb.H, self.pb.W)[0][0]
        for r in recs:
            self.pts.setdefault((a, self.R.key_index(a, self.R.uv(a, r["idx_a"]))), r["ptA_cam"].copy())
            self.pts.setdefault((b, self.R.key_index(b, self.R.uv(b, r["idx_b"]))), r["ptB_cam"].copy())
        return recs

    def chain(self, pairs):
        from bundletrack_amd.ransac import ransac_packed
        nns = [self.nn(a, b) for a, b in pairs]           # NN reads no map state
        out = []
        for (a, b), nn in zip(pairs, nns):
            def rs(recs, a=a, b=b):
                pa, pb = model_points(recs, self.frames[a].pose, self.frames[b].pose)
                return ransac_packed(self.ws, pa, pb, np.array([len(recs)], np.int32))[0]["inlier_ids"]
            neighbor = abs(self.frames[a].id - self.frames[b].id) == 1
            out.append(self.R.find_corres(a, b, neighbor, nn, self.status, rs, lambda f, i: self.pts[(f, i)]))
        return out


class _Gpu:
    def __init__(self, ws, frames, pb, prm):
        from bundletrack_amd.correspondence import MapPointMemory
        self.ws, self.frames, self.pb, self.prm = ws, frames, pb, prm
        self.dev = _dev(frames)
        self.mem = MapPointMemory(ws)
        self.slots = [-1] * len(frames)
        self.status = np.zeros(len(frames), np.int32)

    def register(self, k):
        self.slots[k] = self.mem.register_frame(self.dev[k].kpts_gpu)

    def forget(self, k):
        self.mem.forget_frame(self.slots[k])
        self.slots[k] = -1

    def chain(self, pairs, device_resident=True):
        from bundletrack_amd.correspondence import find_corres_chain
        res = find_corres_chain(self.ws, self.mem, self.dev, pairs, self.slots, self.status, self.prm, K=self.pb.K, H=self.pb.H, W=self.pb.W,
                                device_resident=device_resident)
        self.status = res.status
        return res

    def tracks(self):
        return Counter(export_tracks(self.mem.export(), {s: k for k, s in enumerate(self.slots) if s >= 0}))

    def close(self):
        self.mem.close()


def _ref_tracks(R):
    return Counter(frozenset((f, R.key_index(f, uv)) for f, uv in d.items()) for d in R.img.values())


def _compare(g, r, pairs):
    for (a, b), got, n, sc, (ref, rsc) in zip(pairs, g.per_pair, g.n_out, g.stage_counts, r):
        assert list(sc) == rsc, (a, b, list(sc), rsc)
        assert n == len(ref) and got.tobytes() == ref.tobytes(), (a, b)


def _run_sequence(gpu, ref, chains, check=True):
    results = []
    for pairs in chains:
        for k in sorted({f for p in pairs for f in p}):
            if gpu.slots[k] < 0:
                gpu.register(k)
                if ref is not None:
                    ref.register(k)
        g = gpu.chain(pairs)
        results.append(g)
        if ref is not None and check:
            r = ref.chain(pairs)
            _compare(g, r, pairs)
            assert [bool(s) for s in g.status] == [bool(ref.status.get(k, False)) for k in range(len(gpu.frames))]
    return results


def test_chain_equals_restatement_with_forget_and_slot_reuse(ws, scene):
    pb, kp, frames = scene
    prm = _lib.match_params()
    gpu, ref = _Gpu(ws, frames, pb, prm), _Ref(ws, frames, pb, prm)
    res = _run_sequence(gpu, ref, CHAINS)
    assert gpu.tracks() == _ref_tracks(ref.R)
    assert sum(int((r["dir"] == 2).sum()) for g in res for r in g.per_pair) > 0        # propagation happened
    # forget frame 1 (slot freed) and let the next frame take its slot
    freed = gpu.slots[1]
    gpu.forget(1)
    ref.R.forget(1)
    assert gpu.tracks() == _ref_tracks(ref.R)
    gpu.register(6)
    ref.register(6)
    assert gpu.slots[6] == freed
    _run_sequence(gpu, ref, AFTER_FORGET)
    assert gpu.tracks() == _ref_tracks(ref.R)
    assert gpu.mem.export()["overflow"] == 0
    gpu.close()


def test_one_chain_equals_single_pair_chains_and_is_deterministic(ws, scene):
    pb, kp, frames = scene
    prm = _lib.match_params()
    whole = _Gpu(ws, frames, pb, prm)
    a = _run_sequence(whole, None, CHAINS)
    again = _Gpu(ws, frames, pb, prm)
    b = _run_sequence(again, None, CHAINS)
    single = _Gpu(ws, frames, pb, prm)
    c = _run_sequence(single, None, [[p] for ch in CHAINS for p in ch])
    flat_a = [x for g in a for x in g.per_pair]
    flat_b = [x for g in b for x in g.per_pair]
    flat_c = [g.per_pair[0] for g in c]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(flat_a, flat_b))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(flat_a, flat_c))
    assert list(whole.status) == list(single.status) == list(again.status)
    assert whole.tracks() == single.tracks()
    # the host output form gives the same records
    host = _Gpu(ws, frames, pb, prm)
    for k in range(len(frames) - 1):
        host.register(k)
    flat_h = []
    for pairs in CHAINS:
        flat_h += host.chain(pairs, device_resident=False).per_pair
    assert all(x.tobytes() == y.tobytes() for x, y in zip(flat_a, flat_h))


def test_status_cases(ws, scene):
    pb, kp, frames = scene
    # one-directional matching on planted landmarks: (1, 0) has 6 matches; frame 2 shares only 4 landmarks with frame 1, so (2, 1)
    # marks 2 FAIL at the NN stage, and (2, 0) of the same chain (8 NN matches) is short-circuited by that FAIL: its matches stay
    L = _spread_landmarks(kp, [0, 1, 2], 10)
    small = [_small_frame(kp, frames, 0, L), _small_frame(kp, frames, 1, L[:6]), _small_frame(kp, frames, 2, L[:4] + L[6:])]
    prm = _lib.match_params(mutual=0)
    gpu, ref = _Gpu(ws, small, pb, prm), _Ref(ws, small, pb, prm)
    res = _run_sequence(gpu, ref, [[(1, 0)], [(2, 1), (2, 0)]])
    assert not gpu.status[1] and gpu.status[2]
    assert list(res[1].stage_counts[0]) == [4, 4, 4, 4]
    assert list(res[1].stage_counts[1]) == [8, 8, 8, 8] and res[1].n_out[1] == 8
    gpu.close()
    # a FAIL status coming in short-circuits every pair of A
    gpu2, ref2 = _Gpu(ws, frames, pb, _lib.match_params()), _Ref(ws, frames, pb, _lib.match_params())
    gpu2.status[3] = 1
    ref2.status[3] = True
    res = _run_sequence(gpu2, ref2, [[(3, 2), (3, 0)]])
    assert all(res[0].stage_counts[p][0] > 0 and (res[0].stage_counts[p] == res[0].stage_counts[p][0]).all() for p in range(2))
    gpu2.close()


def _spread_landmarks(kp, frames_k, n, min_dist=0.04):
    """n landmarks seen in every frame of frames_k, pairwise at least min_dist apart in the model (no wrong match passes the gate)."""
    common = set(int(l) for l in kp.landmark[frames_k[0]] if l >= 0)
    for k in frames_k[1:]:
        common &= set(int(l) for l in kp.landmark[k])
    out = []
    for l in sorted(common):
        if all(np.linalg.norm(kp.landmarks_model[l] - kp.landmarks_model[m]) > min_dist for m in out):
            out.append(l)
        if len(out) == n:
            return out
    raise AssertionError("scene has too few spread landmarks")


def _small_frame(kp, frames, k, lms, extra=()):
    """HostFrame of scene frame k with the (undisturbed) keypoints of landmarks lms, plus extra (uv, desc) keypoints."""
    from match_ref import HostFrame
    lm = np.asarray(kp.landmark[k])
    idx = [int(np.nonzero(lm == l)[0][0]) for l in lms]
    kpts, desc = kp.kpts[k][idx], kp.desc[k][idx]
    for uv, d in extra:
        kpts = np.concatenate([kpts, np.asarray(uv, np.float32).reshape(1, 2)])
        desc = np.concatenate([desc, np.asarray(d, np.float32).reshape(1, -1)])
    f = frames[k]
    return HostFrame(f.id, f.pose, np.ascontiguousarray(kpts, np.float32), np.ascontiguousarray(desc, np.float32), f.depth, f.normal)


def test_exactly_five_and_six_matches(ws, scene):
    """One-directional matching on frames of 5 / 6 / 6 planted landmarks: (1, 0) has exactly 5 NN matches -- cleared before RANSAC,
    and the neighbour A marked FAIL by the final gate; (2, 1) has exactly 6 -- RANSAC runs and keeps them."""
    pb, kp, frames = scene
    L = _spread_landmarks(kp, [0, 1, 2], 6)
    small = [_small_frame(kp, frames, 0, L[:5]), _small_frame(kp, frames, 1, L), _small_frame(kp, frames, 2, L)]
    prm = _lib.match_params(mutual=0)
    gpu, ref = _Gpu(ws, small, pb, prm), _Ref(ws, small, pb, prm)
    res = _run_sequence(gpu, ref, [[(1, 0)], [(2, 1)]])
    assert list(res[0].stage_counts[0]) == [5, 5, 0, 0] and res[0].n_out[0] == 0
    assert gpu.status[1] and not gpu.status[2]
    assert list(res[1].stage_counts[0]) == [6, 6, 6, 6]
    gpu.close()


def test_shared_map_point_last_writer(ws, scene):
    """Two B keys of one map point matched by two A keys of the same pair: img[A] is the later match's (the stamp / atomicMax path)."""
    pb, kp, frames = scene
    L = _spread_landmarks(kp, [0, 1, 2], 6)
    rng = np.random.default_rng(9)
    r = rng.normal(size=kp.desc[0].shape[1])
    r /= np.linalg.norm(r)

    def twin(k):                                           # 1.5 px right of landmark L[0], its descriptor pushed along r
        lm = np.asarray(kp.landmark[k])
        i = int(np.nonzero(lm == L[0])[0][0])
        d = kp.desc[k][i] + 0.5 * r
        return (kp.kpts[k][i] + np.float32([1.5, 0.0]), d / np.linalg.norm(d))
    small = [_small_frame(kp, frames, 0, L), _small_frame(kp, frames, 1, L, [twin(1)]), _small_frame(kp, frames, 2, L, [twin(2)])]
    prm = _lib.match_params()
    gpu, ref = _Gpu(ws, small, pb, prm), _Ref(ws, small, pb, prm)
    _run_sequence(gpu, ref, [[(1, 0)], [(2, 1)]])
    R = ref.R
    mp = R.maps[1][R.uv(1, 6)]
    assert R.maps[1][R.uv(1, 0)] == mp                     # the twin joined L[0]'s map point in (1, 0)
    assert R.img[mp][2] == R.uv(2, 6)                      # (2, 1): L[0] of 2 wrote first, the twin of 2 last
    assert gpu.tracks() == _ref_tracks(R)
    assert frozenset({(0, 0), (1, 6), (2, 6)}) in gpu.tracks()
    gpu.close()


def test_propagated_matches_link_planted_landmarks(ws, scene):
    pb, kp, frames = scene
    gpu = _Gpu(ws, frames, pb, _lib.match_params())
    res = _run_sequence(gpu, None, CHAINS)
    good = total = 0
    for pairs, g in zip(CHAINS, res):
        for (a, b), recs in zip(pairs, g.per_pair):
            prop = recs[recs["dir"] == 2]
            total += len(prop)
            good += int(sum(1 for r in prop if kp.landmark[a][r["idx_a"]] >= 0 and
                            kp.landmark[a][r["idx_a"]] == kp.landmark[b][r["idx_b"]]))
    print(f"propagated matches after RANSAC: {good} of {total} link the same planted landmark")   # measured: 15 of 15
    assert total >= 10
    assert good / total >= 0.9, (good, total)


def test_workspace_destroy_returns_the_chain_scratch(scene):
    """A workspace hands its chain scratch back to the device when it is destroyed.  One chain of 2^22 hash-drawn trials makes the
    per-trial regions (48 + 4 bytes a trial) about 218 MB, about 272 MB after the buffer's growth rule; once the memory and the
    workspace are closed, free device memory is back within the 64 MiB that test_scratch_does_not_grow_over_repeated_calls allows
    for allocator noise.  Own workspace: the module's one stays alive."""
    import torch
    from bundletrack_amd.correspondence import MapPointMemory, find_corres_chain
    from bundletrack_amd.optimizer import Workspace
    pb, kp, frames = scene
    L = _spread_landmarks(kp, [0, 1], 36, min_dist=0.02)
    dev = _dev([_small_frame(kp, frames, 0, L), _small_frame(kp, frames, 1, L)])
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    w = Workspace()
    mem = MapPointMemory(w)
    slots = [mem.register_frame(f.kpts_gpu) for f in dev]
    rp = _lib.corres_params(hypothesis=_lib.RANSAC_REFERENCE_SVD | _lib.RANSAC_DRAW_HASH, n_trials=1 << 22)
    res = find_corres_chain(w, mem, dev, [(1, 0)], slots, np.zeros(2, np.int32), _lib.match_params(), rp, K=pb.K, H=pb.H, W=pb.W)
    held = free0 - torch.cuda.mem_get_info()[0]
    assert res.stage_counts[0][0] > 0                      # the chain ran: there were matches to vote on
    mem.close()
    w.close()
    del res
    torch.cuda.synchronize()
    kept = free0 - torch.cuda.mem_get_info()[0]
    print(f"device memory held during the chain {held / 2**20:.1f} MiB, kept after destroy {kept / 2**20:.1f} MiB")
    assert kept < 64 << 20, kept


def _session_driver():
    import ctypes as C
    so = _lib.build_driver("corres_driver")
    f = C.CDLL(so).corres_session
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 5 + \
                 [C.c_int, C.c_void_p, C.c_int64]
    return f


def test_bundler_session_python_equals_cpp(ws, scene):
    """A Bundler session on GpuFeatureManager (window 5, 5 BA frames): Bundler.optimize_gpu hands whole windows to find_corres_chain, the
    frames are tracked, and btba::Bundler on btba::GpuFeatureManager (tests/cpp/corres_driver.cpp) gives the same poses and match sets."""
    import ctypes as C
    import torch
    from bundletrack_amd.bundler import Bundler, FrameRef
    from bundletrack_amd.correspondence import GpuFeatureManager
    from bundletrack_amd.optimizer import OptimizerGpu
    pb, kp, frames = scene
    n = 6
    dev = _dev(frames[:n])
    fm = GpuFeatureManager(ws, pb.K, pb.H, pb.W)
    calls = []
    orig = fm.find_corres_chain
    fm.find_corres_chain = lambda pairs: (calls.append(len(pairs)), orig(pairs))[1]
    b = Bundler(OptimizerGpu(workspace=ws), fm, pb.K, pb.H, pb.W, window_size=5, max_BA_frames=5)
    poses, status = [], []
    for k in range(n):
        d = dev[k]
        fr = FrameRef(id=0, pose_in_model=np.asarray(pb.poses_gt[0], np.float32) if k == 0 else np.eye(4, dtype=np.float32),
                      kpts_gpu=d.kpts_gpu, desc_gpu=d.desc_gpu, depth_gpu=d.depth_gpu, normal_gpu=d.normal_gpu)
        b.process_new_frame(fr)
        poses.append(np.asarray(fr.pose_in_model, np.float32).copy())
        status.append(int(fr.status == "FAIL"))
        assert fr.status != "FAIL"
        r, tr = S.pose_error(fr.pose_in_model, pb.poses_gt[k])
        assert r < 0.02 and tr < 0.01, (k, r, tr)
    assert calls and max(calls) > 1
    records = {k: v for k, v in fm.records.items()}
    fm.close()

    ptr = lambda attr: (C.c_void_p * n)(*[getattr(f, attr).data_ptr() for f in dev])
    K = np.ascontiguousarray(pb.K, np.float32)
    nk = np.array([f.kpts_gpu.shape[0] for f in dev], np.int32)
    pose0 = np.ascontiguousarray(pb.poses_gt[0], np.float32)
    c_poses, c_status = np.zeros((n, 16), np.float32), np.zeros(n, np.int32)
    cap_keys, cap_rec = 64, 200000
    n_keys, keys, counts = np.zeros(1, np.int32), np.zeros((cap_keys, 2), np.int32), np.zeros(cap_keys, np.int32)
    rec = np.zeros(cap_rec, _lib.MATCH_DTYPE)
    rc = _session_driver()(ws.handle.value, n, pb.H, pb.W, K.ctypes.data, int(dev[0].desc_gpu.shape[1]), ptr("desc_gpu"), ptr("kpts_gpu"), nk.ctypes.data,
                           ptr("depth_gpu"), ptr("normal_gpu"), pose0.ctypes.data, 5, 5, c_poses.ctypes.data, c_status.ctypes.data,
                           n_keys.ctypes.data, keys.ctypes.data, counts.ctypes.data, cap_keys, rec.ctypes.data, cap_rec)
    assert rc == 0
    assert list(c_status) == status
    for k in range(n):
        assert np.allclose(c_poses[k].reshape(4, 4), poses[k], atol=2e-5), k
    o, c_records = 0, {}
    for i in range(int(n_keys[0])):
        c_records[(int(keys[i, 0]), int(keys[i, 1]))] = rec[o:o + counts[i]]
        o += int(counts[i])
    assert set(c_records) == set(records)
    for key in records:
        assert c_records[key].tobytes() == records[key].tobytes(), key
