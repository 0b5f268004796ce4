"""A tracking session with the device keyframe memory: tests/test_tracking_session.py's synthetic orbit, rebuilt from bundletrack_amd.synthetic,
through Bundler(memory=KeyframeSession(...)) and through the default host memory.  At every call the device memory's answer is held, on the
poses of that moment, to the restatement (bytes), to the decision bar of tests/test_keyframes_ref.py (every greedy round's pick lies in A;
a gate decision may differ from the host's only inside the bar) and to the host memory wherever every round's A was a singleton."""
import numpy as np
import pytest

import keyframes_ref as G
from bundletrack_amd import synthetic as S
from bundletrack_amd.bundler import Bundler, FrameRef, KeyframeMemory

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
MAX_BA, MIN_ROT = 5, 10.0


class Checked:
    """KeyframeSession behind KeyframeMemory's interface, every answer checked before it is handed on."""

    def __init__(self, session):
        self.session = session
        self.n_select = self.n_greedy = self.n_rounds = self.n_open = self.n_gate = self.n_gate_near = 0

    @property
    def keyframes(self):
        return self.session.keyframes

    def _pool(self):
        kfs = self.session.keyframes
        return G.filled(np.stack([np.asarray(k.pose_in_model, F).reshape(16) for k in kfs]), np.array([k.id for k in kfs], np.int32),
                        np.array([k.id for k in kfs], np.uint64), len(kfs))

    def _host(self):
        return KeyframeMemory(min_rot_deg=MIN_ROT, max_BA_frames=MAX_BA, keyframes=list(self.session.keyframes))

    def check_and_add_keyframe(self, frame):
        kfs = list(self.session.keyframes)
        host = self._host().check_and_add_keyframe(frame)
        got = self.session.check_and_add_keyframe(frame)
        if frame.id != 0 and kfs:
            pose = np.asarray(frame.pose_in_model, F)
            P = np.stack([np.asarray(k.pose_in_model, F) for k in kfs])
            deg64 = np.degrees(np.arccos(G.tmp(np.broadcast_to(pose, P.shape), P).astype(D)))
            near = bool((np.abs(deg64 - MIN_ROT) <= 2 * np.spacing(deg64.astype(F)).astype(D) + (180 / np.pi) * 2.0 ** -22).any())
            self.n_gate += 1
            self.n_gate_near += near
            assert near or got == host, (frame.id, got, host)
        return got

    def select_keyframes_for_ba(self, newframe):
        pool = self._pool()                                               # the poses of this moment
        newpose = np.asarray(newframe.pose_in_model, F)
        got = [f.id for f in self.session.select_keyframes_for_ba(newframe)]
        self.n_select += 1
        singleton = [True]
        P = pool.poses.reshape(-1, 4, 4)

        def on_round(chosen, cand, cum, pick):
            mem = [P[m] for m in sorted(chosen)] + [newpose]
            n = len(mem)
            S64 = sum(np.arccos(G.tmp(P[cand], np.broadcast_to(m, (len(cand), 4, 4))).astype(D)) for m in mem)
            E = n * 2.0 ** -22 + (n - 1) * 0.5 * float(np.spacing(F(S64.max())))
            A = [c for c, v in zip(cand, S64) if v <= S64.min() + 2 * E]
            self.n_rounds += 1
            assert pick in A, (newframe.id, chosen, pick, A)
            if len({P[c].tobytes() for c in A}) > 1:
                self.n_open += 1
                singleton[0] = False

        ref = G.select(pool, newpose, newframe.id, newframe.id, MAX_BA)
        G.greedy_members(pool, newpose, MAX_BA, on_round=on_round)
        assert got == ref["window_frame_id"][: ref["n_window"]].tolist(), newframe.id      # the device's window: the restatement's, admissible round by round
        self.n_greedy += pool.count + 1 > MAX_BA
        if singleton[0]:
            assert got == [f.id for f in self._host().select_keyframes_for_ba(newframe)], newframe.id
        return [newframe if i == newframe.id else next(k for k in self.session.keyframes if k.id == i) for i in got]


def run_session(optimizer, n_frames, memory=None):
    import torch
    seq = S.SyntheticSequence(n_frames=n_frames, seed=S.config_seed(1))
    fm = S.SyntheticFeatureManager(seq, corr_per_pair=300)
    bundler = Bundler(optimizer, fm, seq.K, seq.H, seq.W, window_size=5, max_BA_frames=MAX_BA, min_rot_deg=MIN_ROT, memory=memory)
    frames = []
    for k in range(n_frames):
        depth, normals = seq.render(k)
        fr = FrameRef(id=0, pose_in_model=seq.poses_gt[0].astype(F), n_keypts=300, depth_gpu=torch.from_numpy(depth).cuda(), normal_gpu=torch.from_numpy(normals).cuda())
        fm.register(fr, k)
        bundler.process_new_frame(fr)
        frames.append(fr)
        assert len(bundler.local_frames) <= MAX_BA
    return seq, bundler, frames


def test_session_on_the_device_memory_and_on_the_host_memory():
    from bundletrack_amd.keyframes import KeyframeSession
    from bundletrack_amd.optimizer import OptimizerGpu, Workspace
    n = 30
    ws = Workspace()
    checked = Checked(KeyframeSession(ws, min_rot_deg=MIN_ROT, max_BA_frames=MAX_BA, capacity=64))
    seq, dev, frames_dev = run_session(OptimizerGpu(workspace=ws), n, memory=checked)
    _, hst, frames_hst = run_session(OptimizerGpu(workspace=Workspace()), n)
    print("selects %d (greedy %d, rounds %d, with distinct poses in A %d); gate decisions %d (inside the bar %d); keyframes %s"
          % (checked.n_select, checked.n_greedy, checked.n_rounds, checked.n_open, checked.n_gate, checked.n_gate_near, [k.id for k in dev.keyframes]))
    assert checked.n_select == n - 1 and checked.n_greedy >= 10 and dev.n_ba_calls == n - 1
    assert [k.id for k in dev.keyframes] == [k.id for k in hst.keyframes]                       # the pools agree
    if checked.n_open == 0 and checked.n_gate_near == 0:                                        # then both sessions took the same windows: the same poses, bit for bit
        for a, b in zip(frames_dev, frames_hst):
            assert np.array_equal(a.pose_in_model, b.pose_in_model), a.id
    e = checked.session.mem.export()
    assert e["count"][0] == len(dev.keyframes) and e["overflow"][0] == 0
    assert e["frame_id"][0, : e["count"][0]].tolist() == [k.id for k in dev.keyframes]
    errs = np.array([S.pose_error(f.pose_in_model, seq.poses_gt[k]) for k, f in enumerate(frames_dev)])
    assert errs[:, 0].max() < np.deg2rad(0.5) and errs[:, 1].max() < 0.005, errs.max(0)
