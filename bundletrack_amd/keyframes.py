"""The keyframe memory on the MI355X (btba_keyframes_*, btba_rotation_distances): Bundler::checkAndAddKeyframe and
Bundler::selectKeyFramesForBA for many tracking sessions at once, on device memory.

DeviceKeyframeMemory holds S sessions' pools and takes torch tensors (or anything torch.as_tensor takes); every call but export is
asynchronous on the workspace stream.  KeyframeSession is one session behind bundler.KeyframeMemory's interface, for
Bundler(memory=KeyframeSession(...)).  The exact rules are in include/btba.h ("device keyframe memory"); tests/keyframes_ref.py restates
them.  The distance's arc cosine is the memory's own function (csrc/btba_keyframes_point.hpp), within one float ulp of the C library's."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import check, lib

LDS_LIMIT = 160 * 1024


def max_capacity(max_BA_frames: int) -> int:
    """The largest pool btba_keyframes_create accepts for this max_BA_frames (csrc/btba_keyframes_layout.hpp: the select kernel's LDS)."""
    up = lambda x: (x + 15) & ~15
    return (LDS_LIMIT - 2 * up(4 * max_BA_frames) - 48) // (4 * max_BA_frames)


@dataclass
class DeviceWindows:
    """btba_keyframes_select's outputs, CUDA tensors: rows ordered by frame id, rows at and past n_window keep their previous bytes."""
    n_window: object            # int32 [S]
    slot: object                # int32 [S, max_BA]: the pool slot, -1 for the new frame
    frame_id: object            # int32 [S, max_BA]
    frame_key: object           # int64 [S, max_BA]: the uint64 keys' bits
    pose: object                # float32 [S, max_BA, 4, 4]
    newframe_index: object      # int32 [S]


class DeviceKeyframeMemory:
    def __init__(self, ws, n_sessions: int, capacity: int, max_BA_frames: int = 15, min_rot_deg: float = 10.0, min_feat_num: int = 0):
        self.ws = ws
        self.n_sessions, self.capacity, self.max_BA_frames = int(n_sessions), int(capacity), int(max_BA_frames)
        self.min_rot_deg, self.min_feat_num = float(min_rot_deg), int(min_feat_num)
        h = C.c_void_p()
        check(lib().btba_keyframes_create(ws.handle, self.n_sessions, self.capacity, self.max_BA_frames, C.byref(h)), "btba_keyframes_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().btba_keyframes_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, x, dtype, shape, default=None):
        """x (or a constant `default`) as a contiguous CUDA tensor of this dtype and shape."""
        import torch
        if x is None:
            return torch.full(shape, default, dtype=dtype, device="cuda")
        if isinstance(x, np.ndarray) and x.dtype == np.uint64:
            x = x.view(np.int64)
        t = torch.as_tensor(x).to(device="cuda", dtype=dtype).contiguous()
        if t.numel() != int(np.prod(shape)):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.reshape(shape)

    def _active(self, active):
        import torch
        return None if active is None else self._dev(active, torch.int32, (self.n_sessions,))

    def reset(self, session: int = -1):
        check(lib().btba_keyframes_reset(self._h, int(session)), "btba_keyframes_reset")

    def check_add(self, pose, frame_id, frame_key=None, status_other=None, n_keypts=None, active=None, min_rot_deg=None, min_feat_num=None, out=None):
        """One frame per session: pose [S, 4, 4], frame_id [S], frame_key [S] (uint64 bits; default 0), status_other [S] (default 1),
        n_keypts [S] (default: enough).  Returns int32 [S] on the device: 1 joined, 0 not, -1 the pool is full; inactive sessions keep `out`'s bytes."""
        import torch
        S = self.n_sessions
        mf = self.min_feat_num if min_feat_num is None else int(min_feat_num)
        args = (self._dev(pose, torch.float32, (S, 16)), self._dev(frame_id, torch.int32, (S,)), self._dev(frame_key, torch.int64, (S,), 0),
                self._dev(status_other, torch.int32, (S,), 1), self._dev(n_keypts, torch.int32, (S,), max(mf, 0)), self._active(active))
        added = torch.zeros((S,), dtype=torch.int32, device="cuda") if out is None else out
        check(lib().btba_keyframes_check_add(self._h, self.min_rot_deg if min_rot_deg is None else float(min_rot_deg), mf,
                                             None if args[5] is None else args[5].data_ptr(), args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(),
                                             args[3].data_ptr(), args[4].data_ptr(), added.data_ptr()), "btba_keyframes_check_add")
        return added

    def empty_windows(self) -> DeviceWindows:
        import torch
        S, B = self.n_sessions, self.max_BA_frames
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        return DeviceWindows(z((S,), torch.int32), z((S, B), torch.int32), z((S, B), torch.int32), z((S, B), torch.int64), z((S, B, 4, 4), torch.float32),
                             z((S,), torch.int32))

    def select(self, newpose, new_frame_id, new_frame_key=None, active=None, out: DeviceWindows | None = None) -> DeviceWindows:
        """The BA window of every session for its new frame (not a pool member): newpose [S, 4, 4], new_frame_id [S], new_frame_key [S]."""
        import torch
        S = self.n_sessions
        w = self.empty_windows() if out is None else out
        args = (self._dev(newpose, torch.float32, (S, 16)), self._dev(new_frame_id, torch.int32, (S,)), self._dev(new_frame_key, torch.int64, (S,), 0),
                self._active(active))
        check(lib().btba_keyframes_select(self._h, None if args[3] is None else args[3].data_ptr(), args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(),
                                          w.n_window.data_ptr(), w.slot.data_ptr(), w.frame_id.data_ptr(), w.frame_key.data_ptr(), w.pose.data_ptr(),
                                          w.newframe_index.data_ptr()), "btba_keyframes_select")
        return w

    def writeback(self, n_window, slot, pose, active=None):
        """The solved poses of the windows' keyframes back into the pools: n_window [S], slot [S, max_BA], pose [S, max_BA, 4, 4]."""
        import torch
        S, B = self.n_sessions, self.max_BA_frames
        args = (self._dev(n_window, torch.int32, (S,)), self._dev(slot, torch.int32, (S, B)), self._dev(pose, torch.float32, (S, B, 16)), self._active(active))
        check(lib().btba_keyframes_writeback(self._h, None if args[3] is None else args[3].data_ptr(), args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr()),
              "btba_keyframes_writeback")

    def export(self) -> dict:
        """A synchronising host copy: count, overflow [S], frame_id, frame_key [S, capacity], poses [S, capacity, 4, 4]."""
        S, Cp = self.n_sessions, self.capacity
        out = dict(count=np.zeros(S, np.int32), overflow=np.zeros(S, np.int32), frame_id=np.zeros((S, Cp), np.int32), frame_key=np.zeros((S, Cp), np.uint64),
                   poses=np.zeros((S, Cp, 4, 4), np.float32))
        check(lib().btba_keyframes_export(self._h, out["count"].ctypes.data, out["overflow"].ctypes.data, out["frame_id"].ctypes.data,
                                          out["frame_key"].ctypes.data, out["poses"].ctypes.data), "btba_keyframes_export")
        return out

    def rotation_distances(self, A, B):
        return rotation_distances(self.ws, A, B)


def rotation_distances(ws, A, B):
    """btba_rotation_distances: the memory's distance of n pose pairs ([n, 4, 4] each), float32 [n] on the device."""
    import torch
    A = torch.as_tensor(A).to(device="cuda", dtype=torch.float32).contiguous()
    B = torch.as_tensor(B).to(device="cuda", dtype=torch.float32).contiguous()
    n = A.numel() // 16
    if A.numel() != 16 * n or B.numel() != 16 * n:
        raise ValueError("rotation_distances: two arrays of n 4 x 4 poses")
    out = torch.empty((n,), dtype=torch.float32, device="cuda")
    check(lib().btba_rotation_distances(ws.handle, n, A.data_ptr(), B.data_ptr(), out.data_ptr()), "btba_rotation_distances")
    return out


class KeyframeSession:
    """One tracking session on a DeviceKeyframeMemory of its own, with bundler.KeyframeMemory's interface.  The FrameRefs stay on the host;
    poses that changed since the last call (bundle adjustment moves the window's keyframes) go to the pool through writeback before the
    call's kernel; every call takes one small device-to-host copy."""

    def __init__(self, ws, min_rot_deg: float = 10.0, min_feat_num: int = 0, max_BA_frames: int = 15, capacity: int | None = None):
        self.max_BA_frames = int(max_BA_frames)
        self.mem = DeviceKeyframeMemory(ws, 1, min(1024, max_capacity(self.max_BA_frames)) if capacity is None else capacity, self.max_BA_frames,
                                        min_rot_deg, min_feat_num)
        self.min_rot_deg, self.min_feat_num = self.mem.min_rot_deg, self.mem.min_feat_num
        self.keyframes: list = []
        self._pushed: list = []                  # the pose the pool holds of every keyframe

    def _push_changed_poses(self):
        B = self.max_BA_frames
        changed = [k for k, (kf, p) in enumerate(zip(self.keyframes, self._pushed)) if not np.array_equal(np.asarray(kf.pose_in_model, np.float32), p)]
        for c0 in range(0, len(changed), B):
            part = changed[c0:c0 + B]
            slot, pose = np.full((1, B), -1, np.int32), np.zeros((1, B, 16), np.float32)
            for r, k in enumerate(part):
                self._pushed[k] = np.array(self.keyframes[k].pose_in_model, np.float32)
                slot[0, r], pose[0, r] = k, self._pushed[k].reshape(16)
            self.mem.writeback(np.array([len(part)], np.int32), slot, pose)

    def check_and_add_keyframe(self, frame) -> bool:
        self._push_changed_poses()
        pose = np.asarray(frame.pose_in_model, np.float32).reshape(1, 16)
        added = int(self.mem.check_add(pose, [int(frame.id)], np.array([int(frame.id)], np.uint64), [int(frame.status == "OTHER")],
                                       [int(frame.n_keypts)]).cpu()[0])
        if added < 0:
            raise RuntimeError(f"KeyframeSession: the pool is full ({self.mem.capacity} keyframes)")
        if added:
            self.keyframes.append(frame)
            self._pushed.append(np.array(frame.pose_in_model, np.float32))
        return bool(added)

    def select_keyframes_for_ba(self, newframe) -> list:
        import torch
        self._push_changed_poses()
        w = self.mem.select(np.asarray(newframe.pose_in_model, np.float32).reshape(1, 16), [int(newframe.id)], np.array([int(newframe.id)], np.uint64))
        host = torch.cat([w.n_window, w.slot.reshape(-1)]).cpu().numpy()
        return [newframe if s < 0 else self.keyframes[s] for s in host[1:1 + int(host[0])]]
