"""Map points (feature tracks) and the tracker's whole per-pair findCorres on the MI355X (btba_mappoints_*, btba_corres_chain).

Mirrors SiftManager::findCorres (src/FeatureManager.cpp:173-240): NN matching, propagation of correspondences along the map
points to non-neighbouring pairs (findCorresByMapPoints, :489-521), RANSAC, the map-point update (updateFramePairMapPoints,
:448-487) and the FAIL gates, for an ordered list of frame pairs in one call that keeps every stage on the device.  The rules
are restated in include/btba.h; tests/corres_ref.py is their plain-Python form."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lfnet_model import Handle
from ._lib import MATCH_DTYPE, CorresParams, check, corres_params, lib, match_params
from .matching import _MATCH_WORDS, _dims, _frame_tables, params_from_config


class MapPointMemory(Handle):
    """btba_mappoints on a workspace: frame slots and map points on the device."""
    _destroy = "btba_mappoints_destroy"

    def __init__(self, ws):
        self.ws = ws
        h = C.c_void_p()
        check(lib().btba_mappoints_create(ws.handle, C.byref(h)), "btba_mappoints_create")
        self._h = h

    def register_frame(self, kpts_gpu) -> int:
        """Copy a frame's keypoints (float32 CUDA [n, 2], or None) into a free slot; returns the slot."""
        from .optimizer import _dev_ptr
        n = 0 if kpts_gpu is None else int(kpts_gpu.shape[0])
        slot = C.c_int32(-1)
        check(lib().btba_mappoints_register_frame(self.handle, n, _dev_ptr(kpts_gpu.contiguous(), "keypoints") if n else None, C.byref(slot)),
              "btba_mappoints_register_frame")
        return int(slot.value)

    def forget_frame(self, slot: int) -> None:
        check(lib().btba_mappoints_forget_frame(self.handle, int(slot)), "btba_mappoints_forget_frame")

    def export(self) -> dict:
        """Host copy: {"slot_n": int32 [S] (-1 = free slot), "canon": {slot: int32 [n]}, "map": {slot: int32 [n]}, "img": int32 [M, S]}."""
        L = lib()
        dims = np.zeros(4, np.int32)
        check(L.btba_mappoints_export(self.handle, dims.ctypes.data, None, None, None, None), "btba_mappoints_export")
        S, M, total = int(dims[0]), int(dims[1]), int(dims[2])
        slot_n = np.zeros(max(S, 1), np.int32)
        canon, mp = np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.int32)
        img = np.zeros((max(M, 1), max(S, 1)), np.int32)
        check(L.btba_mappoints_export(self.handle, dims.ctypes.data, slot_n.ctypes.data, canon.ctypes.data, mp.ctypes.data, img.ctypes.data),
              "btba_mappoints_export")
        out = {"slot_n": slot_n[:S], "canon": {}, "map": {}, "img": img[:M, :S], "overflow": int(dims[3])}
        off = 0
        for s in range(S):
            n = int(slot_n[s])
            if n < 0:
                continue
            out["canon"][s], out["map"][s] = canon[off:off + n].copy(), mp[off:off + n].copy()
            off += n
        return out

@dataclass
class ChainResult:
    per_pair: list                  # one MATCH_DTYPE array per pair (host copies)
    n_out: np.ndarray               # int32 [n_pairs]
    stage_counts: np.ndarray        # int32 [n_pairs, 4]: after NN, after propagation, after RANSAC, final
    status: np.ndarray              # int32 [n_frames]: nonzero = FAIL, after the chain
    matches_dev: object = None      # device_resident: int32 CUDA tensor [capacity, 10]


def chain_capacity(frames, pairs, params=None, *, H: int, W: int) -> int:
    """btba_corres_chain_capacity (host-only)."""
    prm = params if params is not None else match_params()
    n_kpts = np.array([0 if f.kpts_gpu is None else int(f.kpts_gpu.shape[0]) for f in frames], np.int32)
    pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    cap = C.c_int64(0)
    check(lib().btba_corres_chain_capacity(C.byref(prm), len(frames), int(H), int(W), _dims(frames), n_kpts.ctypes.data, pr.shape[0],
                                           pr.ctypes.data, C.byref(cap)), "btba_corres_chain_capacity")
    return int(cap.value)


def find_corres_chain(ws, memory: MapPointMemory, frames, pairs, slots, status, params=None, ransac: CorresParams | None = None, *,
                      K, H: int, W: int, device_resident: bool = True) -> ChainResult:
    """btba_corres_chain.  frames: FrameRef-like objects as matching.match_pairs takes them; pairs: [(ia, ib)] indices into frames,
    A newer, in processing order; slots: each frame's MapPointMemory slot; status: int32 [n_frames] (nonzero = FAIL) going in."""
    import torch
    prm = params if params is not None else match_params()
    rp = ransac if ransac is not None else corres_params()
    n = len(frames)
    D = _dims(frames)
    cap = chain_capacity(frames, pairs, prm, H=H, W=W)
    n_kpts, pr, (desc, kpts, depth, normal), poses, ids, Kf = _frame_tables(frames, pairs, K)
    sl = np.ascontiguousarray(np.asarray(slots, np.int32).reshape(n))
    st = np.ascontiguousarray(np.asarray(status, np.int32).reshape(n)).copy()
    P = pr.shape[0]
    n_out = np.zeros(max(P, 1), np.int32)
    stages = np.zeros((max(P, 1), 4), np.int32)
    res = ChainResult(per_pair=[], n_out=n_out[:P], stage_counts=stages[:P], status=st)
    if device_resident:
        dev = next((f.depth_gpu.device for f in frames if f.depth_gpu is not None), torch.device("cuda"))
        res.matches_dev = torch.zeros((max(cap, 1), _MATCH_WORDS), dtype=torch.int32, device=dev)
        out_p = res.matches_dev.data_ptr()
    else:
        host = np.zeros(max(cap, 1), MATCH_DTYPE)
        out_p = host.ctypes.data
    check(lib().btba_corres_chain(ws.handle, memory.handle, C.byref(prm), C.byref(rp), int(bool(device_resident)), n, int(H), int(W), Kf.ctypes.data,
                                  C.cast(desc, C.c_void_p), D, C.cast(kpts, C.c_void_p), n_kpts.ctypes.data, C.cast(depth, C.c_void_p),
                                  C.cast(normal, C.c_void_p), poses.ctypes.data, ids.ctypes.data, sl.ctypes.data, st.ctypes.data, P, pr.ctypes.data,
                                  out_p, n_out.ctypes.data, stages.ctypes.data),
          "btba_corres_chain")
    off = np.concatenate([[0], np.cumsum(res.n_out)]).astype(np.int64)
    total = int(off[-1])
    if device_resident:
        host = res.matches_dev[:total].cpu().numpy().view(MATCH_DTYPE).reshape(-1) if total else np.zeros(0, MATCH_DTYPE)
    res.per_pair = [host[off[p]:off[p + 1]].copy() for p in range(P)]
    return res


class GpuFeatureManager:
    """A concrete feature manager (the slice of SiftManager the Bundler uses) on btba_corres_chain: frames bring kpts_gpu / desc_gpu
    (float32 CUDA), depth_gpu and normal_gpu; matches[(A.id, B.id)] = (ptA_cam [n,3], ptB_cam [n,3]); records[...] keeps the
    btba_match records.  cfg: config_ycbineoat.yml-shaped dict (feature_corres.*, ransac.max_iter / inlier_dist) or None.
    Every processed pair's records also stay on the device: device_segments[(A.id, B.id)] = (first record, count) in
    device_records(), one int32 CUDA tensor [n, 10] -- what window.marshal_windows and window.procrustes_pairs read."""

    def __init__(self, ws, K, H: int, W: int, cfg: dict | None = None, *, seed: int = 0, hypothesis: int = 0):
        self.ws, self.K, self.H, self.W = ws, np.asarray(K, np.float32), int(H), int(W)
        self.params = params_from_config(cfg)
        rc = (cfg or {}).get("ransac", {})
        self.ransac = corres_params(n_trials=int(rc.get("max_iter", 2000)), dist_thres=float(rc.get("inlier_dist", 0.01)),
                                    hypothesis=int(hypothesis), seed=int(seed))
        self.memory = MapPointMemory(ws)
        self.matches: dict = {}
        self.records: dict = {}
        self.stage_counts: dict = {}
        self._slots: dict = {}                 # frame id -> slot
        self.device_segments: dict = {}        # (A.id, B.id) -> (first record, count) in the record pool
        self._pool = None                      # int32 CUDA [capacity, 10]: the live pairs' btba_match records
        self._pool_used = 0

    def _slot(self, frame) -> int:
        if frame.id not in self._slots:
            self._slots[frame.id] = self.memory.register_frame(frame.kpts_gpu)
        return self._slots[frame.id]

    def find_corres(self, frameA, frameB) -> None:
        self.find_corres_chain([(frameA, frameB)])

    def find_corres_chain(self, pairs) -> None:
        """findCorres for every (frameA, frameB) of `pairs` in order (pairs already matched are skipped), one device chain."""
        todo, seen = [], set()
        for fa, fb in pairs:
            key = (fa.id, fb.id)
            if key not in self.matches and key not in seen:
                seen.add(key)
                todo.append((fa, fb))
        if not todo:
            return
        frames, index = [], {}
        for fa, fb in todo:
            for f in (fa, fb):
                if id(f) not in index:
                    index[id(f)] = len(frames)
                    frames.append(f)
        slots = [self._slot(f) for f in frames]
        status = np.array([1 if f.status == "FAIL" else 0 for f in frames], np.int32)
        res = find_corres_chain(self.ws, self.memory, frames, [(index[id(a)], index[id(b)]) for a, b in todo], slots, status,
                                self.params, self.ransac, K=self.K, H=self.H, W=self.W)
        for f, s in zip(frames, res.status):
            if s:
                f.status = "FAIL"
        for (fa, fb), m, sc in zip(todo, res.per_pair, res.stage_counts):
            key = (fa.id, fb.id)
            self.records[key] = m
            self.stage_counts[key] = sc.copy()
            self.matches[key] = (np.ascontiguousarray(m["ptA_cam"]), np.ascontiguousarray(m["ptB_cam"]))
        self._keep_on_device(todo, res)

    def _keep_on_device(self, todo, res) -> None:
        """Append the chain's records (already pair after pair in res.matches_dev) to the pool; a full pool is rebuilt from its live
        segments at twice the size it needs."""
        import torch
        total = int(res.n_out.sum())
        if res.matches_dev is None:
            return
        if self._pool is None or self._pool_used + total > self._pool.shape[0]:
            live = sorted(self.device_segments.items(), key=lambda kv: kv[1][0])
            need = sum(c for _, (_, c) in live) + total
            fresh = torch.zeros((max(2 * need, 4096), _MATCH_WORDS), dtype=torch.int32, device=res.matches_dev.device)
            at = 0
            for key, (first, count) in live:
                fresh[at:at + count] = self._pool[first:first + count]
                self.device_segments[key] = (at, count)
                at += count
            self._pool, self._pool_used = fresh, at
        self._pool[self._pool_used:self._pool_used + total] = res.matches_dev[:total]
        at = self._pool_used
        for (fa, fb), n in zip(todo, res.n_out):
            self.device_segments[(fa.id, fb.id)] = (at, int(n))
            at += int(n)
        self._pool_used = at

    def device_records(self):
        """The record pool (int32 CUDA [capacity, 10]) device_segments index, or None before the first chain."""
        return self._pool

    def forget_frame(self, frame) -> None:
        """SiftManager::forgetFrame: the frame's pairs and its img entries go; its slot is free again."""
        for key in [k for k in self.matches if frame.id in k]:
            del self.matches[key]
            self.records.pop(key, None)
            self.stage_counts.pop(key, None)
            self.device_segments.pop(key, None)
        slot = self._slots.pop(frame.id, None)
        if slot is not None:
            self.memory.forget_frame(slot)

    def procrustes_by_correspondence(self, frameA, frameB) -> np.ndarray:
        """FeatureManager::procrustesByCorrespondence (:523-556), as the C++ host layer: bundler.procrustes_by_correspondence."""
        from .bundler import procrustes_by_correspondence
        return procrustes_by_correspondence(self.matches, frameA, frameB)

    def procrustes_by_correspondence_device(self, frameA, frameB):
        """The same from the pair's device records (window.procrustes_pairs: fp64 moments and rotation, rounded once): returns
        (4x4 float32, err).  Identity for a pair without records, as on the host."""
        from .window import procrustes_pairs
        first, count = self.device_segments.get((frameA.id, frameB.id), (0, 0))
        if self._pool is None or count == 0:
            return np.eye(4, dtype=np.float32), 0.0
        pose, err, _ = procrustes_pairs(self.ws, self._pool, [(first, count)], np.asarray(frameA.pose_in_model, np.float32)[None],
                                        np.asarray(frameB.pose_in_model, np.float32)[None])
        return pose[0].copy(), float(err[0])

    def close(self) -> None:
        self.memory.close()
