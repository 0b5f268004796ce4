"""Plain-Python restatement of the tracker's findCorres with map points (include/btba.h, "map points and the tracker's
findCorres"; src/FeatureManager.cpp:142-240, 448-521, 561-741), built from dicts the way the reference holds them:
map_F = {(u, v): map point}, map point = {frame: (u, v)}.  NN matches come in as records (tests/match_ref.py restates them),
RANSAC inlier lists through a callback, camera points of propagated matches through a callback."""
from __future__ import annotations

import numpy as np

from bundletrack_amd._lib import MATCH_DTYPE


class CorresRef:
    def __init__(self):
        self.kpts: dict = {}          # frame -> float32 [n, 2]
        self.canon: dict = {}         # frame -> {(u, v): lowest keypoint index with that (u, v)}
        self.maps: dict = {}          # frame -> {(u, v): map point id}
        self.img: dict = {}           # map point id -> {frame: (u, v)}
        self._next = 0

    # -- memory ---------------------------------------------------------------------------------------------------------------
    def register(self, frame, kpts) -> None:
        k = np.asarray(kpts, np.float32).reshape(-1, 2)
        if not np.isfinite(k).all():
            raise ValueError("non-finite keypoint")
        c = {}
        for i, (u, v) in enumerate(k.tolist()):
            c.setdefault((u, v), i)          # float keys: -0.0 == 0.0 and they hash alike
        self.kpts[frame], self.canon[frame], self.maps[frame] = k, c, {}

    def forget(self, frame) -> None:
        """SiftManager::forgetFrame (:142-170): img[frame] leaves every map point; empty map points are unreachable and dropped."""
        for mp in list(self.img):
            self.img[mp].pop(frame, None)
            if not self.img[mp]:
                del self.img[mp]
        for d in (self.kpts, self.canon, self.maps):
            d.pop(frame, None)

    def uv(self, frame, i):
        u, v = self.kpts[frame][i].tolist()
        return (u, v)

    def key_index(self, frame, uv) -> int:
        return self.canon[frame][uv]

    def tracks(self) -> set:
        """Map points as a set of frozensets of (frame, canonical keypoint index): the state up to renaming of the ids."""
        return {frozenset((f, self.key_index(f, uv)) for f, uv in d.items()) for d in self.img.values()}

    # -- findCorres -----------------------------------------------------------------------------------------------------------
    def find_corres(self, A, B, neighbor: bool, nn, status: dict, ransac, point):
        """One pair, A newer.  nn: MATCH_DTYPE records of btba_match_pairs for (A, B); status: {frame: FAIL bool}, updated;
        ransac(records) -> ascending inlier indices; point(frame, canonical index) -> float32 [3] camera point.
        Returns (MATCH_DTYPE records, [n after NN, after propagation, after RANSAC, final])."""
        recs = [r for r in np.asarray(nn, MATCH_DTYPE)]
        nA, nB = len(self.kpts[A]), len(self.kpts[B])
        n0 = len(recs) if (nA and nB) else 0
        recs = recs[:n0]
        if nA and nB and neighbor and n0 < 5:                                   # step 1
            status[A] = True
        if status.get(A, False):                                                # step 2
            return _pack(recs), [n0, n0, n0, n0]
        if not neighbor:                                                        # step 3, findCorresByMapPoints
            for uvA in sorted(self.maps[A]):
                mp = self.maps[A][uvA]
                if B not in self.img[mp]:
                    continue
                uvB = self.img[mp][B]
                if any(self.uv(A, r["idx_a"]) == uvA or self.uv(B, r["idx_b"]) == uvB for r in recs):
                    continue
                ia, ib = self.key_index(A, uvA), self.key_index(B, uvB)
                r = np.zeros((), MATCH_DTYPE)
                r["idx_a"], r["idx_b"], r["dist"], r["dir"] = ia, ib, -1.0, 2
                r["ptA_cam"], r["ptB_cam"] = point(A, ia), point(B, ib)
                recs.append(r)
        n1 = len(recs)
        if n1 <= 5:                                                             # step 4, runRansacBetween
            recs = []
        else:
            ids = list(ransac(_pack(recs)))
            assert ids == sorted(ids)
            recs = [recs[i] for i in ids]
            if len(recs) < 5:
                recs = []
        n2 = len(recs)
        for r in recs:                                                          # step 6, updateFramePairMapPoints
            uvA, uvB = self.uv(A, r["idx_a"]), self.uv(B, r["idx_b"])
            if uvA in self.maps[A] and uvB in self.maps[B]:
                continue
            if uvB not in self.maps[B]:
                mp = self._next
                self._next += 1
                self.img[mp] = {B: uvB}
                self.maps[B][uvB] = mp
            else:
                mp = self.maps[B][uvB]
            self.img[mp][A] = uvA
            self.maps[A][uvA] = mp
        if len(recs) < 5:                                                       # step 7
            recs = []
            if neighbor:
                status[A] = True
        return _pack(recs), [n0, n1, n2, len(recs)]


def _pack(recs) -> np.ndarray:
    out = np.zeros(len(recs), MATCH_DTYPE)
    for i, r in enumerate(recs):
        out[i] = r
    return out


def model_points(recs, poseA, poseB):
    """float32 (x, y, z, 1) model-frame points of records the way the matcher computes them: uncontracted, in the written order."""
    def tf(p, T):
        T = np.asarray(T, np.float32)
        p = np.asarray(p, np.float32).reshape(-1, 3)
        rows = [((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)]
        return np.stack(rows + [np.ones(len(p), np.float32)], 1).astype(np.float32)
    return tf(recs["ptA_cam"], poseA), tf(recs["ptB_cam"], poseB)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, MATCH_DTYPE), np.ascontiguousarray(b, MATCH_DTYPE)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def export_tracks(exp: dict, slot_frame: dict) -> set:
    """MapPointMemory.export() -> the same track-set form as CorresRef.tracks(); slot_frame: slot -> frame key."""
    out = set()
    for row in exp["img"]:
        t = frozenset((slot_frame[s], int(k)) for s, k in enumerate(row) if k >= 0)
        if t:
            out.add(t)
    return out
