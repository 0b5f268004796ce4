"""Plain-Python restatement of the tracker's findCorres with map points (include/btba.h, "map points and the tracker's
findCorres"; src/FeatureManager.cpp:142-240, 448-521, 561-741), built from dicts the way the reference holds them:
map_F = {(u, v): map point}, map point = {frame: (u, v)}.  NN matches come in as records (tests/match_ref.py restates them),
RANSAC inlier lists through a callback, camera points of propagated matches through a callback.
CorresModel adds the allocator's high-water mark and per-pair path counts next to it; assert_state compares a whole export()."""
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


# ---- the model with its allocator's observable and the paths a device update takes ------------------------------------------
class CorresModel(CorresRef):
    """CorresRef (behaviour unchanged) plus what the device memory adds to the sequential rule: the high-water mark of the id
    allocator, and per pair the paths k_corres_prop / k_corres_update take on that pair's lists (chunks of 256 matches, conflict
    lanes, free-stack against high-water allocation, compaction passes) -- counted from the model's state, never from the device."""
    CHUNK = 256

    def __init__(self):
        super().__init__()
        self.high_water = 0           # ids only come off the free stack until it is empty: max over time of the live map points
        self.paths: list = []         # one dict per find_corres call

    def end_chain(self) -> None:
        self.high_water = max(self.high_water, len(self.img))

    def forget(self, frame) -> None:
        self.end_chain()
        super().forget(frame)

    def find_corres(self, A, B, neighbor, nn, status, ransac, point):
        st = dict(A=A, B=B, n2=0, chunks=0, conflict=0, max_chunk_conflict=0, par_stack=0, par_mark=0, ser_stack=0, ser_mark=0,
                  skip=0, join=0, cross_a=0, cross_b=0, max_ka=-1, max_kb=-1, prop=0, prop_passes=0, ransac_ran=False, inliers_arange=None,
                  map_a_keys=len(self.maps[A]), cand=0, excl_a_only=0, excl_b_only=0, excl_both=0, excl_walk=0)
        walked = not neighbor and len(self.kpts[A]) and len(self.kpts[B]) and not status.get(A, False)
        if walked:                                            # the walk's candidates against the NN matches' key sets
            nnA, nnB = {self.uv(A, r["idx_a"]) for r in nn}, {self.uv(B, r["idx_b"]) for r in nn}
            for uvA, mp in self.maps[A].items():
                if B in self.img[mp]:
                    a, b = uvA in nnA, self.img[mp][B] in nnB
                    st["cand"] += 1
                    if a or b:
                        st["excl_both" if a and b else "excl_a_only" if a else "excl_b_only"] += 1

        def spy(recs):
            ids = list(ransac(recs))
            st["ransac_ran"], st["inliers_arange"] = True, ids == list(range(len(recs)))
            walk = {self.canon[A][uv]: r for r, uv in enumerate(sorted(self.canon[A]))}
            st["prop_passes"] = len({walk[int(r["idx_a"])] // self.CHUNK for r in recs if r["dir"] == 2})
            if len(ids) >= 5:
                self._update_paths(A, B, [recs[i] for i in ids], st)
            return ids
        out, stages = super().find_corres(A, B, neighbor, nn, status, spy, point)
        st["n0"], st["n1"], st["prop"] = stages[0], stages[1], stages[1] - stages[0]
        assert st["n2"] == stages[2] or not st["ransac_ran"]             # (a FAIL A repeats the NN count)
        if walked:                                            # candidates no NN match excludes, dropped for an earlier candidate's B key
            st["excl_walk"] = st["cand"] - st["excl_both"] - st["excl_a_only"] - st["excl_b_only"] - st["prop"]
        st["map_points"] = len(self.img)
        self.paths.append(st)
        return out, stages

    def _update_paths(self, A, B, recs, st) -> None:
        """Replay step 6 on key sets, chunk by chunk, the way the kernel splits it: a lane whose A key and B key are first in its
        chunk is parallel and decides from the chunk's starting state; the others are conflict lanes.  The free stack holds
        high_water - live ids when the update starts (no forget happens inside a chain, so the mark is settled at its end)."""
        inA, inB = set(self.maps[A]), set(self.maps[B])
        live = len(self.img)
        top = max(self.high_water, live) - live
        seenA, seenB = set(), set()                           # keys of earlier chunks of this update
        st["n2"], st["chunks"] = len(recs), -(-len(recs) // self.CHUNK)
        for c0 in range(0, len(recs), self.CHUNK):
            keys = [(self.uv(A, r["idx_a"]), self.uv(B, r["idx_b"])) for r in recs[c0:c0 + self.CHUNK]]
            st["max_ka"] = max([st["max_ka"]] + [self.canon[A][a] for a, _ in keys])
            st["max_kb"] = max([st["max_kb"]] + [self.canon[B][b] for _, b in keys])
            cA, cB, conf = set(), set(), []
            for a, b in keys:
                conf.append(a in cA or b in cB)
                cA.add(a)
                cB.add(b)
            st["conflict"] += sum(conf)
            st["max_chunk_conflict"] = max(st["max_chunk_conflict"], sum(conf))
            st["cross_a"] += sum(1 for a, _ in keys if a in seenA)
            st["cross_b"] += sum(1 for _, b in keys if b in seenB)
            for serial in (False, True):                      # all parallel lanes take their ids before the first conflict lane
                for (a, b), cf in zip(keys, conf):
                    if cf != serial:
                        continue
                    if a in inA and b in inB:
                        st["skip"] += 1
                        continue
                    if b not in inB:
                        st[("ser_" if serial else "par_") + ("stack" if top > 0 else "mark")] += 1
                        top = max(top - 1, 0)
                        inB.add(b)
                    else:
                        st["join"] += 1
                    inA.add(a)
            seenA |= cA
            seenB |= cB


def assert_state(R: CorresModel, exp: dict, slot_frame: dict) -> None:
    """The whole of MapPointMemory.export() against the model.  slot_frame: slot -> the model's frame key, for every live slot.
    canon per live slot; the multiset of non-empty img rows as track sets; map_F key by key as the track set it names
    ("unmapped" its own value), which needs no bijection of ids; every id of a map_F below the high-water mark and on a
    non-empty row; the high-water mark itself; the overflow flag clear."""
    from collections import Counter
    live = {s for s, n in enumerate(exp["slot_n"]) if n >= 0}
    assert live == set(slot_frame), (sorted(live), sorted(slot_frame))
    assert set(slot_frame.values()) == set(R.kpts)
    M = exp["img"].shape[0]
    assert exp["overflow"] == 0
    assert M == R.high_water, (M, R.high_water)

    def row_track(m):
        return frozenset((slot_frame[s], int(k)) for s, k in enumerate(exp["img"][m]) if k >= 0)
    for m in range(M):                                        # a row holds nothing in a dead slot
        assert all(s in live for s in (exp["img"][m] >= 0).nonzero()[0]), m
    rows = [row_track(m) for m in range(M)]
    assert Counter(t for t in rows if t) == Counter(frozenset((f, R.key_index(f, uv)) for f, uv in d.items()) for d in R.img.values())
    for s, f in slot_frame.items():
        n = len(R.kpts[f])
        assert int(exp["slot_n"][s]) == n, (f, s)
        want = np.array([R.key_index(f, R.uv(f, i)) for i in range(n)], np.int32)
        assert np.array_equal(exp["canon"][s], want), ("canon", f)
        for uv, k in R.canon[f].items():
            m = int(exp["map"][s][k])
            if uv in R.maps[f]:
                d = R.img[R.maps[f][uv]]
                assert 0 <= m < M and rows[m], ("map id", f, k, m)
                assert rows[m] == frozenset((g, R.key_index(g, w)) for g, w in d.items()), ("map track", f, k)
            else:
                assert m == -1, ("unmapped", f, k, m)
