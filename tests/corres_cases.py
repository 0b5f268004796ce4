"""Built inputs that steer btba_corres_chain and btba_mappoints_* down chosen paths, and the model run of them (plain numpy).

Everything goes through the public calls, so a match list is made by the inputs: one fronto-parallel plane (depth 0.5 m, normals
(0, 0, -1), identity poses) in a 64 x 96 image, the gate wide open (max_dist 1e4, cos_max -1: every candidate with depth passes),
and descriptors that are exact copies: A's descriptor i is B's descriptor t(i), so its nearest neighbour has d2 == +0 and, where
B repeats a descriptor, the lowest index.  The map t is the case: a bijection, many onto one, one key reused across a chunk of 256.
A chain can take depth away from chosen keypoints' pixels (`blind`: no NN match there, a propagated point there is (0, 0, 0)) or
raise min_z above the plane (`min_z = 0.6`: no NN match at all, propagated points as usual), which is how propagation is reached.

RANSAC regimes.  "all": dist_thres 1e3, every match is an inlier, the list must be arange(n1).  "geo": default parameters; the
matches meant as inliers have both keypoints in the SAME pixel (A's keypoint is B's pixel plus a sub-pixel offset, so keys stay
distinct and roundf lands on B's pixel: identical camera points), the others are displaced by >= 5 pixels = 2.5 cm.

A Case is frames + steps (register / forget / Chain) + check(run): the floors its device test relies on, asserted on the MODEL's
path counts (corres_ref.CorresModel) -- conditions, not measurements.  ModelRun executes a case on tests/match_ref.restate and
the model alone; tests/test_gpu_corres_model.py runs the device next to it."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from bundletrack_amd import _lib
from corres_ref import CorresModel
from match_ref import HostFrame, restate

H, W = 64, 96
K = np.array([[100.0, 0.0, 48.0], [0.0, 100.0, 32.0], [0.0, 0.0, 1.0]], np.float32)     # 1 pixel = 5 mm on the plane
DEPTH = np.full((H, W), 0.5, np.float32)
NORMAL = np.zeros((H, W, 4), np.float32)
NORMAL[..., 2] = -1.0
POSE = np.eye(4, dtype=np.float32)
SUB = 1.0 / 64.0                       # sub-pixel step of same-pixel keypoints: offsets (a, b) * SUB, a, b in 0 .. 30
FAR = 31.0 * SUB                       # the offset of displaced keypoints: never a same-pixel key


@dataclass
class Chain:
    pairs: list                        # [(id of A, id of B)], A newer
    regime: str = "all"                # "all" | "geo"
    mutual: int = 0
    k: int = 5
    min_z: float = 0.1
    blind: dict = field(default_factory=dict)      # frame id -> keypoint indices whose pixel has no depth in this chain


@dataclass
class Case:
    name: str
    frames: dict                       # id -> HostFrame (frame ids are the model's frame keys; |idA - idB| == 1 = neighbours)
    steps: list                        # ("register", id) | ("forget", id) | Chain
    check: object                      # check(run) -> {count name: value}; asserts the floors


def match_prm(ch: Chain):
    return _lib.match_params(k=ch.k, mutual=ch.mutual, max_dist_neighbor=1e4, cos_max_normal_neighbor=-1.0, max_dist_no_neighbor=1e4,
                             cos_max_normal_no_neighbor=-1.0, min_z=ch.min_z)


def ransac_prm(ch: Chain):
    return _lib.corres_params(dist_thres=1e3) if ch.regime == "all" else _lib.corres_params()


def pixel_of(kp):
    """roundf of a keypoint of these cases (coordinates >= -0.0 with fractions below one half)."""
    return int(np.floor(float(kp[0]) + 0.5)), int(np.floor(float(kp[1]) + 0.5))


def chain_depth(ch: Chain, frame: HostFrame) -> np.ndarray:
    idx = ch.blind.get(frame.id)
    if idx is None:
        return DEPTH
    d = DEPTH.copy()
    for i in idx:
        x, y = pixel_of(frame.kpts[i])
        d[y, x] = 0.0
    return d


_plane = None


def plane_points() -> np.ndarray:
    """float32 [H, W, 3]: the matcher's camera point of every pixel of the plane, from the committed restatement itself (one
    keypoint per pixel matched against a single keypoint)."""
    global _plane
    if _plane is None:
        kp = np.array([[x, y] for y in range(H) for x in range(W)], np.float32)
        desc = np.zeros((H * W, 4), np.float32)
        desc[:, 0] = 1.0
        P, Q = HostFrame(1, POSE, kp, desc, DEPTH, NORMAL), HostFrame(0, POSE, kp[:1], desc[:1], DEPTH, NORMAL)
        recs = restate([Q, P], [(1, 0)], match_prm(Chain([], k=1)), K, H, W)[0][0]
        assert len(recs) == H * W and np.array_equal(recs["idx_a"], np.arange(H * W))
        _plane = recs["ptA_cam"].reshape(H, W, 3).copy()
    return _plane


def numpy_inliers(recs, ch: Chain):
    """The inlier list a case is built for, in fp64 from the records' points (identity poses): all of them, or the matches whose
    two points are within the default 1 cm -- the same-pixel consensus."""
    if ch.regime == "all":
        return list(range(len(recs)))
    d = np.linalg.norm(recs["ptA_cam"].astype(np.float64) - recs["ptB_cam"].astype(np.float64), axis=1)
    return [int(i) for i in np.nonzero(d <= 0.01)[0]]


class ModelRun:
    """A case on the restatements alone.  paths[c][p]: CorresModel's path counts of pair p of the c-th chain; results[c][p] =
    (records, stage counts); marks: (high-water mark, live map points) after every step."""

    def __init__(self, case: Case, inliers=numpy_inliers):
        self.case, self.R, self.status, self.inliers = case, CorresModel(), {}, inliers
        self.paths, self.results, self.marks, self.chains = [], [], [], []

    def run(self):
        for st in self.case.steps:
            self.step(st)
        return self

    def step(self, st):
        if isinstance(st, Chain):
            self.chain(st)
        elif st[0] == "register":
            self.register(st[1])
        else:
            self.forget(st[1])
        self.marks.append((self.R.high_water, len(self.R.img)))

    def register(self, fid):
        self.R.register(fid, self.case.frames[fid].kpts)

    def forget(self, fid):
        self.R.forget(fid)
        self.status.pop(fid, None)

    def chain_frames(self, ch: Chain):
        fids = sorted({f for p in ch.pairs for f in p})
        frames = []
        for f in fids:
            h = self.case.frames[f]
            frames.append(HostFrame(h.id, h.pose, h.kpts, h.desc, chain_depth(ch, h), h.normal))
        return fids, frames

    def point(self, frame: HostFrame, i: int):
        x, y = pixel_of(frame.kpts[i])
        return plane_points()[y, x] if frame.depth[y, x] >= 0.1 else np.zeros(3, np.float32)

    def chain(self, ch: Chain):
        fids, frames = self.chain_frames(ch)
        at = {f: i for i, f in enumerate(fids)}
        nns = restate(frames, [(at[a], at[b]) for a, b in ch.pairs], match_prm(ch), K, H, W)[0]
        first, out = len(self.R.paths), []
        for (a, b), nn in zip(ch.pairs, nns):
            out.append(self.R.find_corres(a, b, abs(a - b) == 1, nn, self.status, lambda recs: self.inliers(recs, ch),
                                          lambda f, i: self.point(frames[at[f]], i)))
        self.R.end_chain()
        self.paths.append(self.R.paths[first:])
        self.results.append(out)
        self.chains.append(ch)
        return out


# ---- construction helpers -----------------------------------------------------------------------------------------------------
def unit(rng, n, D=32):
    v = rng.normal(size=(n, D))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def pixels(rng, n, avoid=()):
    """n distinct keys: integer pixels in random order, then the same pixels shifted by a quarter pixel in u."""
    base = [(float(x), float(y)) for y in range(H) for x in range(W) if (x, y) not in avoid]
    assert n <= 2 * len(base)
    order = rng.permutation(len(base))
    keys = [base[i] for i in order] + [(base[i][0] + 0.25, base[i][1]) for i in order]
    return np.array(keys[:n], np.float32).reshape(n, 2)


def frame(fid, kpts, desc):
    kpts, desc = np.ascontiguousarray(kpts, np.float32).reshape(-1, 2), np.ascontiguousarray(desc, np.float32)
    return HostFrame(fid, POSE, kpts, desc.reshape(kpts.shape[0], -1) if kpts.shape[0] else desc.reshape(0, desc.shape[-1]), DEPTH, NORMAL)


def place(rng, kB, t, same, min_disp=5):
    """A's keypoints against B's kB: same[i] puts A's keypoint i into the pixel of B's keypoint t[i] (its own sub-pixel offset per
    target, so keys stay distinct); the others go to distinct pixels at least min_disp pixels (Chebyshev) from their target's."""
    n = len(t)
    out = np.zeros((n, 2), np.float32)
    rank, used = {}, set()
    for i in range(n):
        bx, by = pixel_of(kB[t[i]])
        if same[i]:
            r = rank.get(int(t[i]), 0)
            rank[int(t[i])] = r + 1
            assert r < 31 * 31
            out[i] = (bx + (r % 31) * SUB, by + (r // 31) * SUB)
        else:
            while True:
                x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
                if (x, y) not in used and max(abs(x - bx), abs(y - by)) >= min_disp:
                    break
            used.add((x, y))
            out[i] = (x + FAR, y + FAR)
    return out


def _only(run, c=-1, p=0):
    return run.paths[c][p]


def _counts(st):
    return {k: st[k] for k in ("n0", "n1", "n2", "chunks", "conflict", "par_stack", "par_mark", "ser_stack", "ser_mark", "skip", "join",
                               "prop", "prop_passes", "map_points")}


# ---- update: chunk edges --------------------------------------------------------------------------------------------------------
CHUNK_EDGES = [5, 6, 255, 256, 257, 512, 513]


def chunk_edges(n2: int, kind: str) -> Case:
    """n2 matches reach the update of one fresh pair: a bijection (every lane parallel) or every A key onto ONE B key (every lane
    after the first of its chunk a conflict lane).  n2 = 5 comes out of RANSAC: six matches, five in the same pixel."""
    rng = np.random.default_rng(1000 + n2)
    nA = max(n2, 6)
    nB = nA if kind == "bijection" else 8
    t = rng.permutation(nB)[:nA] if kind == "bijection" else np.full(nA, 3)
    kB, dB = pixels(rng, nB), unit(rng, nB)
    if n2 == 5:
        kA, regime = place(rng, kB, t, [True] * 5 + [False], min_disp=12), "geo"
    else:
        kA, regime = pixels(rng, nA), "all"
    frames = {0: frame(0, kB, dB), 2: frame(2, kA, dB[t])}

    def check(run):
        st = _only(run)
        chunks = -(-n2 // 256)
        assert (st["n1"], st["n2"], st["chunks"]) == (nA, n2, chunks), st
        assert st["inliers_arange"] == (regime == "all")
        if kind == "bijection":
            assert (st["conflict"], st["par_mark"], st["join"], st["skip"]) == (0, n2, 0, 0), st
        else:
            assert (st["conflict"], st["par_mark"], st["join"], st["skip"]) == (n2 - chunks, 1, n2 - 1, 0), st
            assert st["max_chunk_conflict"] == min(n2, 256) - 1
        assert st["map_points"] == (n2 if kind == "bijection" else 1)
        return _counts(st)
    return Case(f"chunk_edges[{n2}-{kind}]", frames, [("register", 0), ("register", 2), Chain([(2, 0)], regime)], check)


def cross_chunk() -> Case:
    """300 matches.  Match 256 (lane 0 of the second chunk) reuses the B key of match 0 with a fresh A key; match 257 reuses the A
    key of match 1 (a repeated (u, v)) with a fresh B key; match 258 has both keys fresh: parallel lanes that must see what the
    first chunk wrote."""
    rng = np.random.default_rng(11)
    n = 300
    t = rng.permutation(n)
    t[256] = t[0]
    kB, dB, kA = pixels(rng, n), unit(rng, n), pixels(rng, n)
    kA[257] = kA[1]
    frames = {0: frame(0, kB, dB), 2: frame(2, kA, dB[t])}

    def check(run):
        st = _only(run)
        assert (st["n2"], st["chunks"], st["conflict"]) == (300, 2, 0), st
        assert st["cross_b"] == 1 and st["cross_a"] == 1 and st["join"] == 1 and st["skip"] == 0
        assert st["map_points"] == 299 and st["par_mark"] == 299
        return _counts(st)
    return Case("cross_chunk", frames, [("register", 0), ("register", 2), Chain([(2, 0)])], check)


def many_to_one(mutual: int, regime: str) -> Case:
    """900 A keypoints, 40 of them repeating another's (u, v), onto 300 of B's 700; 90 % of them in their target's pixel."""
    rng = np.random.default_rng(12)
    nA, nB = 900, 700
    t = rng.choice(nB, 300, replace=False)[rng.integers(0, 300, nA)]
    kB, dB = pixels(rng, nB), unit(rng, nB)
    kA = place(rng, kB, t, rng.random(nA) < 0.9)
    pick = rng.permutation(nA)
    kA[pick[:40]] = kA[pick[40:80]]
    frames = {0: frame(0, kB, dB), 2: frame(2, kA, dB[t])}

    def check(run):
        st = _only(run)
        assert st["n0"] == (nA + nB if mutual else nA)
        nn = restate([frames[0], frames[2]], [(1, 0)], match_prm(Chain([], mutual=mutual)), K, H, W)[0][0]
        fwd = nn[nn["dir"] == 0]
        assert len(fwd) == nA and np.all(fwd["dist"] == 0.0) and np.array_equal(fwd["idx_b"], t)   # exact copies, found
        assert st["chunks"] >= 3 and st["conflict"] >= 200, st
        assert st["inliers_arange"] == (regime == "all")
        assert st["n2"] < st["n1"] if regime == "geo" else st["n2"] == st["n1"]
        return _counts(st)
    return Case(f"many_to_one[{'mutual' if mutual else 'one-way'}-{regime}]", frames,
                [("register", 0), ("register", 2), Chain([(2, 0)], regime, mutual)], check)


# ---- allocator --------------------------------------------------------------------------------------------------------------------
def _repeat_pair(rng, idB, idA, n_par, n_ser):
    """A pair whose one chunk creates n_par map points in parallel lanes and n_ser more in conflict lanes: A's keypoints
    n_par .. repeat the (u, v) of its first ones (an A key seen earlier in the chunk) and go to fresh B keys."""
    n = n_par + n_ser
    assert n <= 256 and n_par >= 1
    t = rng.permutation(n)
    kB, dB, kA = pixels(rng, n), unit(rng, n), pixels(rng, n)
    for i in range(n_par, n):
        kA[i] = kA[i % n_par]
    return {idB: frame(idB, kB, dB), idA: frame(idA, kA, dB[t])}


def allocator() -> Case:
    """F = 100 map points of two frames, both forgotten (100 ids on the stack, the mark stays).  Then one chunk that creates 150 in
    parallel lanes (100 off the stack, 50 off the mark) and 20 in conflict lanes (the serial allocator starts at an empty stack);
    both frames forgotten again (170 ids); then one chunk that creates 40 in parallel and 200 in conflict lanes: the serial
    allocator starts at 130 ids on the stack and crosses to the mark."""
    rng = np.random.default_rng(13)
    frames = {}
    frames.update(_repeat_pair(rng, 0, 2, 100, 0))
    frames.update(_repeat_pair(rng, 4, 6, 150, 20))
    frames.update(_repeat_pair(rng, 8, 10, 40, 200))
    steps = [("register", 0), ("register", 2), Chain([(2, 0)]), ("forget", 0), ("forget", 2),
             ("register", 4), ("register", 6), Chain([(6, 4)]), ("forget", 4), ("forget", 6),
             ("register", 8), ("register", 10), Chain([(10, 8)])]

    def check(run):
        a, b, c = (run.paths[i][0] for i in range(3))
        assert (a["par_mark"], a["par_stack"], a["conflict"]) == (100, 0, 0)
        assert (b["chunks"], b["par_stack"], b["par_mark"], b["conflict"], b["ser_stack"], b["ser_mark"]) == (1, 100, 50, 20, 0, 20), b
        assert (c["chunks"], c["par_stack"], c["par_mark"], c["conflict"], c["ser_stack"], c["ser_mark"]) == (1, 40, 0, 200, 130, 70), c
        assert [m for m in run.marks] == [(0, 0), (0, 0), (100, 100), (100, 100), (100, 0), (100, 0), (100, 0), (170, 170), (170, 170), (170, 0),
                                          (170, 0), (170, 0), (240, 240)], run.marks
        return {"chain 2": _counts(b), "chain 3": _counts(c)}
    return Case("allocator", frames, steps, check)


# ---- slots ------------------------------------------------------------------------------------------------------------------------
def slots() -> Case:
    """40 frames of 8 keypoints, each chained to its predecessor: 8 tracks that live through the 16 -> 32 and 32 -> 64 re-strides
    of img.  Then every third frame is forgotten and 14 new frames take the freed slots, lowest first; each is matched to frame 38
    and then reaches frame 37 along the tracks alone (min_z above the plane: no NN match)."""
    rng = np.random.default_rng(14)
    d0 = unit(rng, 8)
    frames, steps = {}, []
    for f in range(54):
        frames[f] = frame(f, pixels(rng, 8), d0[rng.permutation(8)])
    steps.append(("register", 0))
    for f in range(1, 40):
        steps += [("register", f), Chain([(f, f - 1)])]
    steps += [("forget", f) for f in range(0, 40, 3)]
    for f in range(40, 54):
        steps += [("register", f), Chain([(f, 38)]), Chain([(f, 37)], min_z=0.6)]

    def check(run):
        assert all(p["n2"] == 8 for c in run.paths for p in c)
        assert run.marks[-1] == (8, 8)
        prop = [c[0]["prop"] for c, ch in zip(run.paths, run.chains) if ch.min_z > 0.5]
        assert prop == [8] * 14
        assert all(len(t) == 40 - 14 + 14 for t in run.R.tracks())
        return {"frames": 54, "tracks": 8, "propagated": sum(prop), "high_water": run.R.high_water}
    return Case("slots", frames, steps, check)


# ---- registration -----------------------------------------------------------------------------------------------------------------
REGISTRATIONS = [(0, "dups"), (1, "dups"), (255, "dups"), (256, "dups"), (257, "dups"), (8192, "dups"), (257, "equal"), (257, "descending"),
                 (8192, "descending")]


def registration_keypoints(rng, n, variant):
    if variant == "equal":
        return np.tile(np.float32([7.0, 9.0]), (n, 1))
    kp = pixels(rng, n, avoid={(0, 5)})
    if variant == "descending":
        return kp[np.lexsort((kp[:, 1], kp[:, 0]))[::-1]].copy()
    for j in (255, 256, n - 1):                    # one (u, v) at 3, 255, 256 and n - 1: across the 256-wide tiles of k_mp_canon / k_mp_order
        if 3 < j < n:
            kp[j] = kp[3]
    if n >= 3:
        kp[1], kp[2] = (-0.0, 5.0), (0.0, 5.0)     # fp32 ==: one key
    return kp


def registration(n: int, variant: str) -> Case:
    """Frame 2 is the frame under test.  (1, 0) and (2, 1) are neighbour pairs that put its keys on tracks; (2, 0) then runs with
    min_z above the plane, so its records are the propagated matches alone: one per tracked key of frame 2, in walk order.
    At 8192 keypoints frame 0 has 64: every key of frame 2 is a candidate and 128 candidates contend for each key of frame 0 (the
    lowest walk rank wins), which also keeps the model's quadratic walk short."""
    rng = np.random.default_rng(2000 + n + len(variant))
    D = 4 if n > 1024 else 32
    m = max(n, 6)
    m0 = m if n <= 1024 else 64
    d0 = unit(rng, m, D)
    t = rng.permutation(m)[:n]
    kz = registration_keypoints(rng, n, variant)
    frames = {0: frame(0, pixels(rng, m0), d0[:m0]), 1: frame(1, pixels(rng, m), d0[rng.permutation(m)]),
              2: frame(2, kz, d0[t] if n else np.zeros((0, D), np.float32))}
    steps = [("register", 0), ("register", 1), ("register", 2), Chain([(1, 0)]), Chain([(2, 1)]), Chain([(2, 0)], min_z=0.6)]

    def check(run):
        R = run.R
        keys = len(R.canon[2])
        if variant == "equal":
            assert keys == min(n, 1)
        elif variant == "descending":
            assert keys == n and R.canon[2][R.uv(2, n - 1)] == n - 1
        else:
            assert keys == n - sum(1 for j in {255, 256, n - 1} if 3 < j < n) - (1 if n >= 3 else 0)
            if n >= 3:
                assert R.key_index(2, R.uv(2, 2)) == 1
            if n > 3:
                assert R.key_index(2, R.uv(2, n - 1)) == 3
        link, walk = run.paths[1][0], run.paths[2][0]
        assert link["n0"] == n and walk["n0"] == 0
        tracked = len(R.maps[2])
        assert tracked == (keys if n >= 6 else 0)
        assert walk["cand"] == tracked
        recs = run.results[2][0][0]
        if n <= 1024:
            assert walk["prop"] == tracked and walk["prop_passes"] == (-(-keys // 256) if tracked > 5 else 0), walk
        else:
            assert (walk["prop"], walk["excl_walk"]) == (m0, tracked - m0) and sorted(recs["idx_b"].tolist()) == list(range(m0)), walk
        if tracked > 5:                                            # the records' order is the walk order: (u, v) ascending
            uv = [R.uv(2, i) for i in recs["idx_a"]]
            assert uv == sorted(uv) and len(recs) == walk["prop"]
        if n == 8192 and variant == "descending":                  # key 8191: the last bit of bitA / bitB, the last LDS table entry
            assert link["max_ka"] == 8191 and link["max_kb"] == 8191
        return {"keys": keys, "tracked": tracked, **{k: walk[k] for k in ("cand", "prop", "prop_passes", "excl_walk")},
                **{"link_" + k: link[k] for k in ("n2", "chunks", "conflict", "skip")}}
    return Case(f"registration[{n}-{variant}]", frames, steps, check)


# ---- propagation ------------------------------------------------------------------------------------------------------------------
def prop_lower_rank_wins() -> Case:
    """Frame 2's keypoint 10 repeats keypoint 0's (u, v): in (2, 0) that one key opens two map points, with frame 0's keys 0 and
    10.  Frame 4 joins both (its keys 0 and 10); in (4, 2) both candidates lead to the same key of frame 2, and frame 4's key 10
    lies at (0, 0), first in the walk: it wins although its index is the higher."""
    rng = np.random.default_rng(15)
    d = unit(rng, 11)
    kx = pixels(rng, 11)
    kx[10] = kx[0]
    kz = pixels(rng, 11, avoid={(0, 0)})
    kz[10] = (0.0, 0.0)
    frames = {0: frame(0, pixels(rng, 11), d), 2: frame(2, kx, d), 4: frame(4, kz, d)}
    steps = [("register", 0), ("register", 2), ("register", 4), Chain([(2, 0)]), Chain([(4, 0)]), Chain([(4, 2)], min_z=0.6)]

    def check(run):
        st, recs = _only(run), run.results[-1][0][0]
        assert (st["n0"], st["cand"], st["excl_walk"], st["prop"]) == (0, 11, 1, 10), st
        assert (int(recs[0]["idx_a"]), int(recs[0]["idx_b"])) == (10, 0) and 0 not in recs["idx_a"].tolist()
        assert run.paths[1][0]["map_a_keys"] == 0 and run.paths[1][0]["cand"] == 0          # a non-neighbour pair with map_A empty
        return {k: st[k] for k in ("cand", "excl_walk", "prop")}
    return Case("prop_lower_rank_wins", frames, steps, check)


def prop_excluded_by_a_key() -> Case:
    """Frame 0 repeats descriptor 3 at index 12.  In (3, 0) the pixel of its keypoint 3 has no depth, so frame 3's keypoint 3 takes
    index 12 (k = 5 walks down the equal distances); the track's candidate (3 -> key 3 of frame 0) is dropped for its A key alone."""
    rng = np.random.default_rng(16)
    d = unit(rng, 12)
    frames = {0: frame(0, pixels(rng, 13), np.concatenate([d, d[3:4]])), 1: frame(1, pixels(rng, 12), d), 3: frame(3, pixels(rng, 12), d)}
    steps = [("register", 0), ("register", 1), ("register", 3), Chain([(1, 0)]), Chain([(3, 1)]), Chain([(3, 0)], blind={0: [3]})]

    def check(run):
        st, recs = _only(run), run.results[-1][0][0]
        assert run.results[0][0][0]["idx_b"].tolist() == list(range(12))                    # equal distances: the lower index
        assert (st["n0"], st["cand"], st["excl_a_only"], st["excl_b_only"], st["prop"]) == (12, 12, 1, 0, 0), st
        assert int(recs[3]["idx_b"]) == 12
        return {k: st[k] for k in ("cand", "excl_a_only", "excl_both", "prop")}
    return Case("prop_excluded_by_a_key", frames, steps, check)


def prop_excluded_by_b_key() -> Case:
    """Frame 3's keypoints 2 and 12 both join the track of key 2 (descriptor e next to d2, and d2 itself).  In (3, 0), k = 1, the
    exact copy of e in frame 0 has no depth: keypoint 2 gets no NN match, and its candidate is dropped for the B key that
    keypoint 12's NN match holds."""
    rng = np.random.default_rng(17)
    d = unit(rng, 12)
    e = d[2].astype(np.float64) + 0.05 * rng.normal(size=32)
    e = (e / np.linalg.norm(e)).astype(np.float32)[None]
    dz = np.concatenate([d, d[2:3]])
    dz[2] = e[0]
    frames = {0: frame(0, pixels(rng, 13), np.concatenate([d, e])), 1: frame(1, pixels(rng, 12), d), 3: frame(3, pixels(rng, 13), dz)}
    steps = [("register", 0), ("register", 1), ("register", 3), Chain([(1, 0)], k=1), Chain([(3, 1)], k=1), Chain([(3, 0)], k=1, blind={0: [12]})]

    def check(run):
        st = _only(run)
        link = run.results[1][0][0]
        assert int(link[2]["idx_b"]) == 2 and int(link[12]["idx_b"]) == 2
        assert (st["n0"], st["cand"], st["excl_a_only"], st["excl_b_only"], st["prop"]) == (12, 13, 0, 1, 0), st
        return {k: st[k] for k in ("cand", "excl_b_only", "excl_both", "prop")}
    return Case("prop_excluded_by_b_key", frames, steps, check)


def prop_passes(n=600) -> Case:
    """600 tracked keys reach a pair with no NN match: 600 propagated records in three compaction passes of 256."""
    rng = np.random.default_rng(18)
    d = unit(rng, n)
    frames = {f: frame(f, pixels(rng, n), d[rng.permutation(n)]) for f in (0, 1, 2)}
    steps = [("register", 0), ("register", 1), ("register", 2), Chain([(1, 0)]), Chain([(2, 1)]), Chain([(2, 0)], min_z=0.6)]

    def check(run):
        st = _only(run)
        assert (st["n0"], st["prop"], st["prop_passes"], st["n2"], st["chunks"], st["skip"]) == (0, n, 3, n, 3, n), st
        return _counts(st)
    return Case("prop_passes", frames, steps, check)


def prop_count(n_prop: int) -> Case:
    """Three NN matches (frame 0 has depth at its first three keypoints only, k = 1) and three propagated ones: n1 = 6, RANSAC runs.
    With frame 3's keypoint 5 on keypoint 4's track, two candidates share a B key and one drops: n1 = 5, the list is cleared
    without RANSAC and the non-neighbour A is not marked FAIL."""
    rng = np.random.default_rng(19)
    d = unit(rng, 6)
    dz = d.copy()
    if n_prop == 2:
        dz[5] = d[4]
    frames = {0: frame(0, pixels(rng, 6), d), 1: frame(1, pixels(rng, 6), d), 3: frame(3, pixels(rng, 6), dz)}
    steps = [("register", 0), ("register", 1), ("register", 3), Chain([(1, 0)], k=1), Chain([(3, 1)], k=1), Chain([(3, 0)], k=1, blind={0: [3, 4, 5]})]

    def check(run):
        st, stages = _only(run), run.results[-1][0][1]
        assert stages == ([3, 6, 6, 6] if n_prop == 3 else [3, 5, 0, 0]), stages
        assert st["ransac_ran"] == (n_prop == 3) and not run.status.get(3, False)
        assert run.paths[1][0]["map_a_keys"] == 0
        return {"stages": stages, "excl_walk": st["excl_walk"]}
    return Case(f"prop_count[{n_prop}]", frames, steps, check)


# ---- matcher ties -----------------------------------------------------------------------------------------------------------------
def tie_frames():
    """Two frames of 200 descriptors each, 4 distinct vectors repeated: every distance occurs 50 times or more, in runs that cross
    the column quarters and the 64-column tiles of k_match_topk.  The pixels of B's first 7 keypoints have no depth, so the gate
    walks down the equal distances: with k = 5 or 8 the answer is the third or fourth copy, with k = 1 there is none."""
    rng = np.random.default_rng(20)
    v = unit(rng, 4)
    a = frame(1, pixels(rng, 200), v[rng.integers(0, 4, 200)])
    b = frame(0, pixels(rng, 200), v[np.arange(200) % 4])
    ch = Chain([], blind={0: list(range(7))})
    b = HostFrame(b.id, b.pose, b.kpts, b.desc, chain_depth(ch, b), b.normal)
    return [b, a]


# ---- a seeded random session ------------------------------------------------------------------------------------------------------
def random_session(seed: int, n_frames=60, window=6) -> Case:
    """60 frames of 4 to 300 keypoints whose descriptors are drawn, with repeats, from one pool of 400: exact copies across and
    inside frames.  A pool entry has a home pixel; 70 % of its keypoints sit in it.  A sliding window of 6 live frames; chains of 1
    to 5 pairs to live older frames; the regime, mutual matching and an NN-silent pass (min_z above the plane) chosen per chain."""
    rng = np.random.default_rng(seed)
    pool, home = unit(rng, 400), pixels(rng, 400)
    frames, steps, live = {}, [], []
    for f in range(n_frames):
        n = 300 if f == 7 else 4 if f == 9 else int(4 * 75.0 ** rng.random())
        g = rng.integers(0, 400, n)
        kp = place(rng, home, g, rng.random(n) < 0.7)
        dup = rng.permutation(n)[:2 * int(rng.integers(0, max(n // 8, 1) + 1))]
        kp[dup[:len(dup) // 2]] = kp[dup[len(dup) // 2:]]
        frames[f] = frame(f, kp, pool[g])
        steps.append(("register", f))
        if live:
            others = [int(o) for o in rng.permutation(live)[:int(rng.integers(1, 6))]]
            if rng.random() < 0.7 and (f - 1) in live and (f - 1) not in others:
                others[0] = f - 1
            regime = "geo" if rng.random() < 0.5 else "all"
            steps.append(Chain([(f, o) for o in others], regime, mutual=int(rng.random() < 0.5)))
            rest = [o for o in live if o not in others and o != f - 1]
            if rest:
                steps.append(Chain([(f, o) for o in rest], regime, min_z=0.6))
        live.append(f)
        while len(live) > window:
            steps.append(("forget", live.pop(0 if rng.random() < 0.7 else int(rng.integers(0, len(live) - 1)))))

    def check(run):
        tot = {k: sum(p[k] for c in run.paths for p in c) for k in ("n2", "chunks", "conflict", "par_stack", "par_mark", "ser_stack", "ser_mark",
                                                                  "skip", "join", "prop", "excl_walk", "excl_a_only", "excl_b_only")}
        tot["pairs"] = sum(len(c) for c in run.paths)
        tot["failed_frames"] = sum(1 for v in run.status.values() if v)
        tot["high_water"] = run.R.high_water
        assert tot["prop"] >= 50 and tot["conflict"] > 100 and tot["par_stack"] > 100 and tot["ser_stack"] > 0 and tot["par_mark"] > 0, tot
        assert any(p["chunks"] >= 2 for c in run.paths for p in c)
        assert {ch.regime for ch in run.chains} == {"all", "geo"}
        return tot
    return Case(f"random_session[{seed}]", frames, steps, check)
