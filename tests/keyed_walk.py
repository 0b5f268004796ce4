"""Random walks over the state btba_optimize_frames_keyed keeps in a workspace, and host models of that state.  numpy only.

include/btba.h promises that the keyed call gives the bits of btba_optimize_frames.  What decides which bytes its kernels read is a
state machine: an LRU pool of cached frames, a pool of correspondence segments with an index keyed by two frame keys, and solver
tables that other entry points rewrite.  This module generates seeded step sequences ("walks", plain JSON) that visit that state in
combination, replays them (Session: which keys, buffers, EntryJ array and poses a step hands to the library) and predicts what the
library may report for every call:

  FrameModel   bounds L <= cache_frames_built <= U that do not depend on which of several equally old slots is recycled first;
  CorrModel    corr_pairs_uploaded, with the pool's capacity unknown: a call that uploads every non-empty pair may have been a reset;
  PoolSim      the library's exact slot policy (pool_resolve in btba_api.hip), to check the bounds on the CPU;
  CorrPoolSim  the library's correspondence pool with a given capacity, to check CorrModel on the CPU.

tests/test_keyed_walk.py checks the generator and the models without a GPU; tests/test_gpu_keyed_walk.py runs the walks.
"""
from __future__ import annotations

import functools
import json

import numpy as np

from bundletrack_amd import synthetic as S

ENTRYJ = S.ENTRYJ_DTYPE
POOLS = ("G1", "G2")
SIZES = {"G1": (96, 128), "G2": (100, 128)}        # frame H x W: caches of 24 x 32 (per-block ranges in use) and 25 x 32 (not in use)
N_POS = 40                                        # orbit positions per pool
FULL, MASKED = 0, 1                               # variants: with the background sphere (every pixel valid), object only (a few percent)
LENGTHS = (0, 1, 37, 200, 680)                    # matches per frame pair, fixed per pair
LENGTH_P = (0.15, 0.15, 0.40, 0.20, 0.10)
LOWER, MORE_VALID, EXPLICIT, HIGHER = 0, 1, 2, 3  # BTBA_PAIRS_*
POLICIES = (LOWER, MORE_VALID, EXPLICIT, HIGHER)
CORR_MIN_BYTES_DEFAULT = 1 << 20                  # BTBA_OPT_KEYED_CORR_MIN_BYTES
FOREIGN = ("optimize", "solve_zn", "objective")
INVALID = 0xFFFFFFFF


def slots_for(n_frames: int) -> int:
    """include/btba.h: pool = max(32, 2 n_frames) slots."""
    return max(32, 2 * n_frames)


# ---------------------------------------------------------------------------------------------------------------------
# frames and matches: pure functions of (pool, position, variant), rendered once per process
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def intrinsics(pool: str) -> np.ndarray:
    H, W = SIZES[pool]
    K = S.NOCS_K.copy()
    K[0] *= W / 640.0
    K[1] *= H / 480.0
    return K


@functools.lru_cache(maxsize=None)
def poses_gt(pool: str) -> np.ndarray:
    rng = np.random.default_rng([4051, POOLS.index(pool)])
    steps = np.deg2rad(rng.uniform(5.0, 6.0, size=N_POS - 1))
    return np.stack([S.orbit_pose(a) for a in np.concatenate([[0.0], np.cumsum(steps)])])


@functools.lru_cache(maxsize=None)
def frame(pool: str, pos: int, var: int):
    """(depth [H,W] f32, normals [H,W,4] f32) the way make_problem renders them."""
    H, W = SIZES[pool]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d, n = S.render(poses_gt(pool)[pos], intrinsics(pool), xs, ys, var == FULL)
    d.setflags(write=False); n.setflags(write=False)
    return d, n


def cache_shape(pool: str, downscale: float):
    H, W = SIZES[pool]
    return int(H / downscale), int(W / downscale)


@functools.lru_cache(maxsize=None)
def cache_valid(pool: str, pos: int, var: int, downscale: float) -> int:
    """Pixels of the frame's cache that carry a depth (what the library counts into n_valid)."""
    H, W = SIZES[pool]
    Hd, Wd = cache_shape(pool, downscale)
    xi, yi = S.cache_source_pixels(H, W, Hd, Wd)
    d = frame(pool, pos, var)[0][yi][:, xi]
    return int((d >= np.float32(0.1)).sum())


def _fid(f):
    return [POOLS.index(f[0]), int(f[1]), int(f[2])]


@functools.lru_cache(maxsize=None)
def pair_matches(a, b, long: bool):
    """Matches of the unordered frame pair {a, b}, a < b: (points in a's camera frame, in b's), float32 [m, 3] each.  Surface points both
    views see + N(0, 1 mm), 5 % outliers displaced 2-5 cm, as make_problem draws them.  m is fixed per pair (long: 680 for every pair)."""
    assert a < b and a[0] == b[0]
    rng = np.random.default_rng([977] + _fid(a) + _fid(b))
    m = 680 if long else int(rng.choice(LENGTHS, p=LENGTH_P))
    T = poses_gt(a[0])
    Ta, Tb = T[a[1]], T[b[1]]
    pts = np.zeros((0, 3))
    for _ in range(4):
        if pts.shape[0] >= m:
            break
        cand, nrm = S._sample_surface(rng, 4096)
        vis = (((Ta[:3, 3] - cand) * nrm).sum(1) > 0.02) & (((Tb[:3, 3] - cand) * nrm).sum(1) > 0.02)
        pts = np.concatenate([pts, cand[vis]])
    if pts.shape[0] < m:                               # no common visible region: 3D-3D residuals do not need one
        pts = np.concatenate([pts, S._sample_surface(rng, m - pts.shape[0])[0]])
    pts = pts[:m]
    out = []
    for Tc in (Ta, Tb):
        inv = np.linalg.inv(Tc)
        out.append(pts @ inv[:3, :3].T + inv[:3, 3] + rng.normal(scale=0.001, size=(m, 3)))
    n_out = int(round(0.05 * m))
    if n_out:
        idx = rng.choice(m, n_out, replace=False)
        dirs = rng.normal(size=(n_out, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        out[1][idx] += dirs * rng.uniform(0.02, 0.05, size=(n_out, 1))
    return out[0].astype(np.float32), out[1].astype(np.float32)


def default_key(f) -> int:
    return 1000 * (POOLS.index(f[0]) + 1) + 2 * f[1] + f[2]


# ---------------------------------------------------------------------------------------------------------------------
# Session: what a step hands to the library
# ---------------------------------------------------------------------------------------------------------------------

class Call:
    """One optimise call, keyed or foreign: everything both sides of the comparison are given."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_frames(self):
        return len(self.frames)

    @property
    def n_pairs(self):
        return self.n_frames * (self.n_frames - 1) // 2

    def nonempty(self):
        return [(self.pair_keys[q], int(c)) for q, c in enumerate(self.nm) if c]


class Session:
    """Replays a walk's steps into concrete inputs.  Frames are (pool, position, variant); a frame's key is default_key until a "reuse"
    step hands it an evicted key; its device buffers are generation 0 until a "rebind" step clones them."""

    def __init__(self, seed: int, long: bool = False):
        self.seed, self.long = int(seed), bool(long)
        self.key_of, self.gen, self.next_key = {}, {}, 900000
        self.dropped, self.invalid = {}, {}           # per unordered pair: entries dropped so far, stride of its invalid entries

    def key(self, f):
        return self.key_of.get(f, default_key(f))

    def ident(self, f):
        """(key, device buffers): what the frame pool tells apart.  The buffers are the frame's, in their current generation."""
        return (self.key(f), f, self.gen.get(f, 0))

    def matches(self, a, b):
        """(pos_i, pos_j, invalid stride) of the pair as the window lists it: a first."""
        lo, hi = (a, b) if a < b else (b, a)
        pl, ph = pair_matches(lo, hi, self.long)
        for e in self.dropped.get((lo, hi), ()):
            pl, ph = np.delete(pl, e, 0), np.delete(ph, e, 0)
        return (pl, ph, self.invalid.get((lo, hi), 0)) if a < b else (ph, pl, self.invalid.get((lo, hi), 0))

    def pair_len(self, a, b):
        return self.matches(a, b)[0].shape[0]

    def window_corr(self, frames):
        """The window's EntryJ array, pair-major in the window's order, and its segment lengths.  pos_i belongs to the frame listed first."""
        blocks, nm = [], []
        for i in range(len(frames)):
            for j in range(i + 1, len(frames)):
                pi, pj, stride = self.matches(frames[i], frames[j])
                blk = np.zeros(pi.shape[0], ENTRYJ)
                blk["imgIdx_i"], blk["imgIdx_j"], blk["pos_i"], blk["pos_j"] = i, j, pi, pj
                if stride:
                    blk["imgIdx_i"][::stride] = INVALID
                blocks.append(blk)
                nm.append(pi.shape[0])
        return (np.concatenate(blocks) if blocks else np.zeros(0, ENTRYJ)), np.asarray(nm, np.int32)

    def poses_init(self, pool, frames, pose_seed):
        """Ground truth perturbed by U(+-2 deg, +-5 mm), the window's first frame exact (make_problem)."""
        rng = np.random.default_rng([self.seed, 31, int(pose_seed)])
        T = poses_gt(pool)
        out = np.stack([T[f[1]] for f in frames])
        for k in range(1, len(frames)):
            out[k] = out[k] @ S.se3_exp(np.deg2rad(rng.uniform(-2.0, 2.0, 3)), rng.uniform(-0.005, 0.005, 3))
        return out.astype(np.float32)

    def call(self, step) -> Call:
        pool = step["pool"]
        frames = [(pool, int(p), int(v)) for p, v in step["window"]]
        mut = step.get("mutation")
        if mut and mut["kind"] == "drop":
            a, b = [(pool, int(p), int(v)) for p, v in mut["pair"]]
            self.dropped.setdefault((min(a, b), max(a, b)), []).append(int(mut["entry"]))
        if mut and mut["kind"] == "invalidate":
            for pr in mut["pairs"]:
                a, b = [(pool, int(p), int(v)) for p, v in pr]
                self.invalid[(min(a, b), max(a, b))] = int(mut["stride"])
        corr, nm = self.window_corr(frames)
        if mut and mut["kind"] == "shuffle":
            corr = corr[np.random.default_rng([self.seed, 57, int(mut["seed"])]).permutation(len(corr))]
        keys = [self.key(f) for f in frames]
        H, W = SIZES[pool]
        return Call(pool=pool, frames=frames, keys=keys, idents=[self.ident(f) for f in frames], H=H, W=W, K=intrinsics(pool).astype(np.float32),
                    downscale=float(step.get("downscale", 4.0)), policy=int(step.get("policy", LOWER)),
                    pairs=None if step.get("pairs") is None else np.asarray(step["pairs"], np.int32).reshape(-1, 2),
                    keyed_corr=bool(step.get("keyed_corr", False)), corr=corr, nm=nm, shuffled=bool(mut and mut["kind"] == "shuffle"),
                    pair_keys=[(keys[i], keys[j]) for i in range(len(keys)) for j in range(i + 1, len(keys))],
                    poses=self.poses_init(pool, frames, step["pose_seed"]))

    def apply(self, step):
        """Non-call steps: returns what the executor has to do, as (verb, argument)."""
        kind = step["kind"]
        if kind == "evict":
            return ("evict", self.key(_frame(step["frame"])))
        if kind == "rebind":
            f = _frame(step["frame"])
            self.gen[f] = self.gen.get(f, 0) + 1
            return ("rebind", f)
        if kind == "reuse":                          # the key of `frm` is evicted and from now on names `to`; `frm` gets a key never used before
            frm, to = _frame(step["frm"]), _frame(step["to"])
            k = self.key(frm)
            self.key_of[to] = k
            self.key_of[frm] = self.next_key
            self.next_key += 1
            return ("evict", k)
        if kind == "clear":
            return ("clear", None)
        if kind == "threshold":
            return ("threshold", int(step["value"]))
        raise ValueError(kind)


def _frame(f):
    return (f[0], int(f[1]), int(f[2]))


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------

class FrameModel:
    """Bounds on cache_frames_built that hold for every least-recently-used policy, whatever its tie rule.

    L: frames that must be built -- never cached, or evicted / cleared / rebound / re-keyed since, or cached before the pool was
    re-allocated (regrowth, change of geometry).  U: L plus the frames LRU may have recycled.  A frame last used in call t is still
    resident at call u if the distinct frames used in calls t .. u number at most the slot count: its slot is only taken when every other
    slot is claimed by this call or was stamped in call t or later, and each of those holds another frame used in t .. u."""

    def __init__(self):
        self.slots, self.geom = 0, None
        self.used = []                # per keyed call since the last re-allocation: the set of idents
        self.last = {}                # ident -> index into self.used of its last use
        self.distinct = set()

    def call(self, geom, idents):
        n = len(idents)
        regrow = geom_change = False
        if geom != self.geom or self.slots < slots_for(n):
            geom_change = self.geom is not None and geom != self.geom
            regrow = self.geom is not None and not geom_change
            self.slots = max(self.slots, slots_for(n))
            self.geom = geom
            self.used, self.last, self.distinct = [], {}, set()
        must, maybe = [], []
        for idn in idents:
            t = self.last.get(idn)
            if t is None:
                must.append(idn)
                continue
            live = set(idents)
            for s in self.used[t:]:
                live |= s
            if len(live) > self.slots:
                maybe.append(idn)
        self.used.append(set(idents))
        for idn in idents:
            self.last[idn] = len(self.used) - 1
        self.distinct |= set(idents)
        return dict(L=len(must), U=len(must) + len(maybe), hits=n - len(must) - len(maybe), regrow=regrow, geom_change=geom_change,
                    pressure=len(self.distinct) > self.slots, slots=self.slots)

    def evict(self, key):
        for idn in [i for i in self.last if i[0] == key]:
            del self.last[idn]

    def clear(self):
        self.last.clear()


class PoolSim:
    """The library's slot policy, after pool_resolve / pool_commit: a hit needs key and buffers; a miss takes the first slot that is not
    live, else the not yet claimed slot with the oldest stamp (the lowest index among equals)."""

    def __init__(self):
        self.slots, self.geom, self.stamp = [], None, 0

    def call(self, geom, idents):
        n = len(idents)
        if geom != self.geom or len(self.slots) < slots_for(n):
            self.slots = [dict(live=False, ident=None, stamp=0) for _ in range(max(slots_for(n), len(self.slots)))]
            self.geom = geom
        slot_of, taken = [None] * n, set()
        for k, idn in enumerate(idents):
            for s, sl in enumerate(self.slots):
                if sl["live"] and sl["ident"] == idn:
                    slot_of[k] = s
                    taken.add(s)
                    break
        built = 0
        for k, idn in enumerate(idents):
            if slot_of[k] is not None:
                continue
            best = None
            for s, sl in enumerate(self.slots):
                if s in taken:
                    continue
                if not sl["live"]:
                    best = s
                    break
                if best is None or sl["stamp"] < self.slots[best]["stamp"]:
                    best = s
            slot_of[k] = best
            taken.add(best)
            self.slots[best].update(live=True, ident=idn)
            built += 1
        self.stamp += 1
        for s in slot_of:
            self.slots[s]["stamp"] = self.stamp
        return built

    def evict(self, key):
        for sl in self.slots:
            if sl["live"] and sl["ident"][0] == key:
                sl.update(live=False, ident=None, stamp=0)

    def clear(self):
        for sl in self.slots:
            sl.update(live=False, ident=None, stamp=0)


class CorrModel:
    """corr_pairs_uploaded of a call that uses the correspondence pool.  The index is the set of (ordered key pair, length) uploaded
    since the last clear, reset or shuffled-array fallback, minus every pair touching an evicted key; a call uploads its non-empty pairs
    that are not in it.  When the pool is full the library resets it and uploads every non-empty pair; the capacity is the allocator's
    business, so a call that reports that count may have been a reset.  Where the two readings differ only in what they leave in the
    index, both are kept as hypotheses until a later count tells them apart."""

    MAX_HYPOTHESES = 64

    def __init__(self):
        self.hyps = [dict(index={}, resets=0, appended=0)]

    @staticmethod
    def _fresh(index, pairs):
        return [(k, c) for k, c in pairs if index.get(k) != c]

    def expect(self, pairs):
        """(counts the hypotheses predict without a reset, the all-pairs count)."""
        return sorted({len(self._fresh(h["index"], pairs)) for h in self.hyps}), len(pairs)

    def observe(self, pairs, uploaded):
        """Keep the hypotheses that explain `uploaded`; False when none does."""
        out = []
        for h in self.hyps:
            fresh = self._fresh(h["index"], pairs)
            if uploaded == len(fresh):
                idx = dict(h["index"]); idx.update(fresh)
                out.append(dict(index=idx, resets=h["resets"], appended=h["appended"] + sum(c for _, c in fresh)))
            if uploaded == len(pairs) and h["index"] and (len(fresh) != len(pairs) or set(h["index"]) - {k for k, _ in pairs}):
                out.append(dict(index=dict(pairs), resets=h["resets"] + 1, appended=sum(c for _, c in pairs)))
        uniq = []                                   # one hypothesis per index: of two histories that end in the same state the one with fewer resets
        for h in sorted(out, key=lambda h: h["resets"]):
            if not any(h["index"] == u["index"] for u in uniq):
                uniq.append(h)
        if not uniq:
            return False
        assert len(uniq) <= self.MAX_HYPOTHESES, "the walk leaves too many readings open: revisit a cached window more often"
        self.hyps = uniq
        return True

    @property
    def resets(self):
        """Resets every surviving hypothesis agrees on."""
        return min(h["resets"] for h in self.hyps)

    @property
    def appended(self):
        return min(h["appended"] for h in self.hyps)

    def evict(self, key):
        for h in self.hyps:
            h["index"] = {k: c for k, c in h["index"].items() if key not in k}

    def drop_all(self):
        """btba_frame_cache_clear, or the fallback on an array that was not pair-major."""
        best = self.resets
        self.hyps = [dict(index={}, resets=best, appended=0)]


class CorrPoolSim:
    """The library's correspondence pool (upload_inputs / pack_fresh) with `slack` extra capacity from its allocator."""

    def __init__(self, headroom: float = 1.25):
        self.index, self.used, self.cap, self.headroom, self.resets = {}, 0, 0, headroom, 0

    def call(self, pairs, kept):
        for attempt in range(2):
            need = sum(c for k, c in pairs if self.index.get(k) != c)
            if self.used + need <= max(self.cap - 64, 0):
                break
            if self.index:
                self.resets += 1
            self.index, self.used = {}, 0
            want = max(16 * kept, 1 << 16) + 64
            if want > self.cap:
                self.cap = int(self.headroom * want)
        fresh = [(k, c) for k, c in pairs if self.index.get(k) != c]
        self.index.update(fresh)
        self.used += sum(c for _, c in fresh)
        return len(fresh)

    def evict(self, key):
        self.index = {k: c for k, c in self.index.items() if key not in k}

    def drop_all(self):
        self.index, self.used = {}, 0


# ---------------------------------------------------------------------------------------------------------------------
# Tracker: Session + models over a walk, step by step
# ---------------------------------------------------------------------------------------------------------------------

class Tracker:
    """Feeds a walk's steps to the Session and both models.  step() returns the executor's action; for a keyed call the action carries
    the Call and the frame bounds, and corr_observe() must be told what the library reported."""

    def __init__(self, walk):
        self.sess = Session(walk["seed"], walk.get("long", False))
        self.frames, self.corr = FrameModel(), CorrModel()
        self.threshold = CORR_MIN_BYTES_DEFAULT

    def step(self, step):
        kind = step["kind"]
        if kind == "call":
            c = self.sess.call(step)
            b = self.frames.call((c.pool, c.downscale), c.idents)
            c.uses_corr_pool = c.keyed_corr and len(c.corr) > 0 and len(c.corr) * ENTRYJ.itemsize >= self.threshold
            return ("call", c, b)
        if kind == "foreign":
            return ("foreign", self.sess.call(step), step["what"])
        verb, arg = self.sess.apply(step)
        if verb == "evict":
            self.frames.evict(arg); self.corr.evict(arg)
        elif verb == "clear":
            self.frames.clear(); self.corr.drop_all()
        elif verb == "threshold":
            self.threshold = arg
        return (verb, arg)

    def corr_observe(self, c: Call, uploaded: int):
        """None when `uploaded` is what the models allow, else a message."""
        if not c.uses_corr_pool:
            return None if uploaded == c.n_pairs else f"corr_pairs_uploaded {uploaded}, expected all {c.n_pairs} pairs (pool not in use)"
        if c.shuffled:                              # the packer flags the array, the pool is dropped and the host buckets everything
            self.corr.drop_all()
            return None if uploaded == c.n_pairs else f"corr_pairs_uploaded {uploaded}, expected all {c.n_pairs} pairs (fallback)"
        exp = self.corr.expect(c.nonempty())
        if not self.corr.observe(c.nonempty(), uploaded):
            return f"corr_pairs_uploaded {uploaded}, the model allows {exp[0]} or, after a reset, {exp[1]}"
        return None


def compaction_side(c: Call) -> bool:
    """True when the automatic choice walks valid-pixel lists: under 60 % of the window's cache pixels carry a depth."""
    Hd, Wd = cache_shape(c.pool, c.downscale)
    tot = sum(cache_valid(f[0], f[1], f[2], c.downscale) for f in c.frames)
    return tot * 10 < len(c.frames) * Hd * Wd * 6


def replay(walk, corr_headroom: float = 1.25):
    """The walk against the exact simulations: per keyed call a record with the bounds, the simulated counts and what coverage() counts."""
    tr, pool, cpool = Tracker(walk), PoolSim(), CorrPoolSim(corr_headroom)
    recs = []
    for i, step in enumerate(walk["steps"]):
        act = tr.step(step)
        if act[0] == "call":
            c, b = act[1], act[2]
            built = pool.call((c.pool, c.downscale), c.idents)
            if c.uses_corr_pool and c.shuffled:
                cpool.drop_all(); up = c.n_pairs
            elif c.uses_corr_pool:
                up = cpool.call(c.nonempty(), len(c.corr))
            else:
                up = c.n_pairs
            msg = tr.corr_observe(c, up)
            recs.append(dict(step=i, call=c, bounds=b, built=built, uploaded=up, corr_msg=msg, pool_resets=cpool.resets))
        elif act[0] == "evict":
            pool.evict(act[1]); cpool.evict(act[1])
        elif act[0] == "clear":
            pool.clear(); cpool.drop_all()
    return recs, tr


# ---------------------------------------------------------------------------------------------------------------------
# generator
# ---------------------------------------------------------------------------------------------------------------------

class Builder:
    """Builds a walk from segments.  Keeps a Tracker of its own so that choices can depend on the state (which pairs were presented,
    which are long enough to lose an entry, which frames were last used long ago)."""

    def __init__(self, name: str, seed: int, long: bool = False, mixed: bool = False):
        self.walk = dict(name=name, seed=int(seed), long=bool(long), steps=[])
        self.rng = np.random.default_rng([int(seed), 7])
        self.tr = Tracker(self.walk)
        self.mixed = mixed                            # combined walk: every call draws its policy and uses the correspondence pool
        self.pool = "G1"
        self.downscale = 4.0
        self.keyed_corr = False
        self.n_calls = 0
        self.cursor = {p: 0 for p in POOLS}
        self.prev = {p: [] for p in POOLS}            # last window per pool
        self.last_use = {}                            # frame -> call number
        self.presented = set()                        # unordered pairs handed to a keyed call so far

    # -- steps ------------------------------------------------------------------------------------------------------
    def _push(self, step):
        self.walk["steps"].append(step)
        return self.tr.step(step)

    def call(self, frames, policy=None, mutation=None, anchor=None):
        n = len(frames)
        if policy is None:
            policy = int(self.rng.choice(POLICIES)) if self.mixed else LOWER
        pairs = None
        if policy == EXPLICIT:
            pairs = [[i, j] if self.rng.random() < 0.5 else [j, i] for i in range(n) for j in range(i + 1, n) if self.rng.random() < 0.7] or [[0, 1]]
        step = dict(kind="call", pool=self.pool, window=[[f[1], f[2]] for f in frames], policy=policy, pairs=pairs, downscale=self.downscale,
                    keyed_corr=self.keyed_corr, mutation=mutation, pose_seed=self.n_calls)
        if anchor:
            step["anchor"] = anchor
        act = self._push(step)
        self.n_calls += 1
        for f in frames:
            self.last_use[f] = self.n_calls
        for i in range(n):
            for j in range(i + 1, n):
                self.presented.add((min(frames[i], frames[j]), max(frames[i], frames[j])))
        self.prev[self.pool] = list(frames)
        return act[1]

    def foreign(self, what, frames, explicit=False):
        n = len(frames)
        pairs = None
        if explicit:
            pairs = [[i, j] if self.rng.random() < 0.5 else [j, i] for i in range(n) for j in range(i + 1, n) if self.rng.random() < 0.7] or [[1, 0]]
        self._push(dict(kind="foreign", what=what, pool=self.pool, window=[[f[1], f[2]] for f in frames], pairs=pairs,
                        policy=EXPLICIT if pairs else LOWER, downscale=self.downscale, pose_seed=10000 + len(self.walk["steps"])))

    def threshold(self, value):
        self._push(dict(kind="threshold", value=int(value)))

    # -- windows ----------------------------------------------------------------------------------------------------
    def _var(self):
        return int(self.rng.integers(0, 2))

    def fresh_frame(self):
        p = self.cursor[self.pool]
        self.cursor[self.pool] = (p + 1) % N_POS
        return (self.pool, p, self._var())

    def slide(self, n):
        w = [f for f in self.prev[self.pool]][-(n - 1):] if n > 1 else []
        while len(w) < n:
            f = self.fresh_frame()
            if all(f[1] != g[1] for g in w):
                w.append(f)
        return w

    def all_new(self, n):
        return self.slide_from([], n)

    def slide_from(self, w, n):
        w = list(w)
        while len(w) < n:
            f = self.fresh_frame()
            if all(f[1] != g[1] for g in w):
                w.append(f)
        return w

    def loop(self, n, age=12):
        old = sorted(f for f, t in self.last_use.items() if f[0] == self.pool and self.n_calls - t >= age)
        self.rng.shuffle(old)
        w = []
        for f in old:
            if len(w) < n and all(f[1] != g[1] for g in w):
                w.append(f)
        return sorted(self.slide_from(w, n), key=lambda f: f[1])

    def permuted(self, reverse=False):
        w = list(self.prev[self.pool])
        if reverse or len(w) == 2:
            return w[::-1]
        return [w[k] for k in self.rng.permutation(len(w))]

    def window(self, n=None):
        n = int(self.rng.integers(2, 10)) if n is None else n
        r = self.rng.random()
        if r < 0.45 or not self.prev[self.pool]:
            return self.slide(n)
        if r < 0.70:
            return self.loop(n)
        if r < 0.85:
            return self.all_new(n)
        return self.permuted()

    # -- segments ---------------------------------------------------------------------------------------------------
    def seg_pool(self, n_calls=60, anchors=False):
        """Sliding, loop closures, pressure, and two regrowths (17 frames: 34 slots, 18 frames: 36)."""
        if anchors:
            self.call(self.all_new(2), policy=LOWER, anchor="size 2")
            self.call(self.slide(9), policy=LOWER, anchor="size 9")
        for k in range(n_calls):
            if k == n_calls // 3:
                self.call(self.slide(17), policy=LOWER if anchors else None, anchor="size 17" if anchors else None)
                self.call(self.slide(17))
            elif k == (2 * n_calls) // 3:
                self.call(self.slide(18))
            else:
                self.call(self.window())
        # pressure on purpose: run through more frames than slots, then close the loop on the most recent third
        for k in range(8):
            self.call(self.all_new(6))
        for k in range(10):
            self.call(self.loop(int(self.rng.integers(3, 8)), age=int(self.rng.integers(2, 7))))

    def seg_geometry(self, anchors=False):
        """G1 -> G2 -> G1 -> G2 -> G1, a downscale change and back, rebinds, evict-and-reuse, clear."""
        def some(n_calls):
            for _ in range(n_calls):
                self.call(self.window(int(self.rng.integers(2, 7))))
        self.pool = "G1"; some(4)
        self.pool = "G2"; self.call(self.all_new(5), policy=LOWER if anchors else None, anchor="geometry G2" if anchors else None); some(4)
        self.pool = "G1"; self.call(self.slide(4), policy=LOWER if anchors else None, anchor="geometry G1" if anchors else None); some(3)
        self.downscale = 2.0; some(3)
        self.downscale = 4.0; some(3)
        for _ in range(2):
            f = self.prev[self.pool][int(self.rng.integers(0, len(self.prev[self.pool])))]
            self._push(dict(kind="rebind", frame=list(f)))
            self.call(self.permuted() if self.rng.random() < 0.5 else list(self.prev[self.pool]))
            some(1)
        self.pool = "G2"; some(3)
        for _ in range(3):
            self.evict_and_reuse()
            some(1)
        self._push(dict(kind="clear"))
        some(2)
        self.pool = "G1"; some(3)

    def evict_and_reuse(self):
        """The key of a frame of the last window is evicted and given to a frame of another position; the next window holds the
        re-keyed frame where the evicted one stood."""
        w = list(self.prev[self.pool])
        k = int(self.rng.integers(0, len(w)))
        frm = w[k]
        to = self.fresh_frame()
        while any(to[1] == g[1] for g in w):
            to = self.fresh_frame()
        self._push(dict(kind="reuse", frm=list(frm), to=list(to)))
        w[k] = to
        self.call(w)

    def seg_policies(self, rounds=6, anchors=False):
        """Every pair policy on windows that mix the variants, on both sides of the 60 % rule; hits carry their stored valid counts."""
        k = 0
        for r in range(rounds):
            for policy in POLICIES:
                n = int(self.rng.integers(3, 8))
                n_full = n - 1 if (k % 2 == 0) else 1            # mostly full frames: above 60 %; one full frame: below
                base = self.slide(n) if self.rng.random() < 0.6 else self.loop(n, age=4)
                flip = set(self.rng.permutation(n)[:n_full].tolist())
                w = [(f[0], f[1], FULL if i in flip else MASKED) for i, f in enumerate(base)]
                a = "mixed variants" if anchors and policy == LOWER and r == 1 else None
                self.call(w, policy=policy, anchor=a)
                if self.rng.random() < 0.5:                      # the same frames again, all hits, in another order: stored counts decide
                    self.call(self.permuted(), policy=policy)
                k += 1

    def seg_corr(self):
        """The correspondence pool: cached calls, length changes, reversed pairs, calls under the threshold, the shuffled-array fallback."""
        self.keyed_corr = True
        self.threshold(0)
        for _ in range(10):
            self.call(self.window(int(self.rng.integers(2, 7))))
        for k in range(5):
            self.call(self.slide(int(self.rng.integers(3, 6))))
            self.call(self.permuted(reverse=True))
            self.drop_entry()
        for _ in range(2):
            self.threshold(CORR_MIN_BYTES_DEFAULT)
            self.call(self.slide(4))
            self.threshold(0)
            self.call(self.slide(4))
        self.invalidate_new()
        self.shuffled()
        for _ in range(4):
            self.call(self.window(int(self.rng.integers(2, 7))))
        self.evict_and_reuse()
        self.call(self.permuted())
        self.drop_entry()
        self.call(self.loop(5, age=6))

    def drop_entry(self):
        """A call on the last window in which one pair has lost an entry."""
        w = list(self.prev[self.pool])
        cands = [(a, b) for i, a in enumerate(w) for b in w[i + 1:] if self.tr.sess.pair_len(a, b) >= 2]
        if not cands:
            w = self.slide_from(w[-2:], 6)
            return self.call(w)
        a, b = cands[int(self.rng.integers(0, len(cands)))]
        e = int(self.rng.integers(0, self.tr.sess.pair_len(a, b)))
        return self.call(w, mutation=dict(kind="drop", pair=[[a[1], a[2]], [b[1], b[2]]], entry=e))

    def invalidate_new(self):
        """A window of pairs no call has presented yet; some of them carry invalid entries from now on."""
        w = self.unpresented(4)
        pairs = [[[a[1], a[2]], [b[1], b[2]]] for i, a in enumerate(w) for b in w[i + 1:] if self.rng.random() < 0.6 and self.tr.sess.pair_len(a, b) > 2]
        return self.call(w, mutation=dict(kind="invalidate", pairs=pairs, stride=int(self.rng.integers(3, 9))))

    def unpresented(self, n):
        for _ in range(200):
            w = self.all_new(n)
            if all((min(a, b), max(a, b)) not in self.presented for i, a in enumerate(w) for b in w[i + 1:]):
                return w
        raise RuntimeError("no window of new pairs left")

    def shuffled(self):
        """A window of new pairs whose array is shuffled: the fresh segments then hold entries of other pairs."""
        for _ in range(50):
            w = self.unpresented(4)
            corr, nm = self.tr.sess.window_corr(w)
            seed = int(self.rng.integers(0, 1 << 30))
            sh = corr[np.random.default_rng([self.walk["seed"], 57, seed]).permutation(len(corr))]
            if len(corr) and (sh["imgIdx_i"] != corr["imgIdx_i"]).any() | (sh["imgIdx_j"] != corr["imgIdx_j"]).any():
                return self.call(w, mutation=dict(kind="shuffle", seed=seed))
        raise RuntimeError("no shuffle moved an entry out of its segment")

    def seg_overflow(self, windows=35):
        """All-new windows of four frames with 680 matches per pair until the appended entries exceed twice the pool's floor."""
        self.keyed_corr = True
        self.threshold(0)
        first = {}
        for k in range(windows):
            self.pool = POOLS[k % 2]
            self.call(self.unpresented(4))
            first.setdefault(self.pool, list(self.prev[self.pool]))
            if k % 9 == 8:
                self.call(self.permuted(reverse=True))
                self.call(self.permuted(reverse=True))       # the window before last again: cached unless a reset fell in between
        for self.pool in POOLS:                              # the first windows again: cached only if the pool was never reset
            self.call(first[self.pool])

    def seg_foreign(self, rounds=6):
        """Keyed calls with the other entry points on the same workspace in between."""
        self.keyed_corr = True
        self.threshold(0)
        self.call(self.slide(5))
        for r in range(rounds):
            for what in (FOREIGN[(r + s) % 3] for s in range(3)):
                n_prev = len(self.prev[self.pool])
                n = [m for m in (3, 4, 6) if m != n_prev][int(self.rng.integers(0, 2))]
                self.foreign(what, self.loop(n, age=0) if self.rng.random() < 0.5 else self.all_new(n), explicit=(what == "solve_zn" or self.rng.random() < 0.3))
                pol = None if self.mixed else int(self.rng.choice(POLICIES))
                self.call(self.slide(n_prev) if self.rng.random() < 0.6 else self.window(), policy=pol)


def walk_frame_pool(seed=11):
    b = Builder("frame_pool", seed); b.seg_pool(anchors=True); return b.walk


def walk_geometry(seed=12):
    b = Builder("geometry", seed); b.seg_geometry(anchors=True); return b.walk


def walk_policies(seed=13):
    b = Builder("policies", seed); b.seg_policies(anchors=True); return b.walk


def walk_corr(seed=14):
    b = Builder("corr_pool", seed); b.seg_corr(); return b.walk


def walk_overflow(seed=15):
    b = Builder("overflow", seed, long=True); b.seg_overflow(); return b.walk


def walk_foreign(seed=16):
    b = Builder("foreign", seed); b.seg_foreign(); return b.walk


def walk_combined(seed=2, name="combined"):
    """Everything on one workspace under a seed of its own: every call draws its pair policy and goes through the correspondence pool."""
    b = Builder(name, seed, mixed=True)
    b.keyed_corr = True
    b.threshold(0)
    b.seg_pool(n_calls=24)
    b.seg_corr()
    b.seg_geometry()
    b.seg_policies(rounds=5)
    b.seg_foreign()
    return b.walk


WALKS = dict(frame_pool=walk_frame_pool, geometry=walk_geometry, policies=walk_policies, corr_pool=walk_corr, overflow=walk_overflow,
             foreign=walk_foreign, combined=walk_combined, combined_b=functools.partial(walk_combined, 3, "combined_b"))


@functools.lru_cache(maxsize=None)
def walk_json(name: str) -> str:
    return json.dumps(WALKS[name](), sort_keys=True)


def get_walk(name: str):
    return json.loads(walk_json(name))


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------

def coverage(walk):
    """What the walk visits, counted on the models and the exact simulations."""
    recs, tr = replay(walk)
    steps = walk["steps"]
    cov = dict.fromkeys(("calls", "U>L", "built>L", "hit+miss under pressure", "regrowths", "geometry returns", "downscale returns", "evict-and-reuse",
                         "rebinds", "clears", "length changes", "reversed pairs", "below-threshold between cached", "shuffled after cached calls",
                         "appended entries", "largest call", "foreign calls"), 0)
    cov.update({f"policy {p}": 0 for p in POLICIES}, **{f"foreign {w}": 0 for w in FOREIGN}, compaction=0, no_compaction=0)
    cov["calls"] = len(recs)
    seen_pairs, cached_so_far, geoms, scales = set(), 0, [], []
    pending_below = None
    for r in recs:
        c, b = r["call"], r["bounds"]
        cov["U>L"] += b["U"] > b["L"]
        cov["built>L"] += r["built"] > b["L"]
        cov["hit+miss under pressure"] += bool(b["pressure"] and b["hits"] >= 1 and b["L"] >= 1)
        cov["regrowths"] += b["regrow"]
        if not geoms or geoms[-1] != c.pool:
            cov["geometry returns"] += c.pool in geoms[:-1]
            geoms.append(c.pool)
        if not scales or scales[-1] != c.downscale:
            cov["downscale returns"] += c.downscale in scales[:-1]
            scales.append(c.downscale)
        mixed = len({f[2] for f in c.frames}) == 2
        if mixed:
            cov[f"policy {c.policy}"] += 1
            cov["compaction" if compaction_side(c) else "no_compaction"] += 1
        mut = steps[r["step"]].get("mutation")
        cov["length changes"] += bool(mut and mut["kind"] == "drop")
        if c.uses_corr_pool:
            cov["reversed pairs"] += sum(1 for k, n in c.nonempty() if (k[1], k[0]) in seen_pairs and k not in seen_pairs)
            seen_pairs |= {k for k, _ in c.nonempty()}
            if c.shuffled and cached_so_far >= 10:
                cov["shuffled after cached calls"] += 1
            if pending_below:
                cov["below-threshold between cached"] += 1
                pending_below = None
            cached_so_far += 1
            cov["largest call"] = max(cov["largest call"], len(c.corr))
        elif c.keyed_corr and cached_so_far:
            pending_below = True
    for i, s in enumerate(steps):
        cov["evict-and-reuse"] += s["kind"] == "reuse"
        cov["rebinds"] += s["kind"] == "rebind"
        cov["clears"] += s["kind"] == "clear"
        if s["kind"] == "foreign":
            cov["foreign calls"] += 1
            cov[f"foreign {s['what']}"] += 1
    # entries an unbounded pool would have appended: beyond twice the floor of the real one, a reset is certain
    unbounded, total = CorrModel(), 0
    t2 = Tracker(walk)
    for s in steps:
        act = t2.step(s)
        if act[0] == "call" and act[1].uses_corr_pool and not act[1].shuffled:
            fresh = CorrModel._fresh(unbounded.hyps[0]["index"], act[1].nonempty())
            total += sum(n for _, n in fresh)
            unbounded.hyps[0]["index"].update(fresh)
        elif act[0] == "evict":
            unbounded.evict(act[1])
    cov["appended entries"] = total
    return {k: int(v) for k, v in cov.items()}


# what each walk is about; the combined walk owes everything but the overflow
REQUIRED = {
    "pressure": {"U>L": 10, "hit+miss under pressure": 10, "regrowths": 2},
    "geometry": {"geometry returns": 2, "downscale returns": 1, "evict-and-reuse": 3, "rebinds": 2, "clears": 1},
    "policies": {"policy 0": 5, "policy 1": 5, "policy 2": 5, "policy 3": 5, "compaction": 3, "no_compaction": 3},
    "corr": {"length changes": 5, "reversed pairs": 5, "below-threshold between cached": 2, "shuffled after cached calls": 1},
    "foreign": {"foreign optimize": 6, "foreign solve_zn": 6, "foreign objective": 6},
}
WALK_OWES = dict(frame_pool=("pressure",), geometry=("geometry",), policies=("policies",), corr_pool=("corr",), overflow=(),
                 foreign=("foreign",), combined=("pressure", "geometry", "policies", "corr", "foreign"))
WALK_OWES["combined_b"] = WALK_OWES["combined"]


def missing_coverage(name, cov):
    out = []
    for group in WALK_OWES[name]:
        for k, n in REQUIRED[group].items():
            if cov[k] < n:
                out.append(f"{k}: {cov[k]} < {n}")
    if name == "overflow":
        floor = max(16 * cov["largest call"], 1 << 16)
        if cov["largest call"] > 4096:
            out.append(f"largest call {cov['largest call']} > 4096 entries")
        if cov["appended entries"] <= 2 * floor:
            out.append(f"appended entries {cov['appended entries']} <= {2 * floor}")
    return out
