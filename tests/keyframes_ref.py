"""numpy / Python-float restatement of the device keyframe memory (include/btba.h, "device keyframe memory"): the three functions of
bundletrack_amd/csrc/btba_keyframes_point.hpp, operation for operation, and the three operations on plain arrays -- the capacity rule and
the tie rule included.  Every float32 step is a numpy float32 operation (IEEE, rounded once), every float64 step a numpy float64 one, so the
bits are the header's.  tests/test_keyframes_ref.py holds it to the oracle; the GPU tests compare the device's bytes with it."""
import numpy as np

F, D = np.float32, np.float64
PI = D(3.141592653589793)
FLT_MAX = np.finfo(F).max


def _mat(A):
    A = np.asarray(A, F)
    return A.reshape(A.shape[:-1] + (4, 4)) if A.shape[-1] == 16 else A


def tmp(A, B):
    """keyframes_tmp: A, B [..., 4, 4] (or [..., 16]) float32 -> float32 [...]."""
    A, B = _mat(A), _mat(B)
    prod = A[..., :3, :3] * B[..., :3, :3]
    dots = (prod[..., 0] + prod[..., 1]) + prod[..., 2]
    trace = (dots[..., 0] + dots[..., 1]) + dots[..., 2]
    t = ((trace - F(1.0)).astype(D) / D(2.0)).astype(F)
    return np.fmax(np.fmin(F(1.0), t), F(-1.0))


def acosf(t):
    """keyframes_acosf: float32 [...] in [-1, 1] -> float32 [...]."""
    t = np.asarray(t, F)
    a = np.abs(t).astype(D)
    u = np.sqrt((D(1.0) - a) / (D(1.0) + a))
    for _ in range(4):
        u = u / (D(1.0) + np.sqrt(D(1.0) + u * u))
    z = u * u
    p = D(1.0) / D(17.0)
    for k in (15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = D(1.0) / D(k) - z * p
    p = D(1.0) - z * p
    r = D(32.0) * (u * p)
    return np.where(t < F(0.0), PI - r, r).astype(F)


def degrees(d):
    """keyframes_degrees."""
    return ((np.asarray(d, F) * F(180.0)).astype(D) / PI).astype(F)


def distance(A, B):
    return acosf(tmp(A, B))


class Pool:
    """One session's pool as the device holds it."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.poses = np.zeros((self.capacity, 16), F)
        self.frame_id = np.zeros(self.capacity, np.int32)
        self.frame_key = np.zeros(self.capacity, np.uint64)
        self.count = 0
        self.overflow = 0

    def copy(self):
        q = Pool(self.capacity)
        q.poses, q.frame_id, q.frame_key, q.count, q.overflow = self.poses.copy(), self.frame_id.copy(), self.frame_key.copy(), self.count, self.overflow
        return q


def check_add(pool, pose, frame_id, frame_key=0, status_other=1, n_keypts=100, min_rot_deg=10.0, min_feat_num=0):
    """btba_keyframes_check_add for one session: 1 joined, 0 not, -1 would have joined a full pool."""
    pose = np.asarray(pose, F).reshape(16)
    join = frame_id == 0
    if not join and status_other and n_keypts >= min_feat_num:
        n = pool.count
        deg = degrees(distance(np.broadcast_to(pose, (n, 16)), pool.poses[:n])) if n else np.zeros(0, F)
        join = not bool((deg < F(min_rot_deg)).any())
    if not join:
        return 0
    if pool.count >= pool.capacity:
        pool.overflow += 1
        return -1
    k = pool.count
    pool.poses[k], pool.frame_id[k], pool.frame_key[k] = pose, frame_id, frame_key
    pool.count = k + 1
    return 1


def greedy_members(pool, newpose, max_BA, on_round=None):
    """The chosen pool slots in joining order (without the new frame).  on_round(chosen_slots, candidates, cum float32 per candidate, pick)."""
    n = pool.count
    if n + 1 <= max_BA:
        return list(range(n))
    newpose = np.asarray(newpose, F).reshape(16)
    P = pool.poses[:n]
    col = {-1: distance(P, np.broadcast_to(newpose, (n, 16))), 0: distance(P, np.broadcast_to(P[0], (n, 16)))}
    chosen = [0]
    while len(chosen) + 1 < max_BA:
        order = sorted(chosen) + [-1]                                 # summation order: slots ascending, the new frame last
        cand = [c for c in range(n) if c not in chosen]
        cum = np.zeros(len(cand), F)
        for m in order:
            cum = (cum + col[m][cand]).astype(F)
        best, pick = FLT_MAX, None
        for c, v in zip(cand, cum):                                   # strict `<`, pool order: the lowest slot on ties
            if v < best:
                best, pick = v, c
        if on_round is not None:
            on_round(list(chosen), cand, cum, pick)
        if pick is None:
            break
        chosen.append(pick)
        col[pick] = distance(P, np.broadcast_to(P[pick], (n, 16)))
    return chosen


def select(pool, newpose, new_frame_id, new_frame_key, max_BA, out=None):
    """btba_keyframes_select for one session.  out: the rows' previous content (rows at and past n_window keep it)."""
    newpose = np.asarray(newpose, F).reshape(16)
    members = greedy_members(pool, newpose, max_BA) + [-1]
    key = lambda m: (int(new_frame_id), 1 << 40) if m < 0 else (int(pool.frame_id[m]), m)
    rows = sorted(members, key=key)
    if out is None:
        out = dict(window_slot=np.zeros(max_BA, np.int32), window_frame_id=np.zeros(max_BA, np.int32), window_frame_key=np.zeros(max_BA, np.uint64),
                   window_pose=np.zeros((max_BA, 16), F))
    out = {k: np.array(v) for k, v in out.items()}
    for r, m in enumerate(rows):
        out["window_slot"][r] = m
        out["window_frame_id"][r] = new_frame_id if m < 0 else pool.frame_id[m]
        out["window_frame_key"][r] = new_frame_key if m < 0 else pool.frame_key[m]
        out["window_pose"][r] = newpose if m < 0 else pool.poses[m]
    out["n_window"] = np.int32(len(rows))
    out["newframe_index"] = np.int32(rows.index(-1))
    return out


def writeback(pool, n_window, window_slot, poses):
    """btba_keyframes_writeback for one session."""
    poses = np.asarray(poses, F).reshape(-1, 16)
    for r in range(int(n_window)):
        s = int(window_slot[r])
        if 0 <= s < pool.count:
            pool.poses[s] = poses[r]


# ---- shared inputs of the GPU tests -------------------------------------------------------------------------------------------------
def random_rotations(n, seed):
    from scipy.spatial.transform import Rotation
    T = np.tile(np.eye(4, dtype=F), (n, 1, 1))
    T[:, :3, :3] = Rotation.random(n, random_state=seed).as_matrix().astype(F)
    T[:, :3, 3] = np.random.default_rng(seed).normal(size=(n, 3)).astype(F) * F(0.05)
    return T


def rotated(T, rotvec_deg):
    from scipy.spatial.transform import Rotation
    out = np.array(T, F)
    out[:3, :3] = (Rotation.from_rotvec(np.deg2rad(np.asarray(rotvec_deg, D))).as_matrix() @ np.asarray(T, D)[:3, :3]).astype(F)
    return out


def select_case():
    """S = 4 sessions, capacity 320, max_BA 6: pools of 3 (fits), 5 (fits exactly), 6 (misses by one) and 300 keyframes -- more than one
    candidate per lane of a 256-thread workgroup.  The 300-pool holds bytewise duplicates at slots 5, 70 and 270 (lane 5 of wave 0, lane 6 of
    wave 1, and lane 14 of wave 0 on its second pass) that sit next to keyframe 0 and the new frame, so they tie for the smallest cum_dist in
    the first rounds.  Returns (pool poses per session, ids per session, keys per session, new poses [4, 16], new ids, new keys)."""
    sizes = (3, 5, 6, 300)
    poses, ids, keys = [], [], []
    new_pose, new_id, new_key = np.zeros((4, 16), F), np.zeros(4, np.int32), np.zeros(4, np.uint64)
    for s, n in enumerate(sizes):
        T = random_rotations(n + 1, 100 + s)
        if n == 300:
            T[5] = rotated(T[0], [0.0, 0.2, 0.0])
            T[70] = T[5]
            T[270] = T[5]
            T[n] = rotated(T[0], [0.3, 0.0, 0.1])
        poses.append(T[:n].reshape(n, 16).copy())
        ids.append((np.arange(n, dtype=np.int32) * 2))                 # ids with gaps: 0, 2, 4, ...
        keys.append((np.arange(n, dtype=np.uint64) + np.uint64(1000 * (s + 1))) << np.uint64(33))
        new_pose[s], new_id[s], new_key[s] = T[n].reshape(16), 2 * n + 1, np.uint64(77 + s) << np.uint64(40)
    return poses, ids, keys, new_pose, new_id, new_key


def filled(poses, ids, keys, capacity):
    """A Pool holding these keyframes (what check_add with min_rot 0 makes of them)."""
    p = Pool(capacity)
    n = len(poses)
    p.poses[:n], p.frame_id[:n], p.frame_key[:n], p.count = poses, ids, keys, n
    return p
