"""The device keyframe memory (bundletrack_amd/keyframes.py over btba_keyframes_* and btba_rotation_distances) against its numpy restatement
(tests/keyframes_ref.py, which tests/test_keyframes_ref.py holds to the oracle): every comparison is == on bytes."""
import numpy as np
import pytest

import keyframes_ref as G
from bundletrack_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
CAP, MAX_BA = 320, 6


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


def fill(mem, poses, ids, keys):
    """The pools of all sessions, frame by frame, through check_add with min_rot 0 (everything joins); the restatement's pools."""
    S = mem.n_sessions
    steps = max(len(p) for p in poses)
    for k in range(steps):
        active = np.array([k < len(p) for p in poses], np.int32)
        pose = np.stack([p[min(k, len(p) - 1)] for p in poses])
        fid = np.array([i[min(k, len(i) - 1)] for i in ids], np.int32)
        key = np.array([q[min(k, len(q) - 1)] for q in keys], np.uint64)
        mem.check_add(pose, fid, key, active=active, min_rot_deg=0.0)
    return [G.filled(poses[s], ids[s], keys[s], mem.capacity) for s in range(S)]


def same_pools(mem, pools):
    e = mem.export()
    for s, p in enumerate(pools):
        n = p.count
        assert e["count"][s] == n and e["overflow"][s] == p.overflow
        assert e["poses"][s, :n].tobytes() == p.poses[:n].tobytes() and e["frame_id"][s, :n].tobytes() == p.frame_id[:n].tobytes()
        assert e["frame_key"][s, :n].tobytes() == p.frame_key[:n].tobytes()


def prefilled(mem):
    """select's outputs with a byte pattern in them: what the call does not write must still be there afterwards."""
    import torch
    w = mem.empty_windows()
    for t in (w.n_window, w.slot, w.frame_id, w.frame_key, w.pose, w.newframe_index):
        t.view(torch.uint8).fill_(0x5A)
    return w


def host(w):
    return dict(n_window=w.n_window.cpu().numpy(), window_slot=w.slot.cpu().numpy(), window_frame_id=w.frame_id.cpu().numpy(),
                window_frame_key=w.frame_key.cpu().numpy().view(np.uint64), window_pose=w.pose.cpu().numpy().reshape(w.pose.shape[0], -1, 16),
                newframe_index=w.newframe_index.cpu().numpy())


def expect(pools, before, new_pose, new_id, new_key, max_BA, active=None):
    """The restatement's outputs for every session from the outputs' previous content."""
    out = {k: np.array(v) for k, v in before.items()}
    for s, p in enumerate(pools):
        if active is not None and not active[s]:
            continue
        prev = {k: before[k][s] for k in ("window_slot", "window_frame_id", "window_frame_key", "window_pose")}
        r = G.select(p, new_pose[s], new_id[s], new_key[s], max_BA, out=prev)
        for k, v in r.items():
            out[k][s] = v
    return out


def same_windows(got, want):
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k


def s4(ws, perm=(0, 1, 2, 3)):
    from bundletrack_amd.keyframes import DeviceKeyframeMemory
    poses, ids, keys, new_pose, new_id, new_key = G.select_case()
    perm = list(perm)
    poses, ids, keys = [poses[i] for i in perm], [ids[i] for i in perm], [keys[i] for i in perm]
    mem = DeviceKeyframeMemory(ws, 4, CAP, MAX_BA)
    pools = fill(mem, poses, ids, keys)
    return mem, pools, new_pose[perm], new_id[perm], new_key[perm]


def test_rotation_distances_bits(ws):
    from scipy.spatial.transform import Rotation
    from bundletrack_amd.keyframes import rotation_distances
    n = 4096
    A, B = G.random_rotations(n, 21), G.random_rotations(n, 22)
    B[0::4] = A[0::4]                                                               # identical
    B[1::4] = A[1::4]; B[1::4, 0, 0] = np.nextafter(A[1::4, 0, 0], F(0))            # nudged by one ulp
    small = Rotation.from_rotvec(np.random.default_rng(5).normal(size=(n // 4, 3)) * 1e-3).as_matrix()
    B[2::4, :3, :3] = (small @ A[2::4, :3, :3].astype(np.float64)).astype(F)       # nearly identical
    A[3], B[3] = np.eye(4, dtype=F), np.diag([1, -1, -1, 1]).astype(F)             # a 180 degree flip: the clamp at -1
    got = rotation_distances(ws, A, B).cpu().numpy()
    want = G.distance(A, B)
    assert got.tobytes() == want.tobytes(), np.nonzero(got != want)[0][:10]
    assert got[3] == F(np.pi) and got[0] == G.distance(A[0], A[0]) and (got[1::4] != got[0::4]).any()
    assert rotation_distances(ws, A[:0], B[:0]).numel() == 0


def test_select_fits_misses_and_ties_across_waves(ws):
    mem, pools, new_pose, new_id, new_key = s4(ws)
    same_pools(mem, pools)
    w = prefilled(mem)
    before = host(w)
    got = host(mem.select(new_pose, new_id, new_key, out=w))
    want = expect(pools, before, new_pose, new_id, new_key, MAX_BA)
    same_windows(got, want)
    assert got["n_window"].tolist() == [4, 6, 6, 6] and got["newframe_index"].tolist() == [3, 5, 5, 5]
    assert got["window_slot"][1].tolist() == [0, 1, 2, 3, 4, -1]                    # fits exactly: everything
    assert got["window_slot"][0, 4:].tobytes() == before["window_slot"][0, 4:].tobytes()      # rows past n_window keep their bytes
    # the 300-pool: the bytewise duplicates tie for the smallest cum_dist and join lowest slot first, across lanes and waves
    joined = G.greedy_members(pools[3], new_pose[3], MAX_BA)
    assert joined[:4] == [0, 5, 70, 270] and got["window_slot"][3].tolist() == sorted(joined) + [-1]
    # twice the same bytes
    again = host(mem.select(new_pose, new_id, new_key, out=prefilled(mem)))
    same_windows(again, got)
    mem.close()


def test_select_max_ba_15_on_make_pools_seeds(ws):
    from bundletrack_amd.keyframes import DeviceKeyframeMemory
    from test_oracle_keyframes import make_pool
    S, B = 24, 15
    cases = [make_pool(seed) for seed in range(S)]
    mem = DeviceKeyframeMemory(ws, S, 48, B)
    pools = [G.Pool(48) for _ in range(S)]
    rots = sorted({c[1] for c in cases})
    for k in range(max(len(c[0]) for c in cases) - 1):
        pose = np.stack([c[0][min(k, len(c[0]) - 2)].reshape(16) for c in cases])
        fid = np.full(S, k, np.int32)
        for r in rots:
            active = np.array([c[1] == r and k < len(c[0]) - 1 for c in cases], np.int32)
            if not active.any():
                continue
            added = mem.check_add(pose, fid, fid.astype(np.uint64), active=active, min_rot_deg=r).cpu().numpy()
            for s in np.nonzero(active)[0]:
                assert added[s] == G.check_add(pools[s], pose[s], k, frame_key=k, min_rot_deg=r), (s, k)
    same_pools(mem, pools)
    new_pose = np.stack([c[0][-1].reshape(16) for c in cases])
    new_id = np.array([len(c[0]) - 1 for c in cases], np.int32)
    new_key = new_id.astype(np.uint64)
    w = prefilled(mem)
    before = host(w)
    got = host(mem.select(new_pose, new_id, new_key, out=w))
    same_windows(got, expect(pools, before, new_pose, new_id, new_key, B))
    assert (got["n_window"] == np.minimum(B, np.array([p.count for p in pools]) + 1)).all() and (got["n_window"] == B).sum() >= 5
    mem.close()


def orbit(n, seed):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    T = np.tile(np.eye(4, dtype=F), (n, 1, 1))
    R = Rotation.identity()
    for k in range(n):
        if k:
            R = Rotation.from_rotvec(np.deg2rad(rng.uniform(1.0, 6.0)) * np.array([0.1 * rng.normal(), 1.0, 0.1 * rng.normal()])) * R
        T[k, :3, :3] = R.as_matrix().astype(F)
    return T.reshape(n, 16)


def test_check_add_orbit_three_min_rots_and_a_full_pool(ws):
    from bundletrack_amd.keyframes import DeviceKeyframeMemory
    n, rots = 40, (5.0, 10.0, 20.0)
    T = [orbit(n, 31 + s) for s in range(3)]
    mem = DeviceKeyframeMemory(ws, 3, 40, MAX_BA, min_feat_num=100)
    small = DeviceKeyframeMemory(ws, 1, 4, MAX_BA, min_rot_deg=5.0)                    # capacity 4: overflows
    pools, tiny = [G.Pool(40) for _ in range(3)], G.Pool(4)
    n_added = 0
    for k in range(n):
        pose = np.stack([t[k] for t in T])
        fid = np.full(3, k, np.int32)
        status = np.array([k % 7 != 3] * 3, np.int32)
        kpts = np.array([50 if k % 5 == 4 else 300] * 3, np.int32)
        for s, r in enumerate(rots):                                                   # one call per min_rot, the other sessions inactive
            active = np.arange(3) == s
            added = mem.check_add(pose, fid, fid.astype(np.uint64) + np.uint64(7), status, kpts, active=active.astype(np.int32), min_rot_deg=r).cpu().numpy()
            want = G.check_add(pools[s], pose[s], k, frame_key=k + 7, status_other=status[s], n_keypts=kpts[s], min_rot_deg=r, min_feat_num=100)
            assert added[s] == want and (added[~active] == 0).all(), (s, k)
            n_added += want
        got = int(small.check_add(pose[:1], fid[:1]).cpu()[0])
        assert got == G.check_add(tiny, pose[0], k, min_rot_deg=5.0), k
    same_pools(mem, pools)
    same_pools(small, [tiny])
    counts = [p.count for p in pools]
    assert counts[0] > counts[1] > counts[2] >= 3 and tiny.count == 4 and tiny.overflow >= 3, (counts, tiny.overflow)
    e = small.export()
    assert e["poses"].shape == (1, 4, 4, 4) and e["overflow"][0] == tiny.overflow
    small.reset()
    assert small.export()["count"][0] == 0 and small.export()["overflow"][0] == 0
    mem.reset(1)
    assert mem.export()["count"].tolist() == [counts[0], 0, counts[2]]
    mem.close(); small.close()


def test_writeback_then_select(ws):
    import torch
    mem, pools, new_pose, new_id, new_key = s4(ws)
    w = mem.select(new_pose, new_id, new_key)
    h = host(w)
    rng = np.random.default_rng(9)
    solved = (h["window_pose"] + rng.normal(size=h["window_pose"].shape).astype(F) * F(1e-3)).astype(F)      # what a solve would hand back
    mem.writeback(w.n_window, w.slot, torch.from_numpy(solved).cuda())
    for s, p in enumerate(pools):
        G.writeback(p, h["n_window"][s], h["window_slot"][s], solved[s])
    same_pools(mem, pools)
    assert pools[3].poses[5].tobytes() == solved[3, 1].tobytes() and pools[3].poses[6].tobytes() != solved[3, 2].tobytes()
    # the solved poses enter the next selection
    nxt = G.random_rotations(4, 77).reshape(4, 16)
    w2 = prefilled(mem)
    before = host(w2)
    got = host(mem.select(nxt, new_id + 2, new_key, out=w2))
    same_windows(got, expect(pools, before, nxt, new_id + 2, new_key, MAX_BA))
    assert got["window_pose"][1, :5].tobytes() == solved[1, :5].tobytes()              # session 1 fits: its five keyframes, as solved
    mem.close()


def test_inactive_sessions_permutations_and_limits(ws):
    from bundletrack_amd.keyframes import DeviceKeyframeMemory
    mem, pools, new_pose, new_id, new_key = s4(ws)
    active = np.array([1, 0, 0, 1], np.int32)
    w = prefilled(mem)
    before = host(w)
    got = host(mem.select(new_pose, new_id, new_key, active=active, out=w))
    same_windows(got, expect(pools, before, new_pose, new_id, new_key, MAX_BA, active=active))
    for k in got:
        assert got[k][1:3].tobytes() == before[k][1:3].tobytes(), k                 # inactive: every byte of the outputs
    import torch
    added = torch.full((4,), 0x5A5A, dtype=torch.int32, device="cuda")
    mem.check_add(new_pose, np.zeros(4, np.int32), active=1 - active, out=added)      # frame id 0 joins sessions 1 and 2 only
    assert added.cpu().numpy().tolist() == [0x5A5A, 1, 1, 0x5A5A]
    for s in (1, 2):
        assert G.check_add(pools[s], new_pose[s], 0) == 1
    same_pools(mem, pools)                                                           # sessions 0 and 3: every byte of the state
    e = mem.export()
    assert not e["poses"][0, pools[0].count:].any() and not e["frame_id"][3, pools[3].count:].any()      # nothing written past the pools
    mem.close()
    # a permutation of the sessions permutes the outputs and nothing else
    perm = (2, 0, 3, 1)
    a, _, pa, ia, ka = s4(ws)
    b, _, pb, ib, kb = s4(ws, perm)
    ha, hb = host(a.select(pa, ia, ka, out=prefilled(a))), host(b.select(pb, ib, kb, out=prefilled(b)))
    for k in ha:
        assert hb[k].tobytes() == ha[k][list(perm)].tobytes(), k
    ea, eb = a.export(), b.export()
    for k in ea:
        assert eb[k].tobytes() == ea[k][list(perm)].tobytes(), k
    a.close(); b.close()
    # sizes outside the limits are refused at creation, never truncated
    for S, cap, ba in ((1, 1024, 40), (1, 10, 1), (1, 10, 86), (1, 0, 6), (0, 10, 6), (1 << 13, (1 << 11) + 1, 2)):
        with pytest.raises(_lib.BtbaError) as err:
            DeviceKeyframeMemory(ws, S, cap, ba)
        assert err.value.status == _lib.BTBA_EINVAL
    big = DeviceKeyframeMemory(ws, 1, 1024, 32)                                      # the stated reach: 1024 keyframes at max_BA 32, 128 KB of table
    T = G.random_rotations(41, 55).reshape(41, 16)
    pools = fill(big, [T[:40]], [np.arange(40, dtype=np.int32)], [np.arange(40, dtype=np.uint64)])
    w = prefilled(big)
    before = host(w)
    same_windows(host(big.select(T[40:41], [40], None, out=w)), expect(pools, before, T[40:41], [40], [0], 32))
    big.close()
