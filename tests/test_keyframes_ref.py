"""The restatement of the device keyframe memory (tests/keyframes_ref.py) against the oracle (oracle/btba_oracle_keyframes.c) and fp64.  CPU only.

The memory's arc cosine is its own function, so its distances differ from the oracle's acosf by up to one float ulp; what the two must share
are DECISIONS, held under a decision bar instead of a tolerance on poses:

  greedy rounds   S64(c): the fp64 sum of arccos(float64(tmp)) over the n chosen members.  Any fp32 evaluation whose terms are within one
                  ulp (<= 2^-22, the terms are below 4) and that adds them with n - 1 fp32 additions lies within
                  E(n) = n 2^-22 + (n - 1) 1/2 spacing32(S_max) of it, so the oracle's pick and the restatement's pick from the SAME chosen
                  set (the restatement's: teacher forcing) both lie in A = {c : S64(c) <= min S64 + 2 E(n)}.  Where A holds only bytewise
                  identical poses the pick is the lowest slot and equals the oracle's.  At most 1 % of the rounds may have an A with distinct poses.
  pool gate       a decision is one comparison `rot_diff < min_rot`: one fp64 degree value against min_rot.  Each equals the oracle's on the
                  same pool except where that value lies within 2 spacing32(deg) + (180 / pi) 2^-22 of min_rot, and so does the frame's
                  outcome unless one of its comparisons lies there.  At most 1 % of the comparisons may lie there.  Measured on the 200
                  pools: 137 of 53171 comparisons (0.26 %), none of them different from the oracle's; they sit in 111 of the 5354 frames
                  (2.07 %), every one a bit-for-bit revisit in a pool with min_rot 0, where the degree value is exactly 0 = min_rot and no
                  evaluation can come out negative.  With min_rot > 0 no comparison lies inside the bar.
"""
import ctypes as C

import numpy as np

import keyframes_ref as G
from oracle import oracle as O
from test_oracle_keyframes import make_pool

F, D = np.float32, np.float64
# keyframes_acosf's fp64 evaluation: 1 division and 1 square root, four half-angle steps of 5 operations, the series (its upper terms weigh
# z <= 0.0025 and less), two products and the subtraction from pi -- fewer than 48 roundings of at most 2^-53 relative on values below 4
E64 = 48 * 2.0 ** -53 * 4


def acos_arguments():
    rng = np.random.default_rng(11)
    t = [rng.uniform(-1.0, 1.0, 10 ** 6).astype(F), np.array([1.0, -1.0, 0.0, -0.0], F)]
    for start, toward in ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (-0.0, -1.0)):
        x, near = F(start), []
        for _ in range(64):
            x = np.nextafter(x, F(toward))
            near.append(x)
        t.append(np.array(near, F))
    T = G.random_rotations(512, 3)
    nudged = T.copy()
    nudged[:, 0, 0] = np.nextafter(nudged[:, 0, 0], F(0))
    t += [G.tmp(T, T), G.tmp(T, nudged)]                                # identical and 1-ulp-nudged rotations
    return np.concatenate(t)


def test_acosf_within_half_an_ulp_of_fp64():
    t = acos_arguments()
    r = G.acosf(t)
    err = np.abs(r.astype(D) - np.arccos(t.astype(D)))
    excess = err - 0.5 * np.spacing(r).astype(D)                      # what the fp64 evaluation's own error has to cover
    print("keyframes_acosf: %d arguments, worst |error| - 1/2 ulp32 = %.3e (allowed %.3e), worst error %.6f ulp32; differs from the rounded fp64 arccos at %d"
          % (len(t), excess.max(), E64, (err / np.spacing(np.maximum(r, F(1e-30)))).max(), int((np.arccos(t.astype(D)).astype(F) != r).sum())))
    assert (excess <= E64).all()
    assert r[t == 1.0].max() == 0.0 and (r[t == -1.0] == F(np.pi)).all()


def test_distance_within_one_ulp_of_the_oracle():
    T, U = G.random_rotations(3000, 1), G.random_rotations(3000, 2)
    U[::3] = T[::3]
    U[1::3, 0, 0] = np.nextafter(T[1::3, 0, 0], F(0)); U[1::3, 0, 1:] = T[1::3, 0, 1:]; U[1::3, 1:] = T[1::3, 1:]
    d = G.distance(T, U)
    o = np.array([O.rotation_geodesic_distance(a, b) for a, b in zip(T, U)], F)
    ulps = np.abs(d.astype(D) - o.astype(D)) / np.spacing(np.maximum(o, d)).astype(D)
    print("distance vs the oracle's acosf: %d of %d differ, at most %.2f ulp" % (int((d != o).sum()), len(d), ulps.max()))
    assert (ulps <= 1.0).all()
    eye, flip = np.eye(4, dtype=F), np.diag([1, -1, -1, 1]).astype(F)
    assert G.distance(eye, eye) == 0.0 and G.distance(eye, flip) == F(np.pi)


def oracle_distances(P, Q):
    return np.array([O.rotation_geodesic_distance(a, b) for a, b in zip(P, Q)], F)


def oracle_gate(poses, pool_list, k, frame_id, min_rot):
    """orc_check_and_add_keyframe for frame k against a GIVEN pool (the restatement's)."""
    f = O.lib().orc_check_and_add_keyframe
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    kf = np.array(list(pool_list) + [0, 0], np.int32)
    n = np.array([len(pool_list)], np.int32)
    flat = np.ascontiguousarray(poses, F).reshape(-1, 16)
    return int(f(flat.ctypes.data, k, frame_id, 1, 100, 0, min_rot, kf.ctypes.data, n.ctypes.data))


def build_pool(poses, min_rot, stats=None):
    """The restatement's pool over frames 0 .. M-2 of make_pool's poses, every decision against the oracle's on the same pool."""
    M = len(poses)
    pool, members = G.Pool(M), []
    for k in range(M - 1):
        mine = G.check_add(pool, poses[k], k, frame_key=k, min_rot_deg=min_rot)
        if stats is not None and k > 0:
            theirs = oracle_gate(poses, members, k, k, min_rot)
            deg64 = np.degrees(np.arccos(G.tmp(np.broadcast_to(poses[k], (len(members), 4, 4)), poses[members]).astype(D)))
            bar = 2 * np.spacing(deg64.astype(F)).astype(D) + (180 / np.pi) * 2.0 ** -22
            near = np.abs(deg64 - min_rot) <= bar
            # every comparison `rot_diff < min_rot` (one fp64 degree value each) against the oracle's own, then the frame's decision
            below = G.degrees(G.distance(np.broadcast_to(poses[k], (len(members), 4, 4)), poses[members])) < F(min_rot)
            below_o = G.degrees(oracle_distances(np.broadcast_to(poses[k], (len(members), 4, 4)), poses[members])) < F(min_rot)
            assert (near | (below == below_o)).all(), (k, np.nonzero(below != below_o)[0])
            assert near.any() or mine == theirs, (k, mine, theirs)
            stats["comparisons"] += len(near)
            stats["near"] += int(near.sum())
            stats["frames"] += 1
            stats["frames_near"] += bool(near.any())
            stats["differ"] += int((below != below_o).sum()) + (mine != theirs)
        if mine == 1:
            members.append(k)
    return pool, members


def test_pool_gate_and_greedy_rounds_under_the_decision_bar():
    gate = dict(comparisons=0, near=0, frames=0, frames_near=0, differ=0)
    n_greedy = n_rounds = n_open = n_pools_equal = n_selections_equal = 0
    for seed in range(200):
        poses, min_rot, max_ba = make_pool(seed)
        M = len(poses)
        pool, members = build_pool(poses, min_rot, gate)
        _, pool_o = O.keyframe_pool(poses[:-1], min_rot_deg=min_rot)
        same_pool = members == pool_o.tolist()
        n_pools_equal += same_pool
        if pool.count + 1 <= max_ba:
            got = G.select(pool, poses[-1], M - 1, 0, max_ba)
            assert got["window_frame_id"][: got["n_window"]].tolist() == members + [M - 1]
            continue
        n_greedy += 1
        P = pool.poses[: pool.count].reshape(-1, 4, 4)
        all_singleton = [True]

        def on_round(chosen, cand, cum, pick):
            nonlocal n_rounds, n_open
            n_rounds += 1
            mem = [P[m] for m in sorted(chosen)] + [poses[-1]]          # summation order: slots ascending, the new frame last
            n = len(mem)
            S64 = np.zeros(len(cand), D)
            o_cum = np.zeros(len(cand), F)
            for m in mem:
                Q = np.broadcast_to(m, (len(cand), 4, 4))
                S64 += np.arccos(G.tmp(P[cand], Q).astype(D))
                o_cum = (o_cum + oracle_distances(P[cand], Q)).astype(F)
            o_pick = cand[int(np.argmin(o_cum))]                        # strict `<` in pool order = the first minimum
            E = n * 2.0 ** -22 + (n - 1) * 0.5 * float(np.spacing(F(S64.max())))
            A = [c for c, v in zip(cand, S64) if v <= S64.min() + 2 * E]
            assert pick in A and o_pick in A, (seed, chosen, pick, o_pick, A)
            if len({P[c].tobytes() for c in A}) == 1:
                assert pick == o_pick == min(A), (seed, chosen, pick, o_pick, A)
            else:
                n_open += 1
                all_singleton[0] = False

        chosen = G.greedy_members(pool, poses[-1], max_ba, on_round=on_round)
        assert len(chosen) + 1 == max_ba and chosen[0] == 0 and len(set(chosen)) == len(chosen)
        if same_pool and all_singleton[0]:                              # then the whole selection is the oracle's
            ids_o = sorted(O.select_keyframes_for_ba(poses, M - 1, pool_o, max_ba).tolist())
            got = G.select(pool, poses[-1], M - 1, 0, max_ba)
            assert got["window_frame_id"][: got["n_window"]].tolist() == ids_o, seed
            assert got["newframe_index"] == max_ba - 1
            n_selections_equal += 1
    print("gate: %d comparisons, %d inside the bar (%.3f %%); %d frames, %d with a comparison inside the bar; %d differ from the oracle; pools equal to the oracle's: %d of 200"
          % (gate["comparisons"], gate["near"], 100.0 * gate["near"] / gate["comparisons"], gate["frames"], gate["frames_near"], gate["differ"], n_pools_equal))
    print("greedy: %d pools, %d rounds, %d with distinct poses in A; whole selections equal to the oracle's: %d" % (n_greedy, n_rounds, n_open, n_selections_equal))
    assert n_greedy >= 100 and n_rounds >= 500
    assert n_open <= 0.01 * n_rounds
    assert gate["near"] <= 0.01 * gate["comparisons"]


def test_fixed_cases():
    from scipy.spatial.transform import Rotation
    poses = np.tile(np.eye(4, dtype=F), (8, 1, 1))
    for k in range(8):
        poses[k, :3, :3] = Rotation.from_euler("y", 15.0 * k, degrees=True).as_matrix()
    # the frame-0 rule, the status gate and the keypoint gate: test_oracle_keyframes.test_check_and_add_keyframe_gates' case
    pool = G.Pool(8)
    got = [G.check_add(pool, poses[k], k, status_other=s, n_keypts=n, min_feat_num=10) for k, (n, s) in enumerate(zip([0, 5, 500, 500], [0, 1, 0, 1]))]
    added_o, pool_o = O.keyframe_pool(poses[:4], status_other=[0, 1, 0, 1], n_keypts=[0, 5, 500, 500], min_feat_num=10)
    assert got == [1, 0, 0, 1] == added_o.astype(int).tolist() and pool.frame_id[: pool.count].tolist() == pool_o.tolist() == [0, 3]
    # frame id 0 joins whatever its pose, status and keypoints
    assert G.check_add(pool, poses[0], 0, status_other=0, n_keypts=0, min_feat_num=10) == 1 and pool.count == 3
    # a pool that fits by exactly one frame, and one that misses by one
    pool = G.Pool(8)
    for k in range(5):
        assert G.check_add(pool, poses[k], k, frame_key=10 + k) == 1
    fit = G.select(pool, poses[7], 7, 99, max_BA=6)
    assert fit["n_window"] == 6 and fit["window_slot"].tolist() == [0, 1, 2, 3, 4, -1] and fit["newframe_index"] == 5
    assert fit["window_frame_key"].tolist() == [10, 11, 12, 13, 14, 99] and np.array_equal(fit["window_pose"][:5], pool.poses[:5])
    miss = G.select(pool, poses[7], 7, 99, max_BA=5)
    ids_o = sorted(O.select_keyframes_for_ba(poses, 7, np.arange(5, dtype=np.int32), 5).tolist())
    assert miss["n_window"] == 5 and miss["window_frame_id"].tolist() == ids_o and miss["window_slot"][0] == 0 and miss["window_slot"][4] == -1
    # capacity reached: -1, the overflow counter, and nothing past the end
    pool = G.Pool(4)
    got = [G.check_add(pool, poses[k], k) for k in range(7)]
    assert got == [1, 1, 1, 1, -1, -1, -1] and pool.count == 4 and pool.overflow == 3 and pool.poses.shape == (4, 16)
    assert G.check_add(pool, poses[3], 9) == 0 and pool.overflow == 3          # a frame the gate refuses does not count as overflow
    # a new frame whose id lies inside the pool's ids takes its row by id; writeback skips it
    pool = G.Pool(8)
    for k in range(4):
        G.check_add(pool, poses[k], 2 * k)
    w = G.select(pool, poses[6], 3, 0, max_BA=6)
    assert w["window_frame_id"][:5].tolist() == [0, 2, 3, 4, 6] and w["newframe_index"] == 2 and w["window_slot"][:5].tolist() == [0, 1, -1, 2, 3]
    before = pool.poses.copy()
    G.writeback(pool, w["n_window"], w["window_slot"], w["window_pose"] + F(1))
    assert np.array_equal(pool.poses[:4], before[:4] + F(1)) and np.array_equal(pool.poses[4:], before[4:])
