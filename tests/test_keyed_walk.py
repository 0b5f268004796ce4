"""The keyed-walk generator and its models (tests/keyed_walk.py), without a GPU: the walks the GPU tests run visit what they are
meant to visit, the frame bounds hold against the library's exact slot policy, the correspondence model explains the library's pool
whatever its capacity, and the generator is deterministic."""
import json

import numpy as np
import pytest

import keyed_walk as KW


@pytest.mark.parametrize("name", sorted(KW.WALKS))
def test_walks_cover_what_they_are_for(name):
    """No GPU run can pass vacuously: each walk holds the minimum counts of the paths it exists for (KW.REQUIRED), the combined walk
    all of them, the overflow walk enough appended entries that a reset of the correspondence pool is certain."""
    cov = KW.coverage(KW.get_walk(name))
    print(name, json.dumps(cov))
    assert KW.missing_coverage(name, cov) == []


def test_masked_valid_counts_differ():
    """BTBA_PAIRS_TARGET_MORE_VALID must not be decided by ties alone, and the variants must lie on both sides of the 60 % rule."""
    for pool in KW.POOLS:
        for ds in (4.0, 2.0):
            Hd, Wd = KW.cache_shape(pool, ds)
            masked = [KW.cache_valid(pool, p, KW.MASKED, ds) for p in range(KW.N_POS)]
            full = [KW.cache_valid(pool, p, KW.FULL, ds) for p in range(KW.N_POS)]
            assert len(set(masked)) >= 4, masked                 # not all equal, and far from it; equal neighbours keep the tie rule in play
            assert all(0 < m < 0.2 * Hd * Wd for m in masked) and all(f == Hd * Wd for f in full)
    assert KW.cache_shape("G1", 4.0) == (24, 32) and KW.cache_shape("G2", 4.0) == (25, 32)      # per-block ranges in use / not in use


def random_pool_walk(seed, n_calls=70):
    """Frame-pool steps alone: (verb, argument) with idents drawn from 80 frames, windows of 2 .. 9 and a few of 17, evictions, clears,
    rebinds and a second geometry."""
    rng = np.random.default_rng([seed, 3])
    gen, out, prev, geom, cursor = {}, [], [], 0, 0
    for _ in range(n_calls):
        r = rng.random()
        if r < 0.04 and prev:
            out.append(("evict", prev[int(rng.integers(0, len(prev)))][0]))
        elif r < 0.05:
            out.append(("clear", None))
        elif r < 0.08 and prev:
            k = prev[int(rng.integers(0, len(prev)))][0]
            gen[k] = gen.get(k, 0) + 1
        elif r < 0.10:
            geom = 1 - geom
            prev = []
        n = 17 if rng.random() < 0.04 else int(rng.integers(2, 10))
        kind = rng.random()
        if kind < 0.5 and prev:                                   # slide by one
            keys = [k for k, _, _ in prev][1:][-(n - 1):]
        elif kind < 0.75:                                         # loop closure / all new: anywhere on the orbit
            keys = []
        else:                                                     # permutation
            keys = [prev[k][0] for k in rng.permutation(len(prev))][:n]
        while len(keys) < n:
            k = 1000 * geom + (cursor if kind < 0.5 else int(rng.integers(0, 80)))
            cursor = (cursor + 1) % 80
            if k not in keys:
                keys.append(k)
        prev = [(k, "buf", gen.get(k, 0)) for k in keys]
        out.append(("call", (geom, prev)))
    return out


def test_frame_bounds_hold_for_the_library_policy():
    """pool_resolve's exact policy (PoolSim) against the tie-free bounds of FrameModel on 200 random walks: the built count lies in
    [L, U] in every call, the bounds are tight in most calls, and pressure really occurs."""
    calls = tight = above = 0
    for seed in range(200):
        model, sim = KW.FrameModel(), KW.PoolSim()
        for verb, arg in random_pool_walk(seed):
            if verb == "evict":
                model.evict(arg); sim.evict(arg)
            elif verb == "clear":
                model.clear(); sim.clear()
            else:
                b, built = model.call(*arg), sim.call(*arg)
                assert b["L"] <= built <= b["U"], (seed, calls, b, built)
                calls += 1
                tight += b["L"] == b["U"]
                above += built > b["L"]
    print(f"{calls} calls, L == U in {tight}, built > L in {above}")
    assert calls >= 14000 and tight > 0.5 * calls and above > 0.05 * calls


@pytest.mark.parametrize("name", sorted(KW.WALKS))
def test_models_explain_the_simulated_library(name):
    """Every generated walk against the simulations: frame bounds hold, and the correspondence model accepts the simulated pool's
    counts under three allocator head-rooms (the model does not know the capacity)."""
    walk = KW.get_walk(name)
    for headroom in (1.0, 1.25, 2.0):
        recs, tr = KW.replay(walk, headroom)
        for r in recs:
            b = r["bounds"]
            assert b["L"] <= r["built"] <= b["U"], (r["step"], b, r["built"])
            assert r["corr_msg"] is None, (r["step"], r["corr_msg"])
        if name == "overflow":
            assert recs[-1]["pool_resets"] >= 1 and tr.corr.resets >= 1          # the model is certain of a reset it was not told about
        elif recs:
            assert tr.corr.resets <= recs[-1]["pool_resets"]


def test_generator_is_deterministic():
    for name, make in KW.WALKS.items():
        a, b = json.dumps(make(), sort_keys=True), json.dumps(make(), sort_keys=True)
        assert a == b, name
        assert json.loads(a) == KW.get_walk(name)
    assert json.dumps(KW.walk_combined(2), sort_keys=True) != json.dumps(KW.walk_combined(3), sort_keys=True)


def test_window_array_is_pair_major_and_reversal_swaps_the_sides():
    sess = KW.Session(5)
    w = [("G1", 3, 0), ("G1", 4, 1), ("G1", 9, 0), ("G1", 10, 1), ("G1", 20, 1)]
    sess.invalid[(w[0], w[2])] = 4
    n = len(w)
    corr, nm = sess.window_corr(w)
    rev, nm_rev = sess.window_corr(w[::-1])
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    assert len(nm) == len(pairs) and nm.sum() == len(corr) and len(set(nm.tolist())) > 1
    off = np.concatenate([[0], np.cumsum(nm)])
    off_rev = np.concatenate([[0], np.cumsum(nm_rev)])
    for q, (i, j) in enumerate(pairs):
        seg = corr[off[q]:off[q + 1]]
        assert (seg["imgIdx_j"] == j).all() and np.isin(seg["imgIdx_i"], (i, KW.INVALID)).all()
        q2 = pairs.index((n - 1 - j, n - 1 - i))                 # the same two frames in the reversed window: the later one is listed first
        twin = rev[off_rev[q2]:off_rev[q2 + 1]]
        assert len(twin) == len(seg)
        assert np.array_equal(twin["pos_i"], seg["pos_j"]) and np.array_equal(twin["pos_j"], seg["pos_i"])
        assert np.array_equal(twin["imgIdx_i"] == KW.INVALID, seg["imgIdx_i"] == KW.INVALID)
    assert (corr["imgIdx_i"] == KW.INVALID).any()
    # pos_i belongs to the frame listed first: moved into the model frame by its pose, the two sides of a match meet
    T = KW.poses_gt("G1")
    seg = corr[off[0]:off[1]] if nm[0] else corr[off[1]:off[2]]
    i, j = (0, 1) if nm[0] else (0, 2)
    if len(seg):
        pi = seg["pos_i"] @ T[w[i][1]][:3, :3].T + T[w[i][1]][:3, 3]
        pj = seg["pos_j"] @ T[w[j][1]][:3, :3].T + T[w[j][1]][:3, 3]
        assert np.median(np.linalg.norm(pi - pj, axis=1)) < 0.01
    # a pair carries the same matches in every window that holds it
    other, nm_o = sess.window_corr([w[2], ("G1", 30, 0), w[4]])
    q = pairs.index((2, 4))
    assert np.array_equal(other[nm_o[0]:nm_o[0] + nm_o[1]]["pos_i"], corr[off[q]:off[q + 1]]["pos_i"])
