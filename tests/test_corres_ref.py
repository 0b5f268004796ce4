"""CPU checks of tests/corres_ref.py (the plain-Python restatement of findCorres with map points) on hand-built cases for every
rule of include/btba.h, and of btba_corres_chain_capacity (host-only argument validation and output bound)."""
import ctypes as C

import numpy as np
import pytest

from bundletrack_amd import _lib
from bundletrack_amd._lib import MATCH_DTYPE
from corres_ref import CorresRef


def _recs(pairs, dirs=None):
    out = np.zeros(len(pairs), MATCH_DTYPE)
    for i, (a, b) in enumerate(pairs):
        out[i]["idx_a"], out[i]["idx_b"], out[i]["dist"] = a, b, 0.5
        out[i]["dir"] = 0 if dirs is None else dirs[i]
        out[i]["ptA_cam"], out[i]["ptB_cam"] = (a, 0, 1), (b, 0, 1)
    return out


def _grid(n, shift=0.0):
    return np.array([[float(i) + shift, 2.0 * i] for i in range(n)], np.float32)


def _all(recs):
    return range(len(recs))


def _pt(frame, i):
    return np.array([i, frame, 1], np.float32)


def _mem(*frames, n=12):
    R = CorresRef()
    for f in frames:
        R.register(f, _grid(n))
    return R


def test_neighbour_pair_links_inliers_into_tracks():
    R, st = _mem(0, 1), {}
    out, stages = R.find_corres(1, 0, True, _recs([(i, i) for i in range(8)]), st, _all, _pt)
    assert stages == [8, 8, 8, 8] and len(out) == 8 and not st.get(1)
    assert R.tracks() == {frozenset({(0, i), (1, i)}) for i in range(8)}


def test_neighbour_fail_below_five_nn_matches_keeps_them():
    R, st = _mem(0, 1), {}
    out, stages = R.find_corres(1, 0, True, _recs([(0, 0), (1, 1), (2, 2), (3, 3)]), st, _all, _pt)
    assert st[1] and stages == [4, 4, 4, 4] and len(out) == 4 and R.tracks() == set()


def test_fail_set_by_an_earlier_pair_short_circuits_later_pairs():
    R, st = _mem(0, 1, 2), {}
    R.find_corres(2, 1, True, _recs([(0, 0)]), st, _all, _pt)
    assert st[2]
    out, stages = R.find_corres(2, 0, False, _recs([(i, i) for i in range(9)]), st, _all, _pt)
    assert stages == [9, 9, 9, 9] and len(out) == 9 and R.tracks() == set()


def test_zero_keypoints_appends_nothing_and_does_not_fail():
    R, st = CorresRef(), {}
    R.register(0, _grid(10))
    R.register(1, np.zeros((0, 2), np.float32))
    out, stages = R.find_corres(1, 0, True, _recs([]), st, _all, _pt)
    assert stages == [0, 0, 0, 0] and len(out) == 0
    assert st[1]                                                            # no FAIL from the NN stage, but the final gate of a neighbour


def test_exactly_five_matches_is_cleared_before_ransac_six_runs_it():
    calls = []

    def ransac(recs):
        calls.append(len(recs))
        return range(len(recs))
    R, st = _mem(0, 1), {}
    out, stages = R.find_corres(1, 0, False, _recs([(i, i) for i in range(5)]), st, ransac, _pt)
    assert stages == [5, 5, 0, 0] and calls == [] and not st.get(1)        # a non-neighbour: no FAIL
    R2, st2 = _mem(0, 1), {}
    out, stages = R2.find_corres(1, 0, True, _recs([(i, i) for i in range(5)]), st2, ransac, _pt)
    assert stages == [5, 5, 0, 0] and st2[1]                                # a neighbour with 5: FAIL at the final gate
    R3, st3 = _mem(0, 1), {}
    out, stages = R3.find_corres(1, 0, True, _recs([(i, i) for i in range(6)]), st3, ransac, _pt)
    assert stages == [6, 6, 6, 6] and calls == [6]


def test_ransac_leaving_four_clears_and_fails_a_neighbour():
    R, st = _mem(0, 1), {}
    out, stages = R.find_corres(1, 0, True, _recs([(i, i) for i in range(9)]), st, lambda r: [0, 2, 4, 6], _pt)
    assert stages == [9, 9, 0, 0] and st[1] and len(out) == 0


def test_propagation_walks_map_a_in_key_order_and_skips_known_keys():
    R, st = _mem(0, 1, 2), {}
    R.find_corres(1, 0, True, _recs([(i, i) for i in range(8)]), st, _all, _pt)          # tracks 0-i / 1-i
    R.find_corres(2, 1, True, _recs([(i, i + 1) for i in range(7)]), st, _all, _pt)      # 2-i joins track (1, i+1)
    # (2, 0): NN already has A key 3 and B key 5 -> those two candidates drop
    out, stages = R.find_corres(2, 0, False, _recs([(3, 0), (6, 5)]), st, _all, _pt)
    prop = out[out["dir"] == 2]
    assert [(int(r["idx_a"]), int(r["idx_b"])) for r in prop] == [(0, 1), (1, 2), (2, 3), (5, 6)]
    assert stages[:2] == [2, 6]
    assert np.all(prop["dist"] == -1.0)
    assert np.array_equal(prop["ptA_cam"][0], _pt(2, 0)) and np.array_equal(prop["ptB_cam"][0], _pt(0, 1))


def test_propagation_drops_a_candidate_whose_b_key_an_earlier_candidate_took():
    R, st = _mem(0, 1, 2), {}
    R.find_corres(1, 0, True, _recs([(i, i) for i in range(8)]), st, _all, _pt)
    # keys 0 and 1 of frame 2 both join the track of (1, 0): last writer wins for img[2], both map_2 entries point at it
    R.find_corres(2, 1, True, _recs([(0, 0), (1, 0)] + [(i, i - 1) for i in range(2, 9)]), st, _all, _pt)
    out, stages = R.find_corres(2, 0, False, _recs([]), st, _all, _pt)
    assert [(int(r["idx_a"]), int(r["idx_b"])) for r in out] == [(0, 0)] + [(i, i - 1) for i in range(2, 9)]
    assert stages == [0, 8, 8, 8]


def test_shared_map_point_last_writer_wins():
    R, st = _mem(0, 1, 2), {}
    # frame 1: keys 0 and 1 both map to ONE map point (uvB 0 first, then key 1 of B joins it through A key 0 ... )
    R.find_corres(1, 0, True, _recs([(0, 0), (2, 1), (3, 2), (4, 3), (5, 4)]), st, _all, _pt)
    R.find_corres(2, 1, True, _recs([(7, 0), (8, 2), (9, 3), (10, 4), (11, 5), (6, 0)]), st, _all, _pt)
    mp = R.maps[1][R.uv(1, 0)]
    assert R.img[mp][2] == R.uv(2, 6)                                       # the later match wrote img[2]
    assert R.maps[2][R.uv(2, 7)] == mp and R.maps[2][R.uv(2, 6)] == mp


def test_mutual_half_repeats_keys_and_sees_earlier_effects():
    R, st = _mem(0, 1), {}
    recs = _recs([(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (1, 1), (0, 0)], dirs=[0, 0, 0, 0, 0, 1, 1])
    out, stages = R.find_corres(1, 0, True, recs, st, _all, _pt)
    assert stages == [7, 7, 7, 7]
    assert len(R.img) == 5                                                  # the repeats found both keys mapped: skipped


def test_duplicate_uv_keypoints_are_one_key():
    R, st = CorresRef(), {}
    k0 = _grid(8)
    k1 = _grid(8)
    k1[5] = k1[2]                                                           # keypoint 5 repeats keypoint 2's (u, v)
    k1[6] = [-0.0, 100.0]                                                   # -0 and +0 are one key
    k1[7] = [0.0, 100.0]
    R.register(0, k0)
    R.register(1, k1)
    assert R.key_index(1, R.uv(1, 5)) == 2 and R.key_index(1, R.uv(1, 7)) == 6
    R.find_corres(1, 0, True, _recs([(2, 0), (5, 1), (6, 2), (7, 3), (0, 4), (1, 5)]), st, _all, _pt)
    # (5, 1) hits A key 2 again: uvB 1 is new, so a new map point takes A key 2 over
    assert R.img[R.maps[1][R.uv(1, 2)]] == {0: R.uv(0, 1), 1: R.uv(1, 2)}
    assert R.img[R.maps[1][R.uv(1, 6)]] == {0: R.uv(0, 3), 1: R.uv(1, 6)}
    with pytest.raises(ValueError):
        R.register(2, np.array([[np.nan, 1.0]], np.float32))


def test_forget_erases_img_and_a_reused_frame_starts_empty():
    R, st = _mem(0, 1, 2), {}
    R.find_corres(1, 0, True, _recs([(i, i) for i in range(6)]), st, _all, _pt)
    R.find_corres(2, 1, True, _recs([(i, i) for i in range(6)]), st, _all, _pt)
    R.forget(1)
    assert R.tracks() == {frozenset({(0, i), (2, i)}) for i in range(6)}
    R.forget(0)
    R.forget(2)
    assert R.tracks() == set()
    R.register(1, _grid(12, shift=0.5))
    assert R.maps[1] == {}


# ---- btba_corres_chain_capacity --------------------------------------------------------------------------------------------
def _cap(n_kpts, pairs, **kw):
    L = _lib.lib()
    prm = _lib.match_params(**kw)
    nk = np.asarray(n_kpts, np.int32)
    pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    cap = C.c_int64(-1)
    rc = L.btba_corres_chain_capacity(C.byref(prm), len(nk), 480, 640, 256, nk.ctypes.data, pr.shape[0], pr.ctypes.data, C.byref(cap))
    return rc, cap.value


def test_chain_capacity_bounds_nn_plus_propagated():
    assert _cap([100, 200, 300], [(1, 0), (2, 0), (2, 1)]) == (0, (200 + 100 + 200) + (300 + 100 + 300) + (300 + 200 + 300))
    assert _cap([100, 200], [(1, 0)], mutual=0) == (0, 200 + 200)
    assert _cap([100, 200], []) == (0, 0)


@pytest.mark.parametrize("n_kpts,pairs,kw", [
    ([10, 10], [(1, 1)], {}),                 # A == B
    ([10, 10], [(1, 2)], {}),                 # index out of range
    ([10, 10], [(1, 0), (1, 0)], {}),         # a pair twice
    ([10, 10, 10], [(1, 0), (0, 1)], {}),     # the same frame pair both ways
    ([10, 9000], [(1, 0)], {}),               # more than 8192 keypoints
    ([10, 10], [(1, 0)], {"k": 0}),
])
def test_chain_capacity_rejects_bad_arguments(n_kpts, pairs, kw):
    assert _cap(n_kpts, pairs, **kw)[0] == _lib.BTBA_EINVAL


def test_corres_params_default_is_the_config():
    p = _lib.corres_params()
    assert (p.n_trials, p.dist_thres, p.hypothesis, p.seed) == (2000, np.float32(0.01), 0, 0)
