"""Descriptor matching (btba_match_pairs) on the CPU: the restatement tests/cpp/match_host.cpp against an independent fp64
transliteration of the reference's matching, its edge cases one by one, and the host-side ABI of the call (no GPU)."""
import ctypes as C
import math

import numpy as np
import pytest

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S
from bundletrack_amd.matching import params_from_config

from match_ref import HostFrame, numpy_fp64, restate, scene_frames

BTBA_EINVAL = _lib.BTBA_EINVAL


def test_match_params_default_and_record_size():
    p = _lib.match_params()
    cos45 = float(np.float32(math.cos(45.0 / 180.0 * math.pi)))
    assert (p.k, p.mutual) == (5, 1)
    assert p.max_dist_neighbor == np.float32(0.03) and p.max_dist_no_neighbor == np.float32(0.02)
    assert p.cos_max_normal_neighbor == cos45 and p.cos_max_normal_no_neighbor == cos45
    assert p.min_z == np.float32(0.1)
    assert _lib.MATCH_DTYPE.itemsize == 40 and C.sizeof(_lib.MatchParams) == 28
    q = params_from_config({"feature_corres": {"mutual": False, "max_dist_neighbor": 10000, "max_normal_neighbor": 180}})
    assert q.mutual == 0 and q.max_dist_neighbor == 10000.0 and q.cos_max_normal_neighbor == -1.0


def _capacity(prm=None, n_frames=3, H=8, W=10, D=8, n_kpts=(4, 5, 0), pairs=((0, 1), (1, 2))):
    prm = _lib.match_params() if prm is None else prm
    nk = np.asarray(n_kpts, np.int32)
    pr = np.asarray(pairs, np.int32).reshape(-1, 2)
    cap = C.c_int64(-1)
    rc = _lib.lib().btba_match_capacity(C.byref(prm) if prm is not False else None, n_frames, H, W, D, nk.ctypes.data, pr.shape[0],
                                        pr.ctypes.data if pr.size else None, C.byref(cap))
    return rc, cap.value


def test_match_capacity_and_every_rejected_argument():
    assert _capacity() == (0, 4 + 5 + 5 + 0)
    assert _capacity(prm=_lib.match_params(mutual=0)) == (0, 4 + 5)
    assert _capacity(pairs=np.zeros((0, 2))) == (0, 0)
    bad = [dict(prm=False), dict(prm=_lib.match_params(k=0)), dict(prm=_lib.match_params(k=9)), dict(D=6), dict(D=0), dict(D=516),
           dict(n_kpts=(4, 8193, 0)), dict(n_kpts=(4, -1, 0)), dict(pairs=((1, 1),)), dict(pairs=((0, 3),)), dict(pairs=((-1, 0),)),
           dict(n_frames=0), dict(H=0), dict(W=0)]
    for kw in bad:
        assert _capacity(**kw)[0] == BTBA_EINVAL, kw
    assert _capacity(D=512, n_kpts=(8192, 8192, 0))[0] == 0


def test_match_pairs_rejects_before_any_device_call():
    L = _lib.lib()
    prm = _lib.match_params()
    nk = np.array([0, 0], np.int32)
    pr = np.array([0, 1], np.int32)
    nullp = (C.c_void_p * 2)()
    n_out = np.zeros(1, np.int32)
    K = np.eye(3, dtype=np.float32)
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(16), 2)
    ids = np.array([0, 1], np.int32)
    args = dict(ws=None, prm=C.byref(prm), dev=0, n=2, H=8, W=10, K=K.ctypes.data, desc=nullp, D=8, kpts=nullp, nk=nk.ctypes.data, depth=nullp,
                normal=nullp, poses=poses.ctypes.data, ids=ids.ctypes.data, n_pairs=1, pairs=pr.ctypes.data, out=None, pa=None, pb=None, n_out=n_out.ctypes.data)
    call = lambda **kw: L.btba_match_pairs(*{**args, **kw}.values())
    assert call() == BTBA_EINVAL                          # no workspace
    for kw in [dict(D=7), dict(prm=None), dict(n_out=None), dict(pairs=None), dict(K=None), dict(poses=None), dict(ids=None)]:
        assert call(**kw) == BTBA_EINVAL, kw


# ---- the restatement against the fp64 transliteration ---------------------------------------------------------

def test_restatement_matches_fp64_reference_up_to_near_ties():
    pb = S.make_problem(5, 10, seed=3, background=False)
    kp = S.make_keypoints(pb, 300, 60, D=64, desc_noise=0.05, seed=1)
    frames = scene_frames(pb, kp)
    pairs = [(a, b) for a in range(5) for b in range(a)]
    prm = _lib.match_params()
    got, _, _, _ = restate(frames, pairs, prm, pb.K, pb.H, pb.W)
    cfg = dict(max_dist_neighbor=prm.max_dist_neighbor, max_dist_no_neighbor=prm.max_dist_no_neighbor,
               cos_neighbor=prm.cos_max_normal_neighbor, cos_no_neighbor=prm.cos_max_normal_no_neighbor)
    ref = numpy_fp64(frames, pairs, cfg, pb.K, pb.H, pb.W)
    total = differ = near_ties = 0
    for g, (r, lists) in zip(got, ref):
        gs = set(zip(g["idx_a"].tolist(), g["idx_b"].tolist(), g["dir"].tolist()))
        rs = set(r)
        total += len(rs)
        differ += len(gs ^ rs)
        for _, _, d2 in lists:
            gaps = np.diff(d2) / np.maximum(d2[1:], 1e-30)
            near_ties += int(np.any(gaps < 1e-5))
    assert total > 1000, total                            # the scene produces real matches
    assert differ <= max(2, near_ties + total // 500), (differ, near_ties, total)


# ---- edge cases on a hand-built scene -----------------------------------------------------------------------

H, W = 8, 10
K = np.array([[100.0, 0, 4.5], [0, 100.0, 3.5], [0, 0, 1]], np.float32)


def _plane(z=0.5):
    depth = np.full((H, W), z, np.float32)
    normal = np.zeros((H, W, 4), np.float32)
    normal[..., 2] = -1.0
    return depth, normal


def _frame(fid, kpts, desc, depth=None, normal=None, pose=None):
    d0, n0 = _plane()
    return HostFrame(fid, np.eye(4, dtype=np.float32) if pose is None else pose, np.asarray(kpts, np.float32).reshape(-1, 2),
                     np.asarray(desc, np.float32).reshape(len(kpts), -1) if len(kpts) else np.zeros((0, 4), np.float32),
                     d0 if depth is None else depth, n0 if normal is None else normal)


def _unit(rng, n, D=4):
    v = rng.normal(size=(n, D))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _pairs_of(frames, pairs=((1, 0),), **kw):
    return restate(frames, list(pairs), _lib.match_params(**kw), K, H, W)[0]


def test_edge_identical_frames_match_everything_in_order():
    rng = np.random.default_rng(0)
    pts = [(1, 1), (2.4, 3), (5, 5), (8, 6)]
    desc = _unit(rng, 4)
    m = _pairs_of([_frame(0, pts, desc), _frame(1, pts, desc)])[0]
    assert m["idx_a"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3] and m["idx_b"].tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    assert m["dir"].tolist() == [0] * 4 + [1] * 4
    assert np.all(m["dist"] == 0.0) and np.all(m["ptA_cam"][:, 2] == np.float32(0.5))


def test_edge_k_larger_than_train_and_empty_frames():
    rng = np.random.default_rng(1)
    a = _frame(1, [(1, 1), (3, 3), (5, 5)], _unit(rng, 3))
    b = _frame(0, [(3, 3)], _unit(rng, 1))
    m = _pairs_of([b, a], k=8)[0]                           # every A keypoint finds the single B keypoint's list of one
    assert m["idx_b"].tolist()[:1] == [0] and len(m) >= 1
    e = _frame(2, [], [])
    assert [len(x) for x in _pairs_of([b, a, e], pairs=((2, 0), (1, 2)))] == [0, 0]


def test_edge_rounding_half_away_and_image_border():
    rng = np.random.default_rng(2)
    d = _unit(rng, 1)
    for kp, inside in [((2.5, 1.0), True), ((-0.5, 1.0), False), ((-0.49, 1.0), True), ((9.49, 1.0), True), ((9.5, 1.0), False),
                       ((1.0, 7.5), False), ((1.0, 7.49), True), ((1e9, 1.0), False), ((float("nan"), 1.0), False)]:
        m = _pairs_of([_frame(0, [kp], d), _frame(1, [kp], d)])[0]
        assert (len(m) == 2) == inside, kp
        if inside:
            u = math.floor(abs(kp[0]) + 0.5) * (1 if kp[0] >= 0 else -1)
            x_expect = np.float32(np.float32(u) * np.float32(0.5)) / np.float32(100)      # pixel u at depth 0.5, cx ignored below
            assert m["ptA_cam"][0, 2] == np.float32(0.5) and abs(m["ptA_cam"][0, 0] - (x_expect - np.float32(4.5 * 0.5 / 100))) < 1e-6


def test_edge_invalid_depth_and_zero_normals():
    rng = np.random.default_rng(3)
    d = _unit(rng, 2)
    depth, normal = _plane()
    depth[1, 1] = 0.0                                      # no depth under keypoint 0
    depth[2, 2] = np.float32(0.0999)                        # below min_z
    m = _pairs_of([_frame(0, [(1, 1), (2, 2)], d, depth=depth), _frame(1, [(1, 1), (2, 2)], d)])[0]
    assert len(m) == 0
    zero = np.zeros((H, W, 4), np.float32)                  # a zero normal stays zero: dot = 0 < cos 45 deg
    assert len(_pairs_of([_frame(0, [(1, 1)], d[:1], normal=zero), _frame(1, [(1, 1)], d[:1])])[0]) == 0
    # ... but passes at the 180 degree threshold (cos = -1), as the NOCS configuration ships
    assert len(_pairs_of([_frame(0, [(1, 1)], d[:1], normal=zero), _frame(1, [(1, 1)], d[:1])], cos_max_normal_no_neighbor=-1.0,
                         cos_max_normal_neighbor=-1.0)[0]) == 2


def test_edge_thresholds_neighbor_and_nocs():
    rng = np.random.default_rng(4)
    d = _unit(rng, 1)
    shift = np.eye(4, dtype=np.float32)
    shift[0, 3] = 0.025                                     # 2.5 cm apart in the model frame
    far = lambda fid: [_frame(0, [(4, 4)], d), _frame(fid, [(4, 4)], d, pose=shift)]
    assert len(_pairs_of(far(1))[0]) == 2                   # neighbours (ids 0, 1): 3 cm gate
    assert len(_pairs_of(far(2))[0]) == 0                   # not neighbours: 2 cm gate
    assert len(_pairs_of(far(2), max_dist_no_neighbor=10000.0, cos_max_normal_no_neighbor=-1.0)[0]) == 2      # NOCS: 10000 m, 180 deg
    tilt = np.eye(4, dtype=np.float32)
    c, s = math.cos(math.radians(50)), math.sin(math.radians(50))
    tilt[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    p = np.array([-0.5 * 0.5 / 100, -0.5 * 0.5 / 100, 0.5])            # the camera point at pixel (4, 3)
    tilt[:3, 3] = p - tilt[:3, :3].astype(np.float64) @ p                  # rotate about it: the same model point, normals 50 deg apart
    tilted = [_frame(0, [(4, 3)], d), _frame(1, [(4, 3)], d, pose=tilt)]
    assert len(_pairs_of(tilted)[0]) == 0
    assert len(_pairs_of(tilted, cos_max_normal_neighbor=-1.0)[0]) == 2


def test_edge_first_passing_neighbour_and_mutual_off():
    rng = np.random.default_rng(5)
    base = _unit(rng, 1)[0]
    # B keypoint 0 is the nearest descriptor but lies off the gate (other side of the image); keypoint 1 is second and passes
    da = base[None]
    db = np.stack([base, base + 0.05]) / np.linalg.norm(np.stack([base, base + 0.05]), axis=1, keepdims=True)
    a = _frame(1, [(2, 2)], da)
    b = _frame(0, [(8, 6), (2, 2)], db)
    m = _pairs_of([b, a], pairs=((1, 0),))[0]
    assert m[m["dir"] == 0]["idx_b"].tolist() == [1]
    mo = _pairs_of([b, a], pairs=((1, 0),), mutual=0)[0]
    assert mo["dir"].tolist() == [0] and mo["idx_b"].tolist() == [1]


def test_edge_duplicate_descriptors_lower_index_wins():
    rng = np.random.default_rng(6)
    d = _unit(rng, 1)
    a = _frame(1, [(3, 3)], d)
    b = _frame(0, [(3, 3), (3, 3), (3, 3)], np.repeat(d, 3, 0))
    m = _pairs_of([b, a], pairs=((1, 0),), k=1)[0]
    assert m[m["dir"] == 0]["idx_b"].tolist() == [0]
    assert m[m["dir"] == 1]["idx_b"].tolist() == [0, 1, 2]
