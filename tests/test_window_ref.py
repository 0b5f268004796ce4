"""Window assembly on the CPU: btba_window_layout (host-only, so callable without a GPU) against bundler.marshal_window on random
windows and on a window of the synthetic sequence, its BTBA_EINVAL cases, the exported symbols, the argument checks of the two
device calls that precede any GPU work, and the restatement tests/window_ref.py itself: marshalling against marshal_window, the
fixed-order moments against math.fsum, the SVD Kabsch on planted transforms and on mirrored planar sets (never a reflection), and
the reference-only margin inside the pose bar of tests/test_gpu_window.py."""
import ctypes as C
import math

import numpy as np
import pytest

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S
from bundletrack_amd.bundler import FrameRef, marshal_window

import window_ref as WR

NEW = ("btba_window_layout", "btba_marshal_windows", "btba_procrustes_pairs")


def _frames(ids):
    return [FrameRef(id=int(i), pose_in_model=np.eye(4, dtype=np.float32)) for i in ids]


def _random_window(rng, n_frames, empty_frac=0.3, max_count=40):
    """(frames, matches dict, counts in canonical order) with frame ids in random order and some empty pairs."""
    ids = np.sort(rng.choice(50, n_frames, replace=False))
    frames = _frames(ids)
    matches, counts = {}, []
    for i in range(n_frames):
        for j in range(i + 1, n_frames):
            m = 0 if rng.random() < empty_frac else int(rng.integers(1, max_count))
            counts.append(m)
            if m:
                matches[(int(ids[j]), int(ids[i]))] = (rng.normal(size=(m, 3)).astype(np.float32), rng.normal(size=(m, 3)).astype(np.float32))
    return frames, matches, np.asarray(counts, np.int32)


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)


def test_symbols_declared_and_exported():
    for name in NEW:
        assert name in _lib.declared_symbols() and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().btba_version() == 105


def test_layout_equals_marshal_window_on_random_windows():
    from bundletrack_amd.window import window_layout
    rng = np.random.default_rng(11)
    for n_frames in (2, 3, 5, 9, 15):
        wins = [_random_window(rng, n_frames, empty_frac=e) for e in (0.0, 0.3, 0.95, 1.0)]
        new_idx = [int(rng.integers(0, n_frames)) for _ in wins]
        for min_edges in (0, 5, 60):
            lay = window_layout(np.stack([w[2] for w in wins]), n_frames, new_idx, min_edges)
            refs = []
            for (frames, matches, counts), k in zip(wins, new_idx):
                shuffled = [frames[i] for i in rng.permutation(n_frames)]
                refs.append(marshal_window(shuffled, matches, frames[k], min_edges))
            assert lay.corr_stride == max(len(r.corr) for r in refs)
            assert lay.max_corr_per_pair == max(int(r.n_match_per_pair.max()) for r in refs)
            for w, r in enumerate(refs):
                assert np.array_equal(r.n_match_per_pair, wins[w][2])
                assert np.array_equal(lay.pair_offsets[w], _offsets(r.n_match_per_pair))
                assert int(lay.n_edges_newframe[w]) == r.n_edges_newframe
                assert bool(lay.run_ba[w]) == r.run_ba


def test_layout_on_a_window_of_the_synthetic_sequence():
    from bundletrack_amd.window import window_layout
    seq = S.SyntheticSequence(8, seed=5)
    fm = S.SyntheticFeatureManager(seq, corr_per_pair=120)
    frames = _frames(range(6))
    for k, f in enumerate(frames):
        fm.register(f, k)
    for i in range(6):
        for j in range(i + 1, 6):
            if (i, j) != (1, 4):                                   # one pair never matched
                fm.find_corres(frames[j], frames[i])
    ref = marshal_window(frames, fm.matches, frames[5], 5)
    lay = window_layout(ref.n_match_per_pair[None], 6, 5, 5)
    assert lay.corr_stride == len(ref.corr) > 0 and lay.max_corr_per_pair == int(ref.n_match_per_pair.max())
    assert np.array_equal(lay.pair_offsets[0], _offsets(ref.n_match_per_pair))
    assert int(lay.n_edges_newframe[0]) == ref.n_edges_newframe and bool(lay.run_ba[0]) == ref.run_ba is True
    # the restatement's marshalling gives marshal_window's bytes from the same matches as records
    recs, segs = [], []
    for i in range(6):
        for j in range(i + 1, 6):
            a, b = fm.matches.get((j, i), (np.zeros((0, 3), np.float32),) * 2)
            r = np.zeros(len(a), WR.MATCH)
            r["ptA_cam"], r["ptB_cam"] = a, b
            segs.append((sum(len(x) for x in recs), len(a)))
            recs.append(r)
    corr, off, edges, run = WR.marshal(np.concatenate(recs), segs, 6, 5, 5)
    assert corr.tobytes() == ref.corr.tobytes() and np.array_equal(off, lay.pair_offsets[0])
    assert edges == ref.n_edges_newframe and run == ref.run_ba


def test_gate_is_strictly_greater():
    from bundletrack_amd.window import window_layout
    counts = np.array([[3, 2, 7]], np.int32)                       # pairs (0,1) (0,2) (1,2); new frame 0 has 5 edges
    assert not window_layout(counts, 3, 0, 5).run_ba[0] and window_layout(counts, 3, 0, 4).run_ba[0]
    assert int(window_layout(counts, 3, 2, 5).n_edges_newframe[0]) == 9


def _layout_rc(n_windows, n_frames, counts, new_idx, outs=True):
    stride, longest = C.c_int64(-7), C.c_uint32(7)
    P = max(n_frames * (n_frames - 1) // 2, 1)
    off = np.full((max(n_windows, 1), P + 1), 7, np.uint32)
    rc = _lib.lib().btba_window_layout(n_windows, n_frames, None if counts is None else counts.ctypes.data,
                                       None if new_idx is None else new_idx.ctypes.data, 5, C.byref(stride), C.byref(longest),
                                       off.ctypes.data if outs else None, None, None)
    return rc, stride.value, off


def test_layout_einval_cases_write_nothing():
    ok_c, ok_n = np.array([1, 2, 3], np.int32), np.array([1], np.int32)
    assert _layout_rc(1, 3, ok_c, ok_n)[0] == _lib.BTBA_OK
    assert _layout_rc(1, 3, ok_c, ok_n, outs=False)[0] == _lib.BTBA_OK                   # every output is optional
    big = np.full(3, 2 ** 31 - 1, np.int32)                                               # 3 * (2^31 - 1) > 2^32 - 1
    cases = {
        "null counts": (1, 3, None, ok_n),
        "null new-frame table": (1, 3, ok_c, None),
        "negative count": (1, 3, np.array([1, -1, 3], np.int32), ok_n),
        "new frame below range": (1, 3, ok_c, np.array([-1], np.int32)),
        "new frame beyond range": (1, 3, ok_c, np.array([3], np.int32)),
        "total beyond uint32": (1, 3, big, ok_n),
        "no window": (0, 3, ok_c, ok_n),
        "one frame": (1, 1, ok_c, ok_n),
        "too many frames": (1, 86, np.zeros(86 * 85 // 2, np.int32), ok_n),
    }
    for what, args in cases.items():
        rc, stride, off = _layout_rc(*args)
        assert rc == _lib.BTBA_EINVAL, what
        assert stride == -7 and (off == 7).all(), what
    two = np.array([2 ** 31 - 1, 2 ** 31 - 1, 1], np.int32)                               # 2^32 - 1 exactly: the largest legal total
    rc, stride, off = _layout_rc(1, 3, two, ok_n)
    assert rc == _lib.BTBA_OK and stride == 2 ** 32 - 1 and int(off[0, 3]) == 2 ** 32 - 1


def test_device_calls_reject_bad_arguments_before_any_gpu_work():
    L = _lib.lib()
    seg = np.array([[0, 6]], np.int32)
    P16 = np.eye(4, dtype=np.float32).reshape(1, 16)
    out, err = np.zeros(16, np.float32), np.zeros(1, np.float32)
    call = lambda ws, n, nrec, s: L.btba_procrustes_pairs(ws, 0, n, 16, nrec, s, P16.ctypes.data, P16.ctypes.data, out.ctypes.data, err.ctypes.data, None)
    assert call(None, 1, 6, seg.ctypes.data) == _lib.BTBA_EINVAL                           # no workspace
    fake = C.c_void_p(1)                                                                   # never dereferenced: every case fails validation first
    assert call(fake, -1, 6, seg.ctypes.data) == _lib.BTBA_EINVAL
    assert call(fake, 1, -1, seg.ctypes.data) == _lib.BTBA_EINVAL
    assert call(fake, 1, 6, None) == _lib.BTBA_EINVAL
    assert call(fake, 1, 5, seg.ctypes.data) == _lib.BTBA_EINVAL                           # the segment leaves the array
    assert call(fake, 1, 6, np.array([[-1, 3]], np.int32).ctypes.data) == _lib.BTBA_EINVAL
    assert call(fake, 1, 6, np.array([[0, -3]], np.int32).ctypes.data) == _lib.BTBA_EINVAL
    assert call(fake, 0, 6, None) == _lib.BTBA_OK                                          # n_pairs == 0: a no-op
    m = lambda ws, nw, nf, rec, nrec, sg, stride, corr, off: L.btba_marshal_windows(ws, nw, nf, rec, nrec, sg, 4, stride, corr, off, None)
    assert m(None, 1, 3, 16, 6, 16, 8, 16, 16) == _lib.BTBA_EINVAL
    for bad in [(fake, 0, 3, 16, 6, 16, 8, 16, 16), (fake, 1, 1, 16, 6, 16, 8, 16, 16), (fake, 1, 86, 16, 6, 16, 8, 16, 16),
                (fake, 1, 3, None, 6, 16, 8, 16, 16), (fake, 1, 3, 16, -1, 16, 8, 16, 16), (fake, 1, 3, 16, 6, None, 8, 16, 16),
                (fake, 1, 3, 16, 6, 16, 0, 16, 16), (fake, 1, 3, 16, 6, 16, 8, None, 16), (fake, 1, 3, 16, 6, 16, 8, 16, None),
                (fake, 1, 3, 8, 6, 16, 8, 16, 16), (fake, 1, 3, 16, 6, 16, 8, 8, 16)]:
        assert m(*bad) == _lib.BTBA_EINVAL, bad


# ---- the restatement itself ----------------------------------------------------------------------------------------------

def _planted(rng, n, noise=0.0, scale=0.05):
    """n records whose model-frame points satisfy b = R a + t (+ noise): ptA_cam = a, ptB_cam = b under identity poses."""
    a = rng.normal(scale=scale, size=(n, 3)) + rng.normal(scale=0.3, size=3)
    w = rng.normal(size=3)
    R = S.so3_exp(w / np.linalg.norm(w) * rng.uniform(0.01, 3.0))
    t = rng.normal(scale=0.2, size=3)
    b = a @ R.T + t + rng.normal(scale=noise, size=(n, 3)) if noise else a @ R.T + t
    rec = np.zeros(n, WR.MATCH)
    rec["ptA_cam"], rec["ptB_cam"] = a, b
    return rec, R, t


def test_slot_tree_sum_is_a_correct_sum_in_the_documented_order():
    rng = np.random.default_rng(3)
    for n in (1, 5, 255, 256, 257, 1000, 5000):
        x = rng.normal(size=n) * 10.0 ** rng.integers(-3, 3, size=n)
        got = float(WR.slot_tree_sum(x))
        assert abs(got - math.fsum(x)) <= 2.0 ** -52 * np.abs(x).sum() * 16       # <= log2(256) + n / 256 roundings deep: far inside
        acc = [0.0] * 256                                                          # the order, in plain Python
        for k, v in enumerate(x):
            acc[k % 256] = acc[k % 256] + float(v)
        s = 128
        while s >= 1:
            for l in range(s):
                acc[l] = acc[l] + acc[l + s]
            s //= 2
        assert got == acc[0]


def test_kabsch_recovers_planted_transforms():
    rng = np.random.default_rng(7)
    I = np.eye(4, dtype=np.float32)
    for n in (5, 6, 64, 300, 1000):
        rec, R, t = _planted(rng, n)
        out = WR.procrustes(rec, I, I)
        assert out["well_conditioned"]
        assert np.abs(out["pose64"][:3, :3] - R).max() < 2e-5 and np.abs(out["pose64"][:3, 3] - t).max() < 2e-5      # fp32 points
        assert out["err"] < 1e-6
        assert np.linalg.det(out["pose64"][:3, :3]) > 0
    rec, _, _ = _planted(rng, 4)
    out = WR.procrustes(rec, I, I)
    assert np.array_equal(out["pose"], I) and out["err"] == 0.0 and out["moments"][0] == 4 and not out["moments"][1:].any()


def test_kabsch_never_returns_a_reflection_on_mirrored_planar_sets():
    rng = np.random.default_rng(9)
    I = np.eye(4, dtype=np.float32)
    for _ in range(20):
        n = int(rng.integers(5, 200))
        a = np.concatenate([rng.normal(scale=0.1, size=(n, 2)), np.zeros((n, 1))], 1)         # a plane
        b = a * np.array([1.0, -1.0, 1.0])                                                    # its mirror image
        w = rng.normal(size=3)
        Q = S.so3_exp(w)
        rec = np.zeros(n, WR.MATCH)
        rec["ptA_cam"], rec["ptB_cam"] = a @ Q.T, b @ Q.T + 0.1
        out = WR.procrustes(rec, I, I)
        R = out["pose64"][:3, :3]
        assert np.linalg.det(R) > 0.999999 and np.abs(R.T @ R - np.eye(3)).max() < 1e-12
        assert np.isfinite(out["pose"]).all()


def test_reference_alone_stays_inside_the_pose_bar():
    """The bar of tests/test_gpu_window.py is |d| <= 4 * 2^-24 * max(1, |x|) against the restatement's fp64 pose: one fp32 rounding
    with a 4x margin.  The restatement's own fp64 error must be negligible against it on well-conditioned input (second singular
    value >= 1e-3 of the first): two fp64 routes to the optimum -- the SVD of S and the SVD of S rotated by a random rotation,
    rotated back -- agree to 1e-11, five orders of magnitude inside the bar (2.4e-7)."""
    rng = np.random.default_rng(13)
    I = np.eye(4, dtype=np.float32)
    worst = 0.0
    for n in (5, 7, 50, 400, 1000):
        for noise in (0.0, 0.002):
            rec, _, _ = _planted(rng, n, noise=noise)
            out = WR.procrustes(rec, I, I)
            assert out["well_conditioned"]
            mom = out["moments"].copy()
            Q = S.so3_exp(rng.normal(size=3))
            rot = mom.copy()
            rot[7:16] = (mom[7:16].reshape(3, 3) @ Q.T).reshape(9)                           # b -> Q b: the optimum becomes Q R
            rot[4:7] = Q @ mom[4:7]
            R2, t2, _, _ = WR.kabsch(rot)
            R, t = out["pose64"][:3, :3], out["pose64"][:3, 3]
            worst = max(worst, np.abs(Q.T @ R2 - R).max(), np.abs(Q.T @ t2 - t).max())
    print(f"restatement, two fp64 routes: worst difference {worst:.3e}")
    assert worst < 1e-11
