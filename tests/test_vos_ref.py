"""The mask propagation (btba_vos_*) on the CPU: the numpy restatement (tests/vos_ref.py) against the reference's own numbers
(tests/golden/vos/vos_reference.npz) under the measured bars, sample_frames in Python, through the C ABI and in a stand-alone C++
program against the reference's lists, both interpolations against torch's, the ring-index rule and the label compaction.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bundletrack_amd import _lib
from bundletrack_amd import vos

import vos_ref as V


@pytest.fixture(scope="module")
def golden():
    return V.load_golden()


def _cases(golden):
    for name, Hd, Wd, H, W, Cn, d, scale, idxs in V.GROUPS:
        feats = V.features(golden[f"{name}_q"], golden[f"{name}_mult"])
        labels, tol = golden[f"{name}_labels"], float(golden[f"tol_{name}"])
        for k, f in enumerate(idxs):
            sel, n_dense = V.sample_frames(f)
            yield name, f, feats[sel], labels[sel], feats[f], n_dense, Hd, Wd, golden[f"{name}_pred"][k], tol


def test_restatement_and_reference_inside_the_measured_bars(golden):
    """fp32 restatement and the reference's stored fp32 result against the fp64 restatement: error within tol = 4 err_ref of the
    group, arg-max equal wherever the fp64 margin is at least 2 tol, at most 2 % of a case under that margin."""
    n = 0
    for name, f, refs, labels, tgt, n_dense, Hd, Wd, pred_ref, tol in _cases(golden):
        p64 = V.predict(refs, labels, tgt, n_dense, Hd, Wd)
        p32 = V.predict(refs, labels, tgt, n_dense, Hd, Wd, dtype=np.float32)
        assert p32.dtype == np.float32
        for what, pred in (("restatement", p32), ("reference", pred_ref)):
            err, ok = V.check(pred, p64, tol)
            assert ok, (name, f, what, err, tol)
        n += 1
    assert n == sum(len(g[-1]) for g in V.GROUPS) == 13


def test_golden_tolerances_are_those_of_fp32_rounding(golden):
    """A wrong sigma, frame or softmax axis is off by 1e-2 or more: the stored bars are orders below that, and a swapped sigma
    is far outside them."""
    for name, *_ in V.GROUPS:
        assert 1e-7 < float(golden[f"tol_{name}"]) < 1e-3
    name, f, refs, labels, tgt, n_dense, Hd, Wd, pred_ref, tol = [c for c in _cases(golden) if c[1] == 17][0]
    swapped = V.predict(refs, labels, tgt, n_dense, Hd, Wd, sigma_dense=21.0, sigma_sparse=8.0)
    assert V.rel_err(pred_ref, swapped) > 1e-2


@pytest.mark.parametrize("ref_num,rng", V.SAMPLE_CONFIGS)
def test_sample_frames_equal_the_reference(golden, ref_num, rng, tmp_path):
    tab = golden[f"sample_{ref_num}_{rng}"]
    want = [row[row >= 0].tolist() for row in tab]
    prm = dict(ref_num=ref_num, range=rng)
    exe = _host_program()
    out = subprocess.run([exe, str(ref_num), str(rng), "300"], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 300
    for f in range(1, 301):
        py, py_dense = V.sample_frames(f, ref_num, rng)
        lib_idx, lib_dense = vos.sample_frames(f, prm)
        cpp = [int(v) for v in out[f - 1].split()]
        dense = min(4, len(want[f - 1])) if f > 15 else len(want[f - 1])
        assert py == want[f - 1] and lib_idx == want[f - 1] and cpp[2:] == want[f - 1] and cpp[0] == f, f
        assert py_dense == lib_dense == cpp[1] == dense, f


def _host_program():
    exe = _lib.build_driver("vos_host", shared=False)
    return exe


def test_sample_frames_refusals():
    L = _lib.lib()
    idx = np.zeros(64, np.int32)
    n, nd = C.c_int32(), C.c_int32()
    ok = _lib.vos_params()
    assert L.btba_vos_sample_frames(C.byref(ok), 20, idx.ctypes.data, C.byref(n), C.byref(nd)) == _lib.BTBA_OK
    assert L.btba_vos_sample_frames(C.byref(ok), 0, idx.ctypes.data, C.byref(n), C.byref(nd)) == _lib.BTBA_EINVAL
    assert L.btba_vos_sample_frames(None, 20, idx.ctypes.data, C.byref(n), C.byref(nd)) == _lib.BTBA_EINVAL
    assert L.btba_vos_sample_frames(C.byref(ok), 20, None, C.byref(n), C.byref(nd)) == _lib.BTBA_EINVAL
    for bad in (dict(ref_num=2), dict(ref_num=33), dict(range=-1), dict(continuous_frames=0), dict(sparse_after=-1), dict(sigma_dense=0.0),
                dict(sigma_sparse=-1.0), dict(temperature=float("nan"))):
        assert L.btba_vos_sample_frames(C.byref(_lib.vos_params(**bad)), 20, idx.ctypes.data, C.byref(n), C.byref(nd)) == _lib.BTBA_EINVAL, bad


def test_defaults():
    p = _lib.vos_params()
    assert {k: getattr(p, k) for k in V.DEFAULTS} == V.DEFAULTS


@pytest.mark.parametrize("H,W", [(52, 68), (64, 64), (8, 8)])
def test_interpolations_equal_torch(golden, H, W):
    """Both directions within 1e-6 absolute of torch's interpolate on the CPU (values in [0, 1], four fp32 weight products)."""
    k = f"interp_{H}x{W}_"
    Hd, Wd = V.grid_of(H, W)
    assert (Hd, Wd) == (-(-H // 8), -(-W // 8)) == vos.grid_of(H, W)
    down = V.first_labels(golden[k + "label"], 3)
    assert down.shape == golden[k + "down"].shape and np.abs(down - golden[k + "down"]).max() <= 1e-6
    cls, up = V.masks(golden[k + "pred"], Hd, Wd, H, W)
    assert up.shape == golden[k + "up"].shape and np.abs(up - golden[k + "up"]).max() <= 1e-6
    ok, left = V.decisions_ok(cls, golden[k + "up"].reshape(3, -1).astype(np.float64), 1e-6)
    assert ok and left <= 0.02 * H * W


@pytest.mark.parametrize("ref_num,rng", V.SAMPLE_CONFIGS)
def test_ring_holds_every_sampled_frame(ref_num, rng):
    """Every index sampled for frame_idx <= 300 lies within the last range + 5 frames, so its ring slot has not been reused (the
    target itself takes slot frame_idx % (range + 5))."""
    slots = rng + 5
    for f in range(1, 301):
        idx, _ = V.sample_frames(f, ref_num, rng)
        assert min(idx) >= max(0, f - rng - 4) and max(idx) < f
        assert len({i % slots for i in idx} | {f % slots}) == len(idx) + 1


def test_compaction_keeps_the_foreground_map():
    """A 0 / 255 label image carried as 256 classes (254 of them empty) and compacted to two give the same class-0 / foreground map."""
    Hd, Wd, H, W, Cn = 7, 9, 52, 68, 8
    img = (V.label_image(H, W, 2, 0, seed=5) * 255).astype(np.uint8)
    small, vals = V.compact_labels(img)
    assert vals.tolist() == [0, 255] and set(np.unique(small)) == {0, 1}
    q, mult, lab2 = V.make_history(77, Hd, Wd, H, W, Cn, 2, 4)
    feats = V.features(q, mult)
    wide = V.first_labels(img, 256).reshape(256, -1)
    narrow = V.first_labels(small, 2).reshape(2, -1)
    assert np.array_equal(wide[[0, 255]], narrow) and not wide[1:255].any()
    lab256 = np.zeros((3, 256, Hd * Wd), np.float32)
    lab256[:, [0, 255]] = lab2[:3]
    lab256[0], lab2[0] = wide, narrow
    p256 = V.predict(feats[:3], lab256, feats[3], 3, Hd, Wd, dtype=np.float32)
    p2 = V.predict(feats[:3], lab2[:3], feats[3], 3, Hd, Wd, dtype=np.float32)
    assert not p256[1:255].any()
    assert np.array_equal(np.argmax(p256, 0) == 255, np.argmax(p2, 0) == 1) and (np.argmax(p2, 0) == 1).any() and (np.argmax(p2, 0) == 0).any()


def test_bundler_hook_is_off_by_default():
    from bundletrack_amd.bundler import Bundler
    b = Bundler(None, None, np.eye(3), 48, 64)
    assert b.segmenter is None and b.mask_propagator is None
    with pytest.raises(ValueError):
        Bundler(None, None, np.eye(3), 48, 64, segmenter=lambda x: x)
