"""The NOCS evaluation (btba_nocs_errors) on the CPU: the restatement tests/cpp/nocs_host.cpp against the reference scorer's own
numbers (tests/golden/nocs/nocs_reference.npz, and live where the reference checkout exists), the contract's special cases, the
report by hand, the pose files.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from bundletrack_amd import _lib
from bundletrack_amd.nocs_eval import (NOCS_CLASSES, load_model_scales, load_nocs_pose_txt, nocs_report, nocs_report_experiments,
                                       save_nocs_pose_txt)

import nocs_ref as N


def test_symbols_declared_and_exported():
    for name in ("btba_nocs_params_default", "btba_nocs_errors"):
        assert name in _lib.declared_symbols() and name in _lib.EXPORTED_SYMBOLS
    p = _lib.nocs_params()
    assert (p.rot_thresh_deg, p.shift_thresh, p.iou_thresh) == (5.0, 50.0, 0.25)
    assert (p.n_sym_steps, p.flip_z180_pred, p.normalize_columns, p.clamp_acos) == (20, 1, 1, 0)
    assert C.sizeof(_lib.NocsParams) == 40


def test_null_workspace_rejected():
    box = np.zeros((1, 8, 3))
    P = np.eye(4).reshape(1, 16).copy()
    o = np.zeros(1)
    one = np.ones(1, np.int32)
    zero = np.zeros(1, np.int32)
    assert _lib.lib().btba_nocs_errors(None, None, 0, 1, box.ctypes.data, 1, one.ctypes.data, None, zero.ctypes.data, P.ctypes.data,
                                       P.ctypes.data, o.ctypes.data, o.ctypes.data, o.ctypes.data) == _lib.BTBA_EINVAL


def test_restatement_against_reference_vectors():
    cs, ref = N.load_golden()
    assert len(ref[0]) >= 240 and ref[0].min() >= 0.05
    N.assert_close(N.restate_cases(cs), ref, "restatement vs reference vectors")


def test_reference_vectors_cover_the_cases():
    cs, (theta, shift, iou) = N.load_golden()
    cid, hv = cs["class_id"], cs["handle_visible"]
    assert set(cid) == {1, 2, 3, 4, 5, 6} and set(hv[cid == 6]) == {0, 1}
    assert np.count_nonzero(iou == 0.0) >= 10
    # the turned bottles: one symmetry step (the unrotated ground truth) scores well below the 20-step maximum
    one = N.restate_cases(cs, n_sym_steps=1)[2]
    assert np.count_nonzero((cid == 1) & (iou > one + 0.1)) >= 10
    assert os.path.getsize(N.GOLDEN) < 100 * 1024


def test_restatement_against_live_reference():
    bm = N.reference_module()
    if bm is None:
        pytest.skip("no reference checkout")
    cs = N.make_cases(1000, 77)
    N.assert_close(N.restate_cases(cs), N.reference_eval(bm, cs), "restatement vs live reference")


def test_identical_poses():
    cs = N.make_cases(200, 5)
    pred = N.Z180 @ cs["gt"]                              # the flip gives the ground truth back, bit for bit
    t, s, u = N.restate(cs["boxes"], cs["class_id"], cs["box_index"], pred, cs["gt"], cs["handle_visible"], clamp_acos=1)
    assert np.all(t <= 2e-5) and np.all(s == 0.0) and np.all(u == 1.0)           # theta <= sqrt(2 eps) rad
    t, s, u = N.restate(cs["boxes"], cs["class_id"], cs["box_index"], pred, cs["gt"], cs["handle_visible"], clamp_acos=0)
    assert np.all(np.isnan(t) | (t <= 2e-5)) and np.all(u == 1.0)
    print(f"identical poses, clamp_acos = 0: {int(np.isnan(t).sum())} of {t.size} are NaN")


def test_bad_bottom_row_and_non_finite():
    cs = N.make_cases(6, 6)
    pred, gt = cs["pred"].copy(), cs["gt"].copy()
    pred[1, 3, 3] = 2.0
    gt[2, 3, 0] = 1e-3
    pred[3, 0, 0] = np.nan
    gt[4, 2, 3] = np.inf
    t, s, u = N.restate(cs["boxes"], cs["class_id"], cs["box_index"], pred, gt, cs["handle_visible"])
    clean = N.restate_cases(cs)
    for e in (1, 2):
        assert t[e] == 10000.0 and s[e] == 10000.0 and np.isnan(u[e])
    for e in (3, 4):
        assert np.isnan(t[e]) and np.isnan(s[e]) and np.isnan(u[e])
    for e in (0, 5):
        assert (t[e], s[e], u[e]) == (clean[0][e], clean[1][e], clean[2][e])


def test_nan_step_is_never_taken():
    cs = N.nan_iou_cases()
    t, s, u = N.restate_cases(cs)
    assert u[0] == 0.0 and np.isnan(u[1]) and np.isfinite(t).all() and np.all(s == 0.0)


def test_report_by_hand():
    #            bottle: hit, miss by angle, miss by shift    camera: hit, NaN theta (counts nowhere but IoU), far off
    theta = np.array([1.0, 7.0, 2.0, 4.0, np.nan, 400.0])
    shift = np.array([10.0, 20.0, 60.0, 49.0, 5.0, 30.0])
    iou = np.array([0.5, 0.3, 0.2, 0.26, 0.9, 0.4])
    cid = np.array([1, 1, 1, 3, 3, 3])
    rep = nocs_report(theta, shift, iou, cid)
    b, c = rep["bottle"], rep["camera"]
    assert b["n"] == 3 and b["acc_5deg5cm"] == 100 * (1 / 3) and b["acc_iou25"] == 100 * (2 / 3)
    assert b["rot_err_deg"] == (1.0 + 7.0) / 2 and b["trans_err"] == (10.0 + 20.0) / 2 and b["trans_err_cm"] == 1.5
    assert c["acc_5deg5cm"] == 100 * (1 / 3) and c["acc_iou25"] == 100.0
    assert c["rot_err_deg"] == 4.0                                    # NaN < 360 and 400 < 360 are both false
    assert c["trans_err"] == (49.0 + 5.0 + 30.0) / 3
    for name in ("bowl", "can", "laptop", "mug"):                     # no items: 0 / 0
        assert rep[name]["n"] == 0 and np.isnan(rep[name]["acc_5deg5cm"]) and np.isnan(rep[name]["rot_err_deg"])
    assert np.isnan(rep["overall"]["acc_5deg5cm"]) and rep["overall"]["n"] == 6
    # listed frames: missing predictions are misses
    rep = nocs_report(theta, shift, iou, cid, n_listed={1: 4, 2: 0, 3: 6, 4: 0, 5: 0, 6: 0})
    assert rep["bottle"]["acc_5deg5cm"] == 25.0 and rep["camera"]["acc_iou25"] == 50.0 and rep["bottle"]["rot_err_deg"] == 4.0
    # other thresholds
    rep = nocs_report(theta, shift, iou, cid, rot_thresh_deg=10.0, shift_thresh=100.0, iou_thresh=0.45)
    assert rep["bottle"]["acc_5deg5cm"] == 100.0 and rep["bottle"]["acc_iou25"] == 100 * (1 / 3) and rep["bottle"]["trans_err"] == 10.0


def test_report_overall_and_experiments():
    cs, (theta, shift, iou) = N.load_golden()
    rep = nocs_report(theta, shift, iou, cs["class_id"])
    acc = rot = 0.0
    for name in NOCS_CLASSES:
        acc = acc + (rep[name]["acc_5deg5cm"] / 100) / 6
        rot = rot + rep[name]["rot_err_deg"] / 6
    assert abs(rep["overall"]["acc_5deg5cm"] - acc * 100) < 1e-12 and rep["overall"]["rot_err_deg"] == rot
    in55, iou25 = N.decisions(theta, shift, iou)
    assert sum(round(rep[n]["acc_iou25"] * rep[n]["n"] / 100) for n in NOCS_CLASSES) == iou25.sum()
    assert sum(round(rep[n]["acc_5deg5cm"] * rep[n]["n"] / 100) for n in NOCS_CLASSES) == in55.sum()
    rep2 = nocs_report(theta[:120], shift[:120], iou[:120], cs["class_id"][:120])
    m = nocs_report_experiments([rep, rep2])
    assert m["acc_5deg5cm"] == (rep["overall"]["acc_5deg5cm"] + rep2["overall"]["acc_5deg5cm"]) / 2
    assert m["trans_err_cm"] == (rep["overall"]["trans_err_cm"] + rep2["overall"]["trans_err_cm"]) / 2


def test_cpp_report_equals_python():
    cs, (theta, shift, iou) = N.load_golden()
    theta = theta.copy()
    theta[5] = np.nan
    for kw in ({}, {"n_listed": {1: 50, 2: 41, 3: 36, 4: 60, 5: 36, 6: 37}}, {"rot_thresh_deg": 10.0, "shift_thresh": 20.0, "iou_thresh": 0.6}):
        py = N.report_rows(nocs_report(theta, shift, iou, cs["class_id"], **kw))
        cpp = N.cpp_report(theta, shift, iou, cs["class_id"], **kw)
        assert np.array_equal(py.view(np.uint64), cpp.view(np.uint64)), kw


def test_pose_file_round_trip(tmp_path):
    cs = N.make_cases(3, 9)
    for e in range(3):
        path = str(tmp_path / f"m_scene_{e}_pose.txt")
        P = cs["pred"][e]
        save_nocs_pose_txt(path, P)
        lines = open(path).read().splitlines()
        assert len(lines) == 4 and all(len(ln.split(" ")) == 3 for ln in lines)
        back = load_nocs_pose_txt(path)
        assert np.array_equal(back[:3], P[:3]) and np.array_equal(back[3], [0, 0, 0, 1])
    box = N.make_boxes(1, np.random.default_rng(1))[0]
    np.savetxt(str(tmp_path / "m.txt"), box, fmt="%.17g")
    assert np.array_equal(load_model_scales(str(tmp_path / "m.txt")), box)
