"""Pose accuracy (btba_pose_errors) on the CPU: the restatement tests/cpp/eval_host.cpp against an independent fp64 evaluation,
the invariants the contract guarantees, the VOCap closed form on worked cases, the C++ host's VOCap, and the ADD / ADD-S AUC of
the oracle-driven c1 tracking session (no GPU)."""
import ctypes as C

import numpy as np
import pytest

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S
from bundletrack_amd.evaluation import load_points_xyz, ob_in_cam, vocap_auc

from eval_ref import driver, fp64, restate, scene_poses, session_errors, symmetric_model, vocap
from helpers import OracleOptimizer


def test_symbols_declared_and_exported():
    assert "btba_pose_errors" in _lib.declared_symbols() and "btba_pose_errors" in _lib.EXPORTED_SYMBOLS


def test_null_workspace_is_rejected_before_any_gpu_work():
    x = np.zeros((4, 3), np.float32)
    ptrs = (C.c_void_p * 1)(x.ctypes.data)
    n = np.array([4], np.int32)
    mi = np.zeros(1, np.int32)
    P = np.eye(4, dtype=np.float32).reshape(1, 16)
    o = np.zeros(1, np.float32)
    assert _lib.lib().btba_pose_errors(None, 0, 1, C.cast(ptrs, C.c_void_p), n.ctypes.data, 1, mi.ctypes.data, P.ctypes.data, P.ctypes.data,
                                       o.ctypes.data, o.ctypes.data) == _lib.BTBA_EINVAL


def test_model_points_on_the_ellipsoid_and_seeded():
    p = S.model_points(500, 3)
    assert p.shape == (500, 3) and p.dtype == np.float32
    assert np.allclose(((p.astype(np.float64) / S.SEMI_AXES) ** 2).sum(1), 1.0, atol=1e-5)
    assert np.array_equal(p, S.model_points(500, 3)) and not np.array_equal(p, S.model_points(500, 4))


def test_restatement_agrees_with_fp64_reference():
    model = S.model_points(2620, 11)
    pred, gt = scene_poses(40, 12)
    add, adds = restate(model, pred, gt)
    add64, adds64 = fp64(model, pred, gt)
    assert np.abs(add - add64).max() < 2e-6 and np.abs(adds - adds64).max() < 2e-6
    assert add.max() > 1e-3 and adds.min() > 0.0               # the scenes have real errors


def test_invariants_adds_below_add_and_identity_zero():
    model = S.model_points(1000, 13)
    pred, gt = scene_poses(30, 14, rot_deg=20.0, trans_m=0.05)
    add, adds = restate(model, pred, gt)
    assert np.all(adds <= add)                                  # float compare: bit order on non-negative finite values
    a0, s0 = restate(model, gt, gt)
    assert np.all(a0 == 0.0) and np.all(s0 == 0.0)


def test_symmetric_model_gives_zero_adds():
    model = symmetric_model(700, 15)
    _, gt = scene_poses(10, 16)
    pred = gt @ np.diag([-1, 1, -1, 1]).astype(np.float32)      # negating two columns: exact in fp32
    add, adds = restate(model, pred, gt)
    assert np.all(adds == 0.0) and np.all(add > 0.01)


def test_nan_pose_gives_nan_for_its_evaluation_only():
    model = S.model_points(300, 17)
    pred, gt = scene_poses(3, 18)
    pred[1, 0, 3] = np.nan
    add, adds = restate(model, pred, gt)
    assert np.isnan(add[1]) and np.isnan(adds[1]) and np.all(np.isfinite(add[[0, 2]]))


@pytest.mark.parametrize("errors, auc", [([0.0], 1.0), ([0.1], 0.0), ([0.05, 0.05], 0.75), ([], 0.0), ([0.1, 0.2, 1.0], 0.0),
                                         ([0.02, 0.06], (0.02 * 1 / 2 + 0.04 * 2 / 2 + 0.04 * 2 / 2) / 0.1)])
def test_vocap_worked_cases(errors, auc):
    assert vocap_auc(errors) == pytest.approx(auc, abs=1e-15)
    assert vocap(errors) == pytest.approx(auc, abs=1e-15)


def test_vocap_python_and_cpp_identical_on_random_sets():
    rng = np.random.default_rng(19)
    L = driver()
    for trial in range(200):
        n = int(rng.integers(1, 300))
        e = rng.exponential(rng.uniform(0.005, 0.08), size=n)
        if trial % 3 == 0:
            e = np.round(e, 2)                                  # tie-heavy sets
        e = np.ascontiguousarray(e, np.float64)
        py = vocap_auc(e)
        assert L.vocap_driver(e.ctypes.data, n, 0.1) == py
        assert abs(vocap(e) - py) < 1e-12


def test_ob_in_cam_and_points_loader(tmp_path):
    T = S.se3_exp(np.array([0.3, -0.2, 0.1]), np.array([0.01, 0.2, 0.7]))
    M = ob_in_cam(T[None])
    assert M.dtype == np.float32 and np.abs(M[0].astype(np.float64) @ T - np.eye(4)).max() < 1e-6
    p = S.model_points(20, 1)
    np.savetxt(tmp_path / "points.xyz", p, fmt="%.9g")
    assert np.array_equal(load_points_xyz(str(tmp_path / "points.xyz")), p)


# ADD-S AUC of the oracle-driven c1 session (test_tracking_session.test_c1_sliding_window_oracle's setup), recorded on the CPU:
# ADD 99.88 / ADD-S 99.88 (x 100, mean ADD 0.13 mm).  The floor leaves room for round-off only.
C1_ORACLE_FLOOR = (99.5, 99.5)


def test_c1_oracle_session_auc(oracle, tmp_path):
    from test_tracking_session import run_session
    seq, bundler, frames, errs = run_session(OracleOptimizer(oracle), 24, tmp_path=str(tmp_path))
    add, adds = session_errors(frames, seq, S.model_points(2000, 0))
    add_auc, adds_auc = 100 * vocap_auc(add), 100 * vocap_auc(adds)
    print(f"c1 oracle session: ADD AUC {add_auc:.2f}, ADD-S AUC {adds_auc:.2f}, mean ADD {add.mean() * 1e3:.2f} mm")
    assert np.all(adds <= add)
    assert add_auc >= C1_ORACLE_FLOOR[0] and adds_auc >= C1_ORACLE_FLOOR[1]
