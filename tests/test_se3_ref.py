"""tests/se3_ref.py (the float64 SE(3) truth of tests/test_gpu_device_math.py) against mpmath at 50 digits and against the CPU oracle
(bit-exact with the reference's own LieDerivUtil.h, tests/test_oracle_vs_reference.py)."""
import mpmath
import numpy as np

import se3_ref as R

mp = mpmath.mp


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def _random_axes(rng, n):
    a = rng.normal(size=(n, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _cases(rng):
    """axis-angle x translation over every branch of the fp32 helpers: zero, tiny, the series thresholds, the cancellation band, up to pi"""
    thetas = np.concatenate([[0.0, 1e-30, 1e-12, 5e-5, 1e-4, 1e-3, 2e-3, 1e-2, 3e-2, 0.1, 1.0, 2.0, 3.0, np.pi - 1e-3, np.pi - 1e-6],
                             10.0 ** rng.uniform(-8, 0.49, 200)])
    thetas = np.minimum(thetas, np.pi - 1e-7)
    rot = _random_axes(rng, len(thetas)) * thetas[:, None]
    trans = _random_axes(rng, len(thetas)) * (10.0 ** rng.uniform(-3, 1, len(thetas)))[:, None]
    return rot, trans


def _mp_twist(rot, trans):
    w, t = [mp.mpf(float(v)) for v in rot], [mp.mpf(float(v)) for v in trans]
    return mp.matrix([[0, -w[2], w[1], t[0]], [w[2], 0, -w[0], t[1]], [-w[1], w[0], 0, t[2]], [0, 0, 0, 0]])


def test_exp_and_log_against_mpmath():
    """Exp against mpmath's expm of the 4x4 twist, Log against its logm (principal branch, theta < pi), and Log(Exp(x)) = x up to
    within 1e-6 of pi, where the axis comes from the symmetric part -- all at 50 digits, to a few float64 ulps of the scale."""
    mp.dps = 50
    rng = np.random.default_rng(7)
    rot, trans = _cases(rng)
    M64 = R.pose_to_matrix(rot, trans)
    worst_exp = worst_log = worst_rt = 0.0
    for k in range(len(rot)):
        E = mp.expm(_mp_twist(rot[k], trans[k]))
        Emp = np.array([[float(E[i, j]) for j in range(4)] for i in range(4)])
        scale = max(1.0, np.linalg.norm(trans[k]))
        worst_exp = max(worst_exp, np.abs(M64[k] - Emp).max() / scale)
        theta = np.linalg.norm(rot[k])
        if theta < 3.0:
            L = mp.logm(E)
            want = np.array([float(L[2, 1]), float(L[0, 2]), float(L[1, 0]), float(L[0, 3]), float(L[1, 3]), float(L[2, 3])])
            r, t = R.matrix_to_pose(Emp)
            worst_log = max(worst_log, np.abs(np.concatenate([r, t]) - want).max() / scale)
        r, t = R.matrix_to_pose(Emp)
        worst_rt = max(worst_rt, np.abs(r - rot[k]).max(), np.abs(t - trans[k]).max() / scale)
    print(f"se3_ref vs mpmath: Exp {worst_exp:.1e}, Log {worst_log:.1e}, Log(Exp) - x {worst_rt:.1e} (relative to max(1, |t|))")
    assert worst_exp < 1e-14 and worst_log < 1e-13
    assert worst_rt < 1e-13


def test_exactly_pi_and_identity():
    for ax in np.eye(3):
        for sgn in (1.0, -1.0):
            rot = sgn * np.pi * ax
            r = R.ln_rotation(R.exp_rotation(rot))
            assert abs(np.linalg.norm(r) - np.pi) < 1e-15 and abs(abs(r @ ax) - np.pi) < 1e-15      # +pi n and -pi n are the same rotation
    r, t = R.matrix_to_pose(np.eye(4))
    assert not r.any() and not t.any()
    assert np.array_equal(R.pose_to_matrix(np.zeros(3), np.zeros(3)), np.eye(4))


def test_against_the_cpu_oracle(oracle):
    """The oracle's fp32 Exp / Log / update / inverse lie within a few fp32 ulps of the truth where the fp32 formulas are well
    conditioned (theta outside the 1 - 2 shtot cancellation band and away from pi)."""
    rng = np.random.default_rng(8)
    thetas = np.concatenate([10.0 ** rng.uniform(-6, -3.5, 60), rng.uniform(0.05, 2.8, 140)])
    rot = (_random_axes(rng, len(thetas)) * thetas[:, None]).astype(np.float32)
    trans = (_random_axes(rng, len(thetas)) * (10.0 ** rng.uniform(-3, 1, len(thetas)))[:, None]).astype(np.float32)
    worst = {}
    for k in range(len(rot)):
        M32 = oracle.pose_to_matrix(rot[k], trans[k])
        M64 = R.pose_to_matrix(rot[k].astype(np.float64), trans[k].astype(np.float64))
        ts = max(1.0, float(np.linalg.norm(trans[k])))
        e_R = np.abs(M32[:3, :3] - M64[:3, :3]).max() / _ulp(1.0)
        e_t = np.abs(M32[:3, 3] - M64[:3, 3]).max() / _ulp(ts)
        r32, t32 = oracle.matrix_to_pose(M32)
        r64, t64 = R.matrix_to_pose(M32.astype(np.float64))
        e_r = np.abs(r32 - r64).max() / _ulp(max(thetas[k], 1e-30))
        e_l = np.abs(t32 - t64).max() / _ulp(ts)
        Mi = oracle.mat4_inverse(M32)
        e_i = np.abs(Mi - R.mat_inverse(M32.astype(np.float64))).max() / _ulp(ts)
        for name, e in (("exp.R", e_R), ("exp.t", e_t), ("log.rot", e_r), ("log.trans", e_l), ("inverse", e_i)):
            worst[name] = max(worst.get(name, 0.0), float(e))
    # the update at the solver's operating point
    d = rng.normal(size=(100, 6)) * 10.0 ** rng.uniform(-4, -2, (100, 1))
    for k in range(len(d)):
        x = np.concatenate([rot[k], trans[k]]).astype(np.float32)
        nW, nT = oracle.lie_update(d[k, :3], d[k, 3:], x[:3], x[3:])
        d32 = d[k].astype(np.float32).astype(np.float64)
        r64, t64 = R.update(d32[:3], d32[3:], x[:3].astype(np.float64), x[3:].astype(np.float64))
        worst["update.rot"] = max(worst.get("update.rot", 0.0), float(np.abs(nW - r64).max() / _ulp(max(1e-3, np.linalg.norm(r64)))))
        worst["update.trans"] = max(worst.get("update.trans", 0.0), float(np.abs(nT - t64).max() / _ulp(max(1.0, np.linalg.norm(t64)))))
    print("oracle vs se3_ref, worst fp32 ulps of scale:", {k: round(v, 2) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 6, (k, v)
