"""SE(3) in float64: the truth the device's fp32 SE(3) helpers (bundletrack_amd/csrc/btba_device.hpp) are measured against.

Vectorised over a leading axis.  Closed forms away from zero, Taylor series below THETA_SERIES (where the closed forms cancel), and the
rotation axis near pi taken from the symmetric part of R (where the antisymmetric part vanishes).  Poses are (rot, trans): rot the
axis-angle vector, trans the SE(3) log's translation part (matrix translation = V(rot) trans), as the product's pose_to_matrix /
matrix_to_pose use them.  Held against mpmath at 50 digits and against the CPU oracle by tests/test_se3_ref.py."""
import numpy as np

THETA_SERIES = 1e-2        # series through theta^10 below: truncation < 1e-22 relative


def _hat(w):
    w = np.asarray(w, np.float64)
    z = np.zeros(w.shape[:-1])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1),
                     np.stack([w[..., 2], z, -w[..., 0]], -1),
                     np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def _coeffs(theta):
    """A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3."""
    t = np.asarray(theta, np.float64)
    t2 = t * t
    small = t < THETA_SERIES
    ts = np.where(small, 1.0, t)                   # keep the closed forms finite where the series is used
    A = np.where(small, 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72 * (1 - t2 / 110)))), np.sin(ts) / ts)
    B = np.where(small, 0.5 * (1 - t2 / 12 * (1 - t2 / 30 * (1 - t2 / 56 * (1 - t2 / 90 * (1 - t2 / 132))))), (1 - np.cos(ts)) / ts ** 2)
    C = np.where(small, (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72 * (1 - t2 / 110 * (1 - t2 / 156))))) / 6, (ts - np.sin(ts)) / ts ** 3)
    return A, B, C


def exp_rotation(w):
    """Rodrigues: [..., 3] -> [..., 3, 3]."""
    w = np.asarray(w, np.float64)
    A, B, _ = _coeffs(np.linalg.norm(w, axis=-1))
    K = _hat(w)
    return np.eye(3) + A[..., None, None] * K + B[..., None, None] * (K @ K)


def pose_to_matrix(rot, trans):
    """Exp: [..., 3], [..., 3] -> [..., 4, 4]."""
    rot, trans = np.asarray(rot, np.float64), np.asarray(trans, np.float64)
    A, B, C = _coeffs(np.linalg.norm(rot, axis=-1))
    K = _hat(rot)
    K2 = K @ K
    I = np.eye(3)
    R = I + A[..., None, None] * K + B[..., None, None] * K2
    V = I + B[..., None, None] * K + C[..., None, None] * K2
    M = np.zeros(rot.shape[:-1] + (4, 4))
    M[..., :3, :3] = R
    M[..., :3, 3] = np.einsum("...ij,...j->...i", V, trans)
    M[..., 3, 3] = 1.0
    return M


def ln_rotation(R):
    """[..., 3, 3] -> axis-angle [..., 3], theta in [0, pi]; the axis near pi from the symmetric part."""
    R = np.asarray(R, np.float64)
    r = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    s = np.linalg.norm(r, axis=-1)
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)
    theta = np.arctan2(s, c)
    # theta / sin(theta) by its series where sin(theta) is tiny and theta is near zero
    t2 = theta * theta
    ratio = np.where(theta < THETA_SERIES, 1 + t2 / 6 * (1 + 7 * t2 / 60 * (1 + 31 * t2 / 294)), theta / np.where(s > 0, s, 1.0))
    out = r * ratio[..., None]
    # near pi: (R + R^T) / 2 - cos I = (1 - cos) n n^T; the column of the largest diagonal entry, signed along r
    near_pi = c < -0.5
    if np.any(near_pi):
        Rp = R[near_pi]
        S = 0.5 * (Rp + np.swapaxes(Rp, -1, -2)) - c[near_pi][..., None, None] * np.eye(3)
        j = np.argmax(np.diagonal(S, axis1=-2, axis2=-1), -1)
        col = S[np.arange(len(j)), :, j]
        n = col / np.linalg.norm(col, axis=-1, keepdims=True)
        sgn = np.where(np.einsum("...i,...i->...", n, r[near_pi]) < 0, -1.0, 1.0)
        out[near_pi] = n * (sgn * theta[near_pi])[..., None]
    return out


def matrix_to_pose(M):
    """Log: [..., 4, 4] -> (rot [..., 3], trans [..., 3]) with trans = V(rot)^-1 t."""
    M = np.asarray(M, np.float64)
    rot = ln_rotation(M[..., :3, :3])
    theta = np.linalg.norm(rot, axis=-1)
    t2 = theta * theta
    small = theta < THETA_SERIES
    ts = np.where(small, 1.0, theta)
    # V^-1 = I - K / 2 + D K^2,  D = (1 - (t / 2) cot(t / 2)) / t^2
    D = np.where(small, 1 / 12 + t2 / 720 + t2 ** 2 / 30240 + t2 ** 3 / 1209600,
                 (1 - 0.5 * ts * np.cos(0.5 * ts) / np.sin(0.5 * ts)) / ts ** 2)
    K = _hat(rot)
    Vinv = np.eye(3) - 0.5 * K + D[..., None, None] * (K @ K)
    return rot, np.einsum("...ij,...j->...i", Vinv, M[..., :3, 3])


def mat_inverse(M):
    return np.linalg.inv(np.asarray(M, np.float64))


def update(dW, dT, rot, trans):
    """The solver's update: Log(Exp(dW, dT) Exp(rot, trans))."""
    return matrix_to_pose(pose_to_matrix(dW, dT) @ pose_to_matrix(rot, trans))
