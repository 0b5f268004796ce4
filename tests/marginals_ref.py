"""The rule of btba_pose_covariances (include/btba.h) restated in numpy fp64, the fixed synthetic matrices its tests share, and the bar they
are held to.

The rule: widen the fp32 matrix (its LOWER triangle) to fp64; Cholesky H = L L^T over the unknowns in their public order, where the pivot
of unknown j is d_j = H_jj - sum_{k<j} L_jk^2 and the factorisation stops at the first j whose d_j is not > 0 or not finite with status
1 + j; M = L^-1; Sigma = M^T M; pivot_ratio = min_j d_j / H_jj.  On a stop every covariance is NaN and pivot_ratio is 0.  Frame 0 is fixed:
its 6 x 6 block is zero and it has no rows in the matrix.  The device sums in another order (four interleaved chains), so the two agree to
rounding, not in bits; both are held to the inverse numpy computes.

The bar: a backward-stable inverse X of H satisfies, to first order, |X - H^-1| <= c u kappa_2(H) ||H^-1||_2 entrywise with u = 2^-53 and a
modest c that grows with the dimension; the tests take c = na.  kappa_2 and the norm come from numpy on the fp32 matrix widened to fp64 --
the reference is the inverse of THAT matrix, so the cast is not part of the error.  Nothing in the bar is measured on the code under test."""
import numpy as np

WINDOWS = (2, 3, 12, 31)             # frames: na = 6, 12, 66 (crosses a wave) and 180 (the limit)
KAPPAS = (1e1, 1e3, 1e5)
SEED = 20261020
KAPPA_CAP = 1e6                      # condition on the inputs: the bar is a first-order bound


def unknowns(n_frames):
    return 6 * (n_frames - 1)


def synthetic(n_frames, kappa, seed=SEED):
    """H = Q diag(lambda) Q^T with lambda log-spaced over 1 .. kappa, symmetrised, cast to fp32."""
    na = unknowns(n_frames)
    rng = np.random.default_rng([seed, n_frames, int(round(np.log10(kappa)))])
    Q, _ = np.linalg.qr(rng.standard_normal((na, na)))
    H = (Q * np.logspace(0.0, np.log10(kappa), na)) @ Q.T
    return (0.5 * (H + H.T)).astype(np.float32)


def synthetic_set():
    """The twelve matrices: {(n_frames, kappa): H float32 [na, na]}."""
    return {(n, k): synthetic(n, k) for n in WINDOWS for k in KAPPAS}


def reference(H32):
    """(inverse, kappa_2, entrywise bar, relative bar of pivot_ratio) of the fp32 matrix widened to fp64, all from numpy."""
    H = np.asarray(H32, np.float64)
    H = np.tril(H) + np.tril(H, -1).T                  # what the rule reads
    inv = np.linalg.inv(H)
    kappa = float(np.linalg.cond(H, 2))
    na = H.shape[0]
    u = 2.0 ** -53
    return inv, kappa, na * u * kappa * float(np.linalg.norm(inv, 2)), na * u * kappa


def zero_frame(H32, frame):
    """The matrix with frame `frame`'s (>= 1) six rows and columns zeroed: nothing constrains that frame."""
    H = np.array(H32, np.float32)
    s = slice(6 * (frame - 1), 6 * frame)
    H[s, :] = 0.0
    H[:, s] = 0.0
    return H


def blocks_of(full, n_frames):
    """[N, 6, 6]: the diagonal blocks of a full [na, na] matrix behind frame 0's zero block."""
    out = np.zeros((n_frames, 6, 6), full.dtype)
    for k in range(1, n_frames):
        out[k] = full[6 * (k - 1):6 * k, 6 * (k - 1):6 * k]
    return out


def pose_covariances(H32):
    """The rule on one matrix.  Returns dict(blocks [N, 6, 6], full [na, na], pivot_ratio, status)."""
    H = np.asarray(H32, np.float64)
    na = H.shape[0]
    n_frames = na // 6 + 1
    L = np.zeros((na, na))
    d = np.zeros(na)
    status = 0
    with np.errstate(all="ignore"):
        for j in range(na):
            d[j] = H[j, j] - L[j, :j] @ L[j, :j]
            if not (d[j] > 0.0) or not np.isfinite(d[j]):
                status = 1 + j
                break
            L[j, j] = np.sqrt(d[j])
            L[j + 1:, j] = (H[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    if status:
        return dict(blocks=np.full((n_frames, 6, 6), np.nan), full=np.full((na, na), np.nan), pivot_ratio=0.0, status=status)
    M = np.zeros((na, na))
    for j in range(na - 1, -1, -1):                    # columns from the last to the first, as the kernel does
        M[j, j] = 1.0 / L[j, j]
        if j + 1 < na:
            M[j + 1:, j] = -(M[j + 1:, j + 1:] @ L[j + 1:, j]) / L[j, j]
    full = M.T @ M
    full = np.tril(full) + np.tril(full, -1).T         # one value per pair of unknowns, written to both triangles
    return dict(blocks=blocks_of(full, n_frames), full=full, pivot_ratio=float(np.min(d / np.diag(H))), status=0)


# ---- the solver's internal [trans, rot] order <-> the public (rot, trans) order ------------------------------------------------------
def public_index(n_frames):
    """For every public unknown (frames 1 .. N - 1, (rot, trans) per frame) its index in the traced 6N x 6N system ([trans, rot] per frame, frame 0 first)."""
    idx = []
    for k in range(1, n_frames):
        idx += [6 * k + 3, 6 * k + 4, 6 * k + 5, 6 * k, 6 * k + 1, 6 * k + 2]
    return np.asarray(idx)


def info_from_trace(A, n_frames):
    """The public matrix out of a traced A [6N, 6N]."""
    p = public_index(n_frames)
    return np.ascontiguousarray(A[np.ix_(p, p)])


def rhs_from_trace(rhs):
    """The public right-hand side out of a traced rhs [N, 6] (traced in the public order): frames 1 .. N - 1."""
    return np.ascontiguousarray(rhs[1:])
