"""The rule of btba_pose_covariances on the CPU (tests/marginals_ref.py): the numpy restatement against np.linalg.inv on the fixed synthetic
set, the breakdown rule, the order permutation, and what of the two new entry points can be checked without a GPU (the symbols, and the
argument checks that come before any HIP call).  The device runs the same matrices in tests/test_gpu_marginals.py."""
import ctypes as C

import numpy as np
import pytest

import marginals_ref as MR
from bundletrack_amd import _lib

SET = MR.synthetic_set()


def test_inputs_meet_the_condition_cap():
    """kappa_2 of every cast matrix is <= 1e6 (the bar is a first-order bound); the twelve measure 10 ... 1e5."""
    for (n, k), H in SET.items():
        _, kappa, _, _ = MR.reference(H)
        print(f"n_frames {n} kappa {k:g}: kappa_2 of the cast matrix {kappa:.4g}")
        assert kappa <= MR.KAPPA_CAP
        assert 0.5 * k <= kappa <= 2.0 * k
        assert np.array_equal(H, H.T) and H.dtype == np.float32 and H.shape == (MR.unknowns(n),) * 2


@pytest.mark.parametrize("key", sorted(SET), ids=[f"N{n}-kappa{k:g}" for n, k in sorted(SET)])
def test_restatement_against_numpy_inverse(key):
    H = SET[key]
    inv, kappa, bar, ratio_bar = MR.reference(H)
    out = MR.pose_covariances(H)
    assert out["status"] == 0
    err = float(np.abs(out["full"] - inv).max())
    print(f"n_frames {key[0]} kappa_2 {kappa:.4g}: max |restatement - inv| {err:.3e}, bar {bar:.3e}, ratio {err / bar:.4f}; pivot_ratio {out['pivot_ratio']:.4g}")
    assert err <= bar
    assert np.abs(out["blocks"] - MR.blocks_of(inv, key[0])).max() <= bar
    assert np.array_equal(out["full"], out["full"].T)
    assert np.array_equal(out["blocks"], MR.blocks_of(out["full"], key[0])) and not out["blocks"][0].any()
    # min_j d_j / H_jj: between 1 / kappa_2 (d_j >= lambda_min, H_jj <= lambda_max) and 1 (d_j <= H_jj)
    assert 1.0 / kappa * (1 - ratio_bar) <= out["pivot_ratio"] <= 1.0


@pytest.mark.parametrize("n_frames,frame", [(2, 1), (3, 1), (3, 2), (12, 1), (12, 7), (12, 11), (31, 30)])
def test_breakdown_names_the_first_unknown_of_an_unconstrained_frame(n_frames, frame):
    out = MR.pose_covariances(MR.zero_frame(SET[(n_frames, 1e3)], frame))
    assert out["status"] == 1 + 6 * (frame - 1)
    assert np.isnan(out["full"]).all() and np.isnan(out["blocks"]).all() and out["pivot_ratio"] == 0.0


def test_breakdown_on_indefinite_and_non_finite_input():
    H = SET[(3, 1e1)].copy()
    H[4, 4] = -1.0
    assert MR.pose_covariances(H)["status"] == 5
    for bad in (np.nan, np.inf):
        H = SET[(3, 1e1)].copy()
        H[7, 7] = bad
        assert MR.pose_covariances(H)["status"] == 8


def test_public_order_permutation():
    """[trans, rot] per frame with frame 0 first -> (rot, trans) per frame without frame 0."""
    N = 4
    n = 6 * N
    A = np.arange(n * n, dtype=np.float32).reshape(n, n)
    info = MR.info_from_trace(A, N)
    assert info.shape == (18, 18)
    assert info[0, 0] == A[9, 9] and info[3, 0] == A[6, 9] and info[0, 5] == A[9, 8] and info[6, 17] == A[15, 20]
    p = MR.public_index(N)
    assert sorted(p.tolist()) == list(range(6, n))
    rhs = np.arange(6 * N, dtype=np.float32).reshape(N, 6)
    assert np.array_equal(MR.rhs_from_trace(rhs), rhs[1:])


def test_new_symbols_resolve_and_are_declared():
    L = _lib.lib()
    for name in ("btba_linearize_batch_zn_aux", "btba_pose_covariances"):
        assert hasattr(L, name) and name in _lib.declared_symbols() and name in _lib.EXPORTED_SYMBOLS
    assert L.btba_version() == 105


def test_argument_checks_before_any_hip_call():
    """Both entry points refuse a NULL workspace and bad sizes with BTBA_EINVAL without touching the device (the checks against a live workspace:
    tests/test_gpu_marginals.py)."""
    L = _lib.lib()
    hip_error = L.btba_last_hip_error()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    for n_frames, stride in ((1, 36), (32, 186 * 186), (2, 35), (2, 36)):
        assert L.btba_pose_covariances(None, 1, n_frames, p, stride, p, None, None, p) == _lib.BTBA_EINVAL
    prm = _lib.default_params()
    w = np.ones(7, np.float32)
    prm.weights_sparse_per_iter = w.ctypes.data
    prm.n_weights_per_iter = 7
    assert L.btba_linearize_batch_zn_aux(None, C.byref(prm), 1, 2, 64, 64, p, p, None, None, 1, None, 0, None, 0, p, p, None) == _lib.BTBA_EINVAL
    assert L.btba_last_hip_error() == hip_error
