"""The objective report's definition on the CPU (tests/objective_ref.py): the input conditions the GPU test relies on, the objective as the
function the solver descends (its gradient is -2 x the solver's right-hand side), the floor of a float32 evaluation of the residuals in units of
the forward-error scale -- gamma of tests/test_gpu_objective.py is 4 x that floor --, mutations of the restatement that the bars must catch,
and the ABI.  The device runs the same inputs in tests/test_gpu_objective.py."""
import ctypes as C

import numpy as np
import pytest

import objective_ref as OR
import sweep_ref as R
from bundletrack_amd import _lib
from oracle import oracle_np as ONP


def test_small_scenes_have_no_borderline_pixel(oracle):
    """INPUT CONDITION of the exact count checks: at the CPU oracle's matrices no ordered pair of a small scene has a borderline pixel."""
    lo, hi = 10**9, 0
    for name in OR.SMALL_SCENES:
        sc = R.scene(name)
        T, Tinv = R.oracle_matrices(sc["poses"])
        refs = OR.scene_pairs(sc, T, Tinv, OR.ALL_PAIRS)
        counts = [r["count"] for r in refs]
        print(f"{name:11s} accepts {counts} borderline {[r['borderline'] for r in refs]}")
        assert all(r["borderline"] == 0 for r in refs), name
        if name != "edge32x24":
            lo, hi = min(lo, min(counts)), max(hi, max(counts))
    print(f"accepts per pair {lo} ... {hi}")
    assert lo > 0


@pytest.mark.parametrize("delta,what", [(10.0, "all inliers"), (1e-9, "all outliers")])
def test_objective_gradient_is_minus_twice_the_solvers_rhs(oracle, delta, what):
    """Central differences of the fp64 objective along every unknown of the solver's left perturbation T_k <- Exp(h e) T_k against -2 x
    sweep_ref.sparse_system's rhs, where the objective is smooth (every entry on one side of the knee).  No fixed tolerance: the disagreement is
    the central difference's own truncation error, so it falls 4 x when the step halves, and Richardson's extrapolation of the two removes it."""
    corr, offs, (poses_init, _), _ = OR.two_sided_case(3)
    prm = dict(robust_delta=delta)
    T = poses_init.astype(np.float64)
    N = T.shape[0]
    d32 = float(np.float32(delta))
    v = corr["imgIdx_i"] != 0xFFFFFFFF
    e = ((np.einsum("nab,nb->na", T[corr["imgIdx_i"][v].astype(int), :3, :3], corr["pos_i"][v].astype(np.float64)) + T[corr["imgIdx_i"][v].astype(int), :3, 3]
          - np.einsum("nab,nb->na", T[corr["imgIdx_j"][v].astype(int), :3, :3], corr["pos_j"][v].astype(np.float64)) - T[corr["imgIdx_j"][v].astype(int), :3, 3]) ** 2).sum(1)
    assert np.all(e <= d32 * d32) or np.all(e > d32 * d32), what
    b = R.sparse_system(corr, T, prm)["b"]          # [trans, rot] per frame

    def central(h):
        g = np.zeros(6 * N)
        for k in range(1, N):
            for a in range(6):
                w, u = np.zeros(3), np.zeros(3)
                (u if a < 3 else w)[a % 3] = h
                Tp, Tm = T.copy(), T.copy()
                Tp[k], Tm[k] = ONP.se3_exp(w, u) @ T[k], ONP.se3_exp(-w, -u) @ T[k]
                g[6 * k + a] = (OR.sparse_objective(corr, Tp, prm) - OR.sparse_objective(corr, Tm, prm)) / (2 * h)
        return g

    h = 1e-3
    g1, g2 = central(h), central(h / 2)
    e1, e2 = np.linalg.norm(g1 + 2 * b), np.linalg.norm(g2 + 2 * b)
    rich = np.linalg.norm((4 * g2 - g1) / 3 + 2 * b)
    print(f"{what}: |grad| {np.linalg.norm(2 * b):.3e}  disagreement h {e1:.3e}  h/2 {e2:.3e}  ratio {e1 / e2:.3f}  extrapolated {rich:.3e}")
    assert 3.5 < e1 / e2 < 4.5
    assert rich < e2 / 16


def test_float32_floor_and_gamma(oracle):
    f = OR.floors()
    print("float32 restatement floor in units of Sc:", {k: f"{v:.3e}" for k, v in f.items()}, "-> gamma = 4 x")
    # A float32 residual is off by a few unit round-offs of its scale rs, and Sc sums |d term / d res| rs over all terms while their errors partly
    # cancel: the floor of a SUM is a small multiple of 2^-24.  One residual alone (_res, in units of its own rs) is not bounded that way: a dense
    # residual also moves with the tap position, whose fp32 error (ulps of a coordinate of up to 275 px) is multiplied by the slope of the
    # blended surface, which rs does not see -- those two floors are measured and printed, not bounded.
    for k, v in f.items():
        assert np.isfinite(v) and v > 0, (k, v)
        if not k.endswith("_res"):
            assert v < 8 * 2.0 ** -24, (k, v)


def test_two_sided_case_populates_both_sides_of_the_knee(oracle):
    for N in (2, 3, 5):
        corr, offs, pose_sets, (p, k) = OR.two_sided_case(N)
        shares = []
        for poses in pose_sets:
            T, _ = R.oracle_matrices(poses)
            recs = OR.sparse_window(corr, offs, T)
            n, out = sum(r["count"] for r in recs), sum(r["n_outlier"] for r in recs)
            shares.append(out / n)
            print(f"N {N}: {out} of {n} beyond the knee; nearest to the knee {min(r['knee_distance'] for r in recs):.2e} m; knee-borderline {sum(r['n_knee'] for r in recs)}")
        assert max(shares) >= 0.2 and 1 - min(shares) >= 0.2, shares
        T, _ = R.oracle_matrices(pose_sets[1])
        assert OR.sparse_window(corr, offs, T)[p]["worst"] == k      # the planted 7 cm match, at the poses the points were generated at


def test_mutations_move_a_field_beyond_its_bar(oracle):
    g = OR.gammas()
    # dense: drop a tile's last accepted pixel
    sc = R.scene("bg50x30")
    T, Tinv = R.oracle_matrices(sc["poses"])
    ref = OR.scene_pairs(sc, T, Tinv, ((0, 1),))[0]
    args = (sc["campos"][[0, 1]], sc["normals"][[0, 1]], sc["intr"], T[1], Tinv[0], ref["accept"])
    good = OR.dense_pair_f32(*args)
    assert good["count"] == ref["count"] and OR.normalised(good["sum_rho"], ref["sum_rho"], 0, ref["sc_rho"]) <= g["dense_rho"]
    last = ref["accept"][ref["accept"] < OR.TILE][-1]
    bad = OR.dense_pair_f32(*args, drop=(int(last),))
    e = OR.normalised(bad["sum_rho"], ref["sum_rho"], 0, ref["sc_rho"])
    print(f"dense, tile 0's last pixel dropped: count {bad['count']} vs {ref['count']}, sum_rho off by {e:.3e} Sc (bar {g['dense_rho']:.3e})")
    assert bad["count"] != ref["count"] and e > g["dense_rho"]
    # sparse: drop the last entry of a segment
    corr, offs, pose_sets, _ = OR.two_sided_case(3)
    T, _ = R.oracle_matrices(pose_sets[1])
    seg = corr[int(offs[1]):int(offs[2])]
    ref = OR.sparse_pair(seg, T[0], T[2])
    bad = OR.sparse_pair(seg, T[0], T[2], dt=np.float32, drop_last=True)
    e = OR.normalised(bad["sum_sq"], ref["sum_sq"], 0, ref["sc_sq"])
    print(f"sparse, last valid entry dropped: count {bad['count']} vs {ref['count']}, sum_sq off by {e:.3e} Sc (bar {g['sparse_sq']:.3e})")
    assert bad["count"] == ref["count"] - 1 and e > g["sparse_sq"]
    # Huber <= -> <: rho is continuous at the knee, so only the outlier count can tell; it does on an entry EXACTLY at the knee -- identity poses and
    # r = (delta, 0, 0) with fp32 delta, every operation exact, so the definition decides it and not round-off
    d = np.float32(R.DEFAULT_PRM["robust_delta"])
    seg = np.zeros(2, R.ENTRYJ)
    seg["imgIdx_j"] = 1
    seg["pos_i"][0] = (d, 0, 0)
    seg["pos_i"][1] = (0, 0.25, 0)
    I = np.eye(4)
    ref, bad = OR.sparse_pair(seg, I, I), OR.sparse_pair(seg, I, I, dt=np.float32, strict=True)
    print(f"Huber < for <=: n_outlier {bad['n_outlier']} vs {ref['n_outlier']}")
    assert ref["n_outlier"] == 1 and bad["n_outlier"] == 2 and bad["sum_rho"] == ref["sum_rho"]


def test_abi_symbol_and_record_sizes():
    L = _lib.lib()
    name = "btba_objective_batch_zn_aux"
    assert hasattr(L, name) and name in _lib.declared_symbols() and name in _lib.EXPORTED_SYMBOLS
    assert _lib.OBJECTIVE_PAIR_DTYPE.itemsize == 40 and _lib.OBJECTIVE_TOTAL_DTYPE.itemsize == 64
    assert L.btba_version() == 105


def test_argument_checks_before_any_hip_call():
    L = _lib.lib()
    hip_error = L.btba_last_hip_error()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    prm = _lib.default_params()
    call = lambda ws, prm_, B, N, poses, total: L.btba_objective_batch_zn_aux(ws, prm_, B, N, 64, 64, p, p, None, None, 1, None, 0, None, 0, poses, total, None, None)
    assert call(None, C.byref(prm), 1, 2, p, p) == _lib.BTBA_EINVAL
    assert L.btba_last_hip_error() == hip_error
