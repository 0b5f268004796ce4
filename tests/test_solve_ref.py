"""CPU checks of tests/solve_ref.py, the stage-by-stage fp64 reference that tests/test_gpu_solve_stages.py holds the system solve to:

- the restatement against its source, oracle/oracle_np.py::solve, to 1e-12 on whole windows and on explicit dense-pair lists;
- the fp32 CPU oracle as the implementation under test: a correct fp32 solve stays inside the bars, so they are not too tight;
- the fp32 floors and the two caps (delta bar <= 1e-4; at most one borderline guard, none at iterate 0) of every GPU case of up to 15 frames;
- deliberately wrong stage outputs through the same comparison functions: each is rejected, in its own stage and only there."""
import numpy as np
import pytest

import solve_ref as SR
import sweep_ref as SW
from bundletrack_amd import synthetic as S
from oracle import oracle_np as ONP

F32 = np.float32
N_PCG = 5
REL = 1e-12


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


def default_pairs(N):
    return [(i, j) for i in range(N) for j in range(i + 1, N)]


def np_poses(poses):
    x = np.stack([np.concatenate(ONP.se3_log(np.asarray(p, np.float64))) for p in poses])
    return x, np.stack([ONP.se3_exp(v[:3], v[3:]) for v in x])


def np_records(cam, nrm, intr, T, pairs, prm):
    """oracle_np.dense_pair_sums' (S, g, count) of every (target, source) as 28-float records, float64."""
    Tinv = np.linalg.inv(T)
    p = dict(SW.DEFAULT_PRM)
    p.update(prm)
    out = []
    for (i, j) in pairs:
        Sx, g, cnt = ONP.dense_pair_sums(cam[[i, j]], nrm[[i, j]], intr, T[i], T[j], Tinv[i], p)
        out.append(np.concatenate([SW.record27(Sx, g), [cnt]]))
    return out


_solved = {}


def np_solve(K, seed, pairs=None, prm=None, no_corr_frame=None):
    """oracle_np.solve of one window, once per (window, list, parameters): (pb, corr, cache, pairs, prm, its output)."""
    key = (K, seed, None if pairs is None else tuple(pairs), tuple(sorted((prm or {}).items())), no_corr_frame)
    if key not in _solved:
        pb, corr = SR.window(K, seed, no_corr_frame)
        cache = S.analytic_cache(pb)
        out = ONP.solve(*cache, corr, pb.poses_init, pairs=pairs, n_pcg_iters=N_PCG, **(prm or {}))
        _solved[key] = (pb, corr, cache, list(pairs) if pairs is not None else default_pairs(K), dict(prm or {}), out)
    return _solved[key]


def restatement_errors(solved):
    """Worst relative difference, over the seven iterates, between every stage of solve_ref fed oracle_np's own inputs and oracle_np.solve."""
    pb, corr, (cam, nrm, intr), pairs, prm, out = solved
    ws, wd = prm.get("weight_sparse", 1.0), prm.get("weight_dense_depth", 1.0)
    x, T = np_poses(pb.poses_init)
    worst = {}
    for it in range(len(out["A"])):
        recs = np_records(cam, nrm, intr, T, pairs, prm) if wd > 0 else []
        ref = SR.assemble_ref(corr, T, recs, pairs, ws, wd > 0)
        pr = SR.pcg_ref(out["A"][it], SW.to_rot_trans(out["b"][it]), SW.to_rot_trans(SW.precond_ref(out["Mdiag"][it], 0 * out["Mdiag"][it])[0]), N_PCG)
        xa, Ta = SR.update_ref(pr["delta"], x)
        e = dict(A=rel(ref["A"], out["A"][it]), b=rel(ref["b"], out["b"][it]), Mdiag=rel(ref["Mdiag"], out["Mdiag"][it]),
                 pcg=rel(pr["scalars"], np.array(out["pcg_scalars"][it])), x_after=rel(xa, out["x_after"][it]), T_after=rel(Ta, out["T_after"][it]))
        assert np.array_equal(ref["rhs"], SW.to_rot_trans(ref["b"])) and np.array_equal(SR.to_trans_rot(ref["rhs"]), ref["b"])
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in e.items()}
        x, T = out["x_after"][it], out["T_after"][it]
    return worst


@pytest.mark.parametrize("K", [2, 3, 6, 7])
def test_restatement_reproduces_oracle_np(K):
    worst = restatement_errors(np_solve(K, 500 + 10 * K))
    print(f"K {K}: worst relative difference from oracle_np.solve over 7 iterates {worst}")
    assert all(v <= REL for v in worst.values()), worst


LISTS_K = 5
EXTRA_LISTS = {"a_reversed_pair": [(0, 1), (0, 2), (2, 1), (1, 3), (3, 4), (0, 4)], "same_pair_in_both_orders": [(0, 1), (1, 2), (2, 1), (3, 4), (4, 3), (0, 3)]}


@pytest.mark.parametrize("name", list(EXTRA_LISTS) + list(SR.explicit_lists(LISTS_K)))
def test_restatement_reproduces_oracle_np_on_explicit_lists(name):
    pairs = EXTRA_LISTS[name] if name in EXTRA_LISTS else SR.explicit_lists(LISTS_K)[name]
    worst = restatement_errors(np_solve(LISTS_K, 500 + 10 * LISTS_K, pairs=pairs))
    print(f"{name}: worst relative difference from oracle_np.solve {worst}")
    assert all(v <= REL for v in worst.values()), worst


def test_dispatch_rule_names_the_kernels():
    assert SR.selected_kernel(6, 15) == "k_solve_small<4>" and SR.selected_kernel(7, 21) == "k_solve_small<8>"
    # 21 frames: k_solve_small<16> holds at most 379 dense pairs in the LDS limit (20 736 fixed floats + 210 x 44 + Pd x 28 + 368 <= 40 960), so
    # every ordered pair (420) goes to k_system_solve, like a list beyond one trip of the kernel's 1 024 lanes
    assert SR.small_solve_lds_floats(21, 420) == 42104 and 4 * SR.small_solve_lds_floats(21, 379) <= SR.LDS_LIMIT < 4 * SR.small_solve_lds_floats(21, 380)
    assert SR.selected_kernel(21, 379) == "k_solve_small<16>" and SR.selected_kernel(21, 380).startswith("k_system_solve[lds")
    assert SR.selected_kernel(21, 420).startswith("k_system_solve[lds") and SR.selected_kernel(21, 513).startswith("k_system_solve[lds")
    assert 4 * SR.mid_solve_lds_floats(31, 465) <= SR.LDS_LIMIT and 4 * SR.general_solve_lds_floats(31, 465) <= SR.LDS_LIMIT < 4 * SR.general_solve_lds_floats(32, 496)
    assert SR.selected_kernel(22, 231) == "k_solve_mid" and SR.selected_kernel(24, 552).startswith("k_system_solve[lds")
    assert SR.selected_kernel(31, 465, 0).startswith("k_system_solve[lds") and SR.selected_kernel(32, 496).startswith("k_system_solve[global")
    lists21 = [c for c in SR.cases() if c["group"] == "lists" and c["K"] == 21]
    assert len(lists21) == 6 and all(c["kernel"] == "k_solve_small<16>" for c in lists21)
    both = next(c["pairs"] for c in lists21 if "both_orders" in c["id"])
    assert len(both) == 354 and sum((j, i) in both for (i, j) in both) == 288            # both orders of 144 pairs
    kernels = {c["kernel"] for c in SR.cases()}
    assert kernels == {"k_solve_small<4>", "k_solve_small<8>", "k_solve_small<12>", "k_solve_small<16>", "k_solve_mid", "k_system_solve[lds,1-wave]", "k_system_solve[global,16-wave]"}


# ---- the fp32 CPU oracle as the implementation under test ----------------------------------------------------------------------
def oracle_stage_results(oracle, K, seed):
    """The fp32 CPU oracle's trace of one window through the three comparison functions.  The oracle traces the SUMMED dense share (dense_JtJ,
    dense_Jtr) instead of per-pair records and applies the sparse J^T J matrix-free, so its dense share enters the reference as one exact term
    per entry and the system its PCG is held to is  fp64(dense_JtJ) + the fp64 sparse matrix at its own T."""
    pb, corr = SR.window(K, seed)
    cam, nrm, intr = S.analytic_cache(pb)
    floor = SR.oracle_floor(corr, pb.poses_init)
    out = {}
    for mode in (0, 1):
        tr = oracle.solve(cam, nrm, intr, corr, pb.poses_init, params=oracle.default_params(accum_mode=mode))
        T, _ = SW.oracle_matrices(pb.poses_init)
        x = np.stack([np.concatenate(oracle.matrix_to_pose(p)) for p in pb.poses_init])
        stage_a, stage_b, stage_c, stats = [], [], [], {}
        for it in range(tr.rhs.shape[0]):
            JtJ, Jtr = tr.dense_JtJ[it].astype(np.float64), tr.dense_Jtr[it].astype(np.float64)
            dn = dict(A=JtJ, b=-Jtr, abs_A=np.abs(JtJ), abs_b=np.abs(Jtr), n_A=(JtJ != 0).astype(np.int64), n_b=(Jtr != 0).astype(np.int64))
            ref = SR.join_system(SW.sparse_system(corr, T), dn)
            bar_A, bar_r, bar_p = SR.assembly_bars(ref, floor)
            stage_a.append((SR._worst(np.abs(tr.rhs[it] - ref["rhs"])[1:], bar_r[1:])[0], SR._worst(np.abs(tr.precond[it] - ref["precond"])[1:], bar_p[1:])[0]))
            stage_b.append((f"mode {mode}", it, SR.compare_pcg(ref["A"], tr.rhs[it], tr.precond[it], tr.pcg_scalars[it], tr.delta[it])))
            stage_c += [f"iterate {it}: {m}" for m in SR.check_update(oracle, tr.x_after[it], tr.T_after[it], tr.delta[it], x, T, stats)]
            x, T = tr.x_after[it], tr.T_after[it]
        out[mode] = (np.max(stage_a, 0), SR.pcg_verdict(stage_b), stage_c, stats)
    return out


@pytest.mark.parametrize("K", [2, 3, 6, 7])
def test_fp32_cpu_oracle_stays_inside_the_bars(oracle, K):
    for mode, (e_a, v, fails_c, stats) in oracle_stage_results(oracle, K, 500 + 10 * K).items():
        print(f"K {K} accum_mode {mode}: stage A rhs {e_a[0]:.3f} precond {e_a[1]:.3f} (units of the bar); stage B floor {v['floor']} bar {v['bar']} oracle {v['worst']} "
              f"borderline {v['borderline']}; stage C {stats}")
        assert np.all(e_a <= 1.0), e_a
        assert not v["fails"], v["fails"]
        assert not fails_c, fails_c


# ---- floors and caps of the GPU cases that are cheap enough here -----------------------------------------------------------------
# (not the per-iteration weights at K = 7: oracle_np.solve takes one weight per term for the whole solve, so that case has no stand-in systems
# here and gets its caps asserted on the GPU, like the windows of more than 15 frames)
CPU_CASES = [c for c in SR.cases() if c["K"] <= SR.CPU_MAX_FRAMES and c["iter_weights"] is None]
_CPU_KEYS = {}
for _c in CPU_CASES:          # cases that differ only in how the device splits its sums share one reference
    _CPU_KEYS.setdefault((_c["K"], _c["seeds"], None if _c["pairs"] is None else tuple(_c["pairs"]), tuple(sorted(_c["prm"].items())), _c["no_corr_frame"]), _c)


@pytest.mark.parametrize("case", list(_CPU_KEYS.values()), ids=[c["id"] for c in _CPU_KEYS.values()])
def test_floors_and_caps_of_the_gpu_cases(case):
    """oracle_np's systems cast to fp32 stand in for the traced ones: the two fp32 restatements' floors are printed, and the case must meet the
    caps on the fp64 reference alone -- a delta bar of at most 1e-4 and at most one borderline guard, none at iterate 0."""
    results = []
    for b, seed in enumerate(case["seeds"]):
        pb, corr, cache, pairs, prm, out = np_solve(case["K"], seed, case["pairs"], case["prm"], case["no_corr_frame"])
        for it in range(len(out["A"])):
            A32 = out["A"][it].astype(F32)
            rhs32 = SW.to_rot_trans(out["b"][it]).astype(F32)
            M32 = SW.to_rot_trans(SW.precond_ref(out["Mdiag"][it], 0 * out["Mdiag"][it])[0]).astype(F32)
            free = SR.pcg_ref(A32, rhs32, M32, N_PCG)
            results.append((f"instance {b}", it, SR.compare_pcg(A32, rhs32, M32, free["scalars"], free["delta"])))
    v = SR.pcg_verdict(results)
    print(f"{case['id']}: fp32 floors (pAp, rz_new, delta) {v['floor']} -> bars {v['bar']}; borderline guards {v['borderline']}")
    assert not v["fails"], v["fails"]


# ---- deliberately wrong stage outputs ---------------------------------------------------------------------------------------------
def pcg32(A, b, Minv, n_pcg, beta_from_previous_step=None):
    """A third fp32 PCG (numpy's matmul and dot on float32), with an optional defect: beta of one step taken from the step before."""
    Aa = np.asarray(A, F32)[6:, 6:]
    ba, Ma = SR.to_trans_rot(b)[6:].astype(F32), SR.to_trans_rot(Minv)[6:].astype(F32)
    d = np.zeros_like(ba); r = ba.copy(); z = Ma * r; p = z.copy(); rz = np.dot(r, z)
    sc = np.zeros((n_pcg, 4), F32)
    for li in range(n_pcg):
        Ap = Aa @ p
        pAp = np.dot(p, Ap)
        alpha = rz / pAp if pAp > F32(SR.GUARD) else F32(0)
        d = d + alpha * p; r = r - alpha * Ap; z = Ma * r
        rzn = np.dot(z, r)
        beta = rzn / rz if rz > F32(SR.GUARD) else F32(0)
        if li == beta_from_previous_step:
            beta = sc[li - 1, 3]
        sc[li] = (pAp, alpha, rzn, beta)
        rz = rzn; p = z + beta * p
    delta = np.zeros((np.asarray(b).reshape(-1, 6).shape[0], 6), F32)
    delta[1:] = SW.to_rot_trans(d)
    return sc, delta


DEFECTS = {None: set(), "cross_block_sign_of_a_reversed_pair": {"A"}, "beta_of_step_3_from_step_2": {"B"}, "one_precond_left_at_1": {"A"}, "delta_of_frame_k_applied_to_k_plus_1": {"C"}}


@pytest.fixture(scope="module")
def fp32_solve(oracle):
    """The inputs of one iterate of a 6-frame window whose list holds a reversed pair, as an fp32 implementation holds them."""
    K, seed = 6, 560
    pb, corr = SR.window(K, seed)
    cam, nrm, intr = S.analytic_cache(pb)
    pairs = [(i, j) for (i, j) in default_pairs(K) if (i, j) != (2, 4)] + [(4, 2)]
    x = np.stack([np.concatenate(oracle.matrix_to_pose(p)) for p in pb.poses_init]).astype(F32)
    T = np.stack([oracle.pose_to_matrix(v[:3], v[3:]) for v in x])
    recs = [r.astype(F32) for r in np_records(cam, nrm, intr, T.astype(np.float64), pairs, {})]
    return dict(K=K, corr=corr, pairs=pairs, x=x, T=T, recs=recs, floor=SR.oracle_floor(corr, pb.poses_init),
                ref=SR.assemble_ref(corr, T, recs, pairs, 1.0, True))


def stage_outputs(w, defect):
    """A correct fp32 implementation's outputs of the three stages -- each stage working on the outputs of the one before, as the kernels do -- with
    one defect planted."""
    ref = w["ref"]
    A, rhs, prec = ref["A"].astype(F32), ref["rhs"].astype(F32), ref["precond"].astype(F32)
    if defect == "cross_block_sign_of_a_reversed_pair":        # (target 4, source 2): the block (2, 4) gets the pair's S with the flipped sign instead of nothing
        Sx = SR.record_blocks(w["recs"][-1])[0].astype(F32)
        A[24:30, 12:18] += Sx; A[12:18, 24:30] += Sx.T
    if defect == "one_precond_left_at_1":                      # the unknown whose M^-1 is nearest 1: the wrong value stays a usable preconditioner, so stage B has a fair case
        k = np.unravel_index(int(np.argmin(np.abs(np.log(prec[1:])))), prec[1:].shape)
        assert abs(prec[1:][k] - 1.0) > 0.05
        prec[1:][k] = 1.0
    sc, delta = pcg32(A, rhs, prec, N_PCG, beta_from_previous_step=3 if defect == "beta_of_step_3_from_step_2" else None)
    applied = delta.copy()
    if defect == "delta_of_frame_k_applied_to_k_plus_1":
        applied[2:] = delta[1:-1]; applied[1] = 0
    xa = SR.update_ref(applied, w["x"])[0].astype(F32)
    xa[0] = w["x"][0]
    Ta = SR.SE.pose_to_matrix(xa[:, :3].astype(np.float64), xa[:, 3:].astype(np.float64)).astype(F32)
    Ta[0] = w["T"][0]
    return A, rhs, prec, sc, delta, xa, Ta


@pytest.mark.parametrize("defect", list(DEFECTS), ids=[str(d) for d in DEFECTS])
def test_wrong_stage_outputs_are_rejected_in_their_own_stage(oracle, fp32_solve, defect):
    w = fp32_solve
    A, rhs, prec, sc, delta, xa, Ta = stage_outputs(w, defect)
    a = SR.check_assembly(A, rhs, prec, w["ref"], w["floor"])
    b = SR.pcg_verdict([("fp32", 0, SR.compare_pcg(A, rhs, prec, sc, delta))])
    c = SR.check_update(oracle, xa, Ta, delta, w["x"], w["T"])
    failed = {s for s, f in (("A", a["fails"]), ("B", b["fails"]), ("C", c)) if f}
    print(f"{defect}: stage A {a['e_A']:.3g} / {a['e_rhs']:.3g} / {a['e_prec']:.3g} of the bar, stage B {b['worst']} against bars {b['bar']}, failures {a['fails'] + b['fails'] + c}")
    assert failed == DEFECTS[defect], (defect, a["fails"], b["fails"], c)
