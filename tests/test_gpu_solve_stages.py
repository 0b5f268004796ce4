"""The system solve's three stages -- assembly, PCG, pose update -- against the fp64 references of tests/solve_ref.py, stage by stage, for
every instance and every Gauss-Newton iterate of one traced solve (7 GN x 5 PCG) per case, kernel by kernel (never one kernel against another).

Each stage is fed the TRACE'S OWN inputs of that iterate, so a fault is named by stage, kernel, window size, iterate and entry:
  A  traced A, rhs, precond        against assemble_ref(correspondences, traced T_before, traced dense records)
  B  traced PCG scalars and delta  against pcg_ref(float64) on the traced A, rhs, precond
  C  traced x_after, T_after       against update_ref(traced delta, traced x_before)
The rules and bars are stated in tests/solve_ref.py; the cases (window sizes at both ends of every kernel instantiation, explicit dense-pair
lists, terms and weights, partials per sum, a batch) in solve_ref.cases(), whose floors and caps tests/test_solve_ref.py checks on the CPU.
Every run prints each case's floors, bars and worst errors per stage before it asserts them (run with -s); DESIGN.md "Testing the system
solve" records the numbers of one MI355X run."""
import numpy as np
import pytest

import solve_ref as SR
from bundletrack_amd import _lib, synthetic as S
from shared_checks import device_poses_and_matrices

pytestmark = pytest.mark.gpu
N_GN, N_PCG = 7, 5
CASES = SR.cases()


@pytest.fixture(scope="module")
def gpu(oracle):
    import torch
    assert torch.cuda.is_available()
    from bundletrack_amd.optimizer import BatchSolver, Workspace

    class G:
        pass
    g = G()
    g.torch, g.dev, g.ws, g.BatchSolver, g.oracle = torch, torch.device("cuda:0"), Workspace(), BatchSolver, oracle      # a workspace of its own: no option leaks
    g.floors, g.traces = {}, {}
    return g


def traced_solve(g, case, seeds=None):
    """One traced solve of the case's batch.  Returns (instances [(pb, corr)], TraceView, the poses the call returned [B, N, 4, 4])."""
    K = case["K"]
    seeds = case["seeds"] if seeds is None else seeds
    insts = [SR.window(K, seed, case["no_corr_frame"]) for seed in seeds]
    pb0 = insts[0][0]
    kw = dict(case["prm"])
    if case["partials"]:
        kw.update(sparse_chunks=case["partials"][0], dense_tiles=case["partials"][1])
    bs = g.BatchSolver(g.ws, n_gn_iters=N_GN, n_pcg_iters=N_PCG, **kw)
    if case["iter_weights"]:
        bs.set_iteration_weights(**case["iter_weights"])
    dp = None
    if case["pairs"] is not None:
        bs.params.pair_policy = _lib.PAIRS_EXPLICIT
        dp = np.asarray(case["pairs"], np.int32)
    corr, offs, mx = bs.pack_correspondences([c for _, c in insts], K)
    B = len(insts)
    zn_d = g.torch.from_numpy(np.stack([S.compact_cache(pb) for pb, _ in insts])).to(g.dev)
    corr_d = g.torch.from_numpy(corr.view(np.uint8).reshape(B, -1, 32)).to(g.dev)
    offs_d = g.torch.from_numpy(offs.astype(np.int32)).to(g.dev)
    poses_d = g.torch.from_numpy(np.stack([pb.poses_init for pb, _ in insts]).astype(np.float32)).to(g.dev)
    try:
        g.ws.set_option(_lib.OPT_SOLVE_SMALL, case["small"])
        tv = bs.trace_view(bs.solve_zn(zn_d, pb0.H, pb0.W, pb0.K, corr_d, offs_d, mx, poses_d, dense_pairs=dp, trace=True))
        st = g.ws.collect_stats()
    finally:
        g.ws.set_option(_lib.OPT_SOLVE_SMALL, 1)
    if case["partials"]:
        assert (st["sparse_chunks"], st["dense_tiles"]) == case["partials"], st
    return insts, tv, poses_d.cpu().numpy()


def record_bytes(tv, b=None):
    """The traced quantities of the whole batch, or of instance b, as bytes (everything in the record but its clock stamps)."""
    fields = (tv.x_after, tv.T_after, tv.rhs, tv.precond, tv.pcg_scalars, tv.delta, tv.dense_pair, tv.A)
    return b"".join(np.ascontiguousarray(f if b is None else f[b]).tobytes() for f in fields)


def floor_of(g, case, seed, corr, poses):
    key = (case["K"], seed, case["no_corr_frame"])
    if key not in g.floors:
        g.floors[key] = SR.oracle_floor(corr, poses)
    return g.floors[key]


def check_case(g, case, insts, tv, poses_out):
    """All three stages of every instance and iterate; prints the case's figures, returns the failures."""
    K = case["K"]
    prm = case["prm"]
    pairs = case["pairs"] if case["pairs"] is not None else [(i, j) for i in range(K) for j in range(i + 1, K)]
    fails, stage_b, stats_c = [], [], {}
    worst_a, floors_a, symmetric = np.zeros(3), np.zeros(3), True
    for b, (pb, corr) in enumerate(insts):
        floor = floor_of(g, case, case["seeds"][b], corr, pb.poses_init)
        floors_a = np.maximum(floors_a, floor)
        x, T, _ = device_poses_and_matrices(g, pb.poses_init)
        for it in range(N_GN):
            where = f"{case['kernel']} K {K} instance {b} iterate {it}"
            ws_it = case["iter_weights"]["sparse"][it] if case["iter_weights"] else prm.get("weight_sparse", 1.0)
            wd_it = case["iter_weights"]["dense"][it] if case["iter_weights"] else prm.get("weight_dense_depth", 1.0)
            dense_on = wd_it > 0 and tv.n_dense_pairs > 0
            A_d, rhs_d, prec_d = tv.A[b, it], tv.rhs[b, it], tv.precond[b, it]
            # stage A
            ref = SR.assemble_ref(corr, T, tv.dense_pair[b, it] if dense_on else [], pairs, ws_it, dense_on)
            a = SR.check_assembly(A_d, rhs_d, prec_d, ref, floor, sparse_on=ws_it > 0)
            worst_a = np.maximum(worst_a, (a["e_A"], a["e_rhs"], a["e_prec"]))
            symmetric &= a["symmetric"]
            fails += [f"stage A, {where}: {m}" for m in a["fails"]]
            # stage B, on the traced system
            stage_b.append((f"instance {b}", it, SR.compare_pcg(A_d, rhs_d, prec_d, tv.pcg_scalars[b, it], tv.delta[b, it])))
            # stage C, on the traced delta
            fails += [f"stage C, {where}: {m}" for m in SR.check_update(g.oracle, tv.x_after[b, it], tv.T_after[b, it], tv.delta[b, it], x, T, stats_c)]
            x, T = tv.x_after[b, it], tv.T_after[b, it]
        if poses_out[b].tobytes() != tv.T_after[b, N_GN - 1].tobytes():
            fails.append(f"stage C, {case['kernel']} K {K} instance {b}: the returned poses are not the bits of T_after[{N_GN - 1}]")
    v = SR.pcg_verdict(stage_b)
    fails += [f"stage B, {case['kernel']} K {K}, {m}" for m in v["fails"]]
    print(f"\n{case['id']}\n  stage A: oracle floors (rhs, precond, A) {floors_a}, worst error in units of the bar A {worst_a[0]:.3f} rhs {worst_a[1]:.3f} precond {worst_a[2]:.3f}; "
          f"A symmetric {'bit for bit' if symmetric else 'within the bar'}\n"
          f"  stage B: fp32 floors (pAp, rz_new, delta) {v['floor']} -> bars {v['bar']}; device {v['worst']}; borderline guards {v['borderline']}; "
          f"alpha / beta of step 0 at most {v['step0_ulps']:.2f} ulp from the quotients with the fp64 rz0\n"
          f"  stage C: worst |dev - truth| / (A e_oracle + B ulp) [ulps of scale] {({k[0]: (round(r, 3), round(q, 2)) for k, (r, q) in stats_c.items()})}")
    return fails


@pytest.mark.parametrize("case", [c for c in CASES if c["group"] != "batch"], ids=[c["id"] for c in CASES if c["group"] != "batch"])
def test_solve_stages_against_fp64(gpu, case):
    insts, tv, poses_out = traced_solve(gpu, case)
    if case["group"] == "sizes":
        gpu.traces[(case["K"], case["small"])] = record_bytes(tv)
    fails = check_case(gpu, case, insts, tv, poses_out)
    assert not fails, "\n".join(fails[:20])


def test_solve_small_option_changes_the_kernel(gpu):
    """The window sizes run under both settings of OPT_SOLVE_SMALL: on at least one of them the two traces differ in some bit."""
    both = [K for (K, small) in gpu.traces if small == 0 and (K, 1) in gpu.traces]
    if not both:                      # run on its own: make the two traces of one window size
        c0, c1 = (next(c for c in CASES if c["group"] == "sizes" and c["K"] == 21 and c["small"] == s) for s in (0, 1))
        gpu.traces[(21, 0)], gpu.traces[(21, 1)] = record_bytes(traced_solve(gpu, c0)[1]), record_bytes(traced_solve(gpu, c1)[1])
        both = [21]
    differ = [K for K in both if gpu.traces[(K, 0)] != gpu.traces[(K, 1)]]
    print(f"window sizes traced under both settings {sorted(both)}; the traces differ at {sorted(differ)}")
    assert differ


def test_solve_stages_in_a_batch_of_three(gpu):
    """Three instances at K = 6; instance 1 solved alone leaves the same trace record, bit for bit."""
    case = next(c for c in CASES if c["group"] == "batch")
    insts, tv, poses_out = traced_solve(gpu, case)
    fails = check_case(gpu, case, insts, tv, poses_out)
    assert not fails, "\n".join(fails[:20])
    _, tv1, poses1 = traced_solve(gpu, case, seeds=case["seeds"][1:2])
    assert record_bytes(tv1, 0) == record_bytes(tv, 1) and poses1[0].tobytes() == poses_out[1].tobytes()
