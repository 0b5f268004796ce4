"""The exact configuration bench.py times (32 distinct c3 instances, 24-byte correspondences, prebuilt block ranges) against the other ways
of handing the library the same batch, bit for bit, and against the reference's own solveBundlingStub
(/root/reference/src/cuda/Solver/SolverBundling.cu:931-1003 compiled for the CPU: oracle/_ref, prebuilt -- nothing under /root/reference is read here);
and the options of the retired chained launch, which are still accepted and change nothing."""
import os

import numpy as np
import pytest

from bundletrack_amd import _lib, synthetic as S

pytestmark = pytest.mark.gpu


class Batch:
    """One batch resident on the GPU the way bench.py holds it."""

    def __init__(self, pbs, masked=False):
        import torch
        from bundletrack_amd.optimizer import BatchSolver
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.pbs, self.N, self.B = pbs, pbs[0].n_frames, len(pbs)
        corr, offs, self.mx = BatchSolver.pack_correspondences([pb.corr for pb in pbs], self.N)
        self.corr_d = torch.from_numpy(corr.view(np.uint8).reshape(self.B, -1, 32)).to(self.dev)
        self.offs_d = torch.from_numpy(offs.astype(np.int32)).to(self.dev)
        self.zn_d = torch.from_numpy(np.stack([S.compact_cache(pb) for pb in pbs])).to(self.dev)
        self.poses0 = torch.from_numpy(np.stack([pb.poses_init for pb in pbs])).to(self.dev)
        self.masked = masked

    def solve(self, corr24=False, aux=False, tiles=0, relayout=True, corr_nt=None, legacy_solve=False, options=()):
        """-> (poses [B, N, 4, 4], stats).  legacy_solve: the system solves by k_system_solve (BTBA_OPT_SOLVE_SMALL = 0; k_solve_small forms the
        same sums in another order).  options: further (option, value) pairs for the workspace, each of which must be accepted."""
        from bundletrack_amd.optimizer import BatchSolver, Workspace
        ws = Workspace()
        ws.set_option(_lib.OPT_SOLVE_SMALL, 0 if legacy_solve else 1)
        ws.set_option(_lib.OPT_RELAYOUT, 1 if relayout else 0)
        for option, value in options:
            assert _lib.lib().btba_workspace_set_option(ws._h, int(option), int(value)) == _lib.BTBA_OK, (option, value)
        if corr_nt is not None:
            ws.set_option(_lib.OPT_CORR_NONTEMPORAL, corr_nt)      # 1 all instances, 0 none, -1 the library's choice
        bs = BatchSolver(ws)
        bs.params.dense_tiles = tiles
        if self.masked:
            bs.params.flags |= _lib.FLAG_COMPACTION
        aux_d = bs.cache_aux(self.zn_d, valid_lists=self.masked) if (aux or corr24) else None
        if corr24:
            aux_d["corr24"], flag = bs.pack_correspondences24(self.corr_d, self.offs_d, self.mx, self.N, check_order=True)
            self.torch.cuda.synchronize()
            assert int(flag.cpu()[0]) == 0
        poses_d = self.poses0.clone()
        pb = self.pbs[0]
        bs.solve_zn(self.zn_d, pb.H, pb.W, pb.K, None if corr24 else self.corr_d, self.offs_d, self.mx, poses_d, aux=aux_d, corr_stride=self.corr_d.shape[1])
        ws.sync()
        st = ws.collect_stats()
        out = poses_d.cpu().numpy()
        ws.close()
        return out, st


@pytest.fixture(scope="module")
def c3x32():
    return Batch([S.make_problem(15, 2000, S.config_seed(5, b), background=True, full_res=False) for b in range(32)])


def test_the_benched_path_is_pinned(c3x32):
    """What `python bench.py` times: btba_solve_batch_zn_aux with B = 32 DISTINCT c3 instances, aux.corr24 (24-byte correspondences packed
    from EntryJ), prebuilt block ranges, the library's own schedule (the fused launch with ONE tile per pair, sparse items closing it) --
      (a) bit-identical to the EntryJ / no-aux call on the plain schedule, the configuration the other parity tests reach;
      (b) instances 0, 13 and 31 against the reference's own solveBundlingStub, < 1e-4 rad / m."""
    bt = c3x32
    benched, st = bt.solve(corr24=True, aux=True)
    assert st["chain_iterations"] == 0 and st["dense_tiles"] == 1 and st["sparse_chunks"] == 1 and st["fused_sweeps"] == 1, st
    plain, st0 = bt.solve()                                      # EntryJ in, re-laid out to 24-byte records by the first iteration's sweep (BTBA_OPT_RELAYOUT = 1)
    assert st0["chain_iterations"] == 0
    assert np.array_equal(benched, plain), f"worst difference {np.abs(benched - plain).max():.3e}"
    wire, _ = bt.solve(relayout=False)                           # ... and with every iteration reading the 32-byte wire format (the default; what bench.py's value_incl_pack times)
    assert np.array_equal(benched, wire)
    legacy, _ = bt.solve(corr24=True, aux=True, legacy_solve=True)          # the same batch with rounds 1-4's system solve (k_system_solve)
    worst = max(max(S.pose_error(benched[b, k], legacy[b, k])) for b in range(bt.B) for k in range(15))
    print(f"k_solve_small vs k_system_solve on the benched batch: worst final pose difference {worst:.2e}")
    assert worst < 1e-4
    from oracle import reference as R
    if not os.path.exists(R.SO_SOLVER):
        pytest.skip("oracle/_ref/libbtba_ref_solver.so not built")
    for b in (0, 13, 31):
        pb = bt.pbs[b]
        campos, normals, intr = S.analytic_cache(pb)
        ref, _ = R.solve(campos, normals, intr, pb.corr, pb.poses_init, weight_dense=1.0)
        worst = max(max(S.pose_error(benched[b, k], ref[k])) for k in range(15))
        print(f"benched path, instance {b}: worst pose difference against the reference's solver {worst:.2e}")
        assert worst < 1e-4, (b, worst)


def test_nontemporal_correspondence_stream_has_the_same_bits(c3x32):
    """Once a batch's frames + correspondences exceed the memory-side cache (c3 x 32: 147 + 161 MB against 256 MB) the sparse items read the
    correspondences of the instances that no longer fit with non-temporal loads (btba_api.hip: corr_nt_auto) -- a cache policy, not arithmetic:
    all / none / the library's choice give the same poses, with 24-byte records and with EntryJ."""
    bt = c3x32
    auto, _ = bt.solve(corr24=True, aux=True)
    for nt in (0, 1):
        out, _ = bt.solve(corr24=True, aux=True, corr_nt=nt)
        assert np.array_equal(auto, out), (nt, np.abs(auto - out).max())
    wire_nt, _ = bt.solve(relayout=False, corr_nt=1)
    wire, _ = bt.solve(relayout=False, corr_nt=0)
    assert np.array_equal(wire_nt, wire) and np.array_equal(wire, auto)


def test_retired_chain_options_are_inert():
    """BTBA_OPT_CHAIN, BTBA_OPT_CHAIN_SPARSE_PERIOD and BTBA_OPT_CHAIN_TIMEOUT_MS keep their ids and their ranges and change nothing: a workspace
    with all three set solves a batch to the bits of a workspace with none set, reports no chained iterations, and synchronises with BTBA_OK;
    values outside the ranges, and the former developer option 1000, are BTBA_EINVAL."""
    from bundletrack_amd.optimizer import Workspace
    pbs = [S.make_problem(4, 200, 900 + 17 * b, background=True, full_res=False) for b in range(9)]
    bt = Batch(pbs)
    plain, st0 = bt.solve(tiles=2)
    opted, st1 = bt.solve(tiles=2, options=[(_lib.OPT_CHAIN, 1), (_lib.OPT_CHAIN_SPARSE_PERIOD, 3), (_lib.OPT_CHAIN_TIMEOUT_MS, 2)])      # (solve() asserts BTBA_OK of every option; its sync() raises otherwise)
    assert st0["chain_iterations"] == 0 and st1["chain_iterations"] == 0, (st0, st1)
    assert np.array_equal(plain, opted), f"worst difference {np.abs(plain - opted).max():.3e}"
    assert np.abs(plain - np.stack([pb.poses_init for pb in pbs])).max() > 1e-4
    ws = Workspace()
    for option, value in ((_lib.OPT_CHAIN, 2), (_lib.OPT_CHAIN_SPARSE_PERIOD, 1), (_lib.OPT_CHAIN_TIMEOUT_MS, 0), (1000, 0), (1000, 64)):
        with pytest.raises(_lib.BtbaError) as err:
            ws.set_option(option, value)
        assert err.value.status == _lib.BTBA_EINVAL, (option, value)
    ws.close()
