"""btba_pose_covariances and btba_linearize_batch_zn_aux on the device.

The kernel alone: the twelve synthetic matrices of tests/marginals_ref.py against numpy's inverse at the bar stated there (na 2^-53 kappa_2
||H^-1||_2, from numpy, nothing measured on the device), exact symmetry, blocks = diagonal blocks, batch position, isolation of a singular
instance.  The linearisation: bit for bit the system a traced one-iterate solve records, the poses untouched, a later solve unchanged.
End to end: the covariances of the device's own matrices against their numpy inverse.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

import marginals_ref as MR
import solve_ref as SR
from bundletrack_amd import _lib, synthetic as S

pytestmark = pytest.mark.gpu
SET = MR.synthetic_set()


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from bundletrack_amd.covariance import pose_covariances
    from bundletrack_amd.optimizer import BatchSolver, Workspace

    class G:
        pass
    g = G()
    g.torch, g.dev, g.Workspace, g.BatchSolver, g.cov = torch, torch.device("cuda:0"), Workspace, BatchSolver, pose_covariances
    g.ws = Workspace()
    return g


def run_cov(g, mats, full=True):
    """pose_covariances on a list of float32 [na, na] matrices -> numpy (blocks, full, pivot_ratio, status)."""
    info = g.torch.from_numpy(np.stack(mats)).to(g.dev)
    out = g.cov(g.ws, info, full=full)
    g.ws.sync()
    return (out.blocks.cpu().numpy(), out.full.cpu().numpy() if full else None, out.pivot_ratio.cpu().numpy(), out.status.cpu().numpy())


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", MR.WINDOWS)
def test_kernel_against_numpy_inverse(gpu, n_frames):
    mats = [SET[(n_frames, k)] for k in MR.KAPPAS]
    blocks, full, ratio, status = run_cov(gpu, mats)
    assert status.tolist() == [0, 0, 0]
    for b, H in enumerate(mats):
        inv, kappa, bar, ratio_bar = MR.reference(H)
        assert kappa <= MR.KAPPA_CAP
        ref = MR.pose_covariances(H)
        e_full = float(np.abs(full[b] - inv).max())
        e_blocks = float(np.abs(blocks[b] - MR.blocks_of(inv, n_frames)).max())
        e_ratio = abs(ratio[b] - ref["pivot_ratio"]) / ref["pivot_ratio"]
        print(f"n_frames {n_frames} kappa_2 {kappa:.4g}: max |dev - inv| full {e_full:.3e} blocks {e_blocks:.3e}, bar {bar:.3e}, ratio {e_full / bar:.4f}; "
              f"pivot_ratio {ratio[b]:.6g} (restatement {ref['pivot_ratio']:.6g}), relative difference {e_ratio:.3e}, bar {ratio_bar:.3e}")
        assert e_full <= bar and e_blocks <= bar
        assert e_ratio <= ratio_bar
        assert full[b].tobytes() == full[b].T.copy().tobytes()
        assert blocks[b].tobytes() == MR.blocks_of(full[b], n_frames).tobytes() and not blocks[b, 0].any()
    # without the full matrix: the same blocks
    blocks_only, none, ratio2, status2 = run_cov(gpu, mats, full=False)
    assert none is None and blocks_only.tobytes() == blocks.tobytes() and ratio2.tobytes() == ratio.tobytes() and status2.tolist() == [0, 0, 0]


@pytest.mark.parametrize("n_frames", (3, 31))
def test_batch_position_does_not_change_the_bits(gpu, n_frames):
    H, other = SET[(n_frames, 1e3)], SET[(n_frames, 1e1)]
    solo = run_cov(gpu, [H])
    batch = run_cov(gpu, [H, other, H])
    for q in range(3):
        assert batch[q][0].tobytes() == solo[q][0].tobytes() and batch[q][2].tobytes() == solo[q][0].tobytes()


@pytest.mark.parametrize("n_frames,frame", [(3, 2), (12, 7), (31, 30)])
def test_a_singular_instance_is_isolated(gpu, n_frames, frame):
    a, c = SET[(n_frames, 1e1)], SET[(n_frames, 1e5)]
    bad = MR.zero_frame(SET[(n_frames, 1e3)], frame)
    blocks, full, ratio, status = run_cov(gpu, [a, bad, c])
    assert status.tolist() == [0, 1 + 6 * (frame - 1), 0]
    assert np.isnan(full[1]).all() and np.isnan(blocks[1]).all() and ratio[1] == 0.0
    for b, H in ((0, a), (2, c)):
        solo = run_cov(gpu, [H])
        assert blocks[b].tobytes() == solo[0][0].tobytes() and full[b].tobytes() == solo[1][0].tobytes() and ratio[b].tobytes() == solo[2][0].tobytes()


def test_argument_checks_on_a_live_workspace(gpu):
    L = _lib.lib()
    t = gpu.torch
    info = t.zeros((1, 186 * 186), dtype=t.float32, device=gpu.dev)
    out = t.zeros((32 * 36 + 186 * 186,), dtype=t.float64, device=gpu.dev)
    st = t.zeros((1,), dtype=t.int32, device=gpu.dev)
    call = lambda n, stride: L.btba_pose_covariances(gpu.ws.handle, 1, n, info.data_ptr(), stride, out.data_ptr(), None, None, st.data_ptr())
    assert call(1, 36) == _lib.BTBA_EINVAL and call(32, 186 * 186) == _lib.BTBA_EINVAL and call(2, 35) == _lib.BTBA_EINVAL
    assert call(31, 180 * 180 - 1) == _lib.BTBA_EINVAL
    assert L.btba_pose_covariances(gpu.ws.handle, 1, 2, info.data_ptr(), 36, None, None, None, st.data_ptr()) == _lib.BTBA_EINVAL
    assert L.btba_pose_covariances(gpu.ws.handle, 0, 2, info.data_ptr(), 36, out.data_ptr(), None, None, st.data_ptr()) == _lib.BTBA_EINVAL
    assert call(2, 36) == _lib.BTBA_OK and call(31, 180 * 180) == _lib.BTBA_OK
    gpu.ws.sync()


# ---- the linearisation -----------------------------------------------------------------------------------------------------------------
def _lin_cases():
    lists5 = SR.explicit_lists(5)
    return [
        dict(id="K2-520", K=2, seeds=(520,)), dict(id="K2-522", K=2, seeds=(522,)),
        dict(id="K3-532", K=3, seeds=(532,)), dict(id="K3-533", K=3, seeds=(533,)),
        dict(id="K5-default-pairs", K=5, seeds=tuple(SR._seeds(5, 1))),
        dict(id="K5-reversed_only", K=5, seeds=tuple(SR._seeds(5, 1)), pairs=lists5["reversed_only"]),
        dict(id="K22-k_solve_mid", K=22, seeds=tuple(SR._seeds(22, 1))),
        dict(id="K32-k_system_solve", K=32, seeds=tuple(SR._seeds(32, 1))),
        dict(id="K6-batch-of-three", K=6, seeds=(560, 561, 562)),
    ]


LIN_CASES = _lin_cases()


class Inputs:
    """One batch of solve_ref windows on the device."""

    def __init__(self, g, K, seeds, pairs=None, no_corr_frames=None, **prm):
        no_corr_frames = no_corr_frames or [None] * len(seeds)
        self.insts = [SR.window(K, seed, f) for seed, f in zip(seeds, no_corr_frames)]
        self.K, self.B, self.prm, self.g = K, len(seeds), prm, g
        self.pb0 = self.insts[0][0]
        self.dp = None if pairs is None else np.asarray(pairs, np.int32)
        corr, offs, self.mx = g.BatchSolver.pack_correspondences([c for _, c in self.insts], K)
        t = g.torch
        self.zn = t.from_numpy(np.stack([S.compact_cache(pb) for pb, _ in self.insts])).to(g.dev)
        self.corr = t.from_numpy(corr.view(np.uint8).reshape(self.B, -1, 32)).to(g.dev)
        self.offs = t.from_numpy(offs.astype(np.int32)).to(g.dev)
        self.poses0 = np.stack([pb.poses_init for pb, _ in self.insts]).astype(np.float32)

    def solver(self, ws, n_gn, n_pcg=5):
        bs = self.g.BatchSolver(ws, n_gn_iters=n_gn, n_pcg_iters=n_pcg, **self.prm)
        if self.dp is not None:
            bs.params.pair_policy = _lib.PAIRS_EXPLICIT
        return bs

    def poses(self):
        return self.g.torch.from_numpy(self.poses0.copy()).to(self.g.dev)

    def solve(self, ws, n_gn, trace=False):
        bs, poses = self.solver(ws, n_gn), self.poses()
        tr = bs.solve_zn(self.zn, self.pb0.H, self.pb0.W, self.pb0.K, self.corr, self.offs, self.mx, poses, dense_pairs=self.dp, trace=trace)
        tv = bs.trace_view(tr) if trace else None
        ws.sync()
        return poses.cpu().numpy(), tv

    def linearize(self, ws, n_gn=7, n_pcg=5, poses=None):
        bs = self.solver(ws, n_gn, n_pcg)
        poses = self.poses() if poses is None else poses
        info, rhs = bs.linearize_zn(self.zn, self.pb0.H, self.pb0.W, self.pb0.K, self.corr, self.offs, self.mx, poses, dense_pairs=self.dp, rhs=True)
        ws.sync()
        return info, rhs, poses


@pytest.mark.parametrize("case", LIN_CASES, ids=[c["id"] for c in LIN_CASES])
def test_linearisation_is_the_traced_system(gpu, case):
    K = case["K"]
    inp = Inputs(gpu, K, case["seeds"], case.get("pairs"))
    kernel = SR.selected_kernel(K, len(case["pairs"]) if case.get("pairs") else K * (K - 1) // 2)
    # workspace A: linearise, then an ordinary seven-iterate solve
    ws_a = gpu.Workspace()
    info, rhs, poses_d = inp.linearize(ws_a)
    assert poses_d.cpu().numpy().tobytes() == inp.poses0.tobytes(), "the call wrote to its poses"
    after, _ = inp.solve(ws_a, 7)
    # workspace B, fresh: the same solve without the call; then the traced one-iterate solve
    ws_b = gpu.Workspace()
    fresh, _ = inp.solve(ws_b, 7)
    assert after.tobytes() == fresh.tobytes(), "a solve after the linearisation differs from the same solve on a fresh workspace"
    _, tv = inp.solve(ws_b, 1, trace=True)
    info_h, rhs_h = info.cpu().numpy(), rhs.cpu().numpy()
    assert info_h.shape == (inp.B, 6 * (K - 1), 6 * (K - 1)) and rhs_h.shape == (inp.B, K - 1, 6)
    for b in range(inp.B):
        want_info, want_rhs = MR.info_from_trace(tv.A[b, 0], K), MR.rhs_from_trace(tv.rhs[b, 0])
        same_info, same_rhs = info_h[b].tobytes() == want_info.tobytes(), rhs_h[b].tobytes() == want_rhs.tobytes()
        print(f"{case['id']} [{kernel}] instance {b}: info bits equal {same_info}, rhs bits equal {same_rhs}, |rhs| {np.linalg.norm(rhs_h[b].astype(np.float64)):.4g}, "
              f"max |info - info^T| {np.abs(info_h[b] - info_h[b].T).max():.3g}")
        assert same_info and same_rhs
        assert np.any(info_h[b])
    # n_gn_iters and n_pcg_iters are ignored; rhs is optional
    info2, _, _ = inp.linearize(ws_a, n_gn=1, n_pcg=2)
    assert info2.cpu().numpy().tobytes() == info_h.tobytes()
    bs = inp.solver(ws_a, 7)
    only = bs.linearize_zn(inp.zn, inp.pb0.H, inp.pb0.W, inp.pb0.K, inp.corr, inp.offs, inp.mx, inp.poses(), dense_pairs=inp.dp)
    ws_a.sync()
    assert only.cpu().numpy().tobytes() == info_h.tobytes()


def test_linearisation_refuses_per_iteration_weights(gpu):
    inp = Inputs(gpu, 3, (532,))
    bs = inp.solver(gpu.ws, 7)
    bs.set_iteration_weights(sparse=[1.0] * 7)
    with pytest.raises(_lib.BtbaError) as e:
        bs.linearize_zn(inp.zn, inp.pb0.H, inp.pb0.W, inp.pb0.K, inp.corr, inp.offs, inp.mx, inp.poses())
    assert e.value.status == _lib.BTBA_EINVAL


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in LIN_CASES if c["K"] in (2, 3, 22) or c["id"] == "K5-default-pairs"],
                         ids=[c["id"] for c in LIN_CASES if c["K"] in (2, 3, 22) or c["id"] == "K5-default-pairs"])
def test_covariances_of_the_device_matrix(gpu, case):
    K = case["K"]
    inp = Inputs(gpu, K, case["seeds"])
    info, _, _ = inp.linearize(gpu.ws)
    out = gpu.cov(gpu.ws, info, full=True)
    gpu.ws.sync()
    H = info.cpu().numpy()
    full, blocks, status, ratio = out.full.cpu().numpy(), out.blocks.cpu().numpy(), out.status.cpu().numpy(), out.pivot_ratio.cpu().numpy()
    for b in range(inp.B):
        inv, kappa, bar, _ = MR.reference(H[b])
        err = float(np.abs(full[b] - inv).max())
        print(f"{case['id']} instance {b}: kappa_2(info) {kappa:.4g}, pivot_ratio {ratio[b]:.4g}, max |dev - inv| {err:.3e}, bar {bar:.3e}, ratio {err / bar:.4f}")
        assert kappa <= MR.KAPPA_CAP
        assert status[b] == 0
        assert err <= bar and np.abs(blocks[b] - MR.blocks_of(inv, K)).max() <= bar


def test_a_frame_without_correspondences_and_no_dense_term(gpu):
    """solve_ref's no_corr_frame window with the dense weight 0: nothing constrains that frame, its block of the matrix is zero, the status names its
    first unknown; the instance beside it in the batch has the covariances it has alone."""
    K, frame = 7, 3
    seed = SR._seeds(K, 1)[0]
    inp = Inputs(gpu, K, (seed, seed), no_corr_frames=[frame, None], weight_dense_depth=0.0)
    info, _, _ = inp.linearize(gpu.ws)
    H = info.cpu().numpy()
    s = slice(6 * (frame - 1), 6 * frame)
    assert not H[0][s, :].any() and not H[0][:, s].any() and H[1][s, s].any()
    out = gpu.cov(gpu.ws, info, full=True)
    solo = gpu.cov(gpu.ws, info[1:2].contiguous(), full=True)
    gpu.ws.sync()
    assert out.status.cpu().tolist() == [1 + 6 * (frame - 1), 0]
    assert np.isnan(out.full[0].cpu().numpy()).all() and np.isnan(out.blocks[0].cpu().numpy()).all() and float(out.pivot_ratio[0]) == 0.0
    assert out.full[1].cpu().numpy().tobytes() == solo.full[0].cpu().numpy().tobytes()
    assert out.blocks[1].cpu().numpy().tobytes() == solo.blocks[0].cpu().numpy().tobytes()
    assert np.isfinite(out.full[1].cpu().numpy()).all()
