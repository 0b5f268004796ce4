"""The objective report (btba_objective_batch_zn_aux, BatchSolver.objective_zn) against the fp64 reference of tests/objective_ref.py, evaluated at
the matrices the device forms of the poses (shared_checks.device_matrices), so both sides read the same matrices.

Per dense pair and per correspondence segment: count exact where the reference has no borderline pixel (within [accepts, accepts + borderline]
otherwise), n_outlier within [sure, sure + knee-borderline (+ borderline)], |sum - ref| <= Bud + gamma Sc for both sums with gamma = 4 x the
float32 restatement's floor (computed by this run, tests/objective_ref.floors), max_abs between the reference's two maxima to within a gamma-scaled
rs, worst the reference's index wherever its runner-up is further below than that margin.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

import objective_ref as OR
import sweep_ref as R
from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S
from bundletrack_amd.objective import residual_variance
from shared_checks import device_matrices

pytestmark = pytest.mark.gpu
SIX = OR.ALL_PAIRS


@pytest.fixture(scope="module")
def gpu(oracle):
    import torch
    assert torch.cuda.is_available()
    from bundletrack_amd.optimizer import BatchSolver, Workspace, pack_zn

    class G:
        pass
    g = G()
    g.torch, g.dev, g.ws = torch, torch.device("cuda:0"), Workspace()
    g.BatchSolver, g.pack_zn, g.Workspace = BatchSolver, pack_zn, Workspace
    g.refs = {}
    return g


@pytest.fixture(scope="module")
def gamma(oracle):
    gm = OR.gammas()
    print("\ngamma = 4 x float32 floor:", {k: f"{v:.3e}" for k, v in gm.items()})
    return gm


def refs_of(g, name, pairs):
    key = (name, tuple(pairs))
    if key not in g.refs:
        sc = R.scene(name)
        T, Tinv = device_matrices(g, sc["poses"])
        g.refs[key] = OR.scene_pairs(sc, T, Tinv, pairs)
    return g.refs[key]


class SceneBatch:
    """the scenes `names` (same cache shape) as one batch of compact caches with their 3 x 40 correspondences"""

    def __init__(self, g, names):
        t = g.torch
        self.g, self.scs = g, [R.scene(n) for n in names]
        cam = t.from_numpy(np.stack([s["campos"] for s in self.scs])).to(g.dev)
        nrm = t.from_numpy(np.stack([s["normals"] for s in self.scs])).to(g.dev)
        self.zn = g.pack_zn(g.ws, cam, nrm)
        B = len(names)
        corr = np.stack([s["corr"] for s in self.scs])
        self.corr = t.from_numpy(corr.view(np.uint8).reshape(B, -1, 32)).to(g.dev)
        self.offs = t.from_numpy(np.tile(np.arange(4, dtype=np.int32) * 40, (B, 1))).to(g.dev)
        self.mx = 40
        self.poses0 = np.stack([s["poses"] for s in self.scs]).astype(np.float32)

    def args(self, poses):
        s = self.scs[0]
        return (self.zn, s["H"], s["W"], s["K"], self.corr, self.offs, self.mx, poses)

    def poses(self):
        return self.g.torch.from_numpy(self.poses0.copy()).to(self.g.dev)

    def objective(self, pairs=None, ws=None, **prm):
        bs = self.g.BatchSolver(ws or self.g.ws, **prm)
        dp = None if pairs is None else np.asarray(pairs, np.int32)
        poses = self.poses()
        out = bs.objective_zn(*self.args(poses), dense_pairs=dp)
        assert poses.cpu().numpy().tobytes() == self.poses0.tobytes(), "the call wrote to its poses"
        return out

    def traced_counts(self, pairs):
        bs = self.g.BatchSolver(self.g.ws, n_gn_iters=1)
        bs.params.pair_policy = _lib.PAIRS_EXPLICIT
        tr = bs.solve_zn(*self.args(self.poses()), dense_pairs=np.asarray(pairs, np.int32), trace=True)
        return bs.trace_view(tr).dense_pair[:, 0, :, 27]


def check_dense(name, recs, refs, pairs, gm, traced=None):
    worst = np.zeros(2)
    for q, ((i, j), rec, ref) in enumerate(zip(pairs, recs, refs)):
        margin = gm["dense_res"] * max(ref["rs_max"], ref["rs_worst"])
        e_sq, e_rho = OR.normalised(rec["sum_sq"], ref["sum_sq"], ref["bud_sq"], ref["sc_sq"]), OR.normalised(rec["sum_rho"], ref["sum_rho"], ref["bud_rho"], ref["sc_rho"])
        gap = ref["max_abs"] - ref["runner_up"]
        print(f"{name:11s} ({i}, {j}): count {rec['count']} (ref {ref['count']} + {ref['borderline']}) outliers {rec['n_outlier']} (sure {ref['n_out_sure']} knee {ref['n_knee']}) "
              f"sum_sq {rec['sum_sq']:.9e} err {e_sq:.2e} Sc  sum_rho {rec['sum_rho']:.9e} err {e_rho:.2e} Sc  (bars {gm['dense_sq']:.2e} / {gm['dense_rho']:.2e})  "
              f"max {rec['max_abs']:.6e} (ref {ref['max_abs']:.6e} .. {ref['max_any']:.6e}) worst {rec['worst']} (ref {ref['worst']}, gap {gap:.2e}, margin {margin:.2e})"
              + (f" traced count {int(traced[q])}" if traced is not None else ""))
        worst = np.maximum(worst, (e_sq, e_rho))
        if ref["borderline"] == 0:
            assert rec["count"] == ref["count"]
        assert ref["count"] <= rec["count"] <= ref["count"] + ref["borderline"]
        assert ref["n_out_sure"] <= rec["n_outlier"] <= ref["n_out_sure"] + ref["n_knee"] + ref["borderline"]
        assert e_sq <= gm["dense_sq"] and e_rho <= gm["dense_rho"]
        assert rec["reserved"] == 0
        if rec["count"] == 0:
            assert rec["max_abs"] == 0 and rec["worst"] == -1 and rec["sum_sq"] == 0 and rec["sum_rho"] == 0
        else:
            assert ref["max_abs"] - margin <= rec["max_abs"] <= ref["max_any"] + margin
            if ref["borderline"] == 0 and gap > 2 * margin:
                assert rec["worst"] == ref["worst"]
            else:
                print(f"    worst not compared: the runner-up is {gap:.3e} below the maximum, margin {margin:.3e}, borderline {ref['borderline']}")
        if traced is not None and ref["borderline"] == 0:
            assert rec["count"] == int(traced[q]), "the report's accept set is not the solver's"
    return worst


@pytest.mark.parametrize("name", OR.SMALL_SCENES)
def test_dense_small_scenes(gpu, gamma, name):
    sb = SceneBatch(gpu, [name])
    total, sparse, dense = sb.objective(pairs=SIX)
    check_dense(name, dense[0], refs_of(gpu, name, SIX), SIX, gamma, traced=sb.traced_counts(SIX)[0])
    _, _, rev = sb.objective(pairs=R.PAIRS_REV)
    check_dense(name + " rev", rev[0], refs_of(gpu, name, R.PAIRS_REV), R.PAIRS_REV, gamma)
    assert rev[0].tobytes() == dense[0][3:].tobytes(), "a pair's record depends on the list it is in"
    _, _, fwd = sb.objective()                     # no list: every i < j as (target i, source j)
    assert fwd[0].tobytes() == dense[0][:3].tobytes()
    assert total["n_dense"][0] == dense[0]["count"].sum() and total["n_sparse"][0] == sparse[0]["count"].sum() == 120


def test_dense_full_size_scene(gpu, gamma):
    name = "bg160x120"
    sb = SceneBatch(gpu, [name])
    _, _, dense = sb.objective(pairs=SIX)
    check_dense(name, dense[0], refs_of(gpu, name, SIX), SIX, gamma)


# ---- sparse ------------------------------------------------------------------------------------------------------------------------
def sparse_inputs(g, N, corr, offs):
    t = g.torch
    zn = t.zeros((1, N, 2, 2, 4), dtype=t.float32, device=g.dev)
    corr_d = t.from_numpy(corr.view(np.uint8).reshape(1, -1, 32)).to(g.dev)
    offs_d = t.from_numpy(offs.astype(np.int32)[None]).to(g.dev)
    mx = int(np.diff(offs.astype(np.int64)).max())
    K = np.array([[4.0, 0, 4.0], [0, 4.0, 4.0], [0, 0, 1]], np.float32)
    return zn, 8, 8, K, corr_d, offs_d, mx


@pytest.mark.parametrize("N", (2, 3, 5))
@pytest.mark.parametrize("c24", (False, True), ids=("entryj", "corr24"))
def test_sparse_segments(gpu, gamma, N, c24):
    corr, offs, pose_sets, (p_out, k_out) = OR.two_sided_case(N)
    zn, H, W, K, corr_d, offs_d, mx = sparse_inputs(gpu, N, corr, offs)
    bs = gpu.BatchSolver(gpu.ws, weight_dense_depth=0.0)
    aux = {"corr24": bs.pack_correspondences24(corr_d, offs_d, mx, N)} if c24 else None
    for s, poses in enumerate(pose_sets):
        T, _ = device_matrices(gpu, poses)
        refs = OR.sparse_window(corr, offs, T)
        poses_d = gpu.torch.from_numpy(poses.copy()).to(gpu.dev)[None].contiguous()
        total, sparse, dense = bs.objective_zn(zn, H, W, K, None if c24 else corr_d, offs_d, mx, poses_d, aux=aux, corr_stride=corr_d.shape[1])
        assert poses_d.cpu().numpy().tobytes() == poses.tobytes()
        for p, (rec, ref) in enumerate(zip(sparse[0], refs)):
            e_sq, e_rho = OR.normalised(rec["sum_sq"], ref["sum_sq"], 0, ref["sc_sq"]), OR.normalised(rec["sum_rho"], ref["sum_rho"], 0, ref["sc_rho"])
            margin = gamma["sparse_res"] * ref["rs_worst"]
            gap = ref["max_abs"] - ref["runner_up"]
            print(f"N {N} set {s} segment {p} ({int(offs[p + 1] - offs[p])} entries): count {rec['count']} (ref {ref['count']}) outliers {rec['n_outlier']} (sure {ref['n_out_sure']} knee {ref['n_knee']}) "
                  f"sum_sq err {e_sq:.2e} Sc sum_rho err {e_rho:.2e} Sc (bars {gamma['sparse_sq']:.2e} / {gamma['sparse_rho']:.2e}) max {rec['max_abs']:.6e} (ref {ref['max_abs']:.6e}) "
                  f"worst {rec['worst']} (ref {ref['worst']}, gap {gap:.2e}, margin {margin:.2e})")
            assert rec["count"] == ref["count"]
            assert ref["n_out_sure"] <= rec["n_outlier"] <= ref["n_out_sure"] + ref["n_knee"]
            assert e_sq <= gamma["sparse_sq"] and e_rho <= gamma["sparse_rho"]
            if ref["count"] == 0:
                assert rec["max_abs"] == 0 and rec["worst"] == -1 and rec["sum_sq"] == 0
            else:
                assert abs(rec["max_abs"] - ref["max_abs"]) <= margin
                if gap > 2 * margin:
                    assert rec["worst"] == ref["worst"]
        if s == 1:
            assert sparse[0][p_out]["worst"] == k_out, "the planted 7 cm match is not the worst"
        assert total["dense_rho"][0] == 0 and total["n_dense"][0] == 0 and np.all(dense[0]["worst"] == -1) and not dense[0]["count"].any()
        assert total["n_residuals"][0] == 3 * total["n_sparse"][0]


# ---- totals, weights -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", ((1.0, 1.0), (0.5, 2.0), (1.0, 0.0)), ids=("1_1", "0.5_2", "1_0"))
def test_totals_are_the_fold_of_the_pair_records(gpu, w):
    sb = SceneBatch(gpu, ["bg50x30"])
    total, sparse, dense = sb.objective(weight_sparse=w[0], weight_dense_depth=w[1])
    t = total[0]
    want = {k: OR.fold(recs, f) for k, recs, f in (("sparse_rho", sparse[0], "sum_rho"), ("sparse_sq", sparse[0], "sum_sq"), ("dense_rho", dense[0], "sum_rho"), ("dense_wsq", dense[0], "sum_sq"))}
    objective = np.float64(np.float32(w[0])) * want["sparse_rho"] + np.float64(np.float32(w[1])) * want["dense_rho"]
    print(f"weights {w}: objective {t['objective']!r} (fold {objective!r}) sparse_rho {t['sparse_rho']!r} dense_rho {t['dense_rho']!r} n {t['n_sparse']} / {t['n_dense']} / {t['n_residuals']}")
    for k, v in want.items():
        assert t[k] == v, k
    assert t["objective"] == objective
    assert t["n_sparse"] == int(sparse[0]["count"].sum()) and t["n_dense"] == int(dense[0]["count"].sum()) and t["n_residuals"] == 3 * t["n_sparse"] + t["n_dense"]
    if w[1] == 0.0:
        assert dense.shape == (1, 3) and not dense[0]["count"].any() and np.all(dense[0]["worst"] == -1) and not dense[0]["sum_rho"].any() and t["dense_rho"] == 0
    else:
        assert dense[0]["count"].all() and t["dense_rho"] > 0
    assert t["sparse_rho"] > 0


def test_batch_position(gpu):
    names = ("bg32x24", "hole32x24", "edge32x24")
    alone = SceneBatch(gpu, [names[0]]).objective(pairs=SIX)
    three = SceneBatch(gpu, [names[0], names[1], names[0]]).objective(pairs=SIX)
    for what, a, b in zip(("total", "sparse", "dense"), alone, three):
        print(f"{what}: alone == item 0 {a[0].tobytes() == b[0].tobytes()}, alone == item 2 {a[0].tobytes() == b[2].tobytes()}")
        assert a[0].tobytes() == b[0].tobytes() == b[2].tobytes()
        assert b[1].tobytes() != b[0].tobytes()


def test_a_later_solve_and_the_stats_are_untouched(gpu):
    sb = SceneBatch(gpu, ["bg32x24"])

    def solve(ws):
        bs = gpu.BatchSolver(ws, n_gn_iters=7)
        poses = sb.poses()
        bs.solve_zn(*sb.args(poses))
        ws.sync()
        return poses.cpu().numpy()

    ws_a, ws_b = gpu.Workspace(), gpu.Workspace()
    first = solve(ws_a)
    keep = {k: v for k, v in ws_a.collect_stats().items() if not k.startswith("ms_")}
    sb.objective(ws=ws_a, pairs=R.PAIRS_REV)
    sb.objective(ws=ws_a)
    after_stats = {k: v for k, v in ws_a.collect_stats().items() if not k.startswith("ms_")}
    print("stats of the solve:", keep)
    assert after_stats == keep and keep["n_frames"] == 3
    after, fresh = solve(ws_a), solve(ws_b)
    assert first.tobytes() == fresh.tobytes() == after.tobytes(), "a solve after the report differs from the same solve without it"


def test_descent_on_the_smoke_window(gpu):
    pb = S.make_problem(4, 200, seed=7, background=False)
    t = gpu.torch
    corr, offs, mx = gpu.BatchSolver.pack_correspondences([pb.corr], 4)
    zn = t.from_numpy(S.compact_cache(pb)[None]).to(gpu.dev)
    corr_d = t.from_numpy(corr.view(np.uint8).reshape(1, -1, 32)).to(gpu.dev)
    offs_d = t.from_numpy(offs.astype(np.int32)).to(gpu.dev)
    poses = t.from_numpy(pb.poses_init.astype(np.float32)[None].copy()).to(gpu.dev)
    bs = gpu.BatchSolver(gpu.ws, n_gn_iters=7)
    args = (zn, pb.H, pb.W, pb.K, corr_d, offs_d, mx)
    before = bs.objective_zn(*args, poses)
    bs.solve_zn(*args, poses)
    after = bs.objective_zn(*args, poses)
    out = lambda r: int(r[1]["n_outlier"].sum() + r[2]["n_outlier"].sum())
    print(f"objective {before[0]['objective'][0]:.9e} -> {after[0]['objective'][0]:.9e}; outliers {out(before)} -> {out(after)}; residuals {before[0]['n_residuals'][0]} -> {after[0]['n_residuals'][0]}; "
          f"residual variance {residual_variance(before[0], 4)[0]:.6e} -> {residual_variance(after[0], 4)[0]:.6e}")
    assert after[0]["objective"][0] < before[0]["objective"][0]
    assert out(after) <= out(before)
    assert np.isnan(residual_variance(np.zeros(1, _lib.OBJECTIVE_TOTAL_DTYPE), 4)[0])


def test_invalid_arguments_return_before_any_launch(gpu):
    sb = SceneBatch(gpu, ["bg32x24"])
    L = _lib.lib()
    s = sb.scs[0]
    Kf = np.ascontiguousarray(s["K"], np.float32).reshape(9)
    poses = sb.poses()
    out = gpu.torch.zeros((256,), dtype=gpu.torch.uint8, device=gpu.dev)
    prm = _lib.default_params()
    hip_error = L.btba_last_hip_error()

    def call(ws=gpu.ws.handle, prm_=prm, B=1, N=3, poses_p=poses.data_ptr(), total_p=out.data_ptr()):
        return L.btba_objective_batch_zn_aux(ws, C.byref(prm_) if prm_ is not None else None, B, N, s["H"], s["W"], Kf.ctypes.data, sb.zn.data_ptr(), None, sb.corr.data_ptr(), 120,
                                             sb.offs.data_ptr(), 40, None, 0, poses_p, total_p, None, None)

    assert call() == _lib.BTBA_OK
    gpu.ws.sync()
    wprm = _lib.default_params()
    w = np.ones(7, np.float32)
    wprm.weights_dense_per_iter, wprm.n_weights_per_iter = w.ctypes.data, 7
    cases = dict(null_ws=dict(ws=None), null_params=dict(prm_=None), null_poses=dict(poses_p=None), null_total=dict(total_p=None), no_instance=dict(B=0), one_frame=dict(N=1),
                 too_many_frames=dict(N=86), per_iteration_weights=dict(prm_=wprm), misaligned_total=dict(total_p=out.data_ptr() + 4))
    out.zero_()
    gpu.ws.sync()
    for name, kw in cases.items():
        rc = call(**kw)
        print(f"{name}: {rc}")
        assert rc == _lib.BTBA_EINVAL, name
    gpu.ws.sync()
    assert not out.cpu().numpy().any(), "a refused call launched something"
    assert L.btba_last_hip_error() == hip_error
