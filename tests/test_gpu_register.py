"""Frame-to-model registration on the MI355X (btba_register_index, btba_register_frames, btba_register_associate) against the numpy
restatement tests/register_ref.py.  Teacher-forced, so that no decision can cascade: iteration t of the reference starts from the device's own
pose of iteration t - 1 in the trace.  Per iteration: the match array, the three counts and the status with ==; H, g and cost within
n 2^-53 sum|term| of the exact sums (the device rounds every term as the restatement does and differs only in the order of at most n - 1
additions); xi against a float64 solve of the device's own H, g within 2 * 6 * 2^-53 kappa_2(H) |xi| (both solves are backward stable, in the
manner of tests/marginals_ref.py); the pose against Exp(xi_device) pose[t - 1] within one float32 ulp per entry plus 1e-15 for the float64
products behind the single rounding.  Small shapes; one module-scoped workspace and scene."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fusion_ref as R
import register_ref as G
from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S

F = np.float32
U = 2.0 ** -53
EYE = np.eye(4, dtype=F)


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


@pytest.fixture(scope="module")
def scene(oracle):
    return G.ellipsoid_scene(oracle)


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cloud(models, boxes, leaf, capacity=None):
    """Reference models (fusion_ref.fuse dicts) as one ObjectCloud on the device, padded (or cut) to `capacity` records per instance."""
    from bundletrack_amd.fusion import ObjectCloud
    B = len(models)
    cap = max(1, max(m["n_out"] for m in models)) if capacity is None else capacity
    xyz, nrm, lin = np.zeros((B, cap, 4), F), np.zeros((B, cap, 4), F), np.full((B, cap), -7, np.int32)
    for b, m in enumerate(models):
        k = min(m["n_out"], cap)
        xyz[b, :k], nrm[b, :k], lin[b, :k] = m["xyz"][:k], m["normal"][:k], m["lin"][:k]
    n_out = np.array([m["n_out"] for m in models], np.int32)
    return ObjectCloud(xyz=_t(xyz), normal=_t(nrm), colour=None, count=None, lin=_t(lin), n_out=_t(n_out), n_outside=None, status=None,
                       box=np.ascontiguousarray(boxes, np.int32).reshape(B, 6), leaf=float(leaf))


def _dev(segs):
    from bundletrack_amd.fusion import Segment
    return [Segment(s["instance"], s["pose"], depth=_t(s.get("depth")), xyz=_t(s.get("xyz")), normal=_t(s.get("normal"))) for s in segs]


def _cut(model, capacity):
    return model if capacity is None else {k: (v[:capacity] if isinstance(v, np.ndarray) else v) for k, v in model.items()}


def _pose4(p):
    T = EYE.copy()
    T[:3] = np.asarray(p, F).reshape(3, 4)
    return T


def _check_items(ws, index, segs, models, prm, K, Ki, capacity=None):
    """register_frames (traced) and associate of `segs` against `index`, every traced iteration held to the restatement started from the
    device's previous pose.  Returns the Registration."""
    import torch
    from bundletrack_amd.registration import associate, register_frames
    kw = {k: v for k, v in prm.items() if k != "leaf"}
    dev = _dev(segs)
    reg = register_frames(ws, index, dev, K, trace=True, **kw)
    torch.cuda.synchronize()
    res, trace, pose_out = reg.result, reg.trace, reg.pose.cpu().numpy()
    box = index.cloud.box
    for i, seg in enumerate(segs):
        b = seg["instance"]
        model = _cut(models[b], capacity)
        cells = G.cell_index(models[b], box[b], capacity)
        T = np.asarray(seg["pose"], F)[:3]
        starts, alive = [T], True
        for t in range(prm["n_iters"]):
            e = trace[i, t] if trace is not None else None
            if not alive:
                assert e["status"] == G.SKIPPED and not np.frombuffer(e.tobytes(), np.uint8)[16:].any() and e["n_valid"] == e["n_matched"] == e["n_beyond"] == 0, (i, t)
                continue
            ref = G.step(seg, T, model, box[b], prm, Ki, cells)
            where = f"item {i} iteration {t}"
            assert (e["n_valid"], e["n_matched"], e["n_beyond"]) == (ref["n_valid"], ref["n_matched"], ref["n_beyond"]), where
            n = max(ref["n_matched"], 1)
            for name, absname in (("H", "abs_H"), ("g", "abs_g")):
                err, bar = np.abs(e[name] - ref[name]), n * U * ref[absname]
                assert (err <= bar).all(), (where, name, err, bar)
            assert abs(e["cost"] - ref["cost"]) <= n * U * ref["cost"], where
            status = G.TOO_FEW if e["n_matched"] < prm["min_matches"] else None
            if status is None:
                status, xi, ratio = G.solve(e["H"], e["g"])                       # of the device's own sums
                if status != G.DEGENERATE:
                    kappa = np.linalg.cond(G.full(e["H"]), 2)
                    bar = 2 * 6 * U * kappa * np.linalg.norm(xi)
                    assert (np.abs(e["xi"] - xi) <= bar).all(), (where, e["xi"], xi, bar)
                    assert abs(e["pivot_ratio"] - ratio) <= 6 * U * kappa * ratio, where
                    want = G.update(T, e["xi"]).astype(np.float64)
                    got = e["pose"].reshape(3, 4).astype(np.float64)
                    assert (np.abs(got - want) <= np.spacing(np.abs(want).astype(F)).astype(np.float64) + 1e-15).all(), (where, got, want)
                    if np.linalg.norm(e["xi"][:3]) < float(F(prm["eps_rot"])) and np.linalg.norm(e["xi"][3:]) < float(F(prm["eps_trans"])):
                        status = G.CONVERGED
            assert e["status"] == status, (where, e["status"], status)
            if status in (G.TOO_FEW, G.DEGENERATE):
                assert not e["xi"].any() and e["pose"].tobytes() == T.tobytes(), where
            T = e["pose"].reshape(3, 4).copy()
            starts.append(T)
            alive = status == G.MAX_ITERS
        done = len(starts) - 1
        final = G.accumulate(seg, T, model, box[b], prm, Ki, cells)
        want_status = trace[i, done - 1]["status"] if done else (G.TOO_FEW if final["n_matched"] < prm["min_matches"] else G.MAX_ITERS)
        assert (res[i]["status"], res[i]["iters_done"]) == (want_status, done), (i, res[i], want_status, done)
        assert (res[i]["n_valid"], res[i]["n_matched"], res[i]["n_beyond"]) == (final["n_valid"], final["n_matched"], final["n_beyond"]), i
        assert abs(res[i]["cost"] - final["cost"]) <= max(final["n_matched"], 1) * U * final["cost"], i
        assert pose_out[i].tobytes() == T.tobytes(), i
        # the association at the initial and at every traced pose, in one call
        at = [dict(seg, pose=_pose4(p)) for p in starts]
        got = associate(ws, index, _dev(at), K, **kw)
        for p, g in zip(starts, got):
            want = G.associate(seg, p, model, box[b], prm, Ki, cells)[0]
            assert np.array_equal(g.cpu().numpy().reshape(-1), want), (i, (g.cpu().numpy().reshape(-1) != want).sum())
    return reg


@pytest.fixture(scope="module")
def index(ws, scene):
    from bundletrack_amd.registration import build_index
    return build_index(ws, _cloud([scene["model"]], scene["box"], scene["leaf"]))


def test_index_is_the_restatements(ws, scene, index):
    assert np.array_equal(index.cell_index.cpu().numpy(), G.cell_index(scene["model"], scene["box"][0]))


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_frame_48x64_every_iteration(ws, scene, index, radius):
    """A 48 x 64 frame is two workgroups' partial records; from 5 degrees / 10 mm."""
    seg = dict(scene["segs"][3], pose=G.perturbed(scene["segs"][3]["pose"], 5.0, 10.0, seed=3))
    prm = G.params(scene["leaf"], n_iters=6, search_radius=radius)
    reg = _check_items(ws, index, [seg], [scene["model"]], prm, scene["K"], scene["Ki"])
    print("radius", radius, reg.status_names, "iterations", reg.iterations, "fitness", reg.fitness, "rms", reg.rms)
    assert reg.n_valid[0] > 500 and (radius == 0 or reg.fitness[0] == 1.0)


def test_frame_7x5_less_than_a_wave(ws, scene, index, oracle):
    K = R.small_K(5, 7)
    pose = R.look_at_pose((0.1, 0.05, -0.45))
    d, n = G.ellipsoid_frame(pose, K, 5, 7)
    seg = {"instance": 0, "pose": G.perturbed(pose, 1.0, 2.0, seed=9), "depth": d, "normal": n}
    reg = _check_items(ws, index, [seg], [scene["model"]], G.params(scene["leaf"], n_iters=3), K, R.kinv4(oracle, K))
    print("7 x 5:", reg.n_valid, reg.n_matched, reg.status_names)
    assert 0 < reg.n_valid[0] < 35


def test_point_lists_of_0_1_65_5000_and_10000(ws, scene, index):
    """10 000 points are five workgroups' partial records, summed in index order by the solve."""
    rng = np.random.default_rng(12)
    surf = scene["model"]["xyz"][:, :3]
    segs = []
    for k, n in enumerate((0, 1, 65, 5000, 10000)):
        pts = surf[rng.integers(0, len(surf), n)] + rng.normal(size=(n, 3)).astype(F) * F(0.002)
        xyz = np.concatenate([pts, np.ones((n, 1))], 1).astype(F)
        if n == 5000:
            xyz[7, 0], xyz[4000, 2] = np.nan, np.inf                     # dropped
        segs.append({"instance": 0, "pose": G.perturbed(EYE, 3.0, 4.0, seed=20 + k), "xyz": xyz, "normal": None})
    reg = _check_items(ws, index, segs, [scene["model"]], G.params(scene["leaf"], n_iters=4), None, None)
    print(reg.status_names, reg.n_valid, reg.n_matched)
    assert reg.status[0] == reg.status[1] == G.TOO_FEW and reg.n_valid.tolist() == [0, 1, 65, 4998, 10000] and reg.n_matched[3] > 4000 and reg.n_matched[4] > 8000


def _grid_model(dims, leaf, normal):
    nx, ny, nz = dims
    lin = np.arange(nx * ny * nz)
    ix, iy, iz = lin % nx, (lin // nx) % ny, lin // (nx * ny)
    xyz = np.stack([(ix + 0.5) * leaf, (iy + 0.5) * leaf, (iz + 0.5) * leaf, np.ones(len(lin))], 1).astype(F)
    return {"xyz": xyz, "normal": np.tile(np.array([*normal, 0.0], F), (len(lin), 1)), "lin": lin.astype(np.int32), "n_out": len(lin)}, \
        np.array([[0, 0, 0, nx, ny, nz]], np.int32)


def _list(pts, normals=None, pose=EYE):
    pts = np.asarray(pts, F).reshape(-1, 3)
    nrm = None if normals is None else np.concatenate([np.asarray(normals, F).reshape(-1, 3), np.zeros((len(pts), 1), F)], 1)
    return {"instance": 0, "pose": pose, "xyz": np.concatenate([pts, np.ones((len(pts), 1), F)], 1), "normal": nrm}


@pytest.mark.parametrize("capacity", [None, 5])
def test_2x2x2_model_ties_gates_and_a_cut_capacity(ws, capacity):
    """The constructed model of tests/test_register_ref.py: ties, the centre cell outside the box, each gate one ulp on either side.  With
    capacity 5 of n_out 8 the index holds records 0 .. 4 only."""
    from bundletrack_amd.registration import build_index
    model, box = _grid_model((2, 2, 2), 1.0, (1.0, 0.0, 0.0))
    idx = build_index(ws, _cloud([model], box, 1.0, capacity))
    assert np.array_equal(idx.cell_index.cpu().numpy(), G.cell_index(model, box[0], capacity))
    up, down = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(-np.inf))
    pts = [[1.0, 0.5, 0.5], [1.0, 1.0, 1.0], [0.5, 1.0, 1.5], [1.25, 0.5, 0.5], [-0.25, 0.5, 0.5], [-1.25, 0.5, 0.5], [down(0.75), 0.5, 0.5], [0.75, 0.5, 0.5],
           [up(0.75), 0.5, 0.5], [65536.0, 0.5, 0.5], [np.nan, 0.5, 0.5], [down(0.625), 0.5, 0.5], [0.625, 0.5, 0.5], [up(0.625), 0.5, 0.5], [1.5, 1.5, 1.5]]
    nrm = [[down(0.5), 0.8, 0], [0.5, 0.8, 0], [up(0.5), 0.8, 0]] * 5
    for seg, kw in ((_list(pts), dict(max_dist=1.0, min_cos=-1.0)), (_list(pts), dict(max_dist=0.25, min_cos=-1.0, huber_delta=0.125)),
                    (_list(pts), dict(max_dist=2.0, min_cos=-1.0, search_radius=2, huber_delta=0.125)), (_list(pts), dict(max_dist=2.0, search_radius=0)),
                    (_list(pts, nrm), dict(max_dist=1.0, min_cos=0.5)), (_list(pts, nrm), dict(max_dist=1.0, min_cos=-1.0))):
        reg = _check_items(ws, idx, [seg], [model], G.params(1.0, n_iters=1, **kw), None, None, capacity)
        assert reg.n_valid[0] == len(pts) - 1


def test_six_items_three_instances_copies_and_reruns(ws, scene):
    """Instance 1 is an empty model, item 3 a frame without a valid pixel: TOO_FEW, the pose returned unchanged, no fault.  Item 5 is a copy of
    item 1 and gives its bytes (pose, result, trace); the whole call twice gives the same bytes."""
    import torch
    from bundletrack_amd.registration import build_index, register_frames
    empty = {"xyz": np.zeros((0, 4), F), "normal": np.zeros((0, 4), F), "lin": np.zeros(0, np.int32), "n_out": 0}
    segs7 = scene["segs"]
    box2 = R.bounds(segs7[:3], 1, scene["Ki"], scene["leaf"])                 # instance 2: a model of three of the views, in a box of its own
    model2 = R.fuse(segs7[:3], 1, scene["Ki"], box2, scene["leaf"], normalize_normals=True, with_colour=False)[0]
    models = [scene["model"], empty, model2]
    boxes = np.concatenate([scene["box"], np.zeros((1, 6), np.int32), box2])
    idx = build_index(ws, _cloud(models, boxes, scene["leaf"]))
    off = idx.voxel_offsets
    cells = idx.cell_index.cpu().numpy()
    assert np.array_equal(cells[off[0]:off[1]], G.cell_index(models[0], boxes[0])) and off[1] == off[2]
    assert np.array_equal(cells[off[2]:off[3]], G.cell_index(model2, boxes[2]))
    blank = dict(segs7[2], depth=np.zeros_like(segs7[2]["depth"]))
    mk = lambda v, inst, seed: dict(segs7[v], instance=inst, pose=G.perturbed(segs7[v]["pose"], 3.0, 6.0, seed=seed))
    segs = [mk(0, 0, 1), mk(1, 2, 2), mk(4, 1, 3), dict(blank, instance=0), mk(5, 0, 4)]
    segs.append(dict(segs[1]))
    prm = G.params(scene["leaf"], n_iters=4)
    reg = _check_items(ws, idx, segs, models, prm, scene["K"], scene["Ki"])
    print(reg.status_names, reg.n_valid, reg.n_matched)
    assert reg.status[2] == reg.status[3] == G.TOO_FEW and reg.n_valid[3] == 0 and reg.n_matched[2] == 0
    pose = reg.pose.cpu().numpy()
    for i in (2, 3):
        assert pose[i].tobytes() == np.asarray(segs[i]["pose"], F)[:3].tobytes()
    raw = lambda r: (r.pose.cpu().numpy().tobytes(), r.result_dev.cpu().numpy(), r.trace_dev.cpu().numpy())
    p, res, tr = raw(reg)
    assert pose[5].tobytes() == pose[1].tobytes() and res[5].tobytes() == res[1].tobytes() and tr[5].tobytes() == tr[1].tobytes()
    again = register_frames(ws, idx, _dev(segs), scene["K"], trace=True, n_iters=4)
    torch.cuda.synchronize()
    p2, res2, tr2 = raw(again)
    assert p2 == p and res2.tobytes() == res.tobytes() and tr2.tobytes() == tr.tobytes()
    alone = register_frames(ws, idx, _dev(segs[1:2]), scene["K"], trace=True, n_iters=4)      # and alone in a call: any n_items
    torch.cuda.synchronize()
    p1, res1, tr1 = raw(alone)
    assert p1 == pose[1].tobytes() and res1[0].tobytes() == res[1].tobytes() and tr1[0].tobytes() == tr[1].tobytes()


def test_zero_iterations_evaluate_a_calls_pose_out(ws, scene, index):
    """The result's evaluated fields (n_valid, n_matched, n_beyond, cost) of a call equal, byte for byte, those of an n_iters = 0 call at its
    pose_out; that call returns the pose unchanged with status MAX_ITERS and iters_done 0.  (status and iters_done describe the loop, which the
    second call does not run: they are not part of the identity.)"""
    import torch
    from bundletrack_amd.registration import register_frames
    segs = [dict(scene["segs"][v], pose=G.perturbed(scene["segs"][v]["pose"], 4.0, 8.0, seed=30 + v)) for v in (2, 6)]
    first = register_frames(ws, index, _dev(segs), scene["K"], n_iters=5)
    at = [dict(s, pose=T) for s, T in zip(segs, first.poses4())]
    check = register_frames(ws, index, _dev(at), scene["K"], n_iters=0, trace=True)
    torch.cuda.synchronize()
    a, b = first.result, check.result
    for k in ("n_valid", "n_matched", "n_beyond", "cost"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert first.result_dev.cpu().numpy()[:, 8:].tobytes() == check.result_dev.cpu().numpy()[:, 8:].tobytes()
    assert b["status"].tolist() == [G.MAX_ITERS] * 2 and b["iters_done"].tolist() == [0, 0] and check.trace.shape == (2, 0)
    assert check.pose.cpu().numpy().tobytes() == first.pose.cpu().numpy().tobytes()
    assert (first.fitness > 0.99).all() and (first.rms < 0.003).all()


def test_plane_model_is_degenerate(ws):
    from bundletrack_amd.registration import build_index
    model, box = _grid_model((6, 5, 1), 0.1, (0.0, 0.0, 1.0))
    idx = build_index(ws, _cloud([model], box, 0.1))
    rng = np.random.default_rng(2)
    pts = np.stack([rng.uniform(0, 0.6, 200), rng.uniform(0, 0.5, 200), rng.uniform(0.03, 0.07, 200)], 1)
    reg = _check_items(ws, idx, [_list(pts)], [model], G.params(0.1, max_dist=0.2, min_cos=-1.0, n_iters=3), None, None)
    assert reg.status[0] == G.DEGENERATE and reg.iterations[0] == 1 and reg.trace[0, 0]["H"][5] == 0.0 and reg.trace[0, 0]["pivot_ratio"] == 0.0
    assert reg.trace[0, 1]["status"] == reg.trace[0, 2]["status"] == G.SKIPPED and reg.pose.cpu().numpy()[0].tobytes() == EYE[:3].tobytes()


def test_converged_item_skips_its_later_iterations(ws, scene, index):
    """From 0.5 degrees / 1 mm, with thresholds of 0.2 mrad / 0.05 mm, the restatement converges at its third iteration of 10; the device's
    later trace entries are zero but for the SKIPPED status (_check_items)."""
    seg = dict(scene["segs"][1], pose=G.perturbed(scene["segs"][1]["pose"], 0.5, 1.0, seed=41))
    prm = G.params(scene["leaf"], n_iters=10, eps_rot=2e-4, eps_trans=5e-5)
    ref = G.register(seg, scene["model"], scene["box"][0], prm, scene["Ki"])
    assert ref["status"] == G.CONVERGED and ref["iters_done"] == 3, (ref["status"], ref["iters_done"])
    reg = _check_items(ws, index, [seg], [scene["model"]], prm, scene["K"], scene["Ki"])
    assert reg.status[0] == G.CONVERGED and reg.iterations[0] == 3 and (reg.trace[0, 3:]["status"] == G.SKIPPED).all()
    rot, trans = G.pose_distance(reg.pose.cpu().numpy()[0], scene["segs"][1]["pose"])
    print(f"{rot * 1e3:.3f} mrad, {trans * 1e3:.3f} mm from the rendering pose")
    assert rot < G.BAR_RAD and trans < G.BAR_M                  # 1.5 x the restatement's floor on this scene (register_ref.FLOOR_*)


def test_bundler_register_to_model(ws, tmp_path):
    """A 4-keyframe synthetic session: the newest frame registered against the session's own fused object stays where bundle adjustment put it
    (well inside the model's 5 mm quantisation), the call changes no state, and n_iters = 0 is the pose check of the same frame."""
    import torch
    from bundletrack_amd.bundler import Bundler, FrameRef
    from bundletrack_amd.optimizer import OptimizerGpu
    from bundletrack_amd.registration import Registration
    n = 4
    seq = S.SyntheticSequence(n_frames=n, seed=S.config_seed(1), background=False)
    fm = S.SyntheticFeatureManager(seq, corr_per_pair=300)
    bundler = Bundler(OptimizerGpu(workspace=ws), fm, seq.K, seq.H, seq.W, window_size=5, max_BA_frames=5, min_rot_deg=0.0, pose_dir=str(tmp_path))
    for k in range(n):
        depth, normals = seq.render(k)[:2]
        fr = FrameRef(id=0, pose_in_model=seq.poses_gt[0].astype(np.float32), n_keypts=300, depth_gpu=_t(depth), normal_gpu=_t(normals))
        fm.register(fr, k)
        bundler.process_new_frame(fr)
        assert fr.status != "FAIL"
    newest = bundler.frames[-1]
    before = np.array(newest.pose_in_model, np.float32).copy()
    n_frames, n_kf = len(bundler.frames), len(bundler.keyframes)
    reg = bundler.register_to_model()
    torch.cuda.synchronize()
    assert isinstance(reg, Registration) and reg.pose.shape == (1, 3, 4)
    assert np.array_equal(np.array(newest.pose_in_model, np.float32), before) and (len(bundler.frames), len(bundler.keyframes)) == (n_frames, n_kf)
    rot, trans = G.pose_distance(reg.pose.cpu().numpy()[0], before)
    print(reg.status_names, "iterations", reg.iterations, "fitness", reg.fitness, "rms", reg.rms, f"moved {rot * 1e3:.3f} mrad {trans * 1e3:.3f} mm")
    assert reg.status[0] in (G.CONVERGED, G.MAX_ITERS) and reg.fitness[0] > 0.95 and reg.rms[0] < 0.002 and rot < 5e-3 and trans < 2.5e-3
    check = bundler.register_to_model(frames=newest, n_iters=0)
    assert check.iterations[0] == 0 and check.pose.cpu().numpy()[0].tobytes() == before[:3].tobytes() and check.fitness[0] > 0.95
