"""Keyframe fusion on the MI355X (btba_fuse_bounds, btba_fuse_frames, btba_voxel_downsample): every output compared byte for byte (==)
with the numpy restatement tests/fusion_ref.py.  Small shapes: 48 x 64 frames of a sphere at 0.5 m, one contended 64 x 64 frame, constructed
edge points, 5 000 random points.  One module-scoped workspace."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fusion_ref as R
from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S

F = np.float32
H, W = 48, 64
LEAF = 0.01


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


@pytest.fixture(scope="module")
def K():
    return R.small_K(H, W)


@pytest.fixture(scope="module")
def Ki(oracle, K):
    return R.kinv4(oracle, K)


@pytest.fixture(scope="module")
def views(K):
    """The sphere from three poses, instance 0 (shared, never modified)."""
    return R.sphere_segments(R.THREE_VIEWS, 0, K, H, W)


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev(segs, colour=True):
    from bundletrack_amd.fusion import Segment
    return [Segment(s["instance"], s["pose"], depth=_t(s.get("depth")), xyz=_t(s.get("xyz")), normal=_t(s.get("normal")),
                    colour=_t(s.get("colour")) if colour else None) for s in segs]


def _host(cloud):
    """Per instance, the device's records trimmed to min(n_out, capacity) as the reference names them, plus the three words."""
    import torch
    torch.cuda.synchronize()
    n_out, n_outside, status = (getattr(cloud, k).cpu().numpy() for k in ("n_out", "n_outside", "status"))
    cap = cloud.xyz.shape[1]
    out = []
    for b in range(len(n_out)):
        k = min(int(n_out[b]), cap)
        d = {"xyz": cloud.xyz[b, :k].cpu().numpy(), "count": cloud.count[b, :k].cpu().numpy().view(np.uint32), "lin": cloud.lin[b, :k].cpu().numpy(),
             "n_out": int(n_out[b]), "n_outside": int(n_outside[b]), "status": int(status[b])}
        if cloud.normal is not None:
            d["normal"] = cloud.normal[b, :k].cpu().numpy()
        if cloud.colour is not None:
            d["colour"] = cloud.colour[b, :k].cpu().numpy()
        out.append(d)
    return out


def _assert_equal(got, ref, keys=("xyz", "normal", "colour", "count", "lin")):
    assert got["n_out"] == ref["n_out"] and got["n_outside"] == ref["n_outside"], (got["n_out"], ref["n_out"], got["n_outside"], ref["n_outside"])
    for k in keys:
        if k in got or k in ref:
            assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
            assert got[k].tobytes() == ref[k].tobytes(), f"{k} differs in {(got[k] != ref[k]).sum()} values"


@pytest.mark.parametrize("normalize_normals", [0, 1])
@pytest.mark.parametrize("require_normals", [0, 1])
@pytest.mark.parametrize("colour", [0, 1])
def test_three_frames_of_a_sphere(ws, K, Ki, views, colour, require_normals, normalize_normals):
    from bundletrack_amd.fusion import fuse_frames
    kw = dict(leaf=LEAF, require_normals=bool(require_normals), normalize_normals=bool(normalize_normals))
    box = R.bounds(views, 1, Ki, LEAF, bool(require_normals))
    ref = R.fuse(views, 1, Ki, box, with_colour=bool(colour), **kw)[0]
    got = _host(fuse_frames(ws, _dev(views, colour), 1, K, box=box, **kw))[0]
    print(f"voxels {ref['n_out']}, points {int(ref['count'].sum())}, most in one voxel {int(ref['count'].max())}")
    assert ref["n_out"] > 300 and ref["count"].max() >= 4 and got["status"] == 0
    assert ("colour" in got) == bool(colour)
    _assert_equal(got, ref)
    if normalize_normals:
        length = np.linalg.norm(got["normal"][:, :3].astype(np.float64), axis=1)
        assert (np.abs(length[length > 0] - 1) < 1e-6).all()


def test_batch_of_six_instances(ws, K, Ki, views):
    """Frame counts (1, 3, 2, 0, 3, 3); instance 5 is a copy of instance 1 and gives its bytes; the whole call twice gives the same bytes (the
    atomics' arrival order does not matter); the instance without frames gives n_out = 0."""
    from bundletrack_amd.fusion import fuse_frames
    other = R.sphere_segments([(0.1, 0.3, -0.45), (-0.3, 0.0, -0.42), (0.0, -0.3, -0.4)], 4, K, H, W, seed=40, radius=0.1)
    segs = [dict(views[0], instance=0)] + [dict(s, instance=1) for s in views] + [dict(s, instance=2) for s in other[:2]] + other + \
           [dict(s, instance=5) for s in views]
    order = np.random.default_rng(0).permutation(len(segs))
    segs = [segs[k] for k in order]                                # instances interleaved: segments name their instance
    box = R.bounds(segs, 6, Ki, LEAF)
    assert (box[3] == 0).all() and (box[1] == box[5]).all()
    ref = R.fuse(segs, 6, Ki, box, LEAF)
    dev = _dev(segs)
    a = fuse_frames(ws, dev, 6, K, leaf=LEAF, box=box)
    got = _host(a)
    b = fuse_frames(ws, dev, 6, K, leaf=LEAF, box=box)
    again = _host(b)
    for i in range(6):
        _assert_equal(got[i], ref[i])
        _assert_equal(again[i], got[i])
        assert got[i]["status"] == 0
    assert got[3]["n_out"] == 0 and got[1]["n_out"] > 300
    _assert_equal(got[5], got[1])
    for k in ("xyz", "normal", "colour", "count", "lin"):           # the padded tensors too: nothing is written behind n_out
        n1 = got[1]["n_out"]
        assert getattr(a, k)[1, :n1].cpu().numpy().tobytes() == getattr(a, k)[5, :n1].cpu().numpy().tobytes()


def test_contention_every_pixel_into_one_voxel(ws, oracle):
    """One 64 x 64 frame at constant depth 0.5 m, a 10 m voxel, a box of dims (1, 1, 1): 4 096 points add to one address."""
    from bundletrack_amd.fusion import fuse_frames
    h = w = 64
    Kc = R.small_K(h, w)
    rng = np.random.default_rng(11)
    nrm = np.zeros((h, w, 4), F)
    nrm[..., :3] = rng.normal(size=(h, w, 3))
    col = np.zeros((h, w, 4), np.uint8)
    col[..., :3] = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    seg = [{"instance": 0, "pose": np.eye(4, dtype=F), "depth": np.full((h, w), 0.5, F), "normal": nrm, "colour": col}]
    Kic = R.kinv4(oracle, Kc)
    box = np.array([[0, 0, 0, 1, 1, 1]], np.int32)
    ref = R.fuse(seg, 1, Kic, box, 10.0)[0]
    # x < 0 or y < 0 for pixels left of / above the principal point: those fall into voxel -1 and are outside this box
    assert ref["n_out"] == 1 and ref["count"][0] + ref["n_outside"] == 4096 and ref["count"][0] == 1024
    got = _host(fuse_frames(ws, _dev(seg), 1, Kc, leaf=10.0, box=box))[0]
    _assert_equal(got, ref)
    box_all = np.array([[-1, -1, 0, 1, 1, 1]], np.int32)            # and the quadrant on the other side, shifted so that all of it is one voxel
    pose = np.eye(4, dtype=F)
    pose[:3, 3] = (-5.0, -5.0, 0.0)
    seg2 = [dict(seg[0], pose=pose)]
    ref2 = R.fuse(seg2, 1, Kic, box_all, 10.0)[0]
    assert ref2["count"].tolist() == [4096] and ref2["n_outside"] == 0
    _assert_equal(_host(fuse_frames(ws, _dev(seg2), 1, Kc, leaf=10.0, box=box_all))[0], ref2)


def _edge_points():
    rng = np.random.default_rng(21)
    grid = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F) * F(0.25)      # on voxel faces, negative too
    jitter = (rng.uniform(-0.99, 0.99, size=(1500, 3))).astype(F)
    below = np.nextafter(grid[:200], F(-np.inf)).astype(F)
    pts = np.concatenate([grid, jitter, below, [[65536.0, 0, 0], [0, -65536.0, 0], [0, 0, 1e30], [70000.0, 70000.0, 0]]]).astype(F)
    pts = np.concatenate([pts, np.ones((len(pts), 1), F)], 1)
    pts[5, 0], pts[17, 1], pts[40, 2], pts[41, 0] = np.nan, np.inf, -np.inf, np.nan
    nrm = np.concatenate([rng.normal(size=(len(pts), 3)), np.zeros((len(pts), 1))], 1).astype(F)
    nrm[100] = (np.nan, 1, 0, 0)                                    # a non-finite normal counts as zero
    nrm[101] = (1e30, 0, 0, 0)
    col = rng.integers(0, 256, size=(len(pts), 4), dtype=np.uint8)
    return pts, nrm, col


def test_edges_faces_negative_coordinates_nan_and_far_points(ws):
    from bundletrack_amd.fusion import voxel_downsample
    pts, nrm, col = _edge_points()
    leaf = 0.25
    ref, box = R.voxel_downsample(pts, leaf, normal=nrm, colour=col)
    assert ref["n_outside"] == 4 and ref["count"].sum() == len(pts) - 8 and box[0, :3].tolist() == [-5, -5, -5]
    cloud = voxel_downsample(ws, _t(pts), _t(nrm), _t(col), leaf=leaf)             # box=None: the device's bounds
    assert np.array_equal(cloud.box, box)
    _assert_equal(_host(cloud)[0], ref)
    # a box that cuts the object; min_points = 3
    cut = np.array([[-2, -1, -3, 3, 4, 2]], np.int32)
    ref_cut, _ = R.voxel_downsample(pts, leaf, normal=nrm, colour=col, box=cut, min_points=3)
    assert 0 < ref_cut["n_out"] < 24 and ref_cut["n_outside"] > 1000
    got = _host(voxel_downsample(ws, _t(pts), _t(nrm), _t(col), leaf=leaf, box=cut, min_points=3))[0]
    _assert_equal(got, ref_cut)


def test_capacity_below_n_out_leaves_the_guard_untouched(ws):
    """btba_fuse_frames on caller-made buffers: capacity 7 of 2 instances, each buffer with a guard region behind it."""
    import torch
    pts, nrm, col = _edge_points()
    leaf, cap, guard = 0.25, 7, 64
    seg = [{"instance": b, "pose": np.eye(4, dtype=F), "xyz": pts, "normal": nrm, "colour": col} for b in range(2)]
    box = R.bounds(seg, 2, None, leaf)
    ref = R.fuse(seg, 2, None, box, leaf)
    assert ref[0]["n_out"] > 100
    dev = _dev(seg)
    from bundletrack_amd.fusion import _segment_array
    arr, _, _, _, keep = _segment_array(dev, 2)
    bufs = {k: torch.full((2 * cap + guard, w), 0x5A, dtype=torch.uint8, device="cuda") for k, w in (("xyz", 16), ("normal", 16), ("colour", 4), ("count", 4), ("lin", 4))}
    words = {k: torch.full((2,), -7, dtype=torch.int32, device="cuda") for k in ("n_out", "n_outside", "status")}
    prm = _lib.fuse_params(leaf=leaf)
    rc = _lib.lib().btba_fuse_frames(ws.handle, C.byref(prm), 2, 2, C.cast(arr, C.c_void_p), 0, 0, None, box.ctypes.data, cap,
                                     *[bufs[k].data_ptr() for k in ("xyz", "normal", "colour", "count", "lin")],
                                     *[words[k].data_ptr() for k in ("n_out", "n_outside", "status")])
    assert rc == 0
    torch.cuda.synchronize()
    assert words["n_out"].cpu().tolist() == [ref[0]["n_out"]] * 2 and words["status"].cpu().tolist() == [_lib.FUSE_OVERFLOW] * 2
    assert words["n_outside"].cpu().tolist() == [ref[0]["n_outside"]] * 2
    for k, key in (("xyz", "xyz"), ("normal", "normal"), ("colour", "colour"), ("count", "count"), ("lin", "lin")):
        h = bufs[k].cpu().numpy()
        assert (h[2 * cap:] == 0x5A).all(), k                                      # the guard
        for b in range(2):
            assert h[b * cap:(b + 1) * cap].tobytes() == ref[b][key][:cap].tobytes(), (k, b)
    # capacity 0: only the words
    rc = _lib.lib().btba_fuse_frames(ws.handle, C.byref(prm), 2, 2, C.cast(arr, C.c_void_p), 0, 0, None, box.ctypes.data, 0,
                                     bufs["xyz"].data_ptr(), None, None, None, None, *[words[k].data_ptr() for k in ("n_out", "n_outside", "status")])
    assert rc == 0
    torch.cuda.synchronize()
    assert words["n_out"].cpu().tolist() == [ref[0]["n_out"]] * 2 and (bufs["xyz"].cpu().numpy()[2 * cap:] == 0x5A).all()


def test_bounds_and_the_box_none_path(ws, K, Ki, views):
    from bundletrack_amd.fusion import fuse_bounds, fuse_frames
    other = R.sphere_segments([(0.1, 0.3, -0.45)], 2, K, H, W, seed=9, radius=0.07)
    segs = views + other                                             # instance 1 has no segment
    for rn in (True, False):
        box = R.bounds(segs, 3, Ki, LEAF, rn)
        got = fuse_bounds(ws, _dev(segs), 3, K, leaf=LEAF, require_normals=rn).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, box), (got, box)
        assert (box[1] == 0).all() and (box[0, 3:] > 10).all()
    box = R.bounds(segs, 3, Ki, LEAF)
    explicit = fuse_frames(ws, _dev(segs), 3, K, leaf=LEAF, box=box)
    derived = fuse_frames(ws, _dev(segs), 3, K, leaf=LEAF)
    assert np.array_equal(derived.box, box)
    ref = R.fuse(segs, 3, Ki, box, LEAF)
    for g, d, r in zip(_host(explicit), _host(derived), ref):
        _assert_equal(g, r)
        _assert_equal(d, r)
    assert derived.instance(0)["xyz"].shape[0] == ref[0]["n_out"] and derived.counts().tolist() == [r["n_out"] for r in ref]


def test_voxel_downsample_of_5000_random_points(ws):
    from bundletrack_amd.fusion import voxel_downsample
    rng = np.random.default_rng(33)
    pts = np.concatenate([rng.normal(size=(5000, 3)) * 0.08, np.ones((5000, 1))], 1).astype(F)
    nrm = np.concatenate([rng.normal(size=(5000, 3)), np.zeros((5000, 1))], 1).astype(F)
    col = rng.integers(0, 256, size=(5000, 4), dtype=np.uint8)
    ref, box = R.voxel_downsample(pts, 0.015, normal=nrm, colour=col)
    assert 1000 < ref["n_out"] < 5000 and ref["count"].max() >= 5
    cloud = voxel_downsample(ws, _t(pts), _t(nrm), _t(col), leaf=0.015)
    _assert_equal(_host(cloud)[0], ref)
    bare_ref, _ = R.voxel_downsample(pts, 0.015)                                   # positions alone
    bare = voxel_downsample(ws, _t(pts), leaf=0.015)
    assert bare.normal is None and bare.colour is None
    _assert_equal(_host(bare)[0], bare_ref, keys=("xyz", "count", "lin"))
    # two clouds in one call, one of them empty
    import torch
    two = voxel_downsample(ws, [_t(pts), torch.zeros((0, 4), device="cuda")], leaf=0.015)
    h = _host(two)
    _assert_equal(h[0], bare_ref, keys=("xyz", "count", "lin"))
    assert h[1]["n_out"] == 0 and (two.box[1] == 0).all()


def test_bundler_reconstruct_equals_fuse_frames(ws, oracle, tmp_path):
    """A 4-keyframe synthetic session: Bundler.reconstruct gives the bytes of fuse_frames on the keyframes' maps and poses, and those of the
    numpy restatement."""
    from bundletrack_amd.bundler import Bundler, FrameRef
    from bundletrack_amd.fusion import frame_segment, fuse_frames
    from bundletrack_amd.optimizer import OptimizerGpu
    n = 4
    seq = S.SyntheticSequence(n_frames=n, seed=S.config_seed(1), background=False)
    fm = S.SyntheticFeatureManager(seq, corr_per_pair=300)
    bundler = Bundler(OptimizerGpu(workspace=ws), fm, seq.K, seq.H, seq.W, window_size=5, max_BA_frames=5, min_rot_deg=0.0, pose_dir=str(tmp_path))
    rng = np.random.default_rng(4)
    for k in range(n):
        depth, normals = seq.render(k)[:2]
        col = np.zeros((seq.H, seq.W, 4), np.uint8)
        col[..., :3] = rng.integers(0, 256, size=(seq.H, seq.W, 3), dtype=np.uint8)
        fr = FrameRef(id=0, pose_in_model=seq.poses_gt[0].astype(np.float32), n_keypts=300, depth_gpu=_t(depth), normal_gpu=_t(normals), color_gpu=_t(col))
        fm.register(fr, k)
        bundler.process_new_frame(fr)
        assert fr.status != "FAIL"
    kfs = list(bundler.keyframes)
    print("keyframes", len(kfs))
    assert len(kfs) == n
    cloud = bundler.reconstruct(leaf=0.005)
    direct = fuse_frames(ws, [frame_segment(f) for f in kfs], 1, seq.K, leaf=0.005)
    g, d = _host(cloud)[0], _host(direct)[0]
    assert g["n_out"] > 500 and g["status"] == 0 and "colour" in g
    _assert_equal(g, d)
    segs = [{"instance": 0, "pose": f.pose_in_model, "depth": f.depth_gpu.cpu().numpy(), "normal": f.normal_gpu.cpu().numpy(), "colour": f.color_gpu.cpu().numpy()}
            for f in kfs]
    Ki = R.kinv4(oracle, seq.K)
    assert np.array_equal(cloud.box, R.bounds(segs, 1, Ki, 0.005))
    _assert_equal(g, R.fuse(segs, 1, Ki, cloud.box, 0.005)[0])
