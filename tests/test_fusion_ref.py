"""The numpy restatement of keyframe fusion (tests/fusion_ref.py) checked against what it claims, and the host side of the C ABI: the
exported symbols, the defaults, btba_fuse_layout, and every BTBA_EINVAL that is decided before any device call.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import fusion_ref as R
from bundletrack_amd import _lib

F = np.float32
H, W = 48, 64


@pytest.fixture(scope="module")
def scene(oracle):
    K = R.small_K(H, W)
    return {"K": K, "Ki": R.kinv4(oracle, K), "segs": R.sphere_segments(R.THREE_VIEWS, 0, K, H, W)}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_backprojection_is_the_oracles_xyz_map(oracle, scene):
    """fusion_ref.backproject restates btba_image.hpp::backproject; the CPU oracle's depth_to_normals writes the same points."""
    d = scene["segs"][1]["depth"]
    xyz = oracle.depth_to_normals(d, scene["K"])[1].reshape(-1, 4)
    c, keep = R.backproject(d, scene["Ki"])
    assert keep.sum() > 300 and np.array_equal(keep, xyz[:, 3] == 1)
    assert c[keep].tobytes() == np.ascontiguousarray(xyz[keep, :3]).tobytes()


def test_centroid_within_the_derived_bar_of_the_fp64_mean(scene):
    """Each point is rounded to a multiple of 2^-20 (error <= 2^-21), the integer mean is exact, the division and the cast to float round
    once more each: |centroid - fp64 mean of the fp32 points| <= 2^-21 + 1/2 ulp32(|mean|) (+ the fp64 roundings, 2^-50 relative)."""
    leaf = 0.01
    box = R.bounds(scene["segs"], 1, scene["Ki"], leaf)
    out = R.fuse(scene["segs"], 1, scene["Ki"], box, leaf)[0]
    assert out["n_out"] > 100 and out["count"].max() >= 4
    p = np.concatenate([R.segment_points(s, scene["Ki"])[0] for s in scene["segs"]])
    c, _ = R.cells(p, leaf)
    i = c - box[0, :3].astype(np.int64)
    lin = i[:, 0] + int(box[0, 3]) * (i[:, 1] + int(box[0, 4]) * i[:, 2])
    worst = 0.0
    for r, l in enumerate(out["lin"]):
        mean = p[lin == l].astype(np.float64).mean(0)
        bar = 2.0 ** -21 + 0.5 * np.spacing(np.abs(mean).astype(F)).astype(np.float64) + 1e-15
        err = np.abs(out["xyz"][r, :3].astype(np.float64) - mean)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (r, err, bar)
    print("worst error / bar", worst)


def test_permuting_points_and_segments_changes_no_byte(scene):
    leaf = 0.01
    box = R.bounds(scene["segs"], 1, scene["Ki"], leaf)
    ref = R.fuse(scene["segs"], 1, scene["Ki"], box, leaf)[0]
    _same(ref, R.fuse(scene["segs"][::-1], 1, scene["Ki"], box, leaf)[0])
    # the frames as point lists, their points shuffled: the same voxels, bytes and all
    rng = np.random.default_rng(5)
    lists = []
    for s in scene["segs"]:
        c, keep = R.backproject(s["depth"], scene["Ki"])
        keep &= (s["normal"].reshape(-1, 4)[:, :3] != 0).any(1)
        order = rng.permutation(np.flatnonzero(keep))
        xyz = np.concatenate([c[order], np.ones((len(order), 1), F)], 1)
        lists.append({"instance": 0, "pose": s["pose"], "xyz": xyz, "normal": s["normal"].reshape(-1, 4)[order], "colour": s["colour"].reshape(-1, 4)[order]})
    _same(ref, R.fuse(lists, 1, scene["Ki"], box, leaf)[0])


def test_floor_not_truncation_and_faces_go_up():
    leaf = 0.25                                           # inv_leaf = 4 exactly: p * inv_leaf is exact
    pts = np.array([[-0.1, 0.1, -0.6, 1], [0.5, -0.25, 0.0, 1], [0.49999997, -0.25000003, -1e-30, 1]], F)
    c, ok = R.cells(pts[:, :3], leaf)
    assert ok.all()
    assert c.tolist() == [[-1, 0, -3], [2, -1, 0], [1, -2, -1]]       # truncation would give 0, 0, -2 in the first row
    out, box = R.voxel_downsample(pts, leaf)
    assert box.tolist() == [[-1, -2, -3, 4, 3, 4]]
    assert out["n_out"] == 3 and out["count"].tolist() == [1, 1, 1]
    assert (np.diff(out["lin"]) > 0).all()


def test_output_order_is_lin_ascending_and_min_points_filters():
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.uniform(-0.2, 0.2, size=(800, 3)), np.ones((800, 1))], 1).astype(F)
    out, box = R.voxel_downsample(pts, 0.05)
    assert (np.diff(out["lin"].astype(np.int64)) > 0).all() and out["count"].sum() == 800
    out3, _ = R.voxel_downsample(pts, 0.05, box=box, min_points=3)
    sel = out["count"] >= 3
    assert 0 < sel.sum() < len(sel)
    assert out3["lin"].tobytes() == out["lin"][sel].tobytes() and out3["xyz"].tobytes() == out["xyz"][sel].tobytes()


def test_downsample_is_fusion_with_the_identity_pose():
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.normal(size=(500, 3)) * 0.1, np.ones((500, 1))], 1).astype(F)
    pts[7, 1] = np.nan
    pts[9, 0] = np.inf
    nrm = np.concatenate([rng.normal(size=(500, 3)), np.zeros((500, 1))], 1).astype(F)
    col = rng.integers(0, 256, size=(500, 4), dtype=np.uint8)
    out, box = R.voxel_downsample(pts, 0.015, normal=nrm, colour=col)
    seg = [{"instance": 0, "pose": np.eye(4, dtype=F), "xyz": pts, "normal": nrm, "colour": col}]
    _same(out, R.fuse(seg, 1, None, box, 0.015)[0])
    assert out["count"].sum() == 498 and out["n_outside"] == 0          # the two non-finite points are dropped, not counted outside


def test_outside_rules():
    pts = np.array([[0.01, 0.01, 0.01, 1], [65536.0, 0, 0, 1], [0, -70000.0, 0, 1], [0.3, 0.0, 0.0, 1]], F)
    box = np.array([[0, 0, 0, 2, 2, 2]], np.int32)
    out, _ = R.voxel_downsample(pts, 0.1, box=box)
    assert out["n_out"] == 1 and out["n_outside"] == 3
    assert R.bounds([{"instance": 0, "pose": np.eye(4, dtype=F), "xyz": pts}], 1, None, 0.1).tolist() == [[0, 0, 0, 4, 1, 1]]


# ---- the C ABI's host side ----------------------------------------------------------------------------------------------------

def test_symbols_and_defaults():
    L = _lib.lib()
    for name in ("btba_fuse_params_default", "btba_fuse_layout", "btba_fuse_bounds", "btba_fuse_frames", "btba_voxel_downsample"):
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib.declared_symbols() and hasattr(L, name)
    p = _lib.fuse_params()
    assert (p.leaf, p.min_points, p.require_normals, p.normalize_normals) == (F(0.005), 1, 1, 0)
    assert C.sizeof(_lib.FuseSegment) == 104 and C.sizeof(_lib.FuseParams) == 16
    assert L.btba_version() == 105


def test_fuse_layout_on_the_host():
    from bundletrack_amd.fusion import fuse_layout
    off, nbytes = fuse_layout([[0, 0, 0, 10, 20, 30], [5, 5, 5, 0, 7, 7], [-3, -3, -3, 1, 1, 1]])
    assert off.tolist() == [0, 6000, 6000, 6001]
    assert nbytes >= 64 * 6001 and nbytes % 256 == 0
    L = _lib.lib()
    bad = lambda box: L.btba_fuse_layout(len(box), np.asarray(box, np.int32).ctypes.data, None, None)
    assert bad([[0, 0, 0, -1, 2, 2]]) == _lib.BTBA_EINVAL
    assert bad([[0, 0, 0, 256, 256, 256]]) == _lib.BTBA_OK                       # exactly 2^24
    assert bad([[0, 0, 0, 256, 256, 257]]) == _lib.BTBA_EINVAL
    assert bad([[0, 0, 0, 256, 256, 128], [0, 0, 0, 256, 256, 128], [0, 0, 0, 1, 1, 1]]) == _lib.BTBA_EINVAL      # the call's total
    assert bad([[0, 0, 0, 2**31 - 1, 2**31 - 1, 2**31 - 1]]) == _lib.BTBA_EINVAL   # no 32-bit wrap to something small
    assert L.btba_fuse_layout(0, np.zeros(6, np.int32).ctypes.data, None, None) == _lib.BTBA_EINVAL
    assert L.btba_fuse_layout(1, None, None, None) == _lib.BTBA_EINVAL


def test_einval_before_any_device_call():
    """A fake workspace and fake device addresses: every rejection below returns before either is touched."""
    L = _lib.lib()
    E = _lib.BTBA_EINVAL
    ws, dev = C.c_void_p(1), 0x10000
    K = np.ascontiguousarray(R.small_K(8, 8)).reshape(9)
    box = np.array([[0, 0, 0, 4, 4, 4]], np.int32)

    def seg(**kw):
        s = (_lib.FuseSegment * 1)()
        s[0].kind, s[0].instance, s[0].n, s[0].geom, s[0].normal, s[0].colour = _lib.FUSE_FRAME, 0, 0, dev, dev, dev
        for k, v in kw.items():
            setattr(s[0], k, v)
        return s

    good = dict(ws=ws, prm=_lib.fuse_params(), B=1, S=1, seg=seg(), H=8, W=8, K=K.ctypes.data, box=box.ctypes.data, cap=16,
                xyz=dev, nrm=dev, col=dev, cnt=dev, lin=dev, n_out=dev, n_outside=dev, status=dev)

    def call(**kw):
        a = {**good, **kw}
        return L.btba_fuse_frames(a["ws"], C.byref(a["prm"]) if a["prm"] is not None else None, a["B"], a["S"], C.cast(a["seg"], C.c_void_p) if a["seg"] is not None else None,
                                  a["H"], a["W"], a["K"], a["box"], a["cap"], a["xyz"], a["nrm"], a["col"], a["cnt"], a["lin"], a["n_out"], a["n_outside"], a["status"])

    for name in ("ws", "prm", "seg", "box", "xyz", "n_out", "n_outside", "status", "K"):
        assert call(**{name: None}) == E, name
    assert call(B=0) == E and call(S=-1) == E and call(cap=-1) == E and call(H=0) == E and call(W=0) == E
    assert call(B=2, cap=2**30, box=np.tile(box, (2, 1)).ctypes.data) == E
    for leaf in (0.0, -0.01, float("nan"), float("inf"), 2.0 ** -15):
        assert call(prm=_lib.fuse_params(leaf=leaf)) == E, leaf
    assert call(prm=_lib.fuse_params(min_points=0)) == E
    assert call(seg=seg(kind=2)) == E and call(seg=seg(instance=1)) == E and call(seg=seg(instance=-1)) == E and call(seg=seg(geom=None)) == E
    assert call(seg=seg(normal=None)) == E                                        # require_normals without a normal map
    assert call(seg=seg(colour=None)) == E                                        # a colour output without a colour map
    assert call(seg=seg(normal=dev + 8)) == E and call(seg=seg(colour=dev + 2)) == E and call(seg=seg(geom=dev + 2)) == E
    assert call(seg=seg(kind=_lib.FUSE_POINTS, n=5, geom=dev + 4)) == E and call(seg=seg(kind=_lib.FUSE_POINTS, n=-1)) == E
    assert call(seg=seg(kind=_lib.FUSE_POINTS, n=2**30 + 1)) == E
    assert call(xyz=dev + 4) == E and call(nrm=dev + 8) == E and call(col=dev + 1) == E and call(cnt=dev + 2) == E and call(lin=dev + 2) == E
    for b in ([0, 0, 0, -1, 4, 4], [2**30 + 1, 0, 0, 4, 4, 4], [0, 0, 0, 512, 512, 512]):
        assert call(box=np.array([b], np.int32).ctypes.data) == E, b
    # btba_fuse_bounds shares the segment checks
    bounds = lambda **kw: L.btba_fuse_bounds(kw.get("ws", ws), C.byref(kw.get("prm", good["prm"])), 1, 1, C.cast(kw.get("seg", good["seg"]), C.c_void_p), 8, 8,
                                             K.ctypes.data, kw.get("out", dev))
    assert bounds(ws=None) == E and bounds(out=None) == E and bounds(seg=seg(kind=7)) == E and bounds(prm=_lib.fuse_params(leaf=0.0)) == E
    # btba_voxel_downsample: its own tables, then btba_fuse_frames' checks
    one = (C.c_void_p * 1)(dev + 4)
    n = np.array([5], np.int64)
    args = lambda xyz_tab, n_tab: (ws, C.byref(good["prm"]), 1, xyz_tab, None, None, n_tab, box.ctypes.data, 16, dev, None, None, None, None, dev, dev, dev)
    assert L.btba_voxel_downsample(*args(None, n.ctypes.data)) == E and L.btba_voxel_downsample(*args(C.cast(one, C.c_void_p), None)) == E
    assert L.btba_voxel_downsample(*args(C.cast(one, C.c_void_p), n.ctypes.data)) == E      # a misaligned float4 list
