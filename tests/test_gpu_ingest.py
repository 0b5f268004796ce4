"""btba_ingest_frames on the MI355X: the decode against the numpy restatement on every code; bit identity of depth, normals, xyz
and colour with the per-frame calls (btba_process_depth + btba_depth_to_normals on the numpy-decoded depth) for both stencil
variants, across a launch chunk and with every optional table left out; float input against the CPU oracle at the per-frame
kernel's own bar; the argument checks; the optimiser fed from ingested frames; and the Python Bundler's hook.  One module-scoped
workspace.  (Bit identity with the per-frame kernels compares two instantiations of one tile function; both are held to the fp64
reference of image_ref.py in test_gpu_image_stages.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S

import ingest_ref as R
from test_depth_processing import noisy_depth

GENERIC = dict(erode_radius=2, erode_ratio=0.5, bf_radius=3, sigma_d=1.5, sigma_r=0.01)
# the same stencils with an erode that keeps the surface (at diff 0.001 it removes all but ~20 pixels of these frames, so the filter passes
# and the normals would be compared on next to nothing): > 4000 depth pixels and > 3000 normals per frame on the CPU oracle
GENERIC_KEEPING = dict(GENERIC, erode_diff=0.05)


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Frame:
    depth_code_gpu = bgr_gpu = depth_gpu = normal_gpu = color_gpu = None


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _ingest(ws, depth, bgr, K, **kw):
    """ingest_frames on fresh frames; host copies (as uint32 / uint8 bits) of what it set, per frame."""
    import torch
    from bundletrack_amd.ingest import ingest_frames
    frames = [_Frame() for _ in depth]
    ingest_frames(ws, frames, [_t(d) for d in depth], None if bgr is None else [None if b is None else _t(b) for b in bgr], K, **kw)
    torch.cuda.synchronize()
    return [{k: _bits(getattr(f, k + "_gpu")) for k in ("depth", "normal", "color", "xyz", "depth_raw") if getattr(f, k + "_gpu", None) is not None}
            for f in frames]


def _per_frame(ws, codes, bgr, K, **kw):
    """The existing per-frame calls on the numpy-decoded depth, and the numpy colour pack."""
    from bundletrack_amd.optimizer import depth_to_normals, process_depth
    out = []
    for c, b in zip(codes, bgr):
        raw = R.decode_depth(c) if c.dtype != np.float32 else c
        d = process_depth(ws, _t(raw), **kw)
        n, xyz = depth_to_normals(ws, d, K, want_xyz=True)
        out.append({"depth": _bits(d), "normal": _bits(n), "xyz": _bits(xyz), "depth_raw": raw.view(np.uint32),
                    **({} if b is None else {"color": R.pack_color(b)})})
    return out


def _assert_equal(got, ref, keys=("depth", "normal", "xyz", "color", "depth_raw")):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        for key in keys:
            assert (key in g) == (key in r), (k, key)
            if key in g:
                assert g[key].dtype == r[key].dtype and np.array_equal(g[key], r[key]), f"frame {k}: {key} differs"


def _scene(seeds, H, W):
    codes, bgr, K = [], [], None
    for s in seeds:
        d, K = noisy_depth(s, H, W)
        codes.append(R.metres_to_codes(d))
        bgr.append(np.random.default_rng(1000 + s).integers(0, 256, size=(H, W, 3), dtype=np.uint8))
    return codes, bgr, K


def test_decode_of_every_code(ws):
    codes = np.random.default_rng(7).permutation(65536).astype(np.uint16).reshape(256, 256)
    got = _ingest(ws, [codes, codes.view(np.int16)], None, S.NOCS_K, want_raw=True)          # torch.uint16 and torch.int16: the same bits
    ref = R.decode_depth(codes).view(np.uint32)
    assert np.array_equal(got[0]["depth_raw"], ref) and np.array_equal(got[1]["depth_raw"], ref)
    assert "color" not in got[0]


@pytest.mark.parametrize("params", [{}, GENERIC, GENERIC_KEEPING], ids=["tracker_stencils", "generic_stencils", "generic_stencils_keeping_erode"])
def test_bit_identical_to_the_per_frame_calls(ws, params):
    codes, bgr, K = _scene(range(10, 14), 53, 117)            # interior and rim workgroups, neither side a multiple of the tile
    got = _ingest(ws, codes, bgr, K, want_xyz=True, want_raw=True, **params)
    _assert_equal(got, _per_frame(ws, codes, bgr, K, **params))
    if params is not GENERIC:                                 # the comparison is of real surfaces, not of empty maps
        assert all((g["depth"] != 0).sum() > 4000 and (g["normal"] != 0).any(-1).sum() > 3000 for g in got)


def test_bit_identical_across_a_launch_chunk(ws):
    import re
    chunk = int(re.search(r"#define BTBA_INGEST_CHUNK (\d+)", open(_lib.HEADER).read()).group(1))
    n = chunk + 1
    codes, bgr, K = _scene(range(100, 100 + n), 13, 17)       # smaller than a tile plus its halo: every workgroup is a rim workgroup
    assert len({c.tobytes() for c in codes}) == n
    got = _ingest(ws, codes, bgr, K, want_xyz=True, want_raw=True)
    _assert_equal(got, _per_frame(ws, codes, bgr, K))


@pytest.mark.parametrize("shape", [(37, 53), (96, 128)])
def test_float_input_matches_the_oracle(ws, oracle, shape):
    d, K = noisy_depth(2, *shape)
    got = _ingest(ws, [d], None, K, want_raw=True)[0]
    assert np.array_equal(got["depth_raw"], d.view(np.uint32))                    # format 1: the floats pass through
    dep = got["depth"].view(np.float32)
    ref = oracle.process_depth(d)
    mism = (dep == 0) != (ref == 0)
    print("zero-pattern mismatches", int(mism.sum()), "max abs diff elsewhere", float(np.abs(dep[~mism] - ref[~mism]).max()))
    assert mism.sum() <= 2
    assert np.abs(dep[~mism] - ref[~mism]).max() < 2e-6


def test_optional_tables(ws):
    codes, bgr, K = _scene(range(20, 23), 53, 117)
    full = _ingest(ws, codes, bgr, K, want_xyz=True, want_raw=True)
    _assert_equal(_ingest(ws, codes, None, K, want_xyz=True, want_raw=True), [{k: v for k, v in g.items() if k != "color"} for g in full])
    holed = _ingest(ws, codes, [bgr[0], None, bgr[2]], K, want_xyz=True, want_raw=True)
    _assert_equal(holed, [{k: v for k, v in g.items() if k != "color" or i != 1} for i, g in enumerate(full)])
    _assert_equal(_ingest(ws, codes, bgr, K, want_raw=True), [{k: v for k, v in g.items() if k != "xyz"} for g in full])
    _assert_equal(_ingest(ws, codes, bgr, K, want_xyz=True), [{k: v for k, v in g.items() if k != "depth_raw"} for g in full])
    _assert_equal(_ingest(ws, codes, bgr, K), [{k: v for k, v in g.items() if k not in ("xyz", "depth_raw")} for g in full])
    # a BGR image off 4-byte alignment takes the bytewise path: the same colour map
    import torch
    from bundletrack_amd.ingest import ingest_frames
    buf = torch.zeros(3 * 53 * 117 + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = _t(bgr[0]).reshape(-1)
    odd = buf[1:].view(53, 117, 3)
    assert odd.data_ptr() % 4 == 1
    f = _Frame()
    ingest_frames(ws, [f], [_t(codes[0])], [odd], K)
    torch.cuda.synchronize()
    assert np.array_equal(f.color_gpu.cpu().numpy(), full[0]["color"])


def test_rejects_bad_arguments_on_a_workspace(ws):
    import torch
    from bundletrack_amd.ingest import ingest_frames
    L = _lib.lib()
    H, W = 8, 12
    codes = torch.full((H, W), 1000, dtype=torch.int16, device="cuda")             # a launch would leave nonzero depth and colour
    bgr = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda")
    dep, raw = (torch.zeros((H, W), device="cuda") for _ in range(2))
    nrm, xyz = (torch.zeros((H, W, 4), device="cuda") for _ in range(2))
    col = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    K = np.ascontiguousarray(S.NOCS_K, np.float32)

    def tab(p):
        return C.cast((C.c_void_p * 1)(p), C.c_void_p)

    good = dict(ws=ws.handle, prm=C.byref(_lib.ingest_params()), n=1, H=H, W=W, K=K.ctypes.data, d_in=tab(codes.data_ptr()), bgr=tab(bgr.data_ptr()),
                d_out=tab(dep.data_ptr()), n_out=tab(nrm.data_ptr()), c_out=tab(col.data_ptr()), raw=tab(raw.data_ptr()), xyz=tab(xyz.data_ptr()))
    call = lambda **kw: L.btba_ingest_frames(*{**good, **kw}.values())
    E = _lib.BTBA_EINVAL
    assert call(ws=None) == E and call(prm=None) == E and call(K=None) == E
    assert call(d_in=None) == E and call(d_out=None) == E and call(n_out=None) == E
    assert call(d_in=tab(None)) == E and call(d_out=tab(None)) == E and call(n_out=tab(None)) == E
    assert call(n=0) == E and call(H=0) == E and call(W=0) == E
    for fmt in (-1, 2):
        assert call(prm=C.byref(_lib.ingest_params(depth_format=fmt))) == E
    for bad in (dict(erode_radius=-1), dict(bf_radius=-1), dict(erode_radius=5, bf_radius=6), dict(sigma_d=0.0), dict(sigma_r=0.0), dict(sigma_r=float("nan"))):
        assert call(prm=C.byref(_lib.ingest_params(**bad))) == E
    assert call(d_in=tab(codes.data_ptr() + 1)) == E                              # uint16 codes: 2-byte aligned
    assert call(n_out=tab(nrm.data_ptr() + 4)) == E and call(xyz=tab(xyz.data_ptr() + 8)) == E and call(c_out=tab(col.data_ptr() + 2)) == E
    assert call(bgr=None) == E and call(bgr=tab(None)) == E                       # a colour output without its BGR input
    for out in ("d_out", "n_out", "c_out", "raw", "xyz"):
        assert call(**{out: tab(codes.data_ptr())}) == E                          # an output on its own frame's depth input
    assert call(prm=C.byref(_lib.ingest_params(depth_format=1)), d_in=tab(dep.data_ptr())) == E
    torch.cuda.synchronize()
    for t in (dep, raw, nrm, xyz, col):
        assert not t.any()                                                        # nothing was launched
    assert call() == _lib.BTBA_OK
    # the Python layer's own checks
    f = _Frame()
    with pytest.raises(ValueError):
        ingest_frames(ws, [f], [codes.to(torch.int32)], None, K)
    with pytest.raises(ValueError):
        ingest_frames(ws, [f], [codes.t()], None, K)
    with pytest.raises(ValueError):
        ingest_frames(ws, [f], [codes], [bgr[:, :, :2]], K)
    with pytest.raises(ValueError):
        ingest_frames(ws, [f], None, None, K)
    torch.cuda.synchronize()


def test_ingested_frames_feed_the_optimiser(ws, oracle):
    """codes -> ingest_frames -> optimizeFrames on the device; the same poses as the all-oracle chain on the numpy-decoded depth."""
    from bundletrack_amd.ingest import ingest_frames
    from bundletrack_amd.optimizer import OptimizerGpu
    pb = S.make_problem(3, 200, seed=77, background=False)
    codes = [R.metres_to_codes(pb.depth[k]) for k in range(3)]
    frames = [_Frame() for _ in range(3)]
    ingest_frames(ws, frames, [_t(c) for c in codes], None, pb.K)
    poses = pb.poses_init.copy()
    OptimizerGpu(workspace=ws).optimizeFrames(pb.corr, pb.n_match_per_pair, 3, pb.H, pb.W, [f.depth_gpu for f in frames], None,
                                              [f.normal_gpu for f in frames], poses, pb.K)
    dep_o = [oracle.process_depth(R.decode_depth(c)) for c in codes]
    nrm_o = [oracle.depth_to_normals(d, pb.K)[0] for d in dep_o]
    caches = [oracle.build_cache(dep_o[k], nrm_o[k], pb.K) for k in range(3)]
    ref = oracle.solve(np.stack([c["campos"] for c in caches]), np.stack([c["normals"] for c in caches]), caches[0]["intr"], pb.corr, pb.poses_init)
    for k in range(3):
        r, t = S.pose_error(poses[k], ref.poses[k])
        print(f"frame {k}: rot {r:.3e} rad, trans {t:.3e} m")
        assert r < 1e-4 and t < 1e-4


def test_python_bundler_ingests_frames_that_bring_only_their_images(ws, tmp_path):
    """A 4-frame session on frames carrying depth_code_gpu / bgr_gpu / mask_gpu saves the poses of the same session on frames
    whose maps the per-frame calls made beforehand."""
    from bundletrack_amd.bundler import Bundler, FrameRef
    from bundletrack_amd.optimizer import OptimizerGpu, depth_to_normals, process_depth
    n = 4
    seq = S.SyntheticSequence(n_frames=n, seed=S.config_seed(1), background=True)

    def session(ingest_first, pose_dir):
        fm = S.SyntheticFeatureManager(seq, corr_per_pair=300)
        bundler = Bundler(OptimizerGpu(workspace=ws), fm, seq.K, seq.H, seq.W, window_size=5, max_BA_frames=5, pose_dir=pose_dir)
        frames = []
        for k in range(n):
            codes = R.metres_to_codes(seq.render(k)[0])
            bgr = np.random.default_rng(k).integers(0, 256, size=(seq.H, seq.W, 3), dtype=np.uint8)
            mask = S.make_mask(seq.poses_gt[k], seq.K, seq.H, seq.W, seed=k)
            fr = FrameRef(id=0, pose_in_model=seq.poses_gt[0].astype(np.float32), n_keypts=300, mask_gpu=_t(mask))
            if ingest_first:
                fr.depth_gpu = process_depth(ws, _t(R.decode_depth(codes)))
                fr.normal_gpu = depth_to_normals(ws, fr.depth_gpu, seq.K)
                fr.color_gpu = _t(R.pack_color(bgr))
            else:
                fr.depth_code_gpu, fr.bgr_gpu = _t(codes), _t(bgr)
            fm.register(fr, k)
            bundler.process_new_frame(fr)
            assert fr.status != "FAIL" and fr.depth_gpu is not None and fr.color_gpu is not None
            frames.append(fr)
        assert bundler.n_ba_calls == n - 1
        return frames

    a = session(True, str(tmp_path / "a"))
    b = session(False, str(tmp_path / "b"))
    for fa, fb in zip(a, b):
        assert np.array_equal(fa.pose_in_model, fb.pose_in_model)
        assert np.array_equal(_bits(fa.depth_gpu), _bits(fb.depth_gpu)) and np.array_equal(_bits(fa.color_gpu), _bits(fb.color_gpu))
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert len(names) == n - 1 and names == sorted(os.listdir(str(tmp_path / "b")))
    for name in names:
        assert open(str(tmp_path / "a" / name)).read() == open(str(tmp_path / "b" / name)).read()


def _driver():
    so = _lib.build_driver("ingest_driver")
    f = C.CDLL(so).ingest_driver
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9
    return f


@pytest.mark.parametrize("via_bundler", [0, 1])
def test_cpp_host_layer_equals_python(ws, via_bundler):
    """btba::ingestFrames, and btba::Bundler::processNewFrame on a frame that brings only its images, write the maps ingest_frames
    writes; the second frame has no BGR image and keeps its colour buffer untouched."""
    import torch
    H, W = 53, 117
    codes, bgr, K = _scene(range(30, 33), H, W)
    bgr[1] = None
    py = _ingest(ws, codes, bgr, K, want_xyz=True, want_raw=True)
    dc = [_t(c) for c in codes]
    db = [None if b is None else _t(b) for b in bgr]
    dep, raw = ([torch.zeros((H, W), device="cuda") for _ in codes] for _ in range(2))
    nrm, xyz = ([torch.zeros((H, W, 4), device="cuda") for _ in codes] for _ in range(2))
    col = [torch.full((H, W, 4), 9, dtype=torch.uint8, device="cuda") for _ in codes]
    ptr = lambda ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    done = np.zeros(3, np.int32)
    Kf = np.ascontiguousarray(K, np.float32)
    rc = _driver()(ws.handle.value, via_bundler, 3, H, W, Kf.ctypes.data, ptr(dc), ptr(db), ptr(dep), ptr(nrm), ptr(col), ptr(raw), ptr(xyz), done.ctypes.data)
    assert rc == 0 and done.all()
    torch.cuda.synchronize()
    for k in range(3):
        assert np.array_equal(_bits(dep[k]), py[k]["depth"]) and np.array_equal(_bits(nrm[k]), py[k]["normal"])
        assert np.array_equal(_bits(raw[k]), py[k]["depth_raw"]) and np.array_equal(_bits(xyz[k]), py[k]["xyz"])
        assert np.array_equal(_bits(col[k]), py[k]["color"]) if k != 1 else (_bits(col[k]) == 9).all()
