"""btba_ingest_frames on the CPU: the numpy restatement (tests/ingest_ref.py) of the depth decode pinned to the host compiler over
all 65 536 codes, the colour pack, the chain through the oracle, the ABI of the new entry points and the Python Bundler's hook."""
import ctypes as C
import os
import subprocess

import numpy as np

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S

import ingest_ref as R
from test_depth_processing import noisy_depth

HERE = os.path.dirname(os.path.abspath(__file__))
ALL_CODES = np.arange(65536, dtype=np.uint32).astype(np.uint16)


def test_decode_equals_the_host_compiler_on_every_code(tmp_path):
    exe = str(tmp_path / "ingest_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "cpp", "ingest_host.cpp")])
    cpp = np.frombuffer(subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout, np.float32)
    assert cpp.shape == (65536,)
    ours = R.decode_depth(ALL_CODES)
    assert np.array_equal(ours.view(np.uint32), cpp.view(np.uint32))
    assert np.array_equal(ours == 0, ALL_CODES < 100)                          # the zero set is exactly u < 100 ...
    assert ours[100] == np.float32(0.1) and ours[99] == 0                      # ... and code 100 -> 0.1f is kept
    short = R.decode_depth_float_shortcut(ALL_CODES)
    assert not np.array_equal(short.view(np.uint32), cpp.view(np.uint32))      # the guard: the float product is NOT the rule
    kept = ALL_CODES >= 100                                                    # (38 850 codes in all, 48 of them below 100 and zeroed either way)
    assert int((short.view(np.uint32) != cpp.view(np.uint32))[kept].sum()) == 38850 - 48
    assert np.array_equal(R.decode_depth(ALL_CODES.view(np.int16)), ours)      # int16 tensors carry the same 16 bits


def test_colour_pack():
    rng = np.random.default_rng(0)
    bgr = rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    c = R.pack_color(bgr)
    assert c.shape == (5, 7, 4) and c.dtype == np.uint8
    assert np.array_equal(c[..., 0], bgr[..., 0]) and np.array_equal(c[..., 1], bgr[..., 1]) and np.array_equal(c[..., 2], bgr[..., 2])
    assert not c[..., 3].any()
    # as the device stores it, one little-endian dword per pixel: B | G << 8 | R << 16
    dw = c.view(np.uint32)[..., 0]
    assert np.array_equal(dw, bgr[..., 0].astype(np.uint32) | (bgr[..., 1].astype(np.uint32) << 8) | (bgr[..., 2].astype(np.uint32) << 16))


def test_restatement_chain_through_the_oracle(oracle):
    d, K = noisy_depth(10, 53, 117)
    codes = R.metres_to_codes(d)
    bgr = np.random.default_rng(1).integers(0, 256, size=(53, 117, 3), dtype=np.uint8)
    raw, depth, normals, xyz, color = R.restate(oracle, codes, bgr, K)
    assert np.abs(raw - d)[codes >= 100].max() <= 0.0005 + 1e-7 and not raw[codes < 100].any()       # millimetre quantisation
    assert np.array_equal(depth, oracle.process_depth(raw))
    n2, x2 = oracle.depth_to_normals(depth, K)
    assert np.array_equal(normals, n2) and np.array_equal(xyz, x2)
    assert (depth > 0).sum() > 0.5 * depth.size and np.array_equal(color, R.pack_color(bgr))


def test_abi_ingest_entry_points():
    names = {"btba_ingest_params_default", "btba_ingest_frames"}
    assert names <= set(_lib.declared_symbols()) and names <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.lib()
    for s in names:
        assert hasattr(L, s)
    assert C.sizeof(_lib.IngestParams) == 28
    p = _lib.ingest_params()
    assert (p.depth_format, p.erode_radius, p.bf_radius) == (0, 1, 2)
    assert (p.erode_diff, p.erode_ratio, p.sigma_d, p.sigma_r) == (np.float32(0.001), np.float32(0.8), 2.0, 100000.0)
    import re
    chunk = int(re.search(r"#define BTBA_INGEST_CHUNK (\d+)", open(_lib.HEADER).read()).group(1))
    assert chunk >= 1
    assert L.btba_version() == 105


def test_ingest_rejects_a_null_workspace():
    L = _lib.lib()
    t = C.cast((C.c_void_p * 1)(C.c_void_p(256)), C.c_void_p)
    o = C.cast((C.c_void_p * 1)(C.c_void_p(4096)), C.c_void_p)
    n = C.cast((C.c_void_p * 1)(C.c_void_p(65536)), C.c_void_p)
    K = np.eye(3, dtype=np.float32)
    assert L.btba_ingest_frames(None, C.byref(_lib.ingest_params()), 1, 4, 4, K.ctypes.data, t, None, o, n, None, None, None) == _lib.BTBA_EINVAL


def test_python_bundler_ingests_only_frames_that_bring_codes(oracle):
    """Bundler.process_new_frame calls Bundler.ingest first for a frame with depth_code_gpu and no depth_gpu, and not for a frame
    that arrives with its maps (numpy host path, an injected stand-in for the GPU ingest)."""
    from bundletrack_amd.bundler import Bundler, FrameRef
    from helpers import OracleOptimizer
    n = 3
    seq = S.SyntheticSequence(n_frames=n, seed=S.config_seed(1))
    ingested = []

    class StandIn(Bundler):
        def ingest(self, frame):
            ingested.append(frame)
            frame.depth_gpu, frame.normal_gpu = frame.maps

    def session(with_codes):
        fm = S.SyntheticFeatureManager(seq, corr_per_pair=300)
        b = StandIn(OracleOptimizer(oracle), fm, seq.K, seq.H, seq.W, window_size=5, max_BA_frames=5)
        frames = []
        for k in range(n):
            depth, normals = seq.render(k)
            fr = FrameRef(id=0, pose_in_model=seq.poses_gt[0].astype(np.float32), n_keypts=300)
            if with_codes:
                fr.depth_code_gpu, fr.maps = R.metres_to_codes(depth), (depth, normals)
            else:
                fr.depth_gpu, fr.normal_gpu = depth, normals
            if k == 1:
                fr.depth_code_gpu = R.metres_to_codes(depth)          # both set: the maps it came with win
                fr.depth_gpu, fr.normal_gpu = depth, normals
            fm.register(fr, k)
            b.process_new_frame(fr)
            frames.append(fr)
        assert b.n_ba_calls == n - 1
        return frames

    plain = session(False)
    assert ingested == []
    coded = session(True)
    assert ingested == [coded[0], coded[2]]
    for a, b in zip(plain, coded):
        assert np.array_equal(a.pose_in_model, b.pose_in_model)
    assert FrameRef(id=0, pose_in_model=np.eye(4)).depth_code_gpu is None and FrameRef(id=0, pose_in_model=np.eye(4)).bgr_gpu is None
