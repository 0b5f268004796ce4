"""The SET-UP of a dense block-walk item: the separable dead-block test (bundletrack_amd/csrc/btba_hull.hpp) and the list of live blocks built from it.

Three frames of one smooth surface, one instance, the three pairs (target 0, source 1), (0, 2), (1, 2); caches of 16 x 16 (4 blocks), 24 x 16, 72 x 40
(45 blocks: not a multiple of 64), one 160 x 120 window (300 blocks: both blocks of a lane) and one of 208 x 168 (546 blocks at one tile: the list compaction's
SECOND pass, which fetches its block ranges inside the loop, handles blocks 512 .. 545 -- less than a wave, a partial ballot).  Frame 1 is moved so that the overlap blob crosses the
right, left, bottom and top image edge in turn (9.3 cache pixels: one column / row of blocks falls out of the target), frame 2 half as far.  Further:
  sideways  frame 1 turned by 0.9 rad: every block of its pairs lies far outside the target, every corner in front of it -- all dead, records all zeros
  behind    frame 1 turned by 180 degrees: every corner behind the camera plane -- all blocks stay, nothing is accepted, records all zeros
  nodepth   frame 1 without a valid depth: as a source no block has a range, as a target nothing is accepted
each with dense_tiles 1 and 2, and one case through the valid-pixel lists (the untouched walk).
Asserted: BTBA_OPT_BLOCK_SKIP 1 against 0 gives identical accepted-pixel counts per pair; the live-block total of BTBA_OPT_COUNT_LIVE equals what the
HOST-compiled header says for the same relative poses (the device's own matrices, multiplied in fp32), block ranges (read back from the device) and
back-projection terms -- tests/cpp/hull_host.cpp built as a shared library.  The header switches FMA contraction off on both sides, so its arithmetic is the same
operation for operation; what the test reproduces in fp32 itself are the header's INPUTS (the relative pose as a numpy fp32 product of the device's matrices, the
back-projection terms), so a verdict could still differ for a block with a form within an ulp of zero, and these scenes have none.  The poses are not read back from
the trace but rebuilt from the input poses through the library's own SE(3) seams (test_gpu_sweep_sums.device_matrices): the same matrices at the FIRST linearisation,
the only one these runs make.  Two runs give the same bits; the sums meet the fp64 reference of tests/sweep_ref.py at the
bars of tests/test_gpu_sweep_sums.py (imported)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sweep_ref as R
import test_gpu_sweep_sums as SS
from test_gpu_sweep_sums import gamma_d, gpu  # noqa: F401  (module-scoped fixtures: the GPU handle and the bars)
from bundletrack_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = R.PAIRS_FWD
Z0 = 0.8
SHIFT = 9.3                     # cache pixels
SIZES = {"16x16": (16, 16), "24x16": (24, 16), "72x40": (72, 40), "160x120": (160, 120), "208x168": (208, 168)}
_scenes = {}


def make_scene(size, case):
    """The dict tests/sweep_ref.scene() returns, for three frames of cache size `size` (see the module docstring)."""
    key = (size, case)
    if key in _scenes:
        return _scenes[key]
    from bundletrack_amd import synthetic as S
    from oracle import oracle as O
    WD, HD = SIZES[size]
    W, H = 4 * WD, 4 * HD
    K = S.NOCS_K.astype(np.float64).copy()
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xn, yn = xs / W - 0.5, ys / H - 0.5
    z = Z0 + 0.012 * xn - 0.008 * yn + 0.02 * (xn * xn + yn * yn)
    X, Y = (xs - K[0, 2]) / K[0, 0] * z, (ys - K[1, 2]) / K[1, 1] * z
    P = np.stack([X, Y, z], -1)
    n = np.cross(np.gradient(P, axis=0), np.gradient(P, axis=1))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n *= -np.sign(n[..., 2:3])
    depth = np.repeat(z[None], 3, 0).astype(np.float32)
    normals = np.zeros((3, H, W, 4), np.float32)
    normals[..., :3] = n
    if case == "nodepth":
        depth[1] = 0.0
        normals[1] = 0.0
    fxc = K[0, 0] * WD / W
    step = {"right": (SHIFT, 0.03), "left": (-SHIFT, 0.03), "bottom": (0.03, SHIFT), "top": (0.03, -SHIFT)}.get(case, (0.05, 0.03))
    T0 = S.orbit_pose(0.3)
    rot1 = {"sideways": np.array([0.0, 0.9, 0.0]), "behind": np.array([0.0, np.pi, 0.0])}.get(case, np.zeros(3))
    poses = np.stack([T0,
                      T0 @ S.se3_exp(rot1, np.array([step[0] * Z0 / fxc, step[1] * Z0 / fxc, 0.0005])),
                      T0 @ S.se3_exp(np.zeros(3), np.array([0.45 * step[0] * Z0 / fxc, -0.45 * step[1] * Z0 / fxc, 0.001]))]).astype(np.float32)
    rng = np.random.default_rng(19)
    corr = np.zeros(120, R.ENTRYJ)
    inv = np.linalg.inv(poses.astype(np.float64))
    for p, (i, j) in enumerate(PAIRS):
        pm = rng.uniform(-0.1, 0.1, (40, 3))
        blk = corr[40 * p:40 * p + 40]
        blk["imgIdx_i"], blk["imgIdx_j"] = i, j
        blk["pos_i"] = pm @ inv[i, :3, :3].T + inv[i, :3, 3]
        blk["pos_j"] = pm @ inv[j, :3, :3].T + inv[j, :3, 3] + rng.normal(scale=0.001, size=(40, 3))
    caches = [O.build_cache(depth[k], normals[k], K.astype(np.float32), 4.0) for k in range(3)]
    sc = dict(name=f"{size} {case}", K=K.astype(np.float32), H=H, W=W, campos=np.stack([c["campos"] for c in caches]), normals=np.stack([c["normals"] for c in caches]),
              intr=caches[0]["intr"], poses=poses, corr=corr)
    assert sc["campos"].shape == (3, HD, WD, 4)
    _scenes[key] = sc
    return sc


def run(g, sc, flags=0, tiles=0, skip=1, count_live=False):
    """One traced first linearisation; returns (records [3, 28], live-block total or None, block ranges [3, bh * bw, 2] read back from the device)."""
    bs = g.BatchSolver(g.ws, n_gn_iters=1, dense_tiles=tiles, flags=flags)
    cam_d = g.torch.from_numpy(sc["campos"][None]).to(g.dev)
    nrm_d = g.torch.from_numpy(sc["normals"][None]).to(g.dev)
    corr_d, offs_d, mx = SS.corr_inputs(g, [sc["corr"]], [np.arange(4, dtype=np.uint32) * 40])
    poses_d = g.torch.from_numpy(sc["poses"][None]).to(g.dev)
    HD, WD = sc["campos"].shape[1:3]
    live = None
    try:
        g.ws.set_option(_lib.OPT_BLOCK_SKIP, skip)
        zn = g.pack_zn(g.ws, cam_d, nrm_d)
        ranges_d = g.torch.zeros((3, (HD // 8) * (WD // 8), 2), device=g.dev)
        _lib.check(_lib.lib().btba_zn_block_ranges(g.ws.handle, 3, HD, WD, zn.data_ptr(), ranges_d.data_ptr()), "btba_zn_block_ranges")
        if count_live:
            g.ws.set_option(_lib.OPT_COUNT_LIVE, 1)
        tr = bs.solve_zn(zn, sc["H"], sc["W"], sc["K"], corr_d, offs_d, mx, poses_d, trace=True)
        tv = bs.trace_view(tr)
        st = g.ws.collect_stats()
        if count_live:
            live = g.ws.live_blocks()
    finally:
        g.ws.set_option(_lib.OPT_BLOCK_SKIP, 1)
        if count_live:
            g.ws.set_option(_lib.OPT_COUNT_LIVE, 0)
    assert not tiles or st["dense_tiles"] == tiles, st
    return tv.dense_pair[0, 0].copy(), live, ranges_d.cpu().numpy(), bs.params


@pytest.fixture(scope="module")
def hull(tmp_path_factory):
    """tests/cpp/hull_host.cpp -- the header compiled for the host -- as a shared library."""
    so = str(tmp_path_factory.mktemp("hull") / "libhull_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cpp", "hull_host.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    L.hull_band_live.restype = ctypes.c_int
    L.hull_band_live.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_float] * 4 + [ctypes.c_int] * 2 + [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_float] * 2 + \
                                [ctypes.c_int] * 2 + [ctypes.c_void_p]
    return L


def host_live_counts(g, hull, sc, ranges, prm):
    """Per pair, the blocks the host-compiled header keeps: relative pose from the device's own matrices, multiplied in fp32."""
    from bundletrack_amd import synthetic as S
    HD, WD = sc["campos"].shape[1:3]
    T, Tinv = SS.device_matrices(g, sc["poses"])
    K = sc["K"].astype(np.float32)
    one = np.float32(1.0)
    xi, yi = S.cache_source_pixels(sc["H"], sc["W"], HD, WD)
    lut = np.concatenate([(one / K[0, 0]) * xi.astype(np.float32) + (-K[0, 2] / K[0, 0]), (one / K[1, 1]) * yi.astype(np.float32) + (-K[1, 2] / K[1, 1])]).astype(np.float32)
    fx, fy, cx, cy = (float(v) for v in np.asarray(sc["intr"], np.float32)[:4])
    out = []
    for i, j in PAIRS:
        Tij = Tinv[i].astype(np.float32) @ T[j].astype(np.float32)
        R9, t3 = np.ascontiguousarray(Tij[:3, :3], np.float32), np.ascontiguousarray(Tij[:3, 3], np.float32)
        rg = np.ascontiguousarray(ranges[j], np.float32)
        out.append(hull.hull_band_live(R9.ctypes.data, t3.ctypes.data, fx, fy, cx, cy, WD, HD, lut.ctypes.data, rg.ctypes.data, prm.depth_min, prm.depth_max, 0, HD // 8, None))
    return out


def reference(g, sc):
    key = ("setup", sc["name"])
    if key not in g.refs:
        T, Tinv = SS.device_matrices(g, sc["poses"])
        g.refs[key] = R.scene_refs(sc, T, Tinv, PAIRS)
    return g.refs[key]


def check_records(recs, refs, gamma, what):
    for (i, j), rec, ref in zip(PAIRS, recs, refs):
        cnt = float(rec[27])
        assert np.all(np.isfinite(rec)), what
        assert cnt == int(cnt) and ref["count"] <= int(cnt) <= ref["count"] + ref["borderline"], f"{what} pair ({i}, {j}): count {cnt}, reference {ref['count']} + {ref['borderline']}"
        e = R.dense_normalised_error(rec, ref)
        print(f"{what} pair ({i}, {j}): count {cnt:.0f}, normalised error S {e[0]:.3e} g {e[1]:.3e} (bars {gamma[0]:.3e} / {gamma[1]:.3e})")
        assert e[0] <= gamma[0] and e[1] <= gamma[1], f"{what} pair ({i}, {j})"


CASES = [(s, c) for s in ("16x16", "24x16", "72x40") for c in ("right", "left", "bottom", "top")] + \
        [("72x40", "sideways"), ("72x40", "behind"), ("72x40", "nodepth"), ("160x120", "right"), ("160x120", "top")]


def check_block_list_set_up(gpu, gamma_d, hull, size, case, tiles):
    sc = make_scene(size, case)
    WD, HD = SIZES[size]
    nblocks = (WD // 8) * (HD // 8)
    recs, live, ranges, prm = run(gpu, sc, tiles=tiles, count_live=True)
    recs_again, _, _, _ = run(gpu, sc, tiles=tiles)
    recs_all, live_all, _, _ = run(gpu, sc, tiles=tiles, skip=0, count_live=True)
    host = host_live_counts(gpu, hull, sc, ranges, prm)
    print(f"{size} {case} tiles {tiles}: live blocks {live} of {3 * nblocks} (host per pair {host}), accepted {recs[:, 27]}")
    assert np.array_equal(recs.view(np.uint32), recs_again.view(np.uint32)), "two runs differ"
    assert np.array_equal(recs[:, 27], recs_all[:, 27]), (recs[:, 27], recs_all[:, 27])      # the skip drops no accepted pixel
    assert live_all == 3 * nblocks                                                                    # no ranges: every block is walked
    assert live == sum(host), (live, host)
    if case in ("right", "left", "bottom", "top"):
        assert 0 < host[0] < nblocks and recs[0, 27] > 0           # the blob crosses the edge: blocks fall out, pixels stay
    if case == "sideways":
        assert host[0] == 0 and host[2] == 0 and np.all(recs[0] == 0.0) and np.all(recs[2] == 0.0) and recs[1, 27] > 0
    if case == "behind":
        assert host[0] == nblocks and host[2] == nblocks and np.all(recs[0] == 0.0) and np.all(recs[2] == 0.0)
    if case == "nodepth":
        assert host[0] == 0 and host[2] == nblocks and np.all(recs[0] == 0.0) and np.all(recs[2] == 0.0)
    check_records(recs, reference(gpu, sc), gamma_d, f"{size} {case} tiles {tiles}")


@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("size,case", CASES, ids=[f"{s}-{c}" for s, c in CASES])
def test_block_list_set_up(gpu, gamma_d, hull, size, case, tiles):
    check_block_list_set_up(gpu, gamma_d, hull, size, case, tiles)


@pytest.mark.parametrize("case", ["right", "top"])
def test_block_list_second_compaction_pass(gpu, gamma_d, hull, case):
    """A band of 513 .. 1024 blocks (208 x 168 at one tile: 546) takes two passes of the list compaction; the second one reads its ranges in the loop."""
    assert 512 < (SIZES["208x168"][0] // 8) * (SIZES["208x168"][1] // 8) <= 1024
    check_block_list_set_up(gpu, gamma_d, hull, "208x168", case, 1)


def test_masked_list_walk_is_untouched(gpu, gamma_d):
    """The valid-pixel lists (BTBA_FLAG_COMPACTION) walk no blocks: the same sums, no block counted."""
    sc = make_scene("72x40", "right")
    recs, live, _, _ = run(gpu, sc, flags=_lib.FLAG_COMPACTION, count_live=True)
    assert live == 0
    check_records(recs, reference(gpu, sc), gamma_d, "72x40 right lists")
