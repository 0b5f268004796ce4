"""The keypoint head (btba_lfnet_*) on the CPU: the numpy restatement (tests/lfnet_ref.py) against the reference's own numbers
(tests/golden/lfnet/lfnet_reference.npz, made under the stand-in ops of tests/golden/make_lfnet_golden.py) within the measured
bars, its stage B exactly, and its pieces against torch on the CPU where torch has the op.  No GPU."""
import os
import subprocess

import numpy as np
import pytest
import torch

import lfnet_ref as R


HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _cases(golden):
    for name, H, W, sf, over, n_cases in R.GROUPS:
        for i in range(n_cases):
            yield name, i, H, W, sf, R.params(**over), {k: float(golden[f"tol_{name}_{k}"]) for k in ("heat", "scale", "kpts", "patch")}


def test_restatement_and_reference_inside_the_measured_bars(golden):
    """The restatement's fp32 path and the stored reference result against the fp64 restatement: each of the four errors within
    tol = 4 err_ref of the group; stage B on the reference's heat map gives the reference's keypoints exactly."""
    n = 0
    for name, i, H, W, sf, prm, tol in _cases(golden):
        maps, photo, ori = R.group_inputs(golden, name, i, sf)
        ref = {k: golden[f"{name}_{i}_ref_{k}"] for k in ("heat", "scale", "kxy", "kpts", "kscale", "kori", "patches")}
        h64, s64 = R.heatmaps(maps, sf, H, W, prm, np.float64)
        kp64, ksc64, kor64, pt64, edge = R.crops(photo, ori, h64, s64, ref["kxy"], prm, np.float64)
        assert edge.mean() <= R.EDGE_SHARE
        h32, s32 = R.heatmaps(maps, sf, H, W, prm, np.float32)
        assert h32.dtype == np.float32 and s32.dtype == np.float32
        kxy = R.select(h32, prm)
        assert np.array_equal(kxy, ref["kxy"]), (name, i)
        assert np.array_equal(R.select(ref["heat"], prm), ref["kxy"]), (name, i)
        kp32, ksc32, kor32, pt32, _ = R.crops(photo, ori, h32, s32, kxy, prm, np.float32)
        rng = photo.max() - photo.min()
        for what, (h, s, kp, pt) in (("restatement", (h32, s32, kp32, pt32)), ("reference", (ref["heat"], ref["scale"], ref["kpts"], ref["patches"]))):
            err = R.errors(h, s, kp, pt, h64, s64, kp64, pt64, edge, sf, rng)
            print(name, i, what, err, tol)
            assert all(err[k] <= tol[k] for k in tol), (name, i, what, err, tol)
        assert np.abs(ref["kscale"] - ksc64).max() <= tol["scale"] * max(max(sf) - min(sf), 1.0)
        assert np.abs(ref["kori"] - kor64).max() == 0.0
        assert R.decision_margin(h64, prm) > 2.0 * tol["heat"]
        n += 1
    assert n == sum(g[-1] for g in R.GROUPS) == 5


def test_the_bars_are_those_of_fp32_rounding_and_a_wrong_tap_is_outside(golden):
    for name, *_ in R.GROUPS:
        assert 1e-9 < float(golden[f"tol_{name}_heat"]) < 1e-5 and float(golden[f"tol_{name}_patch"]) < 1e-3
    name, i, H, W, sf, prm, tol = next(_cases(golden))
    maps, photo, ori = R.group_inputs(golden, name, i, sf)
    h64, s64 = R.heatmaps(maps, sf, H, W, prm)
    # half-pixel centres in the resize (what torch and TF2 do) are far outside the heat bar
    shifted = [np.roll(m, 1, 1) for m in maps]
    assert np.abs(R.heatmaps(shifted, sf, H, W, prm)[0] - h64).max() > 1e3 * tol["heat"]
    # weights from unclamped taps (the border pixel instead of zero) are far outside the patch bar
    kxy = golden[f"{name}_{i}_ref_kxy"]
    _, _, _, pt64, edge = R.crops(photo, ori, h64, s64, kxy, prm)
    padded = np.pad(photo, 64, mode="edge")
    _, _, _, pt_border, _ = R.crops(padded, np.pad(ori, ((64, 64), (64, 64), (0, 0))), np.pad(h64, 64), np.pad(s64, 64), kxy + 64, prm)
    assert np.abs(pt_border - pt64)[~edge].max() > 1e3 * tol["patch"]


@pytest.mark.parametrize("H,W,k", [(9, 9, 15), (12, 17, 5), (33, 20, 31)])
def test_window_maximum_and_sum_against_torch(H, W, k):
    x = np.random.default_rng(H).normal(size=(3, H, W)).astype(np.float32)
    t = torch.from_numpy(x)[None]
    mx = torch.nn.functional.max_pool2d(torch.nn.functional.pad(t, (k // 2,) * 4, value=float("-inf")), k, stride=1)[0].numpy()
    assert np.array_equal(R.window_max(x, k), mx)
    sm = torch.nn.functional.conv2d(t.double().transpose(0, 1), torch.ones(1, 1, k, k, dtype=torch.float64), padding=k // 2)[:, 0].numpy()
    assert np.abs(R.window_sum(x.astype(np.float64), k) - sm).max() < 1e-12


def test_top_k_ties_go_to_the_lower_index_as_torch_sorts_them():
    """A map of repeated values: isolated equal peaks on a grid, more of them than top_k."""
    heat = np.zeros((40, 52), np.float32)
    heat[6:34:3, 6:46:3] = np.random.default_rng(1).integers(1, 4, (10, 14)).astype(np.float32)
    prm = R.params(pad_size=5, crop_radius=5, nms_ksize=3, top_k=37)
    kxy = R.select(heat, prm)
    assert len(kxy) == 37
    sc, pk = R.scores(heat, prm)
    order = torch.sort(torch.from_numpy(sc.reshape(-1).astype(np.float64)), descending=True, stable=True).indices[:37].numpy()
    want = np.sort(order)
    assert np.array_equal(kxy[:, 1] * 52 + kxy[:, 0], want)
    assert np.array_equal(kxy, R.select_bruteforce(heat, prm))


@pytest.mark.parametrize("top_k", [1, 20, 64, 200, 400])
def test_fill_case_against_brute_force(golden, top_k):
    """pad_size < crop_radius: zero-score peaks between the two frames survive while the zero scores before them fit into top_k."""
    name, H, W, sf, over, _ = R.GROUPS[2]
    prm = R.params(**dict(over, top_k=top_k))
    heat = golden[f"{name}_0_ref_heat"]
    kxy = R.select(heat, prm)
    assert np.array_equal(kxy, R.select_bruteforce(heat, prm))
    sc, pk = R.scores(heat, prm)
    n_pos = int((sc > 0).sum())
    assert n_pos < 64
    outside = ~R.frame_mask(H, W, prm["crop_radius"])[kxy[:, 1], kxy[:, 0]]
    if top_k == 64:
        assert outside.sum() == 3 and np.array_equal(kxy, golden[f"{name}_0_ref_kxy"])
    if top_k == 400:
        assert len(kxy) == pk.sum()
    if top_k <= n_pos:
        assert not outside.any() and len(kxy) == top_k


def test_negative_threshold_and_negative_heat_against_brute_force():
    heat = np.random.default_rng(5).normal(size=(12, 12)).astype(np.float32)
    for top_k in (1, 5, 100, 140, 144):
        prm = R.params(pad_size=0, crop_radius=2, nms_ksize=3, nms_thresh=-0.5, top_k=top_k)
        assert np.array_equal(R.select(heat, prm), R.select_bruteforce(heat, prm))


@pytest.mark.parametrize("n,scale,deg", [(32, 1.0, 0.0), (32, 0.70710678, 45.0), (9, 1.41421356, 90.0), (16, 1.0, 180.0)])
def test_crop_against_grid_sample_inside_the_image(n, scale, deg):
    """Strictly inside the image transformer_crop is plain bilinear sampling: grid_sample(align_corners=True) at the same points."""
    H, W = 96, 112
    img = np.random.default_rng(n).random((H, W))
    co, sn = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    out, x, y = R.crop(img, n, 55.3, 47.8, scale * co, scale * -sn, scale * sn, scale * co, np.float64)
    assert x.min() > 0 and x.max() < W - 1 and y.min() > 0 and y.max() < H - 1
    grid = torch.from_numpy(np.stack([2 * x / (W - 1) - 1, 2 * y / (H - 1) - 1], -1))[None]
    want = torch.nn.functional.grid_sample(torch.from_numpy(img)[None, None], grid, mode="bilinear", align_corners=True)[0, 0].numpy()
    assert np.abs(out - want).max() < 1e-12


def test_crop_outside_the_image_is_zero_not_the_border_pixel():
    img = np.ones((20, 20))
    out, x, y = R.crop(img, 32, 3.0, 10.0, 1.0, 0.0, 0.0, 1.0, np.float64)
    assert np.all(out[:, x[0] < 0] == 0.0) and np.all(out[:, (x[0] > 0.5) & (x[0] < 18.5)][8:24] == pytest.approx(1.0))


def test_resize_is_tf1s_not_torchs():
    """No half-pixel centres: output pixel i reads source i * in / out, so column 0 is the source's column 0 and an upsampled
    ramp keeps its slope from the first pixel on."""
    x = np.arange(12, dtype=np.float64).reshape(3, 4)
    out = R.resize(x, 6, 8, np.float64)
    assert np.array_equal(out[0, :7], np.arange(7) * 0.5) and out[0, 7] == 3.0
    assert np.array_equal(out[::2, ::2][:3, :4], x)
    assert np.array_equal(R.resize(x, 3, 4, np.float32), x.astype(np.float32))


def test_stage_b_by_the_devices_route_in_cpp_equals_the_restatement(golden, tmp_path):
    """tests/cpp/lfnet_host.cpp selects as the kernel does (keys, the k-th largest over all positions, ranks among the equal): bit
    for bit the numpy restatement, on stored heat maps and on maps of repeated, zero and negative values."""
    exe = str(tmp_path / "lfnet_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "cpp", "lfnet_host.cpp")])
    rs = np.random.default_rng(9)
    grid = np.zeros((40, 52), np.float32)
    grid[3:37:3, 3:49:3] = 1.0
    maps = [golden["g20x20_fill_0_ref_heat"], golden["g64x64_s5_0_ref_heat"], grid, rs.integers(0, 4, (12, 12)).astype(np.float32),
            rs.normal(size=(33, 47)).astype(np.float32), np.zeros((12, 12), np.float32), -np.ones((9, 9), np.float32)]
    n = 0
    for heat in maps:
        H, W = heat.shape
        for over in (dict(pad_size=2, crop_radius=2, nms_ksize=3, top_k=7), dict(pad_size=2, crop_radius=5, nms_ksize=5, top_k=64),
                     dict(pad_size=0, crop_radius=3, nms_ksize=3, top_k=H * W - 5, nms_thresh=-0.5), dict(crop_radius=1, nms_ksize=1, top_k=50, nms_thresh=0.3),
                     dict(crop_radius=0, nms_ksize=3, top_k=H * W + 10, nms_thresh=-2.0)):
            prm = R.params(**over)
            blob = np.array([H, W, prm["top_k"], prm["crop_radius"], prm["nms_ksize"]], np.int32).tobytes() + np.float32(prm["nms_thresh"]).tobytes() + \
                np.ascontiguousarray(heat, np.float32).tobytes()
            got = np.frombuffer(subprocess.run([exe], input=blob, check=True, stdout=subprocess.PIPE).stdout, np.int32)
            assert np.array_equal(got[1:].reshape(got[0], 2), R.select(heat, prm)), (heat.shape, over)
            n += 1
    assert n == 35
