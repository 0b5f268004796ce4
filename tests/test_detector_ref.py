"""The detector front end on the CPU: the restatement tests/detector_ref.py against an fp64 bilinear resample and hand-computed
cases (weights, copy, box average, padding, grey rule), btba_detector_transform against the restatement and an fp64 inverse, and
the ABI of the new entry points with every BTBA_EINVAL case that needs no GPU."""
import ctypes as C

import numpy as np
import pytest

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S

import detector_ref as R

NEW = ("btba_detector_params_default", "btba_detector_transform", "btba_detector_inputs", "btba_detector_keypoints_to_image")


@pytest.fixture(autouse=True)
def _product_contract():
    """The restatement pins the rules of these entry points: every test here needs them to exist."""
    assert set(NEW) <= set(_lib.declared_symbols()) and hasattr(_lib, "DetectorParams")


def _frame(seed=3, H=480, W=640):
    pb = S.make_problem(2, 10, seed=seed, background=True)
    return S.make_color(pb.poses_gt[1], pb.K, H, W, seed=seed)


def _bilinear64(sq, S_):
    """cv::resize's sample positions with exact fp64 bilinear weights and clamped coordinates."""
    side = sq.shape[0]
    c = (np.arange(S_) + 0.5) * (side / S_) - 0.5
    c = np.clip(c, 0, side - 1)
    i0 = np.floor(c).astype(int)
    i1 = np.minimum(i0 + 1, side - 1)
    f = c - i0
    sq = sq.astype(np.float64)
    h = sq[:, i0] * (1 - f)[None, :, None] + sq[:, i1] * f[None, :, None]
    return h[i0] * (1 - f)[:, None, None] + h[i1] * f[:, None, None]


@pytest.mark.parametrize("roi", [(100.0, 110.0, 200.0, 210.0), (0.0, 639.0, 0.0, 479.0), (37.0, 400.0, 150.0, 171.0),
                                 (300.0, 321.0, 13.0, 470.0), (11.0, 590.0, 40.0, 433.0), (200.0, 601.0, 30.0, 431.0)])
def test_restatement_within_one_level_of_fp64_bilinear(roi):
    col = _frame()
    sq = R.crop_square(col, roi)
    ref = _bilinear64(sq, 400)
    for form in ("simd", "scalar"):
        out = R.resize(sq, 400, form).astype(np.float64)
        assert np.abs(out - ref).max() <= 1.0 + 1e-9, form


def test_upscale_by_two_weights():
    x0, x1, a0, a1 = R.axis_coeffs(8, 4, True)
    assert list(zip(a0[1:7], a1[1:7])) == [(1536, 512), (512, 1536)] * 3
    assert list(x0[1:7]) == [0, 0, 1, 1, 2, 2]
    assert (a0[0], a1[0], x0[0]) == (2048, 0, 0) and (a0[7], a1[7], x0[7]) == (2048, 0, 3)     # both ends zeroed
    y0, y1, b0, b1 = R.axis_coeffs(8, 4, False)
    assert (y0[0], y1[0], b0[0], b1[0]) == (0, 0, 512, 1536)                                  # rows keep fy at the border
    assert (y0[7], y1[7], b0[7], b1[7]) == (3, 3, 1536, 512)


def test_side_equal_to_out_size_is_a_copy():
    col = _frame(5)
    roi = (100.0, 500.0, 40.0, 440.0)
    sq = R.crop_square(col, roi)
    for form in ("simd", "scalar"):
        assert np.array_equal(R.resize(sq, 400, form), sq.astype(np.uint8))
    col = _frame(6)[:300, :300]
    roi = (50.0, 250.0, 10.0, 110.0)                                                    # 200 wide, 100 high: side 200 -> S 200
    sq = R.crop_square(col, roi)
    assert np.array_equal(R.resize(sq, 200), sq.astype(np.uint8)) and not sq[100:].any()


def test_side_twice_out_size_is_the_box_average():
    rng = np.random.default_rng(1)
    col = rng.integers(0, 256, (1000, 1000, 4), dtype=np.uint8)
    roi = (100.0, 900.0, 150.0, 950.0)
    sq = R.crop_square(col, roi).astype(np.int64)
    want = (sq[0::2, 0::2] + sq[0::2, 1::2] + sq[1::2, 0::2] + sq[1::2, 1::2] + 2) // 4
    assert np.array_equal(R.resize(sq, 400), want.astype(np.uint8))


def test_padding_is_zero_and_enters_the_blend_at_the_crop_edge():
    col = np.full((64, 64, 4), 200, np.uint8)
    roi = (0.0, 10.0, 0.0, 40.0)                                        # 10 x 40 crop: side 40, padding right of column 9
    sq = R.crop_square(col, roi)
    assert (sq[:, :10] == 200).all() and not sq[:, 10:].any()
    out = R.resize(sq, 80)                                              # 2x up: output column 19 blends columns 9 and 10
    x0, x1, a0, a1 = R.axis_coeffs(80, 40, True)
    assert (x0[20], x1[20], a0[20], a1[20]) == (9, 10, 512, 1536)
    assert (out[:, :19] == 200).all() and not out[:, 21:].any()
    assert (out[:, 19] == 150).all() and (out[:, 20] == 50).all()      # 200 * 1536 / 2048, 200 * 512 / 2048


def test_grey_rule_within_one_level_of_float_bt601_and_exact_division():
    v = np.arange(1 << 24, dtype=np.int64)
    bgr = np.stack([v & 255, (v >> 8) & 255, v >> 16], -1)
    g = (9798 * bgr[:, 0] + 19235 * bgr[:, 1] + 3735 * bgr[:, 2] + 16384) >> 15
    f = 0.299 * bgr[:, 0] + 0.587 * bgr[:, 1] + 0.114 * bgr[:, 2]        # the server's RGB2GRAY sees B as R
    assert np.abs(g - f).max() <= 1.0 and g.max() == 255
    y = R.grey(bgr[:1 << 16].astype(np.uint8))
    assert np.array_equal(y, ((9798 * bgr[:1 << 16, 0] + 19235 * bgr[:1 << 16, 1] + 3735 * bgr[:1 << 16, 2] + 16384) >> 15).astype(np.float32) / np.float32(255))
    gg = np.arange(256)
    assert np.array_equal(gg.astype(np.float32) / np.float32(255.0), (gg / 255.0).astype(np.float32))   # double rounding is innocuous here


def _transform(roi, S_=400):
    fwd, bwd = np.zeros(9, np.float32), np.zeros(9, np.float32)
    r = np.asarray(roi, np.float32)
    rc = _lib.lib().btba_detector_transform(C.byref(_lib.detector_params(out_size=S_)), r.ctypes.data, fwd.ctypes.data, bwd.ctypes.data)
    return rc, fwd.reshape(3, 3), bwd.reshape(3, 3)


def test_transform_bit_exact_and_close_to_fp64_inverse():
    rng = np.random.default_rng(7)
    worst = 0.0
    for k in range(500):
        S_ = int(rng.choice([4, 100, 400, 1024]))
        umin, vmin = (int(x) for x in rng.integers(0, 2000, 2))
        w, h = (int(x) for x in rng.integers(1, 1500, 2))
        roi = (umin, umin + w, vmin, vmin + h)
        rc, fwd, bwd = _transform(roi, S_)
        assert rc == 0
        rf, rb = R.transform(roi, S_)
        assert fwd.tobytes() == rf.tobytes() and bwd.tobytes() == rb.tobytes(), roi
        inv = np.linalg.inv(fwd.astype(np.float64))
        for (i, j) in ((0, 0), (0, 2), (1, 1), (1, 2), (2, 2)):
            ulp = np.spacing(np.float32(abs(inv[i, j]))) if inv[i, j] else np.float32(1e-45)
            worst = max(worst, abs(float(bwd[i, j]) - inv[i, j]) / float(ulp))
    assert worst <= 2.0, worst
    rc, fwd, _ = _transform((0, 10, 0, 10))
    assert fwd[0, 2] == 0 and not np.signbit(fwd[0, 2])                              # 0 - fl(s * 0) = +0


def test_keypoint_map_inverts_forward_transform():
    rng = np.random.default_rng(2)
    roi = (123.0, 456.0, 78.0, 300.0)
    from bundletrack_amd.detection import detector_transform
    fwd, _ = detector_transform(roi)
    k = rng.uniform(0, 400, (1000, 2)).astype(np.float32)
    full = R.keypoints_to_image(k, roi)
    back = full.astype(np.float64) @ fwd[:2, :2].T.astype(np.float64) + fwd[:2, 2]
    assert np.abs(back - k).max() < 1e-3


def test_abi_detector_entry_points():
    assert set(NEW) <= set(_lib.declared_symbols()) and set(NEW) <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.lib()
    for s in NEW:
        assert hasattr(L, s)
    assert C.sizeof(_lib.DetectorParams) == 4
    assert _lib.detector_params().out_size == 400
    assert L.btba_version() == 105


def test_transform_rejects_bad_arguments():
    L = _lib.lib()
    r = np.array([10, 30, 20, 25], np.float32)
    out = np.zeros(9, np.float32)
    call = lambda prm=C.byref(_lib.detector_params()), roi=r.ctypes.data, f=out.ctypes.data, b=out.ctypes.data: L.btba_detector_transform(prm, roi, f, b)
    assert call() == 0
    assert call(prm=None) == _lib.BTBA_EINVAL and call(roi=None) == _lib.BTBA_EINVAL
    assert call(f=None) == _lib.BTBA_EINVAL and call(b=None) == _lib.BTBA_EINVAL
    for s in (0, 2, 6, 402, 4100, -4):
        assert call(prm=C.byref(_lib.detector_params(out_size=s))) == _lib.BTBA_EINVAL, s
    assert call(prm=C.byref(_lib.detector_params(out_size=4))) == 0 and call(prm=C.byref(_lib.detector_params(out_size=4096))) == 0
    for bad in ([10.5, 30, 20, 25], [10, 30, 20, 25.25], [10, 10, 20, 25], [10, 30, 20, 20], [10, 9, 20, 25], [-1, 30, 20, 25],
                [np.nan, 30, 20, 25], [10, np.inf, 20, 25], [9999, 0, 9999, 0]):
        a = np.array(bad, np.float32)
        assert call(roi=a.ctypes.data) == _lib.BTBA_EINVAL, bad


def test_device_entry_points_reject_bad_arguments_without_a_gpu():
    L = _lib.lib()
    ws = C.c_void_p(16)                                                # never dereferenced: every check comes first
    good_color = C.cast((C.c_void_p * 1)(C.c_void_p(256)), C.c_void_p)
    roi = np.array([10, 30, 20, 25], np.float32)
    prm = C.byref(_lib.detector_params())
    inp = dict(ws=ws, prm=prm, n=1, H=48, W=64, c=good_color, roi=roi.ctypes.data, bgr=C.c_void_p(1024), gray=C.c_void_p(2048))
    call = lambda **kw: L.btba_detector_inputs(*{**inp, **kw}.values())
    assert call(ws=None) == _lib.BTBA_EINVAL and call(prm=None) == _lib.BTBA_EINVAL
    assert call(prm=C.byref(_lib.detector_params(out_size=398))) == _lib.BTBA_EINVAL
    assert call(n=0) == _lib.BTBA_EINVAL and call(H=0) == _lib.BTBA_EINVAL and call(W=0) == _lib.BTBA_EINVAL
    assert call(c=None) == _lib.BTBA_EINVAL and call(roi=None) == _lib.BTBA_EINVAL
    assert call(c=C.cast((C.c_void_p * 1)(None), C.c_void_p)) == _lib.BTBA_EINVAL
    assert call(c=C.cast((C.c_void_p * 1)(C.c_void_p(258)), C.c_void_p)) == _lib.BTBA_EINVAL         # uchar4: 4-byte aligned
    assert call(bgr=C.c_void_p(1026)) == _lib.BTBA_EINVAL and call(gray=C.c_void_p(2052)) == _lib.BTBA_EINVAL
    for bad in ([10.5, 30, 20, 25], [10, 10, 20, 25], [10, 30, 20, 20], [40, 65, 20, 25], [10, 30, 40, 49], [10, 30, 0, 49]):
        a = np.array(bad, np.float32)
        assert call(roi=a.ctypes.data) == _lib.BTBA_EINVAL, bad
    full = np.array([0, 64, 0, 48], np.float32)                        # the crop leaves out column umax and row vmax
    assert call(roi=full.ctypes.data, bgr=None, gray=None) == 0        # nothing to write: returns before any HIP call
    n = np.array([5], np.int32)
    kin = C.cast((C.c_void_p * 1)(C.c_void_p(4096)), C.c_void_p)
    kp = dict(ws=ws, prm=prm, nf=1, roi=roi.ctypes.data, i=kin, n=n.ctypes.data, o=kin)
    callk = lambda **kw: L.btba_detector_keypoints_to_image(*{**kp, **kw}.values())
    assert callk(ws=None) == _lib.BTBA_EINVAL and callk(prm=None) == _lib.BTBA_EINVAL and callk(nf=0) == _lib.BTBA_EINVAL
    assert callk(roi=None) == _lib.BTBA_EINVAL and callk(i=None) == _lib.BTBA_EINVAL and callk(n=None) == _lib.BTBA_EINVAL and callk(o=None) == _lib.BTBA_EINVAL
    null = C.cast((C.c_void_p * 1)(None), C.c_void_p)
    assert callk(i=null) == _lib.BTBA_EINVAL and callk(o=null) == _lib.BTBA_EINVAL
    for bad_n in (-1, 8193):
        a = np.array([bad_n], np.int32)
        assert callk(n=a.ctypes.data) == _lib.BTBA_EINVAL
    thin = np.array([10, 10, 20, 25], np.float32)
    assert callk(roi=thin.ctypes.data) == _lib.BTBA_EINVAL
    assert callk(i=C.cast((C.c_void_p * 1)(C.c_void_p(4100)), C.c_void_p)) == _lib.BTBA_EINVAL      # float2: 8-byte aligned


def test_report_scalar_and_simd_forms_on_synthetic_frames():
    """How often OpenCV's two vertical forms disagree (printed, not asserted): the reference's bytes may be either."""
    diff = total = 0
    for seed, roi in zip(range(4), [(200.0, 420.0, 150.0, 330.0), (150.0, 480.0, 100.0, 400.0), (250.0, 330.0, 200.0, 290.0), (0.0, 639.0, 0.0, 479.0)]):
        sq = R.crop_square(_frame(seed), roi)
        a, b = R.resize(sq, 400, "simd"), R.resize(sq, 400, "scalar")
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 1
        diff += int((a != b).sum())
        total += a.size
    print(f"\nscalar vs SIMD vertical form: {diff} of {total} bytes differ ({100.0 * diff / total:.2f} %), all by one level")
