"""btba_apply_masks on the CPU: the restatement tests/mask_ref.py against independent implementations (scipy's labelling,
dilation and convex hull), the hull-fill invariants, and the ABI of the new entry points."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage
from scipy.spatial import ConvexHull

from bundletrack_amd import _lib
from bundletrack_amd import synthetic as S

import mask_ref as R


def _cases():
    rng = np.random.default_rng(5)
    out = {"random_sparse": rng.random((37, 53)) < 0.25, "random_dense": rng.random((41, 29)) < 0.55}
    spiral = np.zeros((41, 41), bool)
    y, x, d, n = 20, 20, 0, 1
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    while 0 <= y < 41 and 0 <= x < 41:
        for _ in range(2):
            for _ in range(n):
                if 0 <= y < 41 and 0 <= x < 41:
                    spiral[y, x] = True
                y, x = y + steps[d][0], x + steps[d][1]
            d = (d + 1) % 4
        n += 2
    out["spiral"] = spiral
    comb = np.zeros((30, 40), bool)
    comb[0, :] = True
    comb[:, ::3] = True
    out["comb"] = comb
    pb = S.make_problem(2, 10, seed=2, background=True)
    out["silhouette_blobs"] = S.make_mask(pb.poses_gt[1], pb.K, pb.H, pb.W, seed=4, n_blobs=5, n_holes=4, bridge=True) > 0
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_labelling_equals_scipy(name):
    fg = CASES[name]
    ours, _, _ = R.label8(fg)
    ref, n = ndimage.label(fg, structure=np.ones((3, 3), int))
    assert ours.max() == n
    assert np.array_equal(ours, ref)                        # same partition, same raster-order numbering


def test_labelling_8_not_4_connected():
    fg = np.eye(6, dtype=bool)
    assert R.label8(fg)[0].max() == 1
    assert ndimage.label(fg)[1] == 6                         # 4-connected would split the diagonal


@pytest.mark.parametrize("d", [1, 3, 5, 15])
@pytest.mark.parametrize("name", ["random_sparse", "comb", "silhouette_blobs"])
def test_dilation_equals_scipy(name, d):
    fg = CASES[name]
    ref = ndimage.binary_dilation(fg, structure=np.ones((d, d), bool), border_value=0)
    assert np.array_equal(R.dilate(fg.astype(np.uint8), d), ref.astype(np.uint8))


@pytest.mark.parametrize("name", sorted(CASES))
def test_hull_vertices_equal_scipy_and_fill_covers_component(name):
    fg = CASES[name]
    M0, hull, win = R.hull_of_largest(fg)
    ys, xs = np.nonzero(win)
    pts = np.stack([xs, ys], 1).astype(float)
    qh = ConvexHull(pts)
    assert {tuple(int(v) for v in pts[i]) for i in qh.vertices} == set(hull)
    assert M0[win].all()                                     # the filled hull holds every pixel of the component
    assert M0.sum() >= win.sum()
    # every filled point is a convex combination of hull vertices: inside scipy's facets (a x + b y + c <= 0)
    fy, fx = np.nonzero(M0)
    assert (qh.equations[:, :2] @ np.stack([fx, fy]).astype(float) + qh.equations[:, 2:] <= 1e-9).all()


def test_largest_component_tie_goes_to_first_in_raster_order():
    fg = np.zeros((20, 20), bool)
    fg[12:15, 1:4] = True                                    # 9 pixels, later in raster order
    fg[2:5, 10:13] = True                                    # 9 pixels, first
    best, labels, _, _ = R.largest_component(fg)
    assert best == 1 and labels[2, 10] == 1
    M0, hull, _ = R.hull_of_largest(fg)
    assert M0[2:5, 10:13].all() and M0.sum() == 9


def test_degenerate_hulls():
    fg = np.zeros((9, 11), bool)
    fg[4, 6] = True
    M0, hull, _ = R.hull_of_largest(fg)
    assert hull == [(6, 4)] and M0.sum() == 1 and M0[4, 6]
    line = np.zeros((5, 12), bool)
    line[2, 3:10:] = True
    M0, hull, _ = R.hull_of_largest(line)
    assert sorted(hull) == [(3, 2), (9, 2)] and np.array_equal(M0.astype(bool), line)
    diag = np.zeros((7, 7), bool)
    diag[[1, 2, 3, 4], [1, 2, 3, 4]] = True
    M0, hull, _ = R.hull_of_largest(diag)
    assert sorted(hull) == [(1, 1), (4, 4)] and np.array_equal(M0.astype(bool), diag)


def test_empty_and_full_masks():
    M, d, n, c, roi = R.restate(np.zeros((5, 7), np.uint8), np.ones((5, 7), np.float32), np.ones((5, 7, 4), np.float32), None, hull=True, d=5)
    assert M.sum() == 0 and d.sum() == 0 and n.sum() == 0 and roi.tolist() == [9999, 0, 9999, 0]
    M, d, n, c, roi = R.restate(np.ones((5, 7), np.uint8), np.ones((5, 7), np.float32), np.ones((5, 7, 4), np.float32), None, hull=False, d=3)
    assert M.all() and d.all() and roi.tolist() == [0, 6, 0, 4]


def test_five_pixel_blob_fails_the_roi_gate_and_eight_passes():
    for side, width in ((5, 9), (8, 12)):
        m = np.zeros((40, 40), np.uint8)
        m[15:15 + side, 15:15 + side] = 1
        roi = R.roi_of(R.final_mask(m, False, 5))
        assert roi[1] - roi[0] + 1 == width and roi[3] - roi[2] + 1 == width


def test_abi_mask_entry_points():
    assert {"btba_mask_params_default", "btba_apply_masks"} <= set(_lib.declared_symbols())
    assert {"btba_mask_params_default", "btba_apply_masks"} <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.lib()
    for s in ("btba_mask_params_default", "btba_apply_masks"):
        assert hasattr(L, s)
    assert C.sizeof(_lib.MaskParams) == 8
    p = _lib.mask_params()
    assert (p.largest_component_hull, p.dilate) == (0, 5)
    assert L.btba_version() == 105


def test_apply_masks_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib()
    dummy = (C.c_void_p * 1)(C.c_void_p(256))
    t = C.cast(dummy, C.c_void_p)
    good = dict(ws=C.c_void_p(16), prm=C.byref(_lib.mask_params()), n=1, H=4, W=4, m=t, d=t, nr=t, c=None, o=None, roi=None)
    call = lambda **kw: L.btba_apply_masks(*{**good, **kw}.values())
    assert call(ws=None) == _lib.BTBA_EINVAL
    assert call(prm=None) == _lib.BTBA_EINVAL
    for d in (0, 2, 4, 17, -1):
        assert call(prm=C.byref(_lib.mask_params(dilate=d))) == _lib.BTBA_EINVAL
    assert call(n=0) == _lib.BTBA_EINVAL
    assert call(H=0) == _lib.BTBA_EINVAL and call(W=0) == _lib.BTBA_EINVAL
    assert call(H=1 << 16, W=1 << 15) == _lib.BTBA_EINVAL        # H * W = 2^31
    assert call(m=None) == _lib.BTBA_EINVAL and call(d=None) == _lib.BTBA_EINVAL and call(nr=None) == _lib.BTBA_EINVAL
    null = C.cast((C.c_void_p * 1)(None), C.c_void_p)
    assert call(m=null) == _lib.BTBA_EINVAL and call(d=null) == _lib.BTBA_EINVAL and call(nr=null) == _lib.BTBA_EINVAL
    odd = C.cast((C.c_void_p * 1)(C.c_void_p(264)), C.c_void_p)
    assert call(nr=odd) == _lib.BTBA_EINVAL                      # normals are float4: 16-byte aligned
    assert call(o=t) == _lib.BTBA_EINVAL                         # mask_out aliasing the mask
