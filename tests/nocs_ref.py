"""Test-side references for btba_nocs_errors: the CPU restatement (tests/cpp/nocs_host.cpp, written from include/btba.h's
contract), the symmetry-step table, case generators, the loader of the reference-produced vectors
(tests/golden/nocs/nocs_reference.npz), the call into the reference's own scorer where its checkout exists, and the ctypes entry
into the C++ host layer."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from match_ref import HERE, _build

GOLDEN = os.path.join(HERE, "golden", "nocs", "nocs_reference.npz")
CLASS_NAMES = ("BG", "bottle", "bowl", "camera", "can", "laptop", "mug")
Z180 = np.diag([-1.0, -1.0, 1.0, 1.0])

# The bars of the comparison with the reference's numbers.  theta: an acos argument off by ~20 ulp moves theta by eps / sin(theta),
# ~3e-10 deg at theta >= 0.05 deg; shift and iou are short sums and products of O(1e3) values.  All three sit four orders above
# the fp64 re-ordering spread and far below any reported digit.
THETA_ABS_DEG, SHIFT_REL, IOU_ABS = 1e-9, 1e-9, 1e-9

_host = None


def host_lib():
    """tests/cpp/libnocs_host.so (built on first use with g++ -O2 -ffp-contract=off)."""
    global _host
    if _host is None:
        _host = C.CDLL(_build("libnocs_host.so", [os.path.join(HERE, "cpp", "nocs_host.cpp")], []))
        _host.nocs_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _host.nocs_host.restype = None
    return _host


def step_table(n_steps: int) -> np.ndarray:
    """(cos, sin) of ((2 pi) i) / n_steps from the C library in double, [n_steps, 2]: what the library's host side computes."""
    return np.array([[math.cos(2.0 * math.pi * i / float(n_steps)), math.sin(2.0 * math.pi * i / float(n_steps))] for i in range(n_steps)])


def restate(boxes, class_id, box_index, poses_pred, poses_gt, handle_visible=None, n_sym_steps=20, flip_z180_pred=1,
            normalize_columns=1, clamp_acos=0):
    """nocs_host: (theta_deg, shift, iou) float64 [n], the contract of btba_nocs_errors on the CPU."""
    bx = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 8, 3))
    pp = np.ascontiguousarray(np.asarray(poses_pred, np.float64).reshape(-1, 16))
    pg = np.ascontiguousarray(np.asarray(poses_gt, np.float64).reshape(-1, 16))
    n = pp.shape[0]
    cid = np.ascontiguousarray(np.asarray(class_id, np.int32).reshape(-1))
    bi = np.ascontiguousarray(np.asarray(box_index, np.int32).reshape(-1))
    hv = None if handle_visible is None else np.ascontiguousarray(np.asarray(handle_visible, np.int32).reshape(-1))
    assert cid.shape[0] == bi.shape[0] == pg.shape[0] == n and bi.min(initial=0) >= 0 and bi.max(initial=0) < bx.shape[0]
    tab = np.ascontiguousarray(step_table(n_sym_steps))
    out = [np.zeros(max(n, 1)) for _ in range(3)]
    host_lib().nocs_host(bx.ctypes.data, n, cid.ctypes.data, hv.ctypes.data if hv is not None else None, bi.ctypes.data, pp.ctypes.data,
                         pg.ctypes.data, tab.ctypes.data, n_sym_steps, int(flip_z180_pred), int(normalize_columns), int(clamp_acos),
                         *[o.ctypes.data for o in out])
    return tuple(o[:n] for o in out)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_boxes(n_boxes, rng):
    """[n_boxes, 8, 3] corner rows in mm: three distinct extents of 30 .. 150 mm each, a small offset of the centre."""
    out = np.zeros((n_boxes, 8, 3))
    signs = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float64)
    for b in range(n_boxes):
        while True:
            ext = rng.uniform(30.0, 150.0, size=3)
            if min(abs(ext[0] - ext[1]), abs(ext[1] - ext[2]), abs(ext[0] - ext[2])) > 8.0:
                break
        out[b] = signs * ext / 2 + rng.uniform(-3.0, 3.0, size=3)
    return out


def make_cases(n, seed, n_boxes=12, angle_deg=(0.5, 30.0), shift_mm=(2.0, 60.0), classes=(1, 2, 3, 4, 5, 6), spin_deg=None, apart=False):
    """n items as the protocol's files hold them: dict of boxes [n_boxes, 8, 3], class_id, handle_visible, box_index (int32 [n]),
    pred, gt (float64 [n, 4, 4], object-in-camera, mm).  The ground truth carries a scale of 0.1 .. 0.6 in its rotation block (as
    NOCS gt_RTs do); the prediction is the ground truth turned by angle_deg about an axis perpendicular to the object's y (so that
    the error of a rotation-symmetric item is that angle too) and moved by shift_mm, stored before the protocol's z-180 flip.
    spin_deg: an extra turn of the prediction about the object's own y (the winning symmetry step is then not step 0).
    apart: the prediction is moved by 1500 .. 1800 mm along every axis instead: each of its corner coordinates then exceeds every
    coordinate of the ground truth's corners, which is what "disjoint" (IoU exactly 0) means in the reference's IoU (it takes min and
    max per corner over the three coordinates, include/btba.h step 4)."""
    rng = np.random.default_rng(seed)
    boxes = make_boxes(n_boxes, rng)
    cid = np.array([classes[k % len(classes)] for k in range(n)], np.int32)
    hv = np.where(cid == 6, rng.integers(0, 2, size=n), 1).astype(np.int32)
    bi = rng.integers(0, n_boxes, size=n).astype(np.int32)
    pred, gt = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))
    for e in range(n):
        R = _random_rotation(rng)
        t = np.array([rng.uniform(-150, 150), rng.uniform(-150, 150), rng.uniform(500, 1000)])
        phi = rng.uniform(0, 2 * np.pi)
        D = _rot([np.cos(phi), 0.0, np.sin(phi)], rng.uniform(*angle_deg))
        if spin_deg is not None:
            D = D @ _rot([0, 1, 0], rng.uniform(*spin_deg))
        d = rng.normal(size=3)
        d *= rng.uniform(*shift_mm) / np.linalg.norm(d)
        if apart:
            d = rng.uniform(1500.0, 1800.0, size=3)
        G, P = np.eye(4), np.eye(4)
        G[:3, :3], G[:3, 3] = R * rng.uniform(0.1, 0.6), t
        P[:3, :3], P[:3, 3] = R @ D, t + d
        gt[e], pred[e] = G, Z180 @ P
    return {"boxes": boxes, "class_id": cid, "handle_visible": hv, "box_index": bi, "pred": pred, "gt": gt}


def concat_cases(parts):
    """Several make_cases results as one (box indices shifted)."""
    out, off = {k: [] for k in ("boxes", "class_id", "handle_visible", "box_index", "pred", "gt")}, 0
    for p in parts:
        for k in out:
            out[k].append(p[k] + off if k == "box_index" else p[k])
        off += p["boxes"].shape[0]
    return {k: np.concatenate(v).astype(np.int32) if k in ("class_id", "handle_visible", "box_index") else np.concatenate(v) for k, v in out.items()}


def nan_iou_cases():
    """A bottle and a camera whose every IoU is 0 / 0: corner 0 of the box is the origin and both poses translate by (600, 600, 600),
    so that corner's three coordinates are equal, its extent is 0 under both poses and v1 = v2 = inter = 0 (include/btba.h step 4).
    The bottle's symmetric maximum must give 0 (a NaN step is never taken), the camera's single IoU NaN."""
    cs = make_cases(2, 8, n_boxes=1, classes=(1, 3))
    cs["boxes"][0, 0] = 0.0
    cs["gt"][:, :3, 3] = 600.0
    cs["pred"][:, :3, 3] = [-600.0, -600.0, 600.0]        # before the flip
    return cs


def session_cases(frames, seq):
    """A tracking session's final poses (camera -> model, FrameRef.pose_in_model) and the sequence's ground truth as NOCS items:
    object-in-camera in fp64 with the translation in mm, class camera (no symmetry), the box of the ellipsoid's extents in mm.
    Evaluate with flip_z180_pred = 0: these poses never went through the protocol's files."""
    from bundletrack_amd import synthetic as S
    n = len(frames)
    pred = np.linalg.inv(np.stack([np.asarray(f.pose_in_model, np.float64) for f in frames]))
    gt = np.linalg.inv(np.asarray(seq.poses_gt[:n], np.float64))
    pred[:, :3, 3] *= 1000.0
    gt[:, :3, 3] *= 1000.0
    signs = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float64)
    return {"boxes": (signs * S.SEMI_AXES * 1000.0)[None], "class_id": np.full(n, 3, np.int32), "handle_visible": np.ones(n, np.int32),
            "box_index": np.zeros(n, np.int32), "pred": pred, "gt": gt}


def restate_cases(cs, **kw):
    return restate(cs["boxes"], cs["class_id"], cs["box_index"], cs["pred"], cs["gt"], cs["handle_visible"], **kw)


def decisions(theta, shift, iou):
    """(5 deg 5 cm, IoU25) per item at the protocol's thresholds."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(theta) < 5.0) & (np.asarray(shift) < 50.0), np.asarray(iou) > 0.25


def assert_close(got, ref, what=""):
    """got against ref (each (theta, shift, iou)) at the bars above, every decision equal, no item left out."""
    (t, s, u), (rt, rs, ru) = got, ref
    assert np.all(np.isfinite(rt)) and np.all(np.isfinite(rs)) and np.all(np.isfinite(ru)), what
    dt, ds, du = np.abs(t - rt).max(), (np.abs(s - rs) / rs).max(), np.abs(u - ru).max()
    print(f"{what}: n {len(rt)}  max |dtheta| {dt:.3e} deg  max rel dshift {ds:.3e}  max |diou| {du:.3e}")
    assert dt <= THETA_ABS_DEG and ds <= SHIFT_REL and du <= IOU_ABS, (what, dt, ds, du)
    a, b = decisions(t, s, u), decisions(rt, rs, ru)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what


def load_golden():
    """(cases, (theta, shift, iou)) of tests/golden/nocs/nocs_reference.npz: inputs and what the reference's scorer returned for them."""
    z = np.load(GOLDEN)
    cs = {k: z[k] for k in ("boxes", "class_id", "handle_visible", "box_index", "pred", "gt")}
    return cs, (z["theta"], z["shift"], z["iou"])


def reference_dir():
    return os.environ.get("BTBA_REFERENCE_DIR", "/root/reference")


def reference_module():
    """The reference's scripts/benchmark.py loaded by path, or None where the checkout does not exist."""
    path = os.path.join(reference_dir(), "scripts", "benchmark.py")
    if not os.path.exists(path):
        return None
    import importlib.util
    spec = importlib.util.spec_from_file_location("btba_reference_benchmark", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_eval(bm, cs):
    """(theta, shift, iou) of the cases from the reference's own functions, called as its main calls them (the flip, both
    normalizeRotation calls, prediction first for the errors, ground truth first for the IoU)."""
    n = cs["pred"].shape[0]
    theta, shift, iou = np.zeros(n), np.zeros(n), np.zeros(n)
    z180 = np.zeros((4, 4), dtype=np.float32)
    z180[:3, :3] = np.diag([-1, -1, 1])
    z180[3, 3] = 1
    for e in range(n):
        pred = bm.normalizeRotation(np.array(z180 @ cs["pred"][e].tolist()))
        gt = bm.normalizeRotation(np.array(cs["gt"][e]))
        c, hv = int(cs["class_id"][e]), int(cs["handle_visible"][e])
        r = bm.compute_RT_degree_cm_symmetry(pred, gt, c, hv, bm.synset_names)
        bbox = cs["boxes"][cs["box_index"][e]].transpose()
        theta[e], shift[e] = r[0], r[1]
        iou[e] = bm.compute_3d_iou_new(gt, pred, bbox, bbox, hv, bm.synset_names[c], bm.synset_names[c])
    return theta, shift, iou


_driver = None


def driver():
    """tests/cpp/libnocs_driver.so: btba::nocsErrors and btba::nocsReport of the C++ host layer, linked against libbtba.so."""
    global _driver
    if _driver is None:
        from bundletrack_amd import _lib
        so = _lib.build_driver("nocs_driver")
        _driver = C.CDLL(so)
        _driver.nocs_errors_driver.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _driver.nocs_report_driver.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                               C.c_double, C.c_void_p]
    return _driver


REPORT_KEYS = ("n", "acc_5deg5cm", "acc_iou25", "rot_err_deg", "trans_err", "trans_err_cm")


def cpp_report(theta, shift, iou, class_id, n_listed=None, rot_thresh_deg=5.0, shift_thresh=50.0, iou_thresh=0.25):
    """btba::nocsReport as float64 [7, 6]: the rows of classes 1 .. 6 and overall, columns REPORT_KEYS."""
    t, s, u = (np.ascontiguousarray(np.asarray(a, np.float64)) for a in (theta, shift, iou))
    cid = np.ascontiguousarray(np.asarray(class_id, np.int32))
    nl = None if n_listed is None else np.ascontiguousarray(np.asarray([n_listed[c] for c in range(1, 7)], np.int64))
    rows = np.zeros((7, 6))
    assert driver().nocs_report_driver(len(t), t.ctypes.data, s.ctypes.data, u.ctypes.data, cid.ctypes.data,
                                       nl.ctypes.data if nl is not None else None, rot_thresh_deg, shift_thresh, iou_thresh, rows.ctypes.data) == 0
    return rows


def report_rows(rep):
    """A nocs_report dict in cpp_report's layout."""
    from bundletrack_amd.nocs_eval import NOCS_CLASSES
    return np.array([[float(rep[name][k]) for k in REPORT_KEYS] for name in NOCS_CLASSES + ("overall",)])
