"""The NOCS evaluation on the MI355X: 5 deg 5 cm, IoU25, mean rotation and mean translation error (the 6-PACK protocol).

Mirrors the reference's scorer (scripts/benchmark.py): per item the rotation error, the translation error and the box IoU with
its 20-step symmetry maximum (:65-159, called as at :262-272) come from one btba_nocs_errors call for any number of items
(include/btba.h fixes the arithmetic, all of it fp64); the per-class report (:276-319) is counting and averaging on the host.
The dataset walk of the reference's main (list.txt, the ground-truth pickles, _meta.txt) is not here: the functions take arrays.
Poses are OBJECT-IN-CAMERA with the translation in the unit of shift_thresh (the protocol's: mm)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib, nocs_params

NOCS_CLASSES = ("bottle", "bowl", "camera", "can", "laptop", "mug")      # class ids 1 .. 6 (the reference's synset_names)


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _dev_ptr64(t, what: str):
    """Raw device address of a dense float64 CUDA tensor (the C ABI sees a plain pointer)."""
    import torch
    if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float64:
        raise ValueError(f"{what}: expected a contiguous float64 CUDA tensor, got {t.dtype} on {t.device}")
    return t.data_ptr()


def nocs_errors(ws, boxes, class_id, box_index, poses_pred, poses_gt, handle_visible=None, **params):
    """btba_nocs_errors: (theta_deg, shift, iou) float64 [n] for n items.

    boxes: [8, 3] or [n_boxes, 8, 3] corner rows (load_model_scales).  class_id: int [n] in 1 .. 6; box_index: int [n] into boxes;
    handle_visible: int [n] or None (all 1, as the reference's scorer passes).  poses_pred, poses_gt: [n, 4, 4] (or [4, 4]);
    float32 poses are widened.  numpy poses: the call reads and writes host memory and returns numpy arrays; CUDA tensors:
    device_resident, the outputs are CUDA tensors.  params: fields of btba_nocs_params (n_sym_steps, flip_z180_pred,
    normalize_columns, clamp_acos; the thresholds belong to nocs_report)."""
    prm = nocs_params(**params)
    bx = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 8, 3))
    device = _is_torch(poses_pred)
    if device != _is_torch(poses_gt):
        raise ValueError("poses_pred and poses_gt must both be numpy arrays or both CUDA tensors")
    if device:
        import torch
        pp = poses_pred.to(torch.float64).reshape(-1, 16).contiguous()
        pg = poses_gt.to(torch.float64).reshape(-1, 16).contiguous()
    else:
        pp = np.ascontiguousarray(np.asarray(poses_pred, np.float64).reshape(-1, 16))
        pg = np.ascontiguousarray(np.asarray(poses_gt, np.float64).reshape(-1, 16))
    n = pp.shape[0]
    if pg.shape[0] != n:
        raise ValueError(f"{n} predicted poses but {pg.shape[0]} ground-truth poses")
    tables = []
    for name, t in (("class_id", class_id), ("box_index", box_index), ("handle_visible", handle_visible)):
        if t is None:
            tables.append(None)
            continue
        a = np.ascontiguousarray(np.asarray(t.cpu() if _is_torch(t) else t).astype(np.int32).reshape(-1))
        if a.shape[0] != n:
            raise ValueError(f"{name} has {a.shape[0]} entries for {n} items")
        tables.append(a)
    cid, bi, hv = tables
    if device:
        outs = [torch.empty(max(n, 1), dtype=torch.float64, device=pp.device) for _ in range(3)]
        args = [_dev_ptr64(pp, "poses_pred"), _dev_ptr64(pg, "poses_gt")] + [_dev_ptr64(o, "output") for o in outs]
    else:
        outs = [np.empty(max(n, 1), np.float64) for _ in range(3)]
        args = [pp.ctypes.data, pg.ctypes.data] + [o.ctypes.data for o in outs]
    check(lib().btba_nocs_errors(ws.handle, C.byref(prm), int(device), bx.shape[0], bx.ctypes.data, n, cid.ctypes.data,
                                 hv.ctypes.data if hv is not None else None, bi.ctypes.data, *args), "btba_nocs_errors")
    return tuple(o[:n] for o in outs)


def _seq_mean(values) -> float:
    """Sum from 0 in the order given, divided by the count (NaN without values): the order btba::nocsReport uses."""
    v = np.asarray(values, np.float64).reshape(-1)
    return float(np.cumsum(v)[-1]) / v.size if v.size else float("nan")


def nocs_report(theta, shift, iou, class_id, n_listed=None, rot_thresh_deg=5.0, shift_thresh=50.0, iou_thresh=0.25) -> dict:
    """benchmark.py:276-319 for one experiment: {class name: row, ..., "overall": row}.  A row holds
      n             the class's listed frames: n_listed[c] (a dict or a sequence indexed by class id 1 .. 6; the reference's
                    cls_num, which counts frames with ground truth so that missing predictions are misses), default the
                    number of items of the class
      acc_5deg5cm   100 x (items with theta < rot_thresh_deg and shift < shift_thresh) / n
      acc_iou25     100 x (items with iou > iou_thresh) / n
      rot_err_deg   mean theta over the items with iou > iou_thresh and theta < 360
      trans_err     mean shift over the items with iou > iou_thresh; trans_err_cm: the same / 10 (mm -> cm)
    Means are sums from 0 in item order over the count, NaN over nothing (and n == 0 gives NaN shares).  "overall" is
    the sum over the six classes of (row value / 6) in class order, as the reference forms it; its n is the total."""
    theta = np.asarray(theta.cpu() if _is_torch(theta) else theta, np.float64).reshape(-1)
    shift = np.asarray(shift.cpu() if _is_torch(shift) else shift, np.float64).reshape(-1)
    iou = np.asarray(iou.cpu() if _is_torch(iou) else iou, np.float64).reshape(-1)
    cid = np.asarray(class_id.cpu() if _is_torch(class_id) else class_id).astype(np.int64).reshape(-1)
    if not (theta.size == shift.size == iou.size == cid.size):
        raise ValueError("theta, shift, iou and class_id differ in length")
    out = {}
    acc = {"acc_5deg5cm": 0.0, "acc_iou25": 0.0, "rot_err_deg": 0.0, "trans_err": 0.0}
    total = 0
    with np.errstate(invalid="ignore"):
        for c in range(1, 7):
            sel = cid == c
            t, s, u = theta[sel], shift[sel], iou[sel]
            n = int(t.size) if n_listed is None else int(n_listed[c])
            total += n
            in55 = int(np.count_nonzero((t < rot_thresh_deg) & (s < shift_thresh)))
            over = u > iou_thresh
            row = {"n": n,
                   "acc_5deg5cm": in55 / n if n else float("nan"),
                   "acc_iou25": int(np.count_nonzero(over)) / n if n else float("nan"),
                   "rot_err_deg": _seq_mean(t[over & (t < 360.0)]),
                   "trans_err": _seq_mean(s[over])}
            for k in acc:
                acc[k] = acc[k] + row[k] / 6
            row["acc_5deg5cm"] *= 100
            row["acc_iou25"] *= 100
            row["trans_err_cm"] = row["trans_err"] / 10
            out[NOCS_CLASSES[c - 1]] = row
    out["overall"] = {"n": total, "acc_5deg5cm": acc["acc_5deg5cm"] * 100, "acc_iou25": acc["acc_iou25"] * 100,
                      "rot_err_deg": acc["rot_err_deg"], "trans_err": acc["trans_err"], "trans_err_cm": acc["trans_err"] / 10}
    return out


def nocs_report_experiments(reports) -> dict:
    """benchmark.py:316-319: the mean over experiments of the "overall" rows of their nocs_report."""
    reports = list(reports)
    rows = [r["overall"] for r in reports]
    return {k: _seq_mean([r[k] for r in rows]) for k in ("acc_5deg5cm", "acc_iou25", "rot_err_deg", "trans_err", "trans_err_cm")}


def load_nocs_pose_txt(path: str) -> np.ndarray:
    """A protocol *_pose.txt (three rows of R, then one row of t) as a float64 [4, 4] object-in-camera pose."""
    rows = [[float(v) for v in ln.split()] for ln in open(path).read().splitlines() if ln.strip()]
    if len(rows) < 4 or any(len(r) < 3 for r in rows[:4]):
        raise ValueError(f"{path}: expected three rows of R and one row of t")
    M = np.eye(4)
    M[:3, :3] = [r[:3] for r in rows[:3]]
    M[:3, 3] = rows[3][:3]
    return M


def save_nocs_pose_txt(path: str, pose) -> None:
    """Writes pose[:3, :3] row by row and pose[:3, 3] as the fourth line, each value with the digits that read back to it."""
    M = np.asarray(pose, np.float64)
    lines = [" ".join(repr(float(v)) for v in M[r, :3]) for r in range(3)] + [" ".join(repr(float(v)) for v in M[:3, 3])]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def load_model_scales(path: str) -> np.ndarray:
    """A model_scales/<model>.txt: the box's eight corner rows as float64 [8, 3]."""
    b = np.loadtxt(path, dtype=np.float64, ndmin=2)
    if b.shape != (8, 3):
        raise ValueError(f"{path}: expected 8 rows of 3, got {b.shape}")
    return b
