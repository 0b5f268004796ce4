"""Writes tests/golden/nocs/nocs_reference.npz: inputs and the reference scorer's own results for them.

    python tests/golden/make_nocs_golden.py          (needs the reference checkout: BTBA_REFERENCE_DIR, see tests/nocs_ref.py)

The reference's scripts/benchmark.py is loaded by path and its normalizeRotation, compute_RT_degree_cm_symmetry and
compute_3d_iou_new are called as its main calls them (tests/nocs_ref.py::reference_eval).  Only inputs and results are stored.
240 cases: 216 over all six classes (mugs with the handle visible and not) with 0.5 .. 30 deg and 2 .. 60 mm offsets on boxes of
30 .. 150 mm with three distinct extents, 12 that the reference's IoU calls disjoint (exactly 0), 12 bottles whose prediction is turned 60 .. 120 deg about the
object's own y.  The file is written only if every case has theta >= 0.05 deg, no NaN, and no theta, shift or IoU within 1e-6 of
a protocol threshold (5 / 50 / 0.25)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import nocs_ref as N  # noqa: E402


def main():
    bm = N.reference_module()
    if bm is None:
        raise SystemExit(f"no reference checkout at {N.reference_dir()}")
    cs = N.concat_cases([N.make_cases(216, 20211, n_boxes=8),
                         N.make_cases(12, 20212, n_boxes=2, apart=True),
                         N.make_cases(12, 20213, n_boxes=2, classes=(1,), angle_deg=(0.5, 4.0), shift_mm=(2.0, 20.0), spin_deg=(60.0, 120.0))])
    theta, shift, iou = N.reference_eval(bm, cs)
    assert np.all(np.isfinite(theta)) and np.all(np.isfinite(shift)) and np.all(np.isfinite(iou)), "NaN from the reference"
    assert theta.min() >= 0.05, theta.min()
    assert np.abs(theta - 5.0).min() > 1e-6 and np.abs(shift - 50.0).min() > 1e-6 and np.abs(iou - 0.25).min() > 1e-6
    assert set(cs["class_id"]) == {1, 2, 3, 4, 5, 6} and set(cs["handle_visible"][cs["class_id"] == 6]) == {0, 1}
    assert np.count_nonzero(iou == 0.0) >= 10
    in55, iou25 = N.decisions(theta, shift, iou)
    print(f"{len(theta)} cases: theta {theta.min():.3f} .. {theta.max():.3f} deg, shift {shift.min():.2f} .. {shift.max():.2f} mm, "
          f"iou {iou.min():.3f} .. {iou.max():.3f}; 5deg5cm {in55.sum()}, IoU25 {iou25.sum()}, disjoint {np.count_nonzero(iou == 0.0)}")
    os.makedirs(os.path.dirname(N.GOLDEN), exist_ok=True)
    np.savez_compressed(N.GOLDEN, theta=theta, shift=shift, iou=iou, **cs)
    print(N.GOLDEN, os.path.getsize(N.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
