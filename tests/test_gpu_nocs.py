"""btba_nocs_errors on the MI355X: against the reference scorer's own numbers (tests/golden/nocs/nocs_reference.npz) and against the CPU
restatement (tests/cpp/nocs_host.cpp) at every batch shape (odd half wave, workgroup edge, grid tail), the symmetry-step counts,
repeatability, both buffer forms, NaN isolation, the contract's special cases on the device, argument checks, the C++ host layer,
and the 5 deg 5 cm / IoU25 counts of a 60-frame tracking session on the HIP optimiser.  One module-scoped workspace, no subprocesses."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib
from bundletrack_amd.nocs_eval import nocs_errors, nocs_report

import nocs_ref as N


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


def _gpu(ws, cs, **kw):
    return nocs_errors(ws, cs["boxes"], cs["class_id"], cs["box_index"], cs["pred"], cs["gt"], cs["handle_visible"], **kw)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_against_reference_vectors(ws):
    cs, ref = N.load_golden()
    N.assert_close(_gpu(ws, cs), ref, "GPU vs reference vectors")


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 17, 1000])
def test_against_restatement_mixed_batches(ws, n):
    cs = N.make_cases(n, 500 + n)
    N.assert_close(_gpu(ws, cs), N.restate_cases(cs), f"GPU vs restatement, n = {n}")


@pytest.mark.parametrize("steps", [1, 20, 32])
def test_symmetry_step_counts(ws, steps):
    cs = N.concat_cases([N.make_cases(30, 600 + steps), N.make_cases(12, 700 + steps, classes=(1, 6), angle_deg=(0.5, 4.0), spin_deg=(20.0, 160.0))])
    N.assert_close(_gpu(ws, cs, n_sym_steps=steps), N.restate_cases(cs, n_sym_steps=steps), f"GPU vs restatement, {steps} steps")


def test_flags_off(ws):
    cs = N.make_cases(40, 41)
    cs["gt"][:, :3, :3] /= np.linalg.norm(cs["gt"][:, :3, :1], axis=1, keepdims=True)     # unit columns: valid without normalize_columns
    cs["pred"] = N.Z180 @ cs["pred"]                                                         # and without the flip
    kw = dict(flip_z180_pred=0, normalize_columns=0)
    N.assert_close(_gpu(ws, cs, **kw), N.restate_cases(cs, **kw), "GPU vs restatement, flags off")
    N.assert_close(_gpu(ws, cs, **kw), _gpu(ws, dict(cs, pred=N.Z180 @ cs["pred"])), "flags off vs protocol form")


def test_repeatable_and_both_buffer_forms(ws):
    import torch
    cs = N.make_cases(300, 61)
    first = _gpu(ws, cs)
    for _ in range(3):
        assert _same_bits(first, _gpu(ws, cs))
    dev = nocs_errors(ws, cs["boxes"], cs["class_id"], cs["box_index"], torch.from_numpy(cs["pred"]).cuda(), torch.from_numpy(cs["gt"]).cuda(),
                      cs["handle_visible"])
    assert all(o.is_cuda and o.dtype == torch.float64 for o in dev)
    assert _same_bits(first, [o.cpu().numpy() for o in dev])
    f32 = nocs_errors(ws, cs["boxes"], cs["class_id"], cs["box_index"], cs["pred"].astype(np.float32), cs["gt"].astype(np.float32), cs["handle_visible"])
    wide = dict(cs, pred=cs["pred"].astype(np.float32).astype(np.float64), gt=cs["gt"].astype(np.float32).astype(np.float64))
    assert _same_bits(f32, _gpu(ws, wide))                            # float32 poses are widened, nothing else


def test_non_finite_poses_isolated(ws):
    cs = N.make_cases(5, 81)
    clean = _gpu(ws, cs)
    bad = dict(cs, pred=cs["pred"].copy(), gt=cs["gt"].copy())
    bad["pred"][1, 2, 1] = np.nan
    bad["gt"][3, 0, 3] = np.inf
    got = _gpu(ws, bad)
    for o, c in zip(got, clean):
        assert np.isnan(o[[1, 3]]).all() and np.array_equal(_bits(o[[0, 2, 4]]), _bits(c[[0, 2, 4]]))


def test_special_cases_on_the_device(ws):
    cs = N.make_cases(200, 5)
    same = dict(cs, pred=N.Z180 @ cs["gt"])
    t, s, u = _gpu(ws, same, clamp_acos=1)
    assert np.all(t <= 2e-5) and np.all(s == 0.0) and np.all(u == 1.0)
    t, s, u = _gpu(ws, same, clamp_acos=0)
    assert np.all(np.isnan(t) | (t <= 2e-5)) and np.all(u == 1.0)
    rows = dict(cs, pred=cs["pred"].copy(), gt=cs["gt"].copy())
    rows["pred"][1, 3, 3] = 2.0
    rows["gt"][2, 3, 0] = 1e-3
    t, s, u = _gpu(ws, rows)
    assert np.all(t[[1, 2]] == 10000.0) and np.all(s[[1, 2]] == 10000.0) and np.isnan(u[[1, 2]]).all() and np.isfinite(u[[0, 3]]).all()
    t, s, u = _gpu(ws, N.nan_iou_cases())
    assert u[0] == 0.0 and np.isnan(u[1]) and np.isfinite(t).all()


def test_rejected_arguments(ws):
    box = np.zeros((2, 8, 3))
    P = np.tile(np.eye(4).reshape(1, 16), (2, 1))
    o = np.zeros(2)
    ones, zeros = np.ones(2, np.int32), np.zeros(2, np.int32)

    def call(w=ws.handle, prm=None, n_boxes=2, boxes=box, n=2, cid=ones, hv=ones, bi=zeros, pp=P, out=o):
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        return _lib.lib().btba_nocs_errors(w, C.byref(prm) if prm is not None else None, 0, n_boxes, ptr(boxes), n, ptr(cid), ptr(hv), ptr(bi),
                                           ptr(pp), P.ctypes.data, ptr(out), o.ctypes.data, o.ctypes.data)
    assert call() == _lib.BTBA_OK and call(hv=None) == _lib.BTBA_OK
    assert call(n=0, cid=None, bi=None, pp=None, out=None) == _lib.BTBA_OK
    E = _lib.BTBA_EINVAL
    assert call(w=None) == E and call(boxes=None) == E and call(n_boxes=0) == E and call(n=-1) == E
    assert call(cid=None) == E and call(bi=None) == E and call(pp=None) == E and call(out=None) == E
    assert call(bi=np.array([0, 2], np.int32)) == E and call(bi=np.array([-1, 0], np.int32)) == E
    assert call(cid=np.array([0, 1], np.int32)) == E and call(cid=np.array([1, 7], np.int32)) == E
    assert call(prm=_lib.nocs_params(n_sym_steps=0)) == E and call(prm=_lib.nocs_params(n_sym_steps=33)) == E
    assert call(prm=_lib.nocs_params(n_sym_steps=32)) == _lib.BTBA_OK
    with pytest.raises(_lib.BtbaError):
        nocs_errors(ws, box, [1, 9], [0, 0], P.reshape(2, 4, 4), P.reshape(2, 4, 4))


def test_cpp_host_layer_equals_python(ws):
    cs = N.make_cases(37, 401)
    py = _gpu(ws, cs, n_sym_steps=16, clamp_acos=1)
    prm = _lib.nocs_params(n_sym_steps=16, clamp_acos=1)
    out = [np.zeros(37) for _ in range(3)]
    arrs = [np.ascontiguousarray(cs[k]) for k in ("boxes", "class_id", "handle_visible", "box_index", "pred", "gt")]
    assert N.driver().nocs_errors_driver(ws.handle.value, C.addressof(prm), arrs[0].shape[0], arrs[0].ctypes.data, 37, arrs[1].ctypes.data,
                                         arrs[2].ctypes.data, arrs[3].ctypes.data, arrs[4].ctypes.data, arrs[5].ctypes.data,
                                         *[a.ctypes.data for a in out]) == 0
    assert _same_bits(out, py)
    rep = N.report_rows(nocs_report(*py, cs["class_id"]))
    assert np.array_equal(rep.view(np.uint64), N.cpp_report(*py, cs["class_id"]).view(np.uint64))


# 5 deg 5 cm and IoU25 counts of a 60-frame c1 session (poses in metres x 1000, class camera, the ellipsoid's box in mm, no flip).
# The oracle-driven run of the same 60 frames on the CPU, scored through the restatement, gives 60 / 60 and 60 / 60 with mean theta
# 0.1176 deg (max 0.339), mean shift 0.1038 mm (max 0.220) and a smallest IoU of 0.9947: every frame is more than an order away
# from a threshold, the HIP path agrees with the oracle to ~1e-4 per pose, so the counts must be equal.
SESSION_ORACLE = (60, 60)


def test_sixty_frame_session_counts(ws):
    import torch
    from bundletrack_amd.optimizer import OptimizerGpu
    from test_tracking_session import run_session
    seq, bundler, frames, errs = run_session(OptimizerGpu(workspace=ws), 60, to_device=lambda a: torch.from_numpy(a).cuda())
    cs = N.session_cases(frames, seq)
    got = _gpu(ws, cs, flip_z180_pred=0)
    in55, iou25 = N.decisions(*got)
    ref55, ref25 = N.decisions(*N.restate_cases(cs, flip_z180_pred=0))     # the session's theta may lie below the 0.05 deg of the 1e-9 bar
    assert np.array_equal(in55, ref55) and np.array_equal(iou25, ref25)
    rep = nocs_report(*got, cs["class_id"])["camera"]
    print(f"60-frame session: 5deg5cm {in55.sum()} / 60, IoU25 {iou25.sum()} / 60, mean theta {got[0].mean():.4f} deg, "
          f"mean shift {got[1].mean():.4f} mm")
    assert rep["n"] == 60 and rep["acc_5deg5cm"] == 100 * (int(in55.sum()) / 60) and rep["acc_iou25"] == 100 * (int(iou25.sum()) / 60)
    assert (int(in55.sum()), int(iou25.sum())) == SESSION_ORACLE
