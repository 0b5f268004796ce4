"""Depth pre-processing and normals on the MI355X against the gate-aware fp64 references of image_ref.py -- never one kernel against
another.  Entries: process_depth (k_process_depth), ingest_frames on float metres and on uint16 codes (k_ingest_depth<.., float>,
<.., uint16_t>, k_ingest_maps) and depth_to_normals with want_xyz (k_depth_to_normals).  The inputs, their conditions and the planted
faults these assertions reject are in test_image_ref.py; the rules are in image_ref.py's docstring.

Assertions: erode alone (bf_radius = 0) and the back-projection bit for bit; the filter chain, outside flagged pixels, the same zero
pattern and |device - ref| <= MARGIN * bar; the normals the same zero pattern everywhere and |device - ref| <= MARGIN * bar outside
flagged pixels.

MARGIN = 1.  The bar is a bound for the kernel's own operation sequence, and what the device does differently from the fp32 CPU oracle
(whose worst error / bar, the floor, is printed next to the device's) is inside it already:
  * __expf instead of libm's expf: the bar's eps_w takes 2 + 1.16 |x| ulp per weight (the bound CUDA documents for __expf; gfx950's
    lowering, one multiply by log2 e and a 1-ulp v_exp_f32, stays within 1 + |x| / 2 ulp), |x| <= 4.5 on gated taps of a gated centre:
    <= 9e-7 relative, times a spread <= 0.02;
  * FMA contraction in the filter (sum += w * c, the weight's argument): it removes roundings the bar counts;
  * the range term multiplied by 1 / (2 sr^2) instead of divided: three roundings more on that term, counted in eps_w's 7 u |x|.
The normals kernel compiles with contraction off and IEEE sqrt and division, like the oracle: nothing to add.

Figures of one MI355X run are in DESIGN.md, "Testing depth pre-processing and normals"."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import image_ref as R
import ingest_ref

F32 = np.float32
MARGIN = 1.0
CHAIN_SETS = [n for n in R.PARAM_SETS if not n.startswith("erode_alone")]
ERODE_SETS = [n for n in R.PARAM_SETS if n.startswith("erode_alone")]
ENTRIES = ["process_depth", "ingest_float", "ingest_codes"]


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                  # (a copy: the cached inputs are read-only)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


class _Frame:
    depth_code_gpu = bgr_gpu = depth_gpu = normal_gpu = color_gpu = None


def _args(p):
    return (p["erode_radius"], p["erode_diff"], p["erode_ratio"], p["bf_radius"], p["sigma_d"], p["sigma_r"])


def _run(ws, entry, x, p):
    """The device's processed depth for input x (float32 metres, or uint16 codes for ingest_codes) through `entry`; for the ingest
    entries also (raw, normals, xyz, K)."""
    if entry == "process_depth":
        from bundletrack_amd.optimizer import process_depth
        return process_depth(ws, _t(x), **p).cpu().numpy(), None
    from bundletrack_amd.ingest import ingest_frames
    H, W = x.shape
    K = R.intrinsics(W, H)
    f = _Frame()
    ingest_frames(ws, [f], [_t(x)], None, K, want_xyz=True, want_raw=True, **p)
    return f.depth_gpu.cpu().numpy(), (f.depth_raw_gpu.cpu().numpy(), f.normal_gpu.cpu().numpy(), f.xyz_gpu.cpu().numpy(), K)


def _check_maps(dep, maps, x, where):
    """k_ingest_maps on the device's own processed depth: decode and back-projection bit for bit, normals inside their bars."""
    raw, nrm, xyz, K = maps
    want_raw = ingest_ref.decode_depth(x) if x.dtype == np.uint16 else x
    assert np.array_equal(_bits(raw), _bits(want_raw)), where
    P = R.backproject_ref(dep, R.mat4_inverse_ref(K))
    assert np.array_equal(_bits(xyz), _bits(P)), where
    c = R.check_normals(nrm, R.normals_ref(P, dep), MARGIN)
    assert not c["failures"], (where, c["failures"])
    return c


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", CHAIN_SETS)
def test_filter_chain_against_the_reference(ws, oracle, name, entry):
    p = R.PARAM_SETS[name]
    worst = worst_n = 0.0
    for W, H in R.FILTER_SHAPES:
        x, ref = R.filter_case(name, W, H, codes=entry == "ingest_codes")
        got, maps = _run(ws, entry, x, p)
        c = R.check_filter(got, ref, MARGIN)
        floor = R.check_filter(oracle.process_depth(ingest_ref.decode_depth(x) if x.dtype == np.uint16 else x, *_args(p)), ref)["worst"]
        line = (f"{name} {entry} {W}x{H}: interior workgroups {R.interior_workgroups(W, H, R.halo(p))} valid {c['valid']} excluded {c['excluded']} "
                f"bar <= {c['bar_max']:.2e} floor {floor:.3f} device worst/bar {c['worst']:.3f}")
        if maps is not None:
            cn = _check_maps(got, maps, x, (name, entry, W, H))
            worst_n = max(worst_n, cn["worst"])
            line += f"; normals valid {cn['valid']} excluded {cn['excluded']} worst/bar {cn['worst']:.3f}"
        print(line)
        assert not c["failures"], (name, entry, W, H, c["failures"])
        worst = max(worst, c["worst"])
    print(f"{name} {entry}: DEVICE WORST {worst:.3f} bars (normals {worst_n:.3f})")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ERODE_SETS)
def test_erode_alone_bit_for_bit(ws, name, entry):
    """bf_radius = 0: the two passes are the identity on eroded values (asserted of the reference in test_image_ref.py), but for a NaN
    the erode lets through, which they leave 0."""
    p = R.PARAM_SETS[name]
    cases = [R.filter_case(name, W, H, codes=entry == "ingest_codes") for W, H in R.FILTER_SHAPES]
    if entry != "ingest_codes":
        edge = R.edge_value_input()[0]
        cases.append((edge, R.process_ref(edge, **p)))
    for x, ref in cases:
        got, _ = _run(ws, entry, x, p)
        want = np.where(np.isnan(ref["eroded"]), F32(0), ref["eroded"])
        assert np.array_equal(_bits(got), _bits(want)), (name, entry, x.shape)
        assert np.array_equal(ref["value"], want.astype(np.float64))


@pytest.mark.parametrize("shape", R.NORMALS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_normals_against_the_reference(ws, oracle, shape):
    from bundletrack_amd.optimizer import depth_to_normals
    W, H = shape
    K = R.intrinsics(W, H)
    Ki = R.mat4_inverse_ref(K)
    for ph in range(R.NORMALS_PHASES):
        d = R.normals_scene(W, H, ph)
        n, xyz = depth_to_normals(ws, _t(d), K, want_xyz=True)
        n, xyz = n.cpu().numpy(), xyz.cpu().numpy()
        P = R.backproject_ref(d, Ki)
        assert np.array_equal(_bits(xyz), _bits(P)), (shape, ph)
        ref = R.normals_ref(P, d)
        c = R.check_normals(n, ref, MARGIN)
        floor = R.check_normals(oracle.depth_to_normals(d, K)[0], ref)["worst"]
        print(f"normals {W}x{H} phase {ph}: valid {c['valid']} excluded {c['excluded']} bar {c['bar_min']:.2e} .. {c['bar_max']:.2e} "
              f"floor {floor:.3f} device worst/bar {c['worst']:.3f}")
        assert not c["failures"], (shape, ph, c["failures"])


@pytest.mark.parametrize("name", R.IMPULSE_PARAMS)
def test_one_defect_at_the_tile_seams(ws, name):
    """A ramp with one hole or one small flyer at the tile corner (32, 8) and at distances h, h + 1, 2 bf_radius, 2 bf_radius + 1 from
    the seams x = 64, y = 16: the values against the reference, and the support of (device - device on the ramp) against the
    reference's -- nothing changes where the defect is out of reach, everything changes where the reference's change exceeds the bars."""
    from bundletrack_amd.optimizer import process_depth
    p = R.PARAM_SETS[name]
    flat = R.ramp()
    ref_flat = R.process_ref(flat, **p)
    got_flat = process_depth(ws, _t(flat), **p).cpu().numpy()
    assert not R.check_filter(got_flat, ref_flat, MARGIN)["failures"]
    worst = 0.0
    for kind in ("hole", "flyer"):
        for x, y in R.impulse_positions(p):
            d = R.impulse_input(kind, x, y)
            ref = R.process_ref(d, **p)
            got = process_depth(ws, _t(d), **p).cpu().numpy()
            c = R.check_filter(got, ref, MARGIN)
            assert not c["failures"], (name, kind, x, y, c["failures"])
            worst = max(worst, c["worst"])
            changed, same, _ = R.support_ref(ref, ref_flat)
            dev_changed = _bits(got) != _bits(got_flat)
            assert not (dev_changed & same).any(), (name, kind, x, y, "changed out of the defect's reach", np.argwhere(dev_changed & same)[:4].tolist())
            assert not (changed & ~dev_changed).any(), (name, kind, x, y, "unchanged where the reference changes", np.argwhere(changed & ~dev_changed)[:4].tolist())
    print(f"{name}: {2 * len(R.impulse_positions(p))} defects, device worst/bar {worst:.3f}")


@pytest.mark.parametrize("entry", ["process_depth", "ingest_float"])
@pytest.mark.parametrize("name", ["tracker", "generic", "filters_alone_r2", "filters_alone_r3"])
def test_special_depth_values(ws, name, entry):
    """0.1f and its neighbours, both zeros, a denormal, a negative value, NaN, both infinities and 1e30, each alone on a plane: the zero
    pattern and the values per the reference (which the CPU oracle agrees with, test_image_ref.py), every output finite."""
    p = R.PARAM_SETS[name]
    d, where = R.edge_value_input()
    ref = R.process_ref(d, **p)
    got, maps = _run(ws, entry, d, p)
    assert np.isfinite(got).all()
    c = R.check_filter(got, ref, MARGIN)
    print(name, entry, {k: float(got[y, x]) for k, (x, y) in where.items()}, f"worst/bar {c['worst']:.3f}")
    assert not c["failures"], c["failures"]
    assert c["excluded"] == 0
    if maps is not None:
        assert np.array_equal(_bits(maps[0]), _bits(d)) and np.isfinite(maps[1]).all() and np.isfinite(maps[2]).all()


@pytest.mark.parametrize("entry", ["process_depth", "ingest_float"])
def test_underflow_case(ws, oracle, entry):
    """sigma_r = 0.05 and a hole among c ~ 0.69: every weight is ~ exp(-95) ~ 4e-42, an fp32 denormal.  The device has to be one of the
    two whole-map references: "keep" (the hole is filled, inside a bar that carries the denormals' rounding) or "flush" (weights
    below FLT_MIN are 0 and the hole stays).  Which one is printed, and recorded in DESIGN.md."""
    d = R.underflow_input()
    keep, flush = (R.process_ref(d, under=m, **R.UNDERFLOW) for m in ("keep", "flush"))
    got, _ = _run(ws, entry, d, R.UNDERFLOW)
    orc = oracle.process_depth(d, *_args(R.UNDERFLOW))
    ck, cf = R.check_filter(got, keep, MARGIN), R.check_filter(got, flush, MARGIN)
    holes = [(int(y), int(x)) for y, x in np.argwhere(keep["under1"])]
    print(f"underflow {entry}: holes {holes} device {[float(got[h]) for h in holes]} oracle {[float(orc[h]) for h in holes]} "
          f"keep reference {[float(keep['value'][h]) for h in holes]} bar {[float(keep['bar'][h]) for h in holes]}")
    print(f"  against keep: {ck['failures'] or 'agrees'} (worst/bar {ck['worst']:.3f});  against flush: {cf['failures'] or 'agrees'} (worst/bar {cf['worst']:.3f})")
    assert np.isfinite(got).all()
    assert not ck["failures"] or not cf["failures"]
