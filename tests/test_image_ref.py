"""The fp64 references of image_ref.py against the fp32 CPU oracle, the conditions on the test inputs, and the planted faults
(no GPU).

What test_gpu_image_stages.py asserts of the device is asserted here of oracle.erode_depth / gauss_filter_depth / process_depth /
depth_to_normals, through the same check_filter / check_normals: the oracle's worst error over the bar is the measured FLOOR that
the device's margin is argued from.  The inputs are held to their conditions (excluded pixels <= 5 % of the valid ones, >= 200 valid
pixels where the shape can hold them, every difference-scheme combination taken >= 20 times, the tile geometry the shapes were
chosen for), and numpy mutants of the reference that model plausible kernel faults have to be REJECTED by the same checkers:

  short_halo              the chain in 32 x 8 tiles from a window of h - 1
  in_image_denominator    the erode's count divided by the in-image neighbours, not the full window
  one_pass                one filter pass instead of two
  no_range_term           the range term dropped (at sigma_r = 0.01)
  gate_on_centre          the 0.01 gate on |c - centre| instead of |c - mean|
  opposite_neighbour      a normal's one-sided fallback taking the other neighbour
  no_flip                 the normal not turned towards the camera

Figures of one run (the oracle's floors, worst over all cases): filter chain 0.20 bars, one pass alone 0.35, normals 0.38."""
import numpy as np
import pytest

import image_ref as R
import ingest_ref

F32 = np.float32
CHAIN_SETS = [n for n in R.PARAM_SETS if not n.startswith("erode_alone")]


def _args(p):
    return (p["erode_radius"], p["erode_diff"], p["erode_ratio"], p["bf_radius"], p["sigma_d"], p["sigma_r"])


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _input(x):
    return ingest_ref.decode_depth(x) if x.dtype == np.uint16 else x


# ---- the inputs' conditions ----------------------------------------------------------------------------------------------------------------
def test_shapes_have_the_tile_geometry_they_were_chosen_for():
    assert [R.interior_workgroups(W, H, 5) for W, H in R.FILTER_SHAPES_H5] == [0, 1]
    assert [R.interior_workgroups(W, H, 8) for W, H in R.FILTER_SHAPES_H8] == [0, 1]
    assert R.halo(R.TRACKER) == 5 and R.halo(R.GENERIC) == 8 and R.halo(R.PARAM_SETS["radii_2_3"]) == 8
    W, H = R.FILTER_SHAPE_BIG
    assert R.interior_workgroups(W, H, 5) >= 2 and W % 32 and H % 8
    assert all(W * H < 900 for W, H in R.FILTER_SHAPES_SMALL) and all(W * H >= 900 for W, H in R.FILTER_SHAPES if (W, H) not in R.FILTER_SHAPES_SMALL)


@pytest.mark.parametrize("name", list(R.PARAM_SETS))
def test_cap_on_excluded_pixels(name):
    """A condition on the INPUTS, for every parameter set, shape and input format: not a measurement of any implementation."""
    for W, H in R.FILTER_SHAPES:
        for codes in (False, True):
            _, ref = R.filter_case(name, W, H, codes)
            assert not R.cap_failures(ref, W * H), (name, W, H, codes, R.cap_failures(ref, W * H))
            assert not ref["under1"].any() and not ref["under"].any()             # the underflow band has its own case


def test_scene_holds_what_it_is_built_of():
    W, H = R.FILTER_SHAPE_BIG
    for h in (4, 5, 6, 7, 8):
        d = R.scene(W, H, h)
        base = R.plane(W, H, 0)
        delta = d.astype(np.float64) - base
        assert (d == 0).sum() > 2 * W + 3 * (H - 2)                               # dead rows and columns, and holes
        assert ((delta > 0.14) & (delta < 0.16)).sum() >= 3                       # big flyers
        assert ((delta > 0.004) & (delta < 0.006)).sum() >= 4                     # small flyers
        assert (np.abs(delta - R.STEP) < 1e-6).sum() > 100                        # the box
        assert not d.flags.writeable
    # k STEP / n stays clear of the 0.01 gate by 8e-4 for full windows and for band edges (whole columns of a window)
    for n in (25, 49, 5, 7):
        assert min(abs(k * R.STEP / n - 0.01) for k in range(n + 1)) >= 8e-4


# ---- reference against the CPU oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.PARAM_SETS))
def test_erode_is_the_oracles_bit_for_bit(oracle, name):
    p = R.PARAM_SETS[name]
    edge, _ = R.edge_value_input()
    maps = [_input(R.filter_case(name, W, H, c)[0]) for W, H in R.FILTER_SHAPES for c in (False, True)] + [edge]
    for d in maps:
        got = oracle.erode_depth(d, p["erode_radius"], p["erode_diff"], p["erode_ratio"])
        assert np.array_equal(_bits(got), _bits(R.erode_ref(d, p["erode_radius"], p["erode_diff"], p["erode_ratio"])))


@pytest.mark.parametrize("name", CHAIN_SETS)
def test_oracle_filter_and_chain_inside_the_bars(oracle, name):
    p = R.PARAM_SETS[name]
    floor1 = floor2 = 0.0
    for W, H in R.FILTER_SHAPES:
        for codes in (False, True):
            x, ref = R.filter_case(name, W, H, codes)
            d = _input(x)
            # one pass, isolated, on the eroded map
            v, f, b, u = R.filter_pass_ref(ref["eroded"], p["bf_radius"], p["sigma_d"], p["sigma_r"])
            one = dict(value=v, flag=f, bar=b, under=u, valid=v != 0)
            c1 = R.check_filter(oracle.gauss_filter_depth(ref["eroded"], p["bf_radius"], p["sigma_d"], p["sigma_r"]), one)
            c2 = R.check_filter(oracle.process_depth(d, *_args(p)), ref)
            assert not c1["failures"] and not c2["failures"], (name, W, H, codes, c1["failures"], c2["failures"])
            floor1, floor2 = max(floor1, c1["worst"]), max(floor2, c2["worst"])
            print(f"{name} {W}x{H} {'codes' if codes else 'float'}: valid {c2['valid']} excluded {c2['excluded']} bar <= {c2['bar_max']:.2e} "
                  f"oracle worst/bar: pass {c1['worst']:.3f} chain {c2['worst']:.3f}")
    print(f"{name}: FLOOR one pass {floor1:.3f}, chain {floor2:.3f}")
    assert floor2 <= 1.0 and floor1 <= 1.0


@pytest.mark.parametrize("name", [n for n in R.PARAM_SETS if n.startswith("erode_alone")])
def test_with_1x1_windows_the_passes_are_the_identity(oracle, name):
    """bf_radius = 0: mean = c, one weight exp(0) = 1, o = c / 1.  The chain is then the erode, bit for bit (a NaN the erode let
    through -- NaN <= 0.1f is false -- has a NaN weight and leaves 0)."""
    p = R.PARAM_SETS[name]
    edge, _ = R.edge_value_input()
    for d in [R.filter_case(name, W, H)[0] for W, H in R.FILTER_SHAPES] + [edge]:
        ref = R.process_ref(d, **p)
        want = np.where(np.isnan(ref["eroded"]), F32(0), ref["eroded"])
        assert np.array_equal(ref["value"], want.astype(np.float64)) and not ref["flag"].any()
        assert np.array_equal(_bits(oracle.process_depth(d, *_args(p))), _bits(want))


@pytest.mark.parametrize("name", ["tracker", "generic", "filters_alone_r2", "filters_alone_r3", "erode_alone_r1"])
def test_oracle_agrees_on_the_special_values(oracle, name):
    p = R.PARAM_SETS[name]
    d, where = R.edge_value_input()
    assert len(where) == 11 and min(abs(ax - bx) + abs(ay - by) for a, (ax, ay) in where.items() for b, (bx, by) in where.items() if a != b) > 8
    ref = R.process_ref(d, **p)
    assert np.isfinite(ref["value"]).all() and not ref["flag"].any()
    c = R.check_filter(oracle.process_depth(d, *_args(p)), ref)
    print(name, c)
    assert not c["failures"], c["failures"]
    # the asymmetry: 0.1f itself is dropped by the erode (old <= 0.1f) but counts as a valid tap of the filter (c >= 0.1f)
    x, y = where["0.1f"]
    assert ref["eroded"][y, x] == 0
    v, _, _, _ = R.filter_pass_ref(np.full((1, 1), F32(0.1)), 0, 2.0, 1e5)
    assert v[0, 0] == float(F32(0.1))
    assert R.filter_pass_ref(np.full((1, 1), np.nextafter(F32(0.1), F32(0))), 0, 2.0, 1e5)[0][0, 0] == 0


def test_oracle_keeps_denormal_weights_in_the_underflow_case(oracle):
    """sigma_r = 0.05, a hole among c ~ 0.69: the weights are ~ exp(-95) ~ 4e-42.  libm's expf returns those denormals, so the oracle
    fills the hole ("keep"); the model of an exp that flushes them ("flush") leaves it 0 and is a different map."""
    d = R.underflow_input()
    keep, flush = (R.process_ref(d, under=m, **R.UNDERFLOW) for m in ("keep", "flush"))
    holes = np.argwhere(keep["under1"])
    assert holes.tolist() == [[5, 8], [6, 31]]
    got = oracle.process_depth(d, *_args(R.UNDERFLOW))
    ck, cf = R.check_filter(got, keep), R.check_filter(got, flush)
    print("keep:", ck, "\nflush:", cf["failures"])
    assert not ck["failures"] and cf["failures"]
    assert all(got[y, x] != 0 and flush["value"][y, x] == 0 for y, x in holes)


@pytest.fixture(scope="module")
def normals_cases(oracle):
    out = []
    for W, H in R.NORMALS_SHAPES:
        for ph in range(R.NORMALS_PHASES):
            d, K = R.normals_scene(W, H, ph), R.intrinsics(W, H)
            Ki = R.mat4_inverse_ref(K)
            P = R.backproject_ref(d, Ki)
            out.append((W, H, d, K, Ki, P, R.normals_ref(P, d)))
    return out


def test_backprojection_is_the_oracles_bit_for_bit(oracle, normals_cases):
    for W, H, d, K, Ki, P, ref in normals_cases:
        K4 = np.eye(4, dtype=F32)
        K4[:3, :3] = K
        assert np.array_equal(Ki, oracle.mat4_inverse(K4))                      # (signs of zeros aside)
        assert np.array_equal(_bits(P), _bits(oracle.depth_to_normals(d, K)[1]))


def test_oracle_normals_inside_the_bars(oracle, normals_cases):
    floor = 0.0
    for W, H, d, K, Ki, P, ref in normals_cases:
        c = R.check_normals(oracle.depth_to_normals(d, K)[0], ref)
        assert not c["failures"], (W, H, c["failures"])
        assert c["excluded"] == 0
        floor = max(floor, c["worst"])
    print(f"normals FLOOR {floor:.3f}; bars from {min(c['bar_min'] for c in [R.check_normals(r[6]['normals'], r[6]) for r in normals_cases] if c['compared']):.2e}"
          f" to {max(R.check_normals(r[6]['normals'], r[6])['bar_max'] for r in normals_cases):.2e}")
    assert floor <= 1.0
    assert [int(r[6]["valid"].sum()) for r in normals_cases if (r[0], r[1]) in ((1, 1), (2, 2))] == [0] * (2 * R.NORMALS_PHASES)
    assert all(r[6]["valid"].sum() <= 1 and (r[6]["sx"] >= 0).sum() == 1 for r in normals_cases if (r[0], r[1]) == (3, 3))


def test_normals_branch_census(normals_cases):
    cen = R.scheme_census([r[6] for r in normals_cases])
    print("census (sx, sy): pixels", sorted(cen.items()))
    live = (R.CENTRAL, R.PLUS, R.MINUS)
    for a in live:
        for b in live:
            assert cen.get((a, b), 0) >= 20, (a, b)
    assert sum(cen.get((R.NONE, b), 0) for b in live) >= 20                      # ok = false through the first axis only,
    assert sum(cen.get((a, R.NONE), 0) for a in live) >= 20                      # the second only,
    assert cen.get((R.NONE, R.NONE), 0) >= 20                                    # both
    assert sum(int(r[6]["flips"].sum()) for r in normals_cases) >= 20 and sum(int((r[6]["valid"] & ~r[6]["flips"]).sum()) for r in normals_cases) >= 20


def test_impulse_inputs_decide_their_support(oracle):
    """For the GPU test's support comparison.  The erode turns the flyer into a hole and spreads nothing here, so a defect's reach is
    what the two filter passes carry: exactly 2 bf_radius, the square of pixels whose reference value is not bit-equal; from
    that distance it enters the next tile, from one pixel further it does not.  Inside, some pixels change by more than the bars
    (not at radii (2, 3): 49-tap windows thin one tap's removal out to ~1e-5, under the two bars of 9e-6 each; that set keeps the
    exact half of the comparison, nothing changes out of reach)."""
    for name in R.IMPULSE_PARAMS:
        p = R.PARAM_SETS[name]
        r = 2 * p["bf_radius"]
        flat = R.process_ref(R.ramp(), **p)
        assert not flat["flag"].any() and (flat["value"] != 0).all()
        for kind in ("hole", "flyer"):
            for x, y in R.impulse_positions(p):
                ref = R.process_ref(R.impulse_input(kind, x, y), **p)
                changed, same, amb = R.support_ref(ref, flat)
                assert not ref["flag"].any() and (changed.any() or name == "radii_2_3"), (name, kind, x, y)
                assert not R.check_filter(oracle.process_depth(R.impulse_input(kind, x, y), *_args(p)), ref)["failures"]
                assert changed.sum() >= 9 or (name, kind) != ("filters_alone_r2", "flyer")
                ys, xs = np.nonzero(~same)
                assert (xs.min() - x, xs.max() - x, ys.min() - y, ys.max() - y) == (-r, r, -r, r), (name, kind, x, y)
        for (x, y), enters in (((64 - r, 16 - r), True), ((64 - r - 1, 16 - r - 1), False)):
            assert (x, y) in R.impulse_positions(p)
            _, same, _ = R.support_ref(R.process_ref(R.impulse_input("flyer", x, y), **p), flat)
            assert (~same[16:, 64:]).any() == enters


# ---- planted faults --------------------------------------------------------------------------------------------------------------------
def _chain_fault(name, shape, fault):
    d, ref = R.filter_case(name, *shape)
    bad = R.process_ref(d, **R.PARAM_SETS[name], _fault=fault)["value"].astype(F32)
    return R.check_filter(bad, ref)["failures"]


def test_checker_accepts_the_reference_itself_and_its_tiled_form():
    for name in ("tracker", "generic"):
        for shape in (R.FILTER_SHAPE_BIG, R.FILTER_SHAPES_H5[1]):
            d, ref = R.filter_case(name, *shape)
            assert not R.check_filter(ref["value"].astype(F32), ref)["failures"]
            full = R.tiled_process(d, R.PARAM_SETS[name], R.halo(R.PARAM_SETS[name]))
            assert np.array_equal(full, ref["value"])


@pytest.mark.parametrize("name", ["tracker", "radii_2_3", "filters_alone_r2"])
def test_planted_short_halo_is_rejected(name):
    """The ring at distance h reaches a tile's output through one thing only: the erode's decision on a pixel at distance
    2 bf_radius, which the filters then carry to the tile's edge.  The scene's small flyers at those distances make that decision
    matter (kept by a tile that misses some of their neighbours, they pass the gate).  At radii (2, 3) one kept flyer moves the
    tile's edge by 4e-6, half of that set's bar (it arrives through one 49-tap corner tap per pass), so the 101 x 37 scene holds a
    column of four there: 1.6 bars.  Limit, stated: under GENERIC's erode (diff 0.05) the scene holds no decision that ring can
    turn."""
    p = R.PARAM_SETS[name]
    for shape in (R.FILTER_SHAPE_BIG, R.FILTER_SHAPES_H8[1]):
        if name == "radii_2_3" and shape != R.FILTER_SHAPE_BIG:
            continue
        d, ref = R.filter_case(name, *shape)
        fails = R.check_filter(R.tiled_process(d, p, R.halo(p) - 1).astype(F32), ref)["failures"]
        print(name, shape, fails)
        assert fails
    if name == "radii_2_3":
        return
    # and on the impulse test's input with the flyer at distance 2 bf_radius from the seams
    h = R.halo(p)
    x, y = 64 - 2 * p["bf_radius"], 16 - 2 * p["bf_radius"]
    d = R.impulse_input("flyer", x, y)
    assert R.check_filter(R.tiled_process(d, p, h - 1).astype(F32), R.process_ref(d, **p))["failures"]


def test_planted_erode_denominator_is_rejected():
    for name in ("tracker", "erode_alone_r1", "erode_alone_r2"):
        p = R.PARAM_SETS[name]
        d, ref = R.filter_case(name, *R.FILTER_SHAPE_BIG)
        bad = R.erode_ref(d, p["erode_radius"], p["erode_diff"], p["erode_ratio"], _fault="in_image_denominator")
        assert not np.array_equal(_bits(bad), _bits(ref["eroded"])), name
    assert _chain_fault("tracker", R.FILTER_SHAPE_BIG, "in_image_denominator")
    assert _chain_fault("tracker", R.FILTER_SHAPES_H5[1], "in_image_denominator")


@pytest.mark.parametrize("fault,names", [("one_pass", CHAIN_SETS), ("no_range_term", ["generic", "filters_alone_r3"]),
                                         ("gate_on_centre", CHAIN_SETS)])
def test_planted_filter_faults_are_rejected(fault, names):
    for name in names:
        for shape in (R.FILTER_SHAPE_BIG, R.FILTER_SHAPES_H5[1], R.FILTER_SHAPES_SMALL[-1]):
            fails = _chain_fault(name, shape, fault)
            print(fault, name, shape, fails)
            assert fails, (fault, name, shape)


@pytest.mark.parametrize("fault", ["opposite_neighbour", "no_flip"])
def test_planted_normals_faults_are_rejected(normals_cases, fault):
    for W, H, d, K, Ki, P, ref in normals_cases:
        if W < 63:
            continue
        bad = R.normals_ref(P, d, _fault=fault)["normals"].astype(F32)
        fails = R.check_normals(bad, ref)["failures"]
        assert fails, (fault, W, H)
    # and the checker accepts the reference
    assert not R.check_normals(normals_cases[-1][6]["normals"].astype(F32), normals_cases[-1][6])["failures"]
