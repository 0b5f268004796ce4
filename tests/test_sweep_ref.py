"""CPU checks of tests/sweep_ref.py: the threshold-aware fp64 references that tests/test_gpu_sweep_sums.py holds the sweeps to,
and the conditions its inputs must meet (few borderline pixels, enough accepts)."""
import numpy as np
import pytest

import sweep_ref as R
from oracle import oracle_np as ONP

ALL_PAIRS = R.PAIRS_FWD + R.PAIRS_REV
SPECIAL = {"edge32x24"}          # the zero- and one-valid-pixel frames: their point is a count of 0 or 1


@pytest.fixture(scope="module")
def refs(oracle):
    out = {}
    for name in R.SCENES:
        sc = R.scene(name)
        T, Tinv = R.oracle_matrices(sc["poses"])
        out[name] = (sc, T, Tinv, R.scene_refs(sc, T, Tinv, ALL_PAIRS))
    return out


@pytest.mark.parametrize("name", R.SCENES)
def test_classifier_equals_dense_pair_sums_without_borderline(refs, name):
    sc, T, Tinv, rr = refs[name]
    prm = dict(R.DEFAULT_PRM)
    seen = 0
    for (i, j), ref in zip(ALL_PAIRS, rr):
        if ref["borderline"]:
            continue
        S, g, cnt = ONP.dense_pair_sums(sc["campos"][[i, j]], sc["normals"][[i, j]], sc["intr"], T[i].astype(np.float64), T[j].astype(np.float64), Tinv[i].astype(np.float64), prm)
        assert cnt == ref["count"] and np.array_equal(S, ref["S"]) and np.array_equal(g, ref["g"])
        seen += 1
    assert seen >= 3 or name == "bg160x120"          # (the full-size scene has a few borderline pixels in every pair)


@pytest.mark.parametrize("name", R.SCENES)
def test_scale_is_symmetric_and_dominates(refs, name):
    for ref in refs[name][3]:
        assert np.array_equal(ref["sc_S"], ref["sc_S"].T) or np.abs(ref["sc_S"] - ref["sc_S"].T).max() <= 1e-15 * ref["sc_S"].max()
        assert np.all(np.abs(ref["S"]) <= ref["sc_S"] * (1 + 1e-12)) and np.all(np.abs(ref["g"]) <= ref["sc_g"] * (1 + 1e-12))
        assert np.all(ref["bud_S"] >= 0) and np.all(ref["bud_g"] >= 0)


@pytest.mark.parametrize("name", R.SCENES)
def test_inputs_keep_the_reference_inside_the_caps(refs, name):
    """Conditions on every (scene, ordered pair) the GPU test uses: borderline <= 1 % of the accepts, accepts >= 64."""
    sc, _, _, rr = refs[name]
    print(name, "valid pixels", sc["n_valid"], "accepts / borderline per pair", [(r["count"], r["borderline"]) for r in rr])
    for ref in rr:
        if name in SPECIAL:
            assert ref["borderline"] == 0 and ref["count"] in (0, 1)
        else:
            assert ref["count"] >= 64 and ref["borderline"] <= 0.01 * ref["count"]
    if name in SPECIAL:
        assert sc["n_valid"] == [sc["campos"].shape[1] * sc["campos"].shape[2], 1, 0]
        assert [r["count"] for r in rr] == [1, 0, 0, 0, 0, 0]


def test_hole_scene_blends_zero_taps(refs):
    """Accepted pixels whose four taps are all inside the image and of which one is a hole: zeros blend in (ICPUtil.h:83-110), so such a
    pixel passes the 2 cm gate only while the zero tap weighs under ~2 %.  With two or three zero taps no pixel of this cache passes
    (their weights add up), so the 1- and 2-tap blends the reference sees are those of the image border (taps outside the image)."""
    rr = refs["hole32x24"][3]
    census = sum(np.bincount(r["taps"][r["taps_in_image"] == 4], minlength=5) for r in rr[:2])      # target = the frame with the holes
    print("valid taps among accepted interior pixels:", census)
    assert census[3] >= 10 and census[4] > 0
    assert rr[0]["count"] < refs["hole32x24"][0]["n_valid"][0]          # and the holes' other neighbours are rejected
    valid = sum(np.bincount(r["taps"], minlength=5) for r in rr[:2])     # the same scene, VALID taps of all accepted pixels: 1 and 2 at its border
    print("valid taps among all accepted pixels of the hole scene:", valid)
    assert valid[1] > 0 and valid[2] > 0 and valid[3] >= 10
    border = sum(np.bincount(r["taps_in_image"], minlength=5) for name in ("bg32x24", "smooth13x9") for r in refs[name][3])
    print("taps inside the image among accepted pixels:", border)
    assert border[1] > 0 and border[2] > 0 and border[4] > 0


def test_oracle_record_layout(refs):
    """oracle_dense_records: the fp32 oracle's two-frame JtJ / Jtr blocks are S and g of the fp64 reference, sign included."""
    sc, _, _, rr = refs["bg32x24"]
    for rec, ref in zip(R.oracle_dense_records(sc, ALL_PAIRS, 1), rr):
        want = R.record27(ref["S"], ref["g"])
        assert np.abs(rec[:27] - want).max() <= 1e-4 * np.abs(want).max()
        assert rec[27] == ref["count"]


def test_oracle_floor_is_round_off(refs):
    fS, fg, per = R.oracle_dense_floor()
    print(f"fp32 oracle against the fp64 reference: floor S {fS:.3e}, floor g {fg:.3e}; per scene {per}")
    assert 0 < fS < 1e-4 and 0 < fg < 1e-3            # a few tens of ulps; g carries the cancellation inside the residual


# ---- sparse ------------------------------------------------------------------------------------------------------------
def test_sparse_system_equals_oracle_np(oracle):
    from bundletrack_amd import synthetic as S
    pb = S.make_problem(4, 60, seed=5, background=False, full_res=False)
    corr = pb.corr.copy()
    corr["imgIdx_i"][::9] = 0xFFFFFFFF
    sol = ONP.solve(np.zeros((4, 2, 2, 4)), np.zeros((4, 2, 2, 4)), (1, 1, 0, 0), corr, pb.poses_init, n_gn_iters=1, weight_dense_depth=0.0)
    T = np.stack([ONP.se3_exp(*ONP.se3_log(np.asarray(pb.poses_init[k], np.float64))) for k in range(4)])
    sp = R.sparse_system(corr, T)
    for key, want in (("A", sol["A"][0]), ("b", sol["b"][0]), ("Mdiag", sol["Mdiag"][0])):
        assert np.abs(sp[key] - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), key
    assert np.all(np.abs(sp["A"]) <= sp["sc_A"] * (1 + 1e-12)) and np.all(np.abs(sp["b"]) <= sp["sc_b"] * (1 + 1e-12)) and np.all(sp["Mdiag"] <= sp["sc_M"] * (1 + 1e-12))
    assert np.abs(sp["sc_A"] - sp["sc_A"].T).max() <= 1e-12 * sp["sc_A"].max()
    M, scM = R.precond_ref(sp["Mdiag"], sp["sc_M"])
    assert np.all(M[:6] == 1.0) and np.all(scM[:6] == 0.0) and np.all(M[6:] == 1.0 / sp["Mdiag"][6:])


def test_sparse_oracle_layout_and_floor(oracle):
    """The fp32 oracle's rhs / precond are the fp64 b / 1 / Mdiag in (rot, trans) order, to a few ulps of the absolute-value scale."""
    for N in (2, 3, 5):
        corr, poses = R.sparse_case(N)
        fl = R.oracle_sparse_floor(corr, poses)
        print(f"N = {N}: {len(corr)} entries, oracle floor rhs {fl[0]:.3e} precond {fl[1]:.3e} A {fl[2]:.3e}")
        assert 0 < min(fl) and max(fl) < 1e-5
