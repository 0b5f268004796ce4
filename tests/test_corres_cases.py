"""CPU checks of tests/corres_cases.py: every built case of tests/test_gpu_corres_model.py run on the committed restatements alone
(match_ref.restate into corres_ref.CorresModel, inlier lists in fp64 numpy from the built geometry).  Each case's check() asserts
the floors its device test relies on -- chunk counts, conflict lanes, the stack-versus-mark split, compaction passes, inliers that
are not arange in the geometric regime -- so a case that has drifted off its path fails here, on any machine.  Also: the model's
full-state comparison accepts the model's own state written out the way the device exports it, and rejects one wrong entry in each
of its parts."""
import numpy as np
import pytest

import corres_cases as CC
from corres_ref import CorresModel, assert_state


def _run(case):
    run = CC.ModelRun(case).run()
    counts = case.check(run)
    print(f"{case.name}: {counts}")
    return run


@pytest.mark.parametrize("kind", ["bijection", "onto_one"])
@pytest.mark.parametrize("n2", CC.CHUNK_EDGES)
def test_chunk_edges(n2, kind):
    _run(CC.chunk_edges(n2, kind))


def test_cross_chunk():
    _run(CC.cross_chunk())


@pytest.mark.parametrize("regime", ["all", "geo"])
@pytest.mark.parametrize("mutual", [0, 1])
def test_many_to_one(mutual, regime):
    _run(CC.many_to_one(mutual, regime))


def test_allocator():
    _run(CC.allocator())


def test_slots():
    _run(CC.slots())


@pytest.mark.parametrize("n,variant", CC.REGISTRATIONS)
def test_registration(n, variant):
    _run(CC.registration(n, variant))


@pytest.mark.parametrize("build", [CC.prop_lower_rank_wins, CC.prop_excluded_by_a_key, CC.prop_excluded_by_b_key, CC.prop_passes,
                                   lambda: CC.prop_count(3), lambda: CC.prop_count(2)],
                         ids=["lower_rank_wins", "excluded_by_a_key", "excluded_by_b_key", "passes", "count3", "count2"])
def test_propagation(build):
    _run(build())


def test_tie_frames_walk_down_equal_distances():
    frames = CC.tie_frames()
    b, a = frames
    same = lambda i: [j for j in range(200) if np.array_equal(b.desc[j], a.desc[i])]
    for k, mutual in [(1, 0), (5, 0), (8, 1)]:
        recs = CC.restate(frames, [(1, 0)], CC.match_prm(CC.Chain([], k=k, mutual=mutual)), CC.K, CC.H, CC.W)[0][0]
        fwd = recs[recs["dir"] == 0]
        # the first 7 keypoints of B have no depth: the answer is the lowest copy with depth, if the k equal distances reach it
        want = {}
        for i in range(200):
            copies = same(i)
            assert len(copies) == 50                              # longer than k, a column quarter and a 64-column tile
            seen = [j for j in copies[:k] if j >= 7]
            if seen:
                want[i] = seen[0]
        assert {int(r["idx_a"]): int(r["idx_b"]) for r in fwd} == want
        assert np.all(fwd["dist"] == 0.0)
        assert (len(want) == 0) if k == 1 else (len(want) == 200 and max(want.values()) >= 8)
        assert (len(recs) > len(fwd)) == bool(mutual)


@pytest.mark.parametrize("seed", [41, 42])
def test_random_session(seed):
    _run(CC.random_session(seed))


# ---- the full-state comparison itself -----------------------------------------------------------------------------------------
def _export_of(R: CorresModel, slot_frame: dict, extra_rows=0):
    """The model's state in MapPointMemory.export()'s form, ids in creation order."""
    S = max(slot_frame) + 1
    frame_slot = {f: s for s, f in slot_frame.items()}
    ids = {mp: m for m, mp in enumerate(sorted(R.img))}
    img = np.full((len(ids) + extra_rows, S), -1, np.int32)
    for mp, d in R.img.items():
        for f, uv in d.items():
            img[ids[mp], frame_slot[f]] = R.key_index(f, uv)
    exp = {"slot_n": np.full(S, -1, np.int32), "canon": {}, "map": {}, "img": img, "overflow": 0}
    for s, f in slot_frame.items():
        n = len(R.kpts[f])
        exp["slot_n"][s] = n
        exp["canon"][s] = np.array([R.key_index(f, R.uv(f, i)) for i in range(n)], np.int32)
        exp["map"][s] = np.full(n, -1, np.int32)
        for uv, mp in R.maps[f].items():
            exp["map"][s][R.key_index(f, uv)] = ids[mp]
    return exp


def test_assert_state_accepts_the_model_and_rejects_one_wrong_entry():
    run = CC.ModelRun(CC.prop_lower_rank_wins()).run()
    R, sf = run.R, {0: 0, 1: 2, 3: 4}
    assert_state(R, _export_of(R, sf), sf)

    def wrong(edit, extra_rows=0, mark=0):
        exp = _export_of(R, sf, extra_rows)
        edit(exp)
        R.high_water += mark
        try:
            with pytest.raises(AssertionError) as err:
                assert_state(R, exp, sf)
        finally:
            R.high_water -= mark
        return str(err.value)
    wrong(lambda e: e["canon"][1].__setitem__(10, 10))                     # the repeated (u, v) given its own key
    wrong(lambda e: e["map"][3].__setitem__(0, int(e["map"][3][1])))       # a map_F entry naming another live track
    wrong(lambda e: e["map"][3].__setitem__(0, -1))                        # ... or none
    assert "map id" in wrong(lambda e: e["map"][0].__setitem__(0, 11), extra_rows=1, mark=1)     # ... or an empty row below the mark
    assert_state_ok = _export_of(R, sf, 1)                                  # (an empty row below the mark alone is a recycled id: fine)
    R.high_water += 1
    assert_state(R, assert_state_ok, sf)
    R.high_water -= 1
    wrong(lambda e: e["img"].__setitem__((0, 1), 5))                       # one img entry
    wrong(lambda e: e["img"].__setitem__((10, slice(None)), e["img"][9]))  # two rows from one creation
    wrong(lambda e: None, extra_rows=1)                                    # the high-water mark one too high
    wrong(lambda e: e.__setitem__("overflow", 1))
