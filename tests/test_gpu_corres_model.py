"""The map-point memory on the MI355X against its sequential model, on built match lists (tests/corres_cases.py).

Every test runs a case's steps on the device (btba_mappoints_*, btba_corres_chain) and on corres_ref.CorresModel, whose NN matches
come from tests/match_ref.restate and whose RANSAC inliers come from btba_ransac_pairs_ex on the same points with the chain's
parameters.  After EVERY step it compares: each pair's records bit for bit, stage_counts, n_out and the FAIL status (after a
chain), and the full state (corres_ref.assert_state: canon, the img rows as a multiset of track sets, map_F key by key as the
track it names, every id below the high-water mark and on a non-empty row, the high-water mark itself).  Before the device runs,
the case's check() asserts through the model that the case reaches the path it is named for, and prints those counts.
Nothing here has a tolerance.  One module-scoped workspace, no subprocesses."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bundletrack_amd import _lib

import corres_cases as CC
from corres_ref import CorresModel, assert_state, model_points


@pytest.fixture(scope="module")
def ws():
    from bundletrack_amd.optimizer import Workspace
    w = Workspace()
    yield w
    w.close()


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


_shared = {}


def _plane_dev():
    if not _shared:
        _shared["depth"], _shared["normal"] = _cuda(CC.DEPTH), _cuda(CC.NORMAL)
    return _shared["depth"], _shared["normal"]


def _gpu_inliers(ws):
    """The chain's RANSAC on one pair's points: btba_ransac_pairs_ex with the chain's parameters.  In the "all" regime the list
    must be arange: that takes the chain's RANSAC out of the equation."""
    from bundletrack_amd.ransac import ransac_packed

    def inliers(recs, ch):
        rp = CC.ransac_prm(ch)
        pa, pb = model_points(recs, CC.POSE, CC.POSE)
        ids = ransac_packed(ws, pa, pb, np.array([len(recs)], np.int32), n_trials=rp.n_trials, inlier_dist=rp.dist_thres, seed=rp.seed,
                            hypothesis=rp.hypothesis)[0]["inlier_ids"].tolist()
        if ch.regime == "all":
            assert ids == list(range(len(recs))), (len(ids), len(recs))
        return ids
    return inliers


class DeviceRun(CC.ModelRun):
    """ModelRun with the device next to it; every step ends with the comparisons of the module docstring."""

    def __init__(self, ws, case):
        from bundletrack_amd.correspondence import MapPointMemory
        super().__init__(case, _gpu_inliers(ws))
        self.ws, self.mem = ws, MapPointMemory(ws)
        self.slot, self.dev_status, self.dev = {}, {}, {}
        self.bytes = []                                    # everything the device returned, for the run-to-run comparison

    def close(self):
        self.mem.close()

    def _frame(self, ch, h):
        from bundletrack_amd.bundler import FrameRef
        if h.id not in self.dev:
            self.dev[h.id] = (_cuda(h.kpts), _cuda(h.desc))
        depth, normal = _plane_dev()
        if h.id in ch.blind:
            depth = _cuda(CC.chain_depth(ch, h))
        kp, desc = self.dev[h.id]
        return FrameRef(id=h.id, pose_in_model=CC.POSE, kpts_gpu=kp, desc_gpu=desc, depth_gpu=depth, normal_gpu=normal)

    def register(self, fid):
        h = self.case.frames[fid]
        if fid not in self.dev:
            self.dev[fid] = (_cuda(h.kpts), _cuda(h.desc))
        lowest = min(set(range(len(self.slot) + 1)) - set(self.slot.values()))
        self.slot[fid] = self.mem.register_frame(self.dev[fid][0])
        assert self.slot[fid] == lowest, (fid, self.slot[fid], lowest)
        super().register(fid)

    def forget(self, fid):
        self.mem.forget_frame(self.slot.pop(fid))
        self.dev_status.pop(fid, None)
        super().forget(fid)

    def chain(self, ch):
        from bundletrack_amd.correspondence import find_corres_chain
        ref = super().chain(ch)
        fids, frames = self.chain_frames(ch)
        at = {f: i for i, f in enumerate(fids)}
        res = find_corres_chain(self.ws, self.mem, [self._frame(ch, h) for h in frames], [(at[a], at[b]) for a, b in ch.pairs],
                                [self.slot[f] for f in fids], np.array([self.dev_status.get(f, 0) for f in fids], np.int32),
                                CC.match_prm(ch), CC.ransac_prm(ch), K=CC.K, H=CC.H, W=CC.W)
        for f, s in zip(fids, res.status):
            self.dev_status[f] = int(s)
        for (a, b), got, n, sc, (want, stages) in zip(ch.pairs, res.per_pair, res.n_out, res.stage_counts, ref):
            assert list(sc) == stages, (a, b, list(sc), stages)
            assert n == len(want) and got.tobytes() == want.tobytes(), (a, b)
            self.bytes.append(got.tobytes())
        assert [bool(self.dev_status[f]) for f in fids] == [bool(self.status.get(f, False)) for f in fids]
        return ref

    def step(self, st):
        super().step(st)
        exp = self.mem.export()
        assert_state(self.R, exp, {s: f for f, s in self.slot.items()})
        self.bytes += [exp["img"].tobytes()] + [exp[k][s].tobytes() for k in ("canon", "map") for s in sorted(exp[k])]


def _run(ws, case):
    counts = case.check(CC.ModelRun(case, _gpu_inliers(ws)).run())          # the case reaches its path, by the model alone
    print(f"{case.name}: {counts}")
    run = DeviceRun(ws, case)
    try:
        run.run()
    finally:
        run.close()
    return run


@pytest.mark.parametrize("kind", ["bijection", "onto_one"])
@pytest.mark.parametrize("n2", CC.CHUNK_EDGES)
def test_update_chunk_edges(ws, n2, kind):
    _run(ws, CC.chunk_edges(n2, kind))


def test_update_cross_chunk_dependency(ws):
    _run(ws, CC.cross_chunk())


@pytest.mark.parametrize("regime", ["all", "geo"])
@pytest.mark.parametrize("mutual", [0, 1])
def test_update_many_to_one(ws, mutual, regime):
    _run(ws, CC.many_to_one(mutual, regime))


def test_allocator_free_stack_against_high_water_mark(ws):
    run = _run(ws, CC.allocator())
    assert run.R.high_water == 240


def test_slots_restride_and_reuse(ws):
    _run(ws, CC.slots())


def test_slot_limit_returns_enomem_and_changes_nothing(ws):
    """1024 live frames (three of 8 keypoints with tracks between the first two, then frames of one keypoint): the 1025th
    registration is BTBA_ENOMEM, export() is what it was, and a chain on existing frames still runs and matches the model."""
    rng = np.random.default_rng(21)
    d = CC.unit(rng, 8)
    frames = {f: CC.frame(f, CC.pixels(rng, 8), d[rng.permutation(8)]) for f in (0, 1, 2)}
    one = CC.frame(3, [[4.0, 4.0]], d[:1])
    case = CC.Case("slot_limit", frames, [("register", 0), ("register", 1), ("register", 2), CC.Chain([(1, 0)])], None)
    run = DeviceRun(ws, case)
    try:
        run.run()
        kp = _cuda(one.kpts)
        for f in range(3, 1024):
            frames[f] = one
            run.slot[f] = run.mem.register_frame(kp)
            assert run.slot[f] == f
            CorresModel.register(run.R, f, one.kpts)
        slot_frame = {s: f for f, s in run.slot.items()}
        before = run.mem.export()
        assert_state(run.R, before, slot_frame)
        with pytest.raises(_lib.BtbaError) as err:
            run.mem.register_frame(kp)
        assert err.value.status == _lib.BTBA_ENOMEM
        after = run.mem.export()
        assert np.array_equal(before["slot_n"], after["slot_n"]) and before["img"].tobytes() == after["img"].tobytes()
        assert all(np.array_equal(before[k][s], after[k][s]) for k in ("canon", "map") for s in before[k])
        run.step(CC.Chain([(2, 1)]))
        assert run.results[-1][0][1] == [8, 8, 8, 8] and len(run.R.tracks()) == 8
    finally:
        run.close()


@pytest.mark.parametrize("n,variant", CC.REGISTRATIONS)
def test_registration(ws, n, variant):
    _run(ws, CC.registration(n, variant))


@pytest.mark.parametrize("build", [CC.prop_lower_rank_wins, CC.prop_excluded_by_a_key, CC.prop_excluded_by_b_key, CC.prop_passes,
                                   lambda: CC.prop_count(3), lambda: CC.prop_count(2)],
                         ids=["lower_rank_wins", "excluded_by_a_key", "excluded_by_b_key", "passes", "count3", "count2"])
def test_propagation(ws, build):
    _run(ws, build())


@pytest.mark.parametrize("mutual", [0, 1])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_matcher_ties_lower_index_wins(ws, k, mutual):
    """Exact duplicate descriptors: equal d2 in runs of 50, longer than k and a column quarter and across the 64-column tiles; the
    device's candidate lists must rank them by index, bit for bit with the restatement."""
    from bundletrack_amd.bundler import FrameRef
    from bundletrack_amd.matching import match_pairs
    frames = CC.tie_frames()
    prm = CC.match_prm(CC.Chain([], k=k, mutual=mutual))
    want = CC.restate(frames, [(1, 0)], prm, CC.K, CC.H, CC.W)[0][0]
    dev = [FrameRef(id=h.id, pose_in_model=CC.POSE, kpts_gpu=_cuda(h.kpts), desc_gpu=_cuda(h.desc), depth_gpu=_cuda(h.depth),
                    normal_gpu=_plane_dev()[1]) for h in frames]
    got = match_pairs(ws, dev, [(1, 0)], prm, K=CC.K, H=CC.H, W=CC.W).per_pair[0]
    print(f"matcher ties k={k} mutual={mutual}: {len(want)} matches, {int((want['dist'] == 0).sum())} at distance 0")
    # A -> B: the lowest copy with depth is the third or fourth (none within k = 1); B -> A: B's 7 keypoints without depth ask nothing
    assert len(want) == (0 if k == 1 else 200) + (193 if mutual else 0)
    assert got.tobytes() == want.tobytes()


def test_random_session_and_determinism(ws):
    first = _run(ws, CC.random_session(41))
    again = DeviceRun(ws, CC.random_session(41))
    try:
        again.run()
    finally:
        again.close()
    assert len(first.bytes) == len(again.bytes) and all(x == y for x, y in zip(first.bytes, again.bytes))


def test_random_session_second_seed(ws):
    _run(ws, CC.random_session(42))
