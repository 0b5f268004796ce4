"""btba_optimize_frames_keyed against the stateless call along random walks over its workspace state (tests/keyed_walk.py).

include/btba.h: "Results are bit-identical to btba_optimize_frames."  Each test keeps ONE Workspace alive through a whole walk -- frame
pool, correspondence pool, cached pair and solve tables -- and compares every keyed call with the same call through
OptimizerGpu(workspace=None): btba_optimize_frames with no workspace, which carries nothing from call to call.  The bar is == on the
poses' bytes.  Beside it the reported counts are held to host models: L <= cache_frames_built <= U (bounds that hold for any
least-recently-used policy) and corr_pairs_uploaded (the pool's index, with a reset allowed wherever the count is the all-pairs one).

The reference chain is closed in this file: for six calls spread over the walks the stateless result itself is compared with the CPU
oracle (oracle.solve on oracle.build_cache of the same frames), under the bars tests/test_gpu_parity.py::
test_edge_shapes_through_the_boundary uses -- 5e-4 for its many-frame windows of 128 x 96 frames (here: the window of 17), 1e-4
(TOL_R) for its windows of a few frames (here: 2 .. 9 frames).

On a mismatch the walk's prefix up to the failing step is written to tmp_path as JSON; KW.Tracker and Runner replay it as it is.
"""
import json

import numpy as np
import pytest

from bundletrack_amd import _lib, synthetic as S

import keyed_walk as KW

pytestmark = pytest.mark.gpu
BAR_FEW_FRAMES, BAR_MANY_FRAMES = 1e-4, 5e-4


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from bundletrack_amd import optimizer as O

    class G:
        pass
    g = G()
    g.torch, g.dev, g.O = torch, torch.device("cuda:0"), O
    g.base = {}                      # frame -> (depth, normals) on the device: uploaded once, shared by every walk, never written
    g.aux_ws = O.Workspace()         # builds the compact caches the foreign solve / objective calls are given
    g.report = {}
    assert _lib.LIB_PATH and KW.CORR_MIN_BYTES_DEFAULT == 1 << 20
    return g


class Runner:
    def __init__(self, g, walk, tmp_path, oracle=None):
        self.g, self.walk, self.tmp_path, self.oracle = g, walk, tmp_path, oracle
        self.ws = g.O.Workspace()
        self.tr = KW.Tracker(walk)
        self.clones = {}
        self.stats = dict(calls=0, U_gt_L=0, built_gt_L=0, foreign=0, anchors={})

    def buffers(self, f):
        g = self.g
        if f not in g.base:
            d, n = KW.frame(*f)
            g.base[f] = (g.torch.from_numpy(np.array(d)).to(g.dev), g.torch.from_numpy(np.array(n)).to(g.dev))
        gen = self.tr.sess.gen.get(f, 0)
        if gen == 0:
            return g.base[f]
        if (f, gen) not in self.clones:                  # "rebind": the same key on cloned device buffers
            self.clones[(f, gen)] = tuple(t.clone() for t in g.base[f])
        return self.clones[(f, gen)]

    def fail(self, i, msg):
        path = self.tmp_path / f"{self.walk['name']}_prefix_{i}.json"
        path.write_text(json.dumps(dict(self.walk, steps=self.walk["steps"][:i + 1]), sort_keys=True))
        pytest.fail(f"walk {self.walk['name']}, step {i} ({self.walk['steps'][i]['kind']}): {msg}\nprefix: {path}", pytrace=False)

    def optimize(self, c, ws, keyed):
        g = self.g
        opt = g.O.OptimizerGpu(workspace=ws, keyed_correspondences=c.keyed_corr and keyed, pair_policy=c.policy, image_downscale=c.downscale)
        bufs = [self.buffers(f) for f in c.frames]
        poses = c.poses.copy()
        opt.optimizeFrames(c.corr, c.nm, c.n_frames, c.H, c.W, [b[0] for b in bufs], None, [b[1] for b in bufs], poses, c.K, dense_pairs=c.pairs,
                           frame_keys=c.keys if keyed else None)
        return poses, opt.last_stats

    def keyed_call(self, i, step, c, b):
        try:
            ref, st_ref = self.optimize(c, None, False)
            got, st = self.optimize(c, self.ws, True)
        except Exception as e:                                  # a status (BTBA_ENUMERIC, ...) is a finding like any other
            self.fail(i, f"{type(e).__name__}: {e}")
        N = c.n_frames
        if not (np.isfinite(got).all() and np.isfinite(ref).all()):
            self.fail(i, "poses are not finite")
        if got.tobytes() != ref.tobytes():
            worst = max(max(S.pose_error(got[k], ref[k])) for k in range(N))
            self.fail(i, f"keyed poses differ from the stateless call's (worst pose distance {worst:.3e}); window {c.frames}, policy {c.policy}")
        if np.array_equal(ref, c.poses):
            self.fail(i, "the solve left the poses where they were: the comparison would be vacuous")
        if st["n_frames"] != N or st_ref["n_frames"] != N:
            self.fail(i, f"n_frames {st['n_frames']}, window has {N}")
        if st_ref["cache_frames_built"] != N or st_ref["corr_pairs_uploaded"] != c.n_pairs:
            self.fail(i, f"stateless call reports {st_ref['cache_frames_built']} frames built, {st_ref['corr_pairs_uploaded']} pairs uploaded")
        built = st["cache_frames_built"]
        if not b["L"] <= built <= b["U"]:
            self.fail(i, f"cache_frames_built {built} outside [{b['L']}, {b['U']}] ({b['slots']} slots)")
        msg = self.tr.corr_observe(c, st["corr_pairs_uploaded"])
        if msg:
            self.fail(i, msg)
        s = self.stats
        s["calls"] += 1; s["U_gt_L"] += b["U"] > b["L"]; s["built_gt_L"] += built > b["L"]
        if step.get("anchor") and self.oracle is not None:
            O = self.oracle
            caches = [O.build_cache(*KW.frame(*f), c.K, c.downscale) for f in c.frames]
            sol = O.solve(np.stack([x["campos"] for x in caches]), np.stack([x["normals"] for x in caches]), caches[0]["intr"], c.corr, c.poses)
            worst = max(max(S.pose_error(ref[k], sol.poses[k])) for k in range(N))
            s["anchors"][step["anchor"]] = worst
            print(f"anchor '{step['anchor']}' ({N} frames, {c.pool}): stateless call vs oracle, worst pose distance {worst:.2e}")
            bar = BAR_MANY_FRAMES if N >= 17 else BAR_FEW_FRAMES
            if not worst < bar:
                self.fail(i, f"stateless call is {worst:.3e} from the oracle (bar {bar:g})")

    def foreign_call(self, i, c, what):
        """Another entry point on the walk's workspace: its own result must be that of a fresh workspace."""
        g, N = self.g, c.n_frames
        outs = []
        try:
            if what == "optimize":
                outs = [self.optimize(c, ws, False)[0].tobytes() for ws in (self.ws, None)]
            else:
                bufs = [self.buffers(f) for f in c.frames]
                zn, _, _ = g.O.build_cache_zn(g.aux_ws, [b[0] for b in bufs], [b[1] for b in bufs], c.H, c.W, c.K, c.downscale)
                g.aux_ws.sync()
                for ws in (self.ws, g.O.Workspace()):
                    bs = g.O.BatchSolver(ws, image_downscale=c.downscale)
                    corr, offs, mx = bs.pack_correspondences([c.corr], N)
                    corr_d = g.torch.from_numpy(corr.view(np.uint8).reshape(1, -1, 32)).to(g.dev)
                    offs_d = g.torch.from_numpy(offs.astype(np.int32)).to(g.dev)
                    poses_d = g.torch.from_numpy(c.poses[None].copy()).to(g.dev)
                    if what == "solve_zn":
                        bs.solve_zn(zn[None], c.H, c.W, c.K, corr_d, offs_d, mx, poses_d, dense_pairs=c.pairs)
                        ws.sync()
                        outs.append(poses_d.cpu().numpy().tobytes())
                        if not np.isfinite(poses_d.cpu().numpy()).all():
                            self.fail(i, "foreign solve: poses are not finite")
                    else:
                        res = bs.objective_zn(zn[None], c.H, c.W, c.K, corr_d, offs_d, mx, poses_d, dense_pairs=c.pairs)
                        outs.append(b"".join(np.ascontiguousarray(a[name]).tobytes() for a in res for name in a.dtype.names if name != "reserved"))
        except Exception as e:
            self.fail(i, f"{type(e).__name__}: {e}")
        if outs[0] != outs[1]:
            self.fail(i, f"foreign {what} call on the walk's workspace differs from the same call on a fresh one")
        self.stats["foreign"] += 1

    def run(self):
        from bundletrack_amd.optimizer import frame_cache_clear, frame_cache_evict
        for i, step in enumerate(self.walk["steps"]):
            act = self.tr.step(step)
            if act[0] == "call":
                self.keyed_call(i, step, act[1], act[2])
            elif act[0] == "foreign":
                self.foreign_call(i, act[1], act[2])
            elif act[0] == "evict":
                frame_cache_evict(self.ws, act[1])
            elif act[0] == "clear":
                frame_cache_clear(self.ws)
            elif act[0] == "threshold":
                self.ws.set_option(_lib.OPT_KEYED_CORR_MIN_BYTES, act[1])
        s = dict(self.stats, resets=self.tr.corr.resets)
        print(f"walk {self.walk['name']}: {json.dumps(s)}")
        self.g.report[self.walk["name"]] = s
        self.ws.close()
        return s


def run_walk(gpu, name, tmp_path, oracle=None):
    walk = KW.get_walk(name)
    assert KW.missing_coverage(name, KW.coverage(walk)) == []          # (also a CPU test: a GPU run must not pass vacuously)
    s = Runner(gpu, walk, tmp_path, oracle).run()
    assert s["calls"] == sum(st["kind"] == "call" for st in walk["steps"])
    assert s["foreign"] == sum(st["kind"] == "foreign" for st in walk["steps"])
    return s


def test_frame_pool_walk(gpu, oracle, tmp_path):
    """Sliding windows, loop closures, pressure on a full pool, regrowth at 17 and 18 frames.  Default pair policy, no keyed
    correspondences.  Oracle anchors: windows of 2, 9 and 17 frames."""
    s = run_walk(gpu, "frame_pool", tmp_path, oracle)
    assert set(s["anchors"]) == {"size 2", "size 9", "size 17"}
    assert s["U_gt_L"] >= 10


def test_geometry_walk(gpu, oracle, tmp_path):
    """G1 -> G2 -> G1 -> G2 -> G1 (caches with and without per-block ranges in one workspace), image_downscale 4 -> 2 -> 4, the same
    key on cloned buffers, evicted keys handed to other frames, clear.  Oracle anchors: one call per geometry."""
    s = run_walk(gpu, "geometry", tmp_path, oracle)
    assert set(s["anchors"]) == {"geometry G1", "geometry G2"}


def test_pair_policy_walk(gpu, oracle, tmp_path):
    """Every pair policy on windows that mix full and object-only frames, on both sides of the 60 % rule: BTBA_PAIRS_TARGET_MORE_VALID
    and the compaction choice read the pool's stored valid counts.  Oracle anchor: one mixed-variant window."""
    s = run_walk(gpu, "policies", tmp_path, oracle)
    assert set(s["anchors"]) == {"mixed variants"}


def test_correspondence_pool_walk(gpu, tmp_path):
    """BTBA_FLAG_KEYED_CORR: segments that lose an entry, the same two frames in the opposite order, calls under
    BTBA_OPT_KEYED_CORR_MIN_BYTES between cached ones (the pool is bypassed and stays as it was), a shuffled array in the middle of a
    populated pool, segments with invalid entries, an evicted key whose segments must not serve the frame that inherits it."""
    run_walk(gpu, "corr_pool", tmp_path)


def test_correspondence_pool_overflow_walk(gpu, tmp_path):
    """All-new windows until the appended entries exceed twice what the pool can hold: the library resets the pool in mid-session,
    nobody tells the model when, and the counts of the windows presented again afterwards prove that it did."""
    s = run_walk(gpu, "overflow", tmp_path)
    assert s["resets"] >= 1


def test_foreign_calls_walk(gpu, tmp_path):
    """A stateless optimise of another window size, a solve with an explicit pair list and an objective call on the same workspace
    between keyed calls: each gives what it gives on a fresh workspace, and the next keyed call is byte-equal to the stateless one
    although its pair table, work formula, solve tables and pinned blocks were rewritten in between."""
    s = run_walk(gpu, "foreign", tmp_path)
    assert s["foreign"] >= 18


@pytest.mark.parametrize("name", ["combined", "combined_b"])
def test_combined_walk(gpu, tmp_path, name):
    """Everything above on one workspace under seeds of its own: every call draws its pair policy and goes through the correspondence pool."""
    s = run_walk(gpu, name, tmp_path)
    assert s["U_gt_L"] >= 10


def test_pool_holds_twice_the_window(gpu, tmp_path):
    """include/btba.h: pool = max(32, 2 n_frames) slots.  After a small window has created the pool with 32 slots, two disjoint windows
    of 17 frames must still fit (34 slots): the first of them is cached when it comes back.  (The pool used to grow only once a window
    exceeded its slot count, so it stayed at 32 and the second window of 17 recycled two frames of the first.  Found by the upper bound
    of the frame-pool walk; this is its shortest form.)"""
    frames = [[p, KW.MASKED] for p in range(38)]
    steps = [dict(kind="call", pool="G1", window=w, policy=KW.LOWER, pairs=None, downscale=4.0, keyed_corr=False, mutation=None, pose_seed=k)
             for k, w in enumerate((frames[34:], frames[:17], frames[17:34], frames[:17]))]
    r = Runner(gpu, dict(name="two_windows_of_17", seed=1, long=False, steps=steps), tmp_path)
    for i, step in enumerate(steps):
        act = r.tr.step(step)
        assert (act[2]["L"], act[2]["U"]) == [(4, 4), (17, 17), (17, 17), (0, 0)][i]          # the bounds leave no room
        r.keyed_call(i, step, act[1], act[2])
    assert r.stats["calls"] == 4
