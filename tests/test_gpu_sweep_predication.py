"""The sweeps' handling of REJECTED pixels and INVALID correspondences: a rejected lane runs no accumulate (dense: the tail of a pixel sits under the
exec mask of its accept test; sparse: a wave whose entries are all valid skips the masking selects) and the counts are popcounts of the accept / valid
masks.  Every sum must be what summing exact zeros for those lanes gives, so the records are held to the fp64 references of tests/sweep_ref.py at the
bars of tests/test_gpu_sweep_sums.py (its fixtures and helpers, imported), and the counts are exact.

Dense: two frames with a 16 x 8 cache -- two 8 x 8 blocks, one wave each in the block walk; lane = 8 * row + column inside a block -- one instance,
one pair (target 0, source 1).  Both frames see one smooth surface from nearly the same pose, so a source pixel lands within a pixel of the
target pixel of the same index and is accepted unless the scene says otherwise:
  accept       nothing else: every pixel accepted
  reject       every source normal turned by 90 degrees: both blocks are live (their pixels project into the image, their taps are gathered) and the
               normal test rejects every pixel -- the record is all zeros, the count exactly 0
  lane0/lane63 the same with ONE true normal left, at lane 0 of block 0 resp. lane 63 of block 1
  edge         the source camera moved 5.3 cache pixels sideways: block 1 straddles the target's right edge, whole 2 x 2 quads of it are out of the image
  hole         a 5 x 5 hole in the target's depth; `poisoned`: the same frames with NaN and inf normals in the hole's inner 3 x 3 texels, which only
               lanes whose four taps all lie in the hole -- blended depth 0, rejected whatever the normals are -- can reach
each through the block walk, the row-strip walk, the valid-pixel lists and the fused launch (they share the per-pixel code).
Sparse: two frames, one pair, segments of 0, 1, 255, 256, 257, 511 and 513 entries as seven instances of one launch; all valid / invalid entries (first
word 0xFFFFFFFF, NaN payload) at the first, the last and a middle position / one invalid entry inside a wave of valid ones; EntryJ and 24-byte layout."""
import numpy as np
import pytest

import sweep_ref as R
import test_gpu_sweep_sums as SS
from test_gpu_sweep_sums import gamma_d, gpu, sparse_cases  # noqa: F401  (module-scoped fixtures: the GPU handle and the bars)
from bundletrack_amd import _lib

pytestmark = pytest.mark.gpu

HD, WD, H, W = 8, 16, 32, 64
PAIR = ((0, 1),)
Z0 = 0.8
_scenes = {}


def dense_scene(name):
    """The dict tests/sweep_ref.scene() returns, for the two-frame scene `name` (see the module docstring)."""
    if name in _scenes:
        return _scenes[name]
    from bundletrack_amd import synthetic as S
    from oracle import oracle as O
    K = S.NOCS_K.astype(np.float64).copy()
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0                                  # the focal length stays: a cache pixel is 5 mm wide at 0.8 m, so the fraction of a pixel by
                                                                         # which the cache's rounded sampling positions misregister a tiny frame stays far inside the distance gate
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xn, yn = xs / W - 0.5, ys / H - 0.5
    z = Z0 + 0.012 * xn - 0.008 * yn + 0.02 * (xn * xn + yn * yn)        # nearly flat: 5 pixels sideways stay inside the 2 cm distance gate
    X, Y = (xs - K[0, 2]) / K[0, 0] * z, (ys - K[1, 2]) / K[1, 1] * z
    P = np.stack([X, Y, z], -1)
    n = np.cross(np.gradient(P, axis=0), np.gradient(P, axis=1))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n *= -np.sign(n[..., 2:3])
    depth = np.repeat(z[None], 2, 0).astype(np.float32)
    normals = np.zeros((2, H, W, 4), np.float32)
    normals[..., :3] = n
    xi, yi = S.cache_source_pixels(H, W, HD, WD)
    sel = np.ix_(yi, xi)                                                 # the full-resolution pixels the cache samples
    if name in ("reject", "lane0", "lane63"):
        turned = np.cross(n[sel], np.array([1.0, 0.0, 0.0]))             # perpendicular to the true normal: the cosine against the target's is ~0
        turned /= np.linalg.norm(turned, axis=-1, keepdims=True)
        if name == "lane0":
            turned[0, 0] = n[sel][0, 0]                                  # block 0, row 0, column 0
        if name == "lane63":
            turned[7, 15] = n[sel][7, 15]                                # block 1, row 7, column 7
        src = normals[1, :, :, :3]
        src[sel] = turned
    if name in ("hole", "poisoned"):
        hole = np.zeros((HD, WD), bool)
        hole[2:7, 10:15] = True
        full = np.zeros((H, W), bool)
        full[sel] = hole
        depth[0][full] = 0.0
        normals[0][full] = 0.0
    fxc = K[0, 0] * WD / W
    sx, sy, tz = (5.3, 0.03, 0.0005) if name == "edge" else (0.05, 0.03, 0.001)       # (cache pixels, cache pixels, metres)
    T0 = S.orbit_pose(0.3)
    poses = np.stack([T0, T0 @ S.se3_exp(np.zeros(3), np.array([sx * Z0 / fxc, sy * Z0 / fxc, tz]))]).astype(np.float32)
    rng = np.random.default_rng(11)
    corr = np.zeros(40, R.ENTRYJ)
    pm = rng.uniform(-0.1, 0.1, (40, 3))
    inv = np.linalg.inv(poses.astype(np.float64))
    corr["imgIdx_i"], corr["imgIdx_j"] = 0, 1
    corr["pos_i"] = pm @ inv[0, :3, :3].T + inv[0, :3, 3]
    corr["pos_j"] = pm @ inv[1, :3, :3].T + inv[1, :3, 3] + rng.normal(scale=0.001, size=(40, 3))
    caches = [O.build_cache(depth[k], normals[k], K.astype(np.float32), 4.0) for k in range(2)]
    sc = dict(name=name, K=K.astype(np.float32), H=H, W=W, campos=np.stack([c["campos"] for c in caches]), normals=np.stack([c["normals"] for c in caches]),
              intr=caches[0]["intr"], poses=poses, corr=corr)
    assert sc["campos"].shape == (2, HD, WD, 4)
    _scenes[name] = sc
    return sc


def poison(g):
    """NaN and inf normals in the inner 3 x 3 texels of the target's hole (compact cache [B, frame, y, x, (z, nx, ny, nz)])."""
    def apply(zn):
        g.ws.sync()
        assert float(zn[0, 0, 2:7, 10:15, 0].abs().max()) == 0.0         # the hole: gated depth 0
        bad = g.torch.tensor([float("nan"), float("inf"), -float("inf")], device=g.dev)
        for k, (y, x) in enumerate((y, x) for y in range(3, 6) for x in range(11, 14)):
            zn[0, 0, y, x, 1:4] = bad.roll(k)
        g.torch.cuda.synchronize()
    return apply


WALKS = {"blocks": dict(), "strips": dict(opts=((_lib.OPT_BLOCK_WALK, 0),)), "lists": dict(flags=_lib.FLAG_COMPACTION),
         "fused": dict(tiles=64, chunks=64, want_fused=True)}


def run_dense(g, sc, flags=0, tiles=0, chunks=0, opts=(), want_fused=None, edit=None):
    """One traced first linearisation of the scene; returns its 28-float record (test_gpu_sweep_sums.run_dense for two frames)."""
    bs = g.BatchSolver(g.ws, n_gn_iters=1, dense_tiles=tiles, sparse_chunks=chunks, flags=flags)
    cam_d = g.torch.from_numpy(sc["campos"][None]).to(g.dev)
    nrm_d = g.torch.from_numpy(sc["normals"][None]).to(g.dev)
    corr_d, offs_d, mx = SS.corr_inputs(g, [sc["corr"]], [np.array([0, len(sc["corr"])], np.uint32)])
    poses_d = g.torch.from_numpy(sc["poses"][None]).to(g.dev)
    try:
        for o, v in opts:
            g.ws.set_option(o, v)
        zn = g.pack_zn(g.ws, cam_d, nrm_d)
        if edit is not None:
            edit(zn)
        tr = bs.solve_zn(zn, sc["H"], sc["W"], sc["K"], corr_d, offs_d, mx, poses_d, trace=True)
        tv = bs.trace_view(tr)
        st = g.ws.collect_stats()
    finally:
        for o, _ in opts:
            g.ws.set_option(o, SS.DEFAULT_OPTS[o])
    if want_fused is not None:
        assert st["fused_sweeps"] == int(want_fused), st
    assert tv.dense_pair.shape[2] == 1
    return tv.dense_pair[0, 0, 0]


def dense_ref(g, name):
    key = ("predication", name)
    if key not in g.refs:
        sc = dense_scene(name)
        T, Tinv = SS.device_matrices(g, sc["poses"])
        g.refs[key] = R.scene_refs(sc, T, Tinv, PAIR)[0]
    return g.refs[key]


def check_record(rec, ref, gamma, what):
    cnt = float(rec[27])
    print(f"{what}: count {cnt} (reference {ref['count']} + {ref['borderline']} borderline)", end="")
    assert cnt == int(cnt) and ref["count"] <= int(cnt) <= ref["count"] + ref["borderline"], what
    assert np.all(np.isfinite(rec)), what
    e = R.dense_normalised_error(rec, ref)
    print(f", normalised error S {e[0]:.3e} g {e[1]:.3e} (bars {gamma[0]:.3e} / {gamma[1]:.3e})")
    assert e[0] <= gamma[0] and e[1] <= gamma[1], what


# what the reference itself must say about each scene (accepted pixels, borderline pixels): the cases are what the docstring claims
EXPECT = {"accept": (HD * WD, 0), "reject": (0, 0), "lane0": (1, 0), "lane63": (1, 0)}


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("name", ["accept", "reject", "lane0", "lane63", "edge", "hole"])
def test_dense_rejected_pixels_add_nothing(gpu, gamma_d, name, walk):
    sc, ref = dense_scene(name), dense_ref(gpu, name)
    if name in EXPECT:
        assert (ref["count"], ref["borderline"]) == EXPECT[name], (ref["count"], ref["borderline"])
    if name in ("lane0", "lane63"):
        assert int(np.flatnonzero(ref["accept_mask"])[0]) == (0 if name == "lane0" else 7 * WD + 15)
    if name == "edge":
        # block 1 straddles the right edge: its last quad column projects out of the image, its first one into it, and pixels are accepted
        T, Tinv = SS.device_matrices(gpu, sc["poses"])
        cs = sc["campos"][1].reshape(-1, 4)[:, :3].astype(np.float64)
        q = cs @ (Tinv[0] @ T[1])[:3, :3].T + (Tinv[0] @ T[1])[:3, 3]
        u = (q[:, 0] * sc["intr"][0] / q[:, 2] + sc["intr"][2]).reshape(HD, WD)
        assert np.all(u[:, 14:] > WD - 0.5 + R.EPS) and np.all(u[:, 8:10] < WD - 0.5 - R.EPS) and ref["count"] >= HD * 8
    rec = run_dense(gpu, sc, **WALKS[walk])
    check_record(rec, ref, gamma_d, f"{name} {walk}")
    if name == "reject":
        assert np.all(rec == 0.0), rec


@pytest.mark.parametrize("walk", list(WALKS))
def test_dense_poisoned_target_normals_are_never_read(gpu, gamma_d, walk):
    """Texels only rejected lanes reach carry NaN / inf normals: the record is finite and has the unpoisoned run's bits."""
    sc = dense_scene("poisoned")
    clean = run_dense(gpu, sc, **WALKS[walk])
    dirty = run_dense(gpu, sc, edit=poison(gpu), **WALKS[walk])
    assert np.all(np.isfinite(dirty)), dirty
    assert np.array_equal(clean.view(np.uint32), dirty.view(np.uint32)), (clean, dirty)
    check_record(dirty, dense_ref(gpu, "poisoned"), gamma_d, f"poisoned {walk}")


# ---- sparse ------------------------------------------------------------------------------------------------------------
LENS = (0, 1, 255, 256, 257, 511, 513)
_sparse = {}


def sparse_inputs(variant):
    """(list of one EntryJ segment per length in LENS, poses [2, 4, 4]): tests/sweep_ref.sparse_case's recipe for two frames."""
    if variant in _sparse:
        return _sparse[variant]
    from bundletrack_amd import synthetic as S
    pb = S.make_problem(2, 8, seed=72, background=False, full_res=False)
    rng = np.random.default_rng(7002)
    inv = np.linalg.inv(pb.poses_gt)
    blocks = []
    for m in LENS:
        blk = np.zeros(m, R.ENTRYJ)
        pts, _ = S._sample_surface(rng, m)
        pi = pts @ inv[0, :3, :3].T + inv[0, :3, 3] + rng.normal(scale=0.001, size=(m, 3))
        pj = pts @ inv[1, :3, :3].T + inv[1, :3, 3] + rng.normal(scale=0.001, size=(m, 3))
        out = rng.random(m) < 0.05
        d = rng.normal(size=(m, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pj[out] += (d * rng.uniform(0.02, 0.05, (m, 1)))[out]
        blk["imgIdx_i"], blk["imgIdx_j"], blk["pos_i"], blk["pos_j"] = 0, 1, pi, pj
        bad = []
        if variant == "first_last_middle" and m:
            bad = sorted({0, m // 2, m - 1})
        if variant == "one_in_wave" and m > 70:
            bad = [70]                                   # wave 1 of the first trip: 63 valid neighbours, valid waves all around
        blk["imgIdx_i"][bad] = 0xFFFFFFFF
        blk["pos_i"][bad] = np.nan
        blk["pos_j"][bad] = np.nan
        blocks.append(blk)
    _sparse[variant] = (blocks, np.ascontiguousarray(pb.poses_init, np.float32))
    return _sparse[variant]


def run_sparse(g, blocks, poses, chunks, form):
    """One traced first linearisation of the feature term, one instance per segment; returns (rhs, precond, A) [B, ...]."""
    B = len(blocks)
    bs = g.BatchSolver(g.ws, n_gn_iters=1, weight_dense_depth=0.0, sparse_chunks=chunks)
    corr_d, offs_d, mx = SS.corr_inputs(g, blocks, [np.array([0, len(b)], np.uint32) for b in blocks])
    poses_d = g.torch.from_numpy(np.repeat(poses[None], B, 0)).to(g.dev)
    zn = g.torch.zeros((B, 2, 8, 8, 4), device=g.dev)
    K = np.array([[30, 0, 16], [0, 30, 16], [0, 0, 1]], np.float32)
    if form == "c24":
        c24, flag = bs.pack_correspondences24(corr_d, offs_d, mx, 2, check_order=True)
        tr = bs.solve_zn(zn, 32, 32, K, None, offs_d, mx, poses_d, trace=True, aux={"corr24": c24}, corr_stride=corr_d.shape[1])
    else:
        tr = bs.solve_zn(zn, 32, 32, K, corr_d, offs_d, mx, poses_d, trace=True)
    tv = bs.trace_view(tr)
    st = g.ws.collect_stats()
    if form == "c24":
        assert int(flag.cpu()[0]) == 0
    assert st["fused_sweeps"] == 0 and st["sparse_chunks"] == chunks, st
    return tv.rhs[:, 0].copy(), tv.precond[:, 0].copy(), tv.A[:, 0].copy()


@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("variant", ["all_valid", "first_last_middle", "one_in_wave"])
def test_sparse_invalid_entries_add_nothing(gpu, sparse_cases, variant, chunks):
    _, bars = sparse_cases
    blocks, poses = sparse_inputs(variant)
    key = ("predication sparse", variant)
    if key not in gpu.refs:
        T, _ = SS.device_matrices(gpu, poses)
        gpu.refs[key] = [R.sparse_system(b, T) for b in blocks]
    out = {form: run_sparse(gpu, blocks, poses, chunks, form) for form in ("entryj", "c24")}
    for form, (rhs, precond, A) in out.items():
        for b, (blk, sp) in enumerate(zip(blocks, gpu.refs[key])):
            n_valid = int((blk["imgIdx_i"] != 0xFFFFFFFF).sum())
            # the count is the translation diagonal of frame 1's block of A ([trans, rot] layout, weight 1): exact
            assert np.all(np.diag(A[b])[6:9] == float(n_valid)), (form, LENS[b], np.diag(A[b])[6:9], n_valid)
            assert np.all(np.isfinite(A[b])) and np.all(np.isfinite(rhs[b])) and np.all(np.isfinite(precond[b]))
            e = np.array(R.sparse_normalised(rhs[b], precond[b], A[b], sp))
            print(f"sparse {variant} chunks {chunks} {form} len {LENS[b]}: valid {n_valid}, normalised error rhs {e[0]:.3e} precond {e[1]:.3e} A {e[2]:.3e}   (bars {bars})")
            assert np.all(e <= bars), (form, LENS[b], e, bars)
    for a, c in zip(out["entryj"], out["c24"]):
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), "the two layouts differ"
