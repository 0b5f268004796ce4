"""The dense and sparse sweeps' SUMS of the first linearisation against the threshold-aware fp64 references of tests/sweep_ref.py,
pair by pair and variant by variant (every variant against the reference, never against another variant).

Dense: per traced 28-float record   accepts <= count <= accepts + borderline   (integers) and, for the 27 sums,
|gpu - ref| <= Bud + gamma * Sc with gamma = 4 x the floor of the project's fp32 CPU oracle against the same reference in the same
units, measured at run time over the same scenes in both accumulation modes -- separately for the 21 entries of S and the 6 of g
(each floor is at most the joint one, so neither bar is wider than 4 x the joint floor).  The reference is evaluated at the matrices
the device forms (Exp(Log(pose)) and its inverse through the library's own SE(3) seams), the oracle's floor at the oracle's own.
Sparse: traced A, rhs, precond against the fp64 system, each within 4 x the oracle's own floor for that quantity, in a launch of
its own and inside the fused launch (dense term on over frames without a valid pixel: exact zeros).

Measured on an MI355X (the numbers are printed by every run; DESIGN.md "Testing the sweeps' sums" records them)."""
import numpy as np
import pytest

import sweep_ref as R
from bundletrack_amd import _lib
from shared_checks import device_matrices

pytestmark = pytest.mark.gpu
FACTOR = 4.0


@pytest.fixture(scope="module")
def gpu(oracle):
    import torch
    assert torch.cuda.is_available()
    from bundletrack_amd.optimizer import BatchSolver, Workspace, pack_zn

    class G:
        pass
    g = G()
    g.torch, g.dev, g.ws = torch, torch.device("cuda:0"), Workspace()        # a workspace of its own: no option leaks into other modules
    g.BatchSolver, g.pack_zn = BatchSolver, pack_zn
    g.refs = {}
    return g


@pytest.fixture(scope="module")
def gamma_d(oracle):
    fS, fg, per = R.oracle_dense_floor()
    print(f"\ndense: fp32 oracle floor S {fS:.3e} g {fg:.3e} -> bars {FACTOR * fS:.3e} / {FACTOR * fg:.3e}; per scene {per}")
    return FACTOR * fS, FACTOR * fg


def refs_of(g, name, pairs):
    key = (name, pairs)
    if key not in g.refs:
        sc = R.scene(name)
        T, Tinv = device_matrices(g, sc["poses"])
        g.refs[key] = R.scene_refs(sc, T, Tinv, pairs)
    return g.refs[key]


def corr_inputs(g, corr_list, offs_list):
    stride = max(1, max(len(c) for c in corr_list))
    corr = np.zeros((len(corr_list), stride), R.ENTRYJ)
    corr["imgIdx_i"] = corr["imgIdx_j"] = 0xFFFFFFFF
    for b, c in enumerate(corr_list):
        corr[b, :len(c)] = c
    offs = np.stack(offs_list).astype(np.int32)
    mx = int(max(np.diff(o.astype(np.int64)).max() for o in offs_list))
    return g.torch.from_numpy(corr.view(np.uint8).reshape(len(corr_list), stride, 32)).to(g.dev), g.torch.from_numpy(offs).to(g.dev), mx


def run_dense(g, names, api="zn", flags=0, tiles=0, chunks=0, opts=(), pairs=None, want_fused=None):
    """One traced solve (n_gn_iters = 1, both terms on) of the batch of scenes `names` (same shape); returns records [B, Pd, 28]."""
    scs = [R.scene(n) for n in names]
    sc0 = scs[0]
    bs = g.BatchSolver(g.ws, n_gn_iters=1, dense_tiles=tiles, sparse_chunks=chunks, flags=flags)
    cam_d = g.torch.from_numpy(np.stack([s["campos"] for s in scs])).to(g.dev)
    nrm_d = g.torch.from_numpy(np.stack([s["normals"] for s in scs])).to(g.dev)
    offs = np.arange(4, dtype=np.uint32) * 40
    corr_d, offs_d, mx = corr_inputs(g, [s["corr"] for s in scs], [offs] * len(scs))
    poses_d = g.torch.from_numpy(np.stack([s["poses"] for s in scs])).to(g.dev)
    dp = None if pairs is None else np.asarray(pairs, np.int32)
    if dp is not None:
        bs.params.pair_policy = _lib.PAIRS_EXPLICIT
    try:
        for o, v in opts:
            g.ws.set_option(o, v)
        if api == "f4":
            tr = bs.solve(cam_d, nrm_d, sc0["intr"], corr_d, offs_d, mx, poses_d, dense_pairs=dp, trace=True)
        else:
            zn = g.pack_zn(g.ws, cam_d, nrm_d)
            tr = bs.solve_zn(zn, sc0["H"], sc0["W"], sc0["K"], corr_d, offs_d, mx, poses_d, dense_pairs=dp, trace=True)
        tv = bs.trace_view(tr)
        st = g.ws.collect_stats()
    finally:
        for o, _ in opts:
            g.ws.set_option(o, DEFAULT_OPTS[o])
    if want_fused is not None:
        assert st["fused_sweeps"] == int(want_fused), st
    return tv.dense_pair[:, 0], st


DEFAULT_OPTS = {_lib.OPT_TILE_MAJOR: 1, _lib.OPT_DENSE_ORDER: 1, _lib.OPT_BLOCK_WALK: 1, _lib.OPT_BLOCK_SKIP: 1, _lib.OPT_RELAYOUT: 0, _lib.OPT_SPARSE_TAIL: -1}


def check_records(g, name, recs, pairs, gamma, what):
    """recs [Pd, 28] of one instance against the reference of scene `name`."""
    gS, gg = gamma
    worst = np.zeros(2)
    for (i, j), rec, ref in zip(pairs, recs, refs_of(g, name, tuple(pairs))):
        cnt = float(rec[27])
        assert cnt == int(cnt) and ref["count"] <= int(cnt) <= ref["count"] + ref["borderline"], \
            f"{what} {name} pair ({i}, {j}): count {cnt}, reference accepts {ref['count']} + {ref['borderline']} borderline"
        e = np.array(R.dense_normalised_error(rec, ref))
        worst = np.maximum(worst, e)
        assert e[0] <= gS and e[1] <= gg, f"{what} {name} pair ({i}, {j}): normalised error S {e[0]:.3e} (bar {gS:.3e}) g {e[1]:.3e} (bar {gg:.3e})"
    print(f"{what:46s} {name:11s} HIP normalised error S {worst[0]:.3e} g {worst[1]:.3e}   (bars {gS:.3e} / {gg:.3e})")
    return worst


C, NC, NF = _lib.FLAG_COMPACTION, _lib.FLAG_NO_COMPACTION, _lib.FLAG_NO_FUSE
VARIANTS = [
    # (id, scene, run_dense keywords)
    ("f4_default", "bg32x24", dict(api="f4")),
    ("f4_13x9", "smooth13x9", dict(api="f4")),
    ("f4_50x30", "bg50x30", dict(api="f4")),
    ("f4_275x8", "bg275x8", dict(api="f4")),
    ("f4_hole", "hole32x24", dict(api="f4")),
    ("f4_edge", "edge32x24", dict(api="f4")),
    ("f4_fullsize", "bg160x120", dict(api="f4")),
    ("zn_pinhole", "bg32x24", dict()),
    ("zn_13x9", "smooth13x9", dict()),
    ("zn_50x30", "bg50x30", dict()),
    ("zn_275x8", "bg275x8", dict()),
    ("zn_hole", "hole32x24", dict()),
    ("zn_fullsize", "bg160x120", dict()),
    ("zn_skewed_K", "skew32x24", dict()),
    ("zn_skewed_K_lists", "skew32x24", dict(flags=C)),
    ("lists_masked", "mask80x60", dict(flags=C)),
    ("no_lists_masked", "mask80x60", dict(flags=NC)),
    ("lists_full", "bg32x24", dict(flags=C)),
    ("no_lists_full", "bg32x24", dict(flags=NC)),
    ("lists_hole", "hole32x24", dict(flags=C)),
    ("lists_zero_and_one_valid", "edge32x24", dict(flags=C)),
    ("no_lists_zero_and_one_valid", "edge32x24", dict(flags=NC)),
    ("lists_zero_and_one_valid_75_tiles", "edge32x24", dict(flags=C, tiles=75)),
] + [(f"zn_tiles{t}", "bg32x24", dict(tiles=t)) for t in (1, 3, 7, 75)] \
  + [(f"lists_tiles{t}", "bg32x24", dict(tiles=t, flags=C)) for t in (1, 3, 7, 75)] \
  + [(f"lists_masked_tiles{t}", "mask80x60", dict(tiles=t, flags=C)) for t in (7, 75)] \
  + [(f"f4_tiles{t}", "bg50x30", dict(api="f4", tiles=t)) for t in (1, 3, 7, 75)] \
  + [("zn_fused", "bg32x24", dict(tiles=22, chunks=22, want_fused=True)), ("zn_no_fuse", "bg32x24", dict(tiles=22, chunks=22, flags=NF, want_fused=False)),
     ("lists_fused", "mask80x60", dict(tiles=22, chunks=22, flags=C, want_fused=True)), ("f4_fused", "bg50x30", dict(api="f4", tiles=22, chunks=22, want_fused=True)),
     ("f4_no_fuse", "bg50x30", dict(api="f4", tiles=22, chunks=22, flags=NF, want_fused=False))] \
  + [(f"opt{o}_{v}_{sc}", sc, dict(opts=((o, v),), tiles=t, chunks=22))
     for o in (_lib.OPT_TILE_MAJOR, _lib.OPT_DENSE_ORDER, _lib.OPT_BLOCK_WALK, _lib.OPT_BLOCK_SKIP, _lib.OPT_RELAYOUT) for v in (0, 1) for sc, t in (("bg32x24", 22), ("bg160x120", 0))]


@pytest.mark.parametrize("vid,name,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_dense_sums_against_fp64(gpu, gamma_d, vid, name, kw):
    recs, st = run_dense(gpu, [name], **kw)
    check_records(gpu, name, recs[0], R.PAIRS_FWD, gamma_d, vid)


@pytest.mark.parametrize("api,name,flags", [("f4", "bg32x24", 0), ("zn", "bg32x24", 0), ("zn", "bg32x24", C), ("zn", "skew32x24", 0), ("zn", "mask80x60", C), ("zn", "hole32x24", 0),
                                            ("zn", "bg50x30", 0), ("zn", "bg160x120", 0)])
def test_dense_sums_reversed_pairs(gpu, gamma_d, api, name, flags):
    """PAIRS_EXPLICIT with target > source: the FLIPPED epilogue; and a mixed list."""
    recs, _ = run_dense(gpu, [name], api=api, flags=flags, pairs=R.PAIRS_REV)
    check_records(gpu, name, recs[0], R.PAIRS_REV, gamma_d, f"reversed {api} flags {flags}")
    mixed = (R.PAIRS_REV[0], R.PAIRS_FWD[1], R.PAIRS_REV[2])
    recs, _ = run_dense(gpu, [name], api=api, flags=flags, pairs=mixed)
    check_records(gpu, name, recs[0], mixed, gamma_d, f"mixed {api} flags {flags}")


@pytest.mark.parametrize("api,flags", [("f4", 0), ("zn", 0), ("zn", C)])
def test_dense_sums_batch_of_two_instances(gpu, gamma_d, api, flags):
    """Two different instances in one launch: instance 1's records meet instance 1's reference."""
    names = ["bg32x24", "hole32x24"]
    recs, _ = run_dense(gpu, names, api=api, flags=flags)
    for b, name in enumerate(names):
        check_records(gpu, name, recs[b], R.PAIRS_FWD, gamma_d, f"batch instance {b} {api} flags {flags}")


# ---- sparse ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse_cases(oracle):
    """Per window size the inputs and, as ONE bar per quantity, 4 x the oracle's worst floor over the window sizes: (rhs, precond, A)."""
    out = {}
    for N in (2, 3, 5):
        corr, poses = R.sparse_case(N)
        out[N] = (corr, poses, R.oracle_sparse_floor(corr, poses))
    floor = np.max([v[2] for v in out.values()], 0)
    print(f"\nsparse: fp32 oracle floor (rhs, precond, A) per N {[(N, v[2]) for N, v in out.items()]} -> bars {FACTOR * floor}")
    return out, FACTOR * floor


def run_sparse(g, cases, N, chunks, form, fused=False, tiles=0, tail=None):
    """One traced first linearisation of the feature term of window N; returns the normalised errors (rhs, precond, A).
    fused: the dense term is ON over frames without a single valid pixel -- it adds exact zeros to the system and its `tiles` x pairs
    items put the sparse items into k_fused_sweeps (asserted), where OPT_SPARSE_TAIL places them."""
    corr, poses, _ = cases[N]
    key = ("sparse", N)
    if key not in g.refs:
        T, _ = device_matrices(g, poses)
        g.refs[key] = R.sparse_system(corr, T)
    sp = g.refs[key]
    bs = g.BatchSolver(g.ws, n_gn_iters=1, weight_dense_depth=1.0 if fused else 0.0, sparse_chunks=chunks, dense_tiles=tiles)
    corr_d, offs_d, mx = corr_inputs(g, [corr], [R.sparse_offsets(N)])
    poses_d = g.torch.from_numpy(poses[None].astype(np.float32)).to(g.dev)
    zn = g.torch.zeros((1, N, 8, 8, 4), device=g.dev)
    K = np.array([[30, 0, 16], [0, 30, 16], [0, 0, 1]], np.float32)
    try:
        if tail is not None:
            g.ws.set_option(_lib.OPT_SPARSE_TAIL, tail)
        if form == "c24":
            c24, flag = bs.pack_correspondences24(corr_d, offs_d, mx, N, check_order=True)
            tr = bs.solve_zn(zn, 32, 32, K, None, offs_d, mx, poses_d, trace=True, aux={"corr24": c24}, corr_stride=corr_d.shape[1])
        else:
            tr = bs.solve_zn(zn, 32, 32, K, corr_d, offs_d, mx, poses_d, trace=True)
        tv = bs.trace_view(tr)
        st = g.ws.collect_stats()
    finally:
        g.ws.set_option(_lib.OPT_SPARSE_TAIL, DEFAULT_OPTS[_lib.OPT_SPARSE_TAIL])
    if form == "c24":
        assert int(flag.cpu()[0]) == 0
    assert st["fused_sweeps"] == int(fused) and st["sparse_chunks"] == chunks, st
    if fused:
        assert np.all(tv.dense_pair[0, 0] == 0)                      # the dense records are exact zeros
    assert np.all(tv.A[0, 0][:6] == 0) and np.all(tv.A[0, 0][:, :6] == 0)
    return np.array(R.sparse_normalised(tv.rhs[0, 0], tv.precond[0, 0], tv.A[0, 0], sp))


@pytest.mark.parametrize("form", ["entryj", "c24"])
@pytest.mark.parametrize("chunks", R.SPARSE_CHUNKS)
@pytest.mark.parametrize("N", [2, 3, 5])
def test_sparse_sums_against_fp64(gpu, sparse_cases, N, chunks, form):
    """k_sparse_sweep (a launch of its own: dense weight 0)."""
    cases, bars = sparse_cases
    e = run_sparse(gpu, cases, N, chunks, form)
    print(f"sparse N {N} chunks {chunks} {form}: HIP normalised error rhs {e[0]:.3e} precond {e[1]:.3e} A {e[2]:.3e}   (bars {bars})")
    assert np.all(e <= bars), (e, bars)


# (N, chunks, tiles): chunks x pairs >= 64 and tiles x pairs >= 64, the fuse rule
@pytest.mark.parametrize("form", ["entryj", "c24"])
@pytest.mark.parametrize("tail", [0, 100, 256])
@pytest.mark.parametrize("N,chunks,tiles", [(5, 7, 7), (3, 22, 22), (2, 64, 64)])
def test_sparse_sums_in_the_fused_launch(gpu, sparse_cases, N, chunks, tiles, tail, form):
    """The sparse items of k_fused_sweeps, interleaved with the dense items (tail 0), all at the end (256) and split (100)."""
    cases, bars = sparse_cases
    e = run_sparse(gpu, cases, N, chunks, form, fused=True, tiles=tiles, tail=tail)
    print(f"fused sparse N {N} chunks {chunks} tail {tail} {form}: HIP normalised error rhs {e[0]:.3e} precond {e[1]:.3e} A {e[2]:.3e}   (bars {bars})")
    assert np.all(e <= bars), (e, bars)
