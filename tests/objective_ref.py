"""fp64 reference of the objective report (btba_objective_batch_zn_aux), numpy only; test infrastructure.

The report sums, per dense pair and per correspondence segment, rho(e) and the (weighted) square of fp32 residuals behind the solver's hard
accept tests.  tests/sweep_ref.py classifies every dense pixel as accept / reject / borderline; this module takes that classification UNCHANGED
(dense_pair_ref's accept mask at eps = +EPS; the mask at eps = -EPS is "not decisively rejected", so the difference of the two is the borderline
set) and gives, per pair:

  sum_sq, sum_rho, count, max_abs, worst      over the accepts (the fields of btba_objective_pair)
  bud_sq, bud_rho                             sum of |term| over the borderline pixels: an implementation may take or leave each
  max_any                                     max |res| over accepts and borderline pixels
  n_out_sure, n_knee                          accepts beyond the Huber knee by more than KNEE, and accepts within KNEE of it
  sc_sq, sc_rho                               forward-error scales  sum |d term / d res| rs   with rs the residual's round-off scale:
                                              dense  rs = sum_k (|ci_k| + |q_k|) |ni_k|,  sparse (per component)  |T_i pos_i|_k + |T_j pos_j|_k
                                              (the absolute-value forms of DESIGN 3.1 / sweep_ref.sparse_system)

KNEE = 1e-6 m: twice the 5e-7 m residual error that sweep_ref's header derives -- a term further than that from the knee is on the same side of
it in any correct fp32 evaluation.  Bound for an implementation's sum X of a reference sum R:  |X - R| <= Bud + gamma Sc, with gamma = 4 x the
floor of the float32 restatement below against this reference, in units of Sc (tests/test_objective_ref.py measures it in every run)."""
from __future__ import annotations

import numpy as np

import sweep_ref as R
from oracle import oracle_np as ONP

KNEE = 1e-6
FACTOR = 4.0
TILE = 1024          # pixels of a dense tile / entries of a sparse chunk of the kernels (btba_objective_layout.hpp)


def rho(e, delta, strict=False):
    """huberLoss: e inside the knee (e <= delta^2; strict: the mutation e < delta^2), 2 delta sqrt(e) - delta^2 beyond it"""
    e = np.asarray(e, np.float64)
    inside = (e < delta * delta) if strict else (e <= delta * delta)
    return np.where(inside, e, 2.0 * delta * np.sqrt(e) - delta * delta), ~inside


def _delta(prm):
    p = dict(R.DEFAULT_PRM)
    p.update(prm or {})
    return float(np.float32(p["robust_delta"])), p


def _first_argmax(x):
    """(max, lowest index attaining it, runner-up value); (0, -1, 0) for an empty array"""
    if x.size == 0:
        return 0.0, -1, 0.0
    k = int(np.argmax(x))
    rest = np.delete(x, k)
    return float(x[k]), k, float(rest.max()) if rest.size else 0.0


def _bilinear(img, u, v, dt):
    """oracle_np.bilinear4 in the float type dt"""
    H, W = img.shape[:2]
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    al, be = (u - x0.astype(dt)).astype(dt), (v - y0.astype(dt)).astype(dt)
    one = dt(1)

    def tap(x, y):
        ok = ((x >= 0) & (x < W) & (y >= 0) & (y < H)).astype(dt)
        return ok, img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(dt)

    o00, v00 = tap(x0, y0); o10, v10 = tap(x0 + 1, y0); o01, v01 = tap(x0, y0 + 1); o11, v11 = tap(x0 + 1, y0 + 1)
    w0, w1 = o00 * (one - al) + o10 * al, o01 * (one - al) + o11 * al
    s0 = (o00 * (one - al))[:, None] * v00 + (o10 * al)[:, None] * v10
    s1 = (o01 * (one - al))[:, None] * v01 + (o11 * al)[:, None] * v11
    with np.errstate(divide="ignore", invalid="ignore"):
        p0, p1 = s0 / w0[:, None], s1 / w1[:, None]
        u0, u1 = w0 > 0, w1 > 0
        ww = u0 * (one - be) + u1 * be
        ss = np.where(u0[:, None], (one - be)[:, None] * p0, 0) + np.where(u1[:, None], be[:, None] * p1, 0)
        return (ss / ww[:, None]).astype(dt)


def dense_residuals(campos, normals, intr, Tj, Tinv_i, sel, dt=np.float64):
    """(res, rs) of the source pixels `sel` (indices): res = (c_i - q) . n_i evaluated in the float type dt, rs its round-off scale"""
    fx, fy, cx, cy = [dt(v) for v in intr]
    Tij = (np.asarray(Tinv_i, dt) @ np.asarray(Tj, dt)).astype(dt)
    cs = campos[1].reshape(-1, 4)[sel, :3].astype(dt)
    q = (cs @ Tij[:3, :3].T + Tij[:3, 3]).astype(dt)
    u, v = (q[:, 0] * fx / q[:, 2] + cx).astype(dt), (q[:, 1] * fy / q[:, 2] + cy).astype(dt)
    ci, ni = _bilinear(campos[0], u, v, dt)[:, :3], _bilinear(normals[0], u, v, dt)[:, :3]
    res = ((ci - q) * ni).sum(1).astype(dt)
    rs = ((np.abs(ci) + np.abs(q)) * np.abs(ni)).sum(1).astype(np.float64)
    return res, rs


def dense_terms(res, delta, strict=False):
    """(w res^2, rho(res^2), outlier flag, |d wsq / d res|, |d rho / d res|) per residual, fp64 behind the residual"""
    r = np.abs(np.asarray(res, np.float64))
    e = r * r
    rh, out = rho(e, delta, strict)
    w = np.where(out, delta / np.where(r > 0, r, 1.0), 1.0)
    return w * e, rh, out, np.where(out, delta, 2.0 * r), np.where(out, 2.0 * delta, 2.0 * r)


def dense_pair(campos, normals, intr, Ti, Tj, Tinv_i, prm=None):
    """The reference record of one (target, source) pair; campos / normals [2, Hd, Wd, 4] = (target, source), matrices as the implementation holds them."""
    delta, p = _delta(prm)
    ref = R.dense_pair_ref(campos, normals, intr, Ti, Tj, Tinv_i, prm)
    alive = R.dense_pair_ref(campos, normals, intr, Ti, Tj, Tinv_i, prm, eps=-R.EPS)["accept_mask"]
    accept = ref["accept_mask"]
    border = alive & ~accept
    assert not np.any(accept & ~alive) and int(border.sum()) == ref["borderline"], (int(border.sum()), ref["borderline"])
    ia, ib = np.nonzero(accept)[0], np.nonzero(border)[0]
    res, rs = dense_residuals(campos, normals, intr, Tj, Tinv_i, ia)
    wsq, rh, out, d_sq, d_rho = dense_terms(res, delta)
    r = np.abs(res)
    mx, k, second = _first_argmax(r)
    rb, _ = dense_residuals(campos, normals, intr, Tj, Tinv_i, ib)
    wsq_b, rh_b, _, _, _ = dense_terms(rb, delta)
    knee = np.abs(r - delta) < KNEE
    return dict(sum_sq=float(wsq.sum()), sum_rho=float(rh.sum()), count=int(ia.size), borderline=int(ib.size),
                max_abs=mx, worst=int(ia[k]) if k >= 0 else -1, runner_up=second, rs_worst=float(rs[k]) if k >= 0 else 0.0,
                max_any=max(mx, float(np.abs(rb).max()) if ib.size else 0.0),
                n_out_sure=int((out & ~knee).sum()), n_knee=int(knee.sum()),
                bud_sq=float(np.abs(wsq_b).sum()), bud_rho=float(np.abs(rh_b).sum()),
                sc_sq=float((d_sq * rs).sum()), sc_rho=float((d_rho * rs).sum()),
                rs_max=float(rs.max()) if ia.size else 0.0, accept=ia, res=res, rs=rs)


def dense_pair_f32(campos, normals, intr, Tj, Tinv_i, accept, prm=None, strict=False, drop=()):
    """The float32 restatement: the residuals of the reference's accepts in fp32, everything behind them in fp64, summed tile by tile as
    the kernel does.  strict / drop: the mutations (Huber < for <=; accepts to leave out)."""
    delta, _ = _delta(prm)
    ia = np.asarray([s for s in accept if s not in set(drop)], np.int64)
    res, _ = dense_residuals(campos, normals, intr, Tj, Tinv_i, ia, np.float32)
    wsq, rh, out, _, _ = dense_terms(res, delta, strict)
    r = np.abs(res.astype(np.float64))
    mx, k, _ = _first_argmax(r)
    tiles = ia // TILE
    sq = sum(float(wsq[tiles == t].sum()) for t in np.unique(tiles))
    rr = sum(float(rh[tiles == t].sum()) for t in np.unique(tiles))
    return dict(sum_sq=sq, sum_rho=rr, count=int(ia.size), n_outlier=int(out.sum()), max_abs=mx, worst=int(ia[k]) if k >= 0 else -1)


def scene_pairs(sc, T, Tinv, pairs, prm=None):
    """dense_pair of every (target, source) in pairs at the matrices T, Tinv [3, 4, 4]"""
    return [dense_pair(sc["campos"][[i, j]], sc["normals"][[i, j]], sc["intr"], T[i], T[j], Tinv[i], prm) for (i, j) in pairs]


# ---- sparse ----------------------------------------------------------------------------------------------------------------
def sparse_residuals(seg, Ti, Tj, dt=np.float64):
    """(valid indices, r [n, 3], rs [n, 3]) of one segment (ENTRYJ records): r = T_i pos_i - T_j pos_j in the float type dt"""
    idx = np.nonzero(seg["imgIdx_i"] != 0xFFFFFFFF)[0]
    Ti, Tj = np.asarray(Ti, dt), np.asarray(Tj, dt)
    pi, pj = seg["pos_i"][idx].astype(dt), seg["pos_j"][idx].astype(dt)
    wi, wj = (pi @ Ti[:3, :3].T + Ti[:3, 3]).astype(dt), (pj @ Tj[:3, :3].T + Tj[:3, 3]).astype(dt)
    Wi = np.abs(pi).astype(np.float64) @ np.abs(Ti[:3, :3]).T.astype(np.float64) + np.abs(Ti[:3, 3])
    Wj = np.abs(pj).astype(np.float64) @ np.abs(Tj[:3, :3]).T.astype(np.float64) + np.abs(Tj[:3, 3])
    return idx, (wi - wj).astype(dt), Wi + Wj


def sparse_pair(seg, Ti, Tj, prm=None, dt=np.float64, strict=False, drop_last=False):
    """The record of one segment.  dt = float32: the restatement (chunk by chunk as the kernel sums); strict / drop_last: the mutations."""
    delta, _ = _delta(prm)
    idx, r, rs = sparse_residuals(seg, Ti, Tj, dt)
    if drop_last and idx.size:
        idx, r, rs = idx[:-1], r[:-1], rs[:-1]
    r = r.astype(np.float64)
    e = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    rh, out = rho(e, delta, strict)
    root = np.sqrt(e)
    comp = np.abs(r).max(1) if idx.size else np.zeros(0)
    mx, k, second = _first_argmax(comp)
    d_sq = 2.0 * np.abs(r)
    d_rho = np.where(out[:, None], 2.0 * delta * np.abs(r) / np.where(root > 0, root, 1.0)[:, None], 2.0 * np.abs(r))
    knee = np.abs(root - delta) < KNEE
    chunks = idx // TILE
    return dict(sum_sq=sum(float(e[chunks == c].sum()) for c in np.unique(chunks)), sum_rho=sum(float(rh[chunks == c].sum()) for c in np.unique(chunks)),
                count=int(idx.size), n_outlier=int(out.sum()), n_out_sure=int((out & ~knee).sum()), n_knee=int(knee.sum()),
                max_abs=mx, worst=int(idx[k]) if k >= 0 else -1, runner_up=second, rs_worst=float(rs[k].max()) if k >= 0 else 0.0,
                sc_sq=float((d_sq * rs).sum()), sc_rho=float((d_rho * rs).sum()), knee_distance=float(np.abs(root - delta).min()) if idx.size else np.inf)


def sparse_window(corr, offsets, T, prm=None, **kw):
    """sparse_pair of every canonical pair of a window: corr pair-major with segment offsets [P + 1], T [N, 4, 4]"""
    N = T.shape[0]
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
    return [sparse_pair(corr[int(offsets[p]):int(offsets[p + 1])], T[i], T[j], prm, **kw) for p, (i, j) in enumerate(pairs)]


def sparse_objective(corr, T, prm=None):
    """weight_sparse * sum rho over all valid entries (any order of entries), fp64: the function whose gradient the gradient test takes"""
    delta, p = _delta(prm)
    T = np.asarray(T, np.float64)
    v = corr["imgIdx_i"] != 0xFFFFFFFF
    ci, cj = corr["imgIdx_i"][v].astype(np.int64), corr["imgIdx_j"][v].astype(np.int64)
    wi = np.einsum("nab,nb->na", T[ci, :3, :3], corr["pos_i"][v].astype(np.float64)) + T[ci, :3, 3]
    wj = np.einsum("nab,nb->na", T[cj, :3, :3], corr["pos_j"][v].astype(np.float64)) + T[cj, :3, 3]
    r = wi - wj
    return p["weight_sparse"] * float(rho((r * r).sum(1), delta)[0].sum())


def two_sided_case(N):
    """(corr, offsets, pose sets): sweep_ref.sparse_case(N) with TWO pose sets -- its poses_init (nearly every entry beyond the 5 mm knee) and the
    poses its points were generated at (1 mm noise: nearly every entry inside) --, and one entry of the longest segment moved 7 cm off: the worst match."""
    from bundletrack_amd import synthetic as S
    corr, poses_init = R.sparse_case(N)
    corr = corr.copy()
    offs = R.sparse_offsets(N)
    poses_gt = np.ascontiguousarray(S.make_problem(N, 8, seed=70 + N, background=False, full_res=False).poses_gt, np.float32)
    p = int(np.argmax(np.diff(offs.astype(np.int64))))
    seg = corr[int(offs[p]):int(offs[p + 1])]
    k = int(np.nonzero(seg["imgIdx_i"] != 0xFFFFFFFF)[0][len(seg) // 2 if len(seg) > 4 else 0])
    seg["pos_j"][k] = seg["pos_j"][k] + np.array([0.07, 0.0, 0.0], np.float32)
    return corr, offs, (np.ascontiguousarray(poses_init, np.float32), poses_gt), (p, k)


SMALL_SCENES = ("bg32x24", "skew32x24", "bg50x30", "bg275x8", "mask80x60", "smooth13x9", "hole32x24", "edge32x24")
ALL_PAIRS = R.PAIRS_FWD + R.PAIRS_REV
_floor_cache = {}


def floors():
    """dict(dense_sq, dense_rho, sparse_sq, sparse_rho): the float32 restatement's error against the fp64 reference, max over the small scenes'
    ordered pairs (at the CPU oracle's matrices) resp. over the segments of two_sided_case(2, 3, 5) at both pose sets, in units of Sc.
    Needs the CPU oracle (tests' `oracle` fixture).  gamma = FACTOR x these."""
    if _floor_cache:
        return _floor_cache
    f = dict(dense_sq=0.0, dense_rho=0.0, dense_res=0.0, sparse_sq=0.0, sparse_rho=0.0, sparse_res=0.0)      # (_res: one residual, in units of its rs)
    for name in SMALL_SCENES:
        sc = R.scene(name)
        T, Tinv = R.oracle_matrices(sc["poses"])
        for (i, j), ref in zip(ALL_PAIRS, scene_pairs(sc, T, Tinv, ALL_PAIRS)):
            x = dense_pair_f32(sc["campos"][[i, j]], sc["normals"][[i, j]], sc["intr"], T[j], Tinv[i], ref["accept"])
            r32, _ = dense_residuals(sc["campos"][[i, j]], sc["normals"][[i, j]], sc["intr"], T[j], Tinv[i], ref["accept"], np.float32)
            if ref["count"]:
                f["dense_res"] = max(f["dense_res"], float((np.abs(r32.astype(np.float64) - ref["res"]) / ref["rs"]).max()))
            f["dense_sq"] = max(f["dense_sq"], normalised(x["sum_sq"], ref["sum_sq"], 0.0, ref["sc_sq"]))
            f["dense_rho"] = max(f["dense_rho"], normalised(x["sum_rho"], ref["sum_rho"], 0.0, ref["sc_rho"]))
    for N in (2, 3, 5):
        corr, offs, pose_sets, _ = two_sided_case(N)
        for poses in pose_sets:
            T, _ = R.oracle_matrices(poses)
            N_, q = T.shape[0], 0
            for i in range(N_):
                for j in range(i + 1, N_):
                    seg = corr[int(offs[q]):int(offs[q + 1])]
                    q += 1
                    (_, r32, rs), (_, r64, _) = sparse_residuals(seg, T[i], T[j], np.float32), sparse_residuals(seg, T[i], T[j])
                    if r64.size:
                        f["sparse_res"] = max(f["sparse_res"], float((np.abs(r32.astype(np.float64) - r64) / rs).max()))
            for x, ref in zip(sparse_window(corr, offs, T, dt=np.float32), sparse_window(corr, offs, T)):
                f["sparse_sq"] = max(f["sparse_sq"], normalised(x["sum_sq"], ref["sum_sq"], 0.0, ref["sc_sq"]))
                f["sparse_rho"] = max(f["sparse_rho"], normalised(x["sum_rho"], ref["sum_rho"], 0.0, ref["sc_rho"]))
    _floor_cache.update(f)
    return _floor_cache


def gammas():
    return {k: FACTOR * v for k, v in floors().items()}


def fold(records, field):
    """sum of a field over records in index order, from 0.0 (the order of k_objective_fold)"""
    s = 0.0
    for r in records:
        s = s + float(r[field])
    return s


def normalised(x, ref, bud, sc):
    """(|x - ref| - bud) / sc, 0 inside the budget; a sum whose scale is zero must be inside the budget exactly"""
    d = abs(float(x) - float(ref)) - float(bud)
    return 0.0 if d <= 0 else (d / sc if sc > 0 else np.inf)
