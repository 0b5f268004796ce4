"""fp64 references for the three stages of the per-instance system solve (numpy only; test infrastructure).

The solve turns the sweeps' pair sums into the next iterate in three stages.  Each is restated here from oracle/oracle_np.py::solve as
a function over TRACED inputs, every fp32 input taken as exact, so that a test can say which stage of which kernel is wrong:

  A  assembly   (correspondences, T_before, 28-float dense records)  ->  A, rhs, M^-1          assemble_ref
  B  PCG        (A, rhs, M^-1)                                       ->  scalars per step, delta pcg_ref
  C  update     (delta, x_before)                                    ->  x_after, T_after      update_ref

and the comparison functions that tests/test_gpu_solve_stages.py (device traces) and tests/test_solve_ref.py (the fp32 CPU oracle,
fp32 restatements and deliberately wrong outputs) share: check_assembly, compare_pcg + pcg_verdict, check_update.

Layouts: A [6N, 6N] in [trans, rot] order per frame (oracle_np's and the trace's); rhs / precond / delta / x [N, 6] in the trace's
(rot, trans) order.  Frame 0 is fixed: its rows and columns of A, its rhs and its delta are zero.

Bars.
  A  |dev - ref| <= FACTOR floor sc_sparse + gamma_n sc_dense per entry.  sc_sparse: sweep_ref.sparse_system's absolute-value scale,
     floor: the fp32 CPU oracle's own error against the same fp64 system in units of that scale (oracle_floor: in windows of up to
     12 frames every linearisation of its own solve, not the first alone), FACTOR = 4 (the rule of tests/test_gpu_sweep_sums.py).
     The dense records are exact inputs, so the dense share's only round-off is its additions: gamma_n = n u / (1 - n u), u = 2^-24, n = records summed into the entry + 1 (joining the sparse share), times the
     sum of the absolute values of the entry's dense terms.  An entry whose scales are both zero must be exact.
  B  pAp and rz_new in units of the running maximum of the reference's values up to that step, delta in units of max |delta64|;
     bar = FACTOR x floor, floor = the largest error in the same units of two fp32 restatements of the same recurrences (numpy's
     reductions; a sequential loop over the reversed terms) over ALL iterates and steps of a case.  A case whose delta bar exceeds
     DELTA_CAP = 1e-4 is ill-chosen and fails.  alpha / beta are not compared with fp64 (noise over noise once CG has converged): they
     are held to the device's own traced numerator and denominator, and the guards to the device's own numbers, exactly.
  C  the A / B rule of tests/test_gpu_device_math.py::test_update_composition (shared_checks._bound, A_FAST, B_FAST, the fp32 CPU
     oracle's lie_update / pose_to_matrix as comparator).  x_after against Log(Exp(delta) Exp(x_before)); T_after against Exp of the
     TRACED x_after (an fp32 input like any other: the stage's last step, held to its own truth)."""
from __future__ import annotations

import numpy as np

import se3_ref as SE
import sweep_ref as SW
from oracle import oracle_np as ONP
from shared_checks import A_FAST, B_FAST, _bound, _ulp

U32 = 2.0 ** -24
GUARD = ONP.EPS                 # FLOAT_EPSILON of the pAp / rz guards and of the Jacobi guard
FACTOR = 4.0
DELTA_CAP = 1e-4
ORDERS = ("numpy", "reversed")


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U32 / (1.0 - n * U32)


def to_trans_rot(v):
    """[N, 6] in the traced (rot, trans) order -> [6N] in oracle_np's [trans, rot] order."""
    v = np.asarray(v).reshape(-1, 6)
    return np.concatenate([v[:, 3:], v[:, :3]], 1).reshape(-1)


# ---- stage A -------------------------------------------------------------------------------------------------------------
def record_blocks(rec):
    """A traced 28-float dense record -> (S [6, 6] symmetric, g [6]) in [trans, rot] order, as float64."""
    rec = np.asarray(rec, np.float64)
    S = np.zeros((6, 6))
    for q, (r, c) in enumerate(SW.TRI):
        S[r, c] = S[c, r] = rec[q]
    return S, rec[21:27].copy()


def dense_scatter(N, records, pairs):
    """The dense share as oracle_np.solve places it, from per-pair records; pairs = (target i, source j).  +S on both diagonal blocks,
    -g on the source and +g on the target, -S / -S^T on the cross blocks for i < j only (the cross block of a reversed pair is erased),
    nothing for frame 0.  Returns dict(A, b, abs_A, abs_b, n_A, n_b): the sums, the sums of the terms' absolute values, the term counts."""
    dim = 6 * N
    A, b, aA, ab = np.zeros((dim, dim)), np.zeros(dim), np.zeros((dim, dim)), np.zeros(dim)
    nA, nb = np.zeros((dim, dim), np.int64), np.zeros(dim, np.int64)
    for rec, (i, j) in zip(records, pairs):
        i, j = int(i), int(j)
        S, g = record_blocks(rec)
        for k, sign in ((j, -1.0), (i, 1.0)):
            if k > 0:
                s = slice(6 * k, 6 * k + 6)
                A[s, s] += S; aA[s, s] += np.abs(S); nA[s, s] += 1
                b[s] += sign * g; ab[s] += np.abs(g); nb[s] += 1
        if 0 < i < j:
            si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
            A[sj, si] -= S; A[si, sj] -= S.T
            aA[sj, si] += np.abs(S); aA[si, sj] += np.abs(S.T)
            nA[sj, si] += 1; nA[si, sj] += 1
    return dict(A=A, b=b, abs_A=aA, abs_b=ab, n_A=nA, n_b=nb)


def join_system(sp, dn):
    """sweep_ref.sparse_system's dict + a dense share (dense_scatter's dict, or None) -> the reference system and its scales."""
    dim = sp["b"].shape[0]
    if dn is None:
        dn = dict(A=np.zeros((dim, dim)), b=np.zeros(dim), abs_A=np.zeros((dim, dim)), abs_b=np.zeros(dim),
                  n_A=np.zeros((dim, dim), np.int64), n_b=np.zeros(dim, np.int64))
    A, b = sp["A"] + dn["A"], sp["b"] + dn["b"]
    Minv, sc_Minv = SW.precond_ref(sp["Mdiag"], sp["sc_M"])
    return dict(A=A, b=b, Mdiag=sp["Mdiag"], Minv=Minv, rhs=SW.to_rot_trans(b), precond=SW.to_rot_trans(Minv),
                sp_A=sp["sc_A"], dn_A=dn["abs_A"], n_A=dn["n_A"], sp_b=sp["sc_b"], dn_b=dn["abs_b"], n_b=dn["n_b"], sc_Minv=sc_Minv)


def assemble_ref(corr, T_before, dense_records, dense_pairs, w_sparse, w_dense_on):
    """The fp64 system of one iterate: A and b weighted by w_sparse, M^-1 from the UNWEIGHTED Jacobi diagonal behind its > 1e-6 guard
    (sweep_ref.precond_ref), the dense share from the traced records (which carry the dense weight already; w_dense_on = False: none).
    Returns join_system's dict: A [6N, 6N], b / Mdiag / Minv [6N] in [trans, rot] order, rhs / precond [N, 6] in (rot, trans) order, and the
    round-off scales sp_* (sparse share, absolute-value sums), dn_* (dense share, sums of |terms|), n_* (dense terms per entry), sc_Minv."""
    T = np.asarray(T_before, np.float64)
    sp = SW.sparse_system(corr, T, dict(weight_sparse=float(w_sparse)))
    dn = dense_scatter(T.shape[0], dense_records, dense_pairs) if (w_dense_on and len(dense_pairs)) else None
    return join_system(sp, dn)


FLOOR_ALL_ITERATES_UP_TO = 12       # frames


def oracle_floor(corr, poses, n_gn=7):
    """(rhs, precond, A): the fp32 CPU oracle's worst error against the fp64 sparse system at its own matrices, in units of the absolute-value
    scales, over both accumulation modes of its own feature-term-only solve (the matrix probed column by column: the oracle applies J^T J
    matrix-free).  Windows of more than FLOOR_ALL_ITERATES_UP_TO frames: the first linearisation, i.e. sweep_ref.oracle_sparse_floor.
    Smaller windows: ALL n_gn linearisations.  In a window of two frames the first linearisation's floor is the largest of six numbers per
    quantity, and the same oracle was measured 10 x further out two iterates later (precond: 3.2e-8 at iterate 0, 4.9e-7 at iterate 2), so a
    bar of 4 x the first linearisation's floor failed the oracle itself; seven linearisations sample what one does in a window of 13 frames."""
    return SW.oracle_sparse_floor(corr, poses, n_gn if poses.shape[0] <= FLOOR_ALL_ITERATES_UP_TO else 1)


def assembly_bars(ref, floor):
    """Per-entry absolute bars (A [6N, 6N]; rhs, precond [N, 6]) from the oracle's floor (rhs, precond, A) in units of the sparse scales."""
    f_r, f_p, f_A = (float(f) for f in floor)
    bar_A = FACTOR * f_A * ref["sp_A"] + gamma(ref["n_A"] + (ref["n_A"] > 0)) * ref["dn_A"]
    bar_b = FACTOR * f_r * ref["sp_b"] + gamma(ref["n_b"] + (ref["n_b"] > 0)) * ref["dn_b"]
    return bar_A, SW.to_rot_trans(bar_b), SW.to_rot_trans(FACTOR * f_p * ref["sc_Minv"])


def _worst(diff, bar):
    """(error in units of the bar, index of the worst entry); an entry with a zero bar must be exact."""
    e = np.where(diff == 0, 0.0, np.where(bar > 0, diff / np.where(bar > 0, bar, 1.0), np.inf))
    k = np.unravel_index(int(np.argmax(e)), e.shape) if e.size else ()
    return (float(e[k]) if e.size else 0.0), tuple(int(v) for v in k)


def check_assembly(A_dev, rhs_dev, prec_dev, ref, floor, sparse_on=True):
    """Traced A [6N, 6N], rhs, precond [N, 6] against assemble_ref's dict.  Returns dict(e_A, e_rhs, e_prec: worst error in units of the
    entry's bar, <= 1 passes; symmetric: A equals its transpose bit for bit; fails: what is wrong, naming the entry)."""
    A_dev, rhs_dev, prec_dev = (np.asarray(v, np.float64) for v in (A_dev, rhs_dev, prec_dev))
    bar_A, bar_r, bar_p = assembly_bars(ref, floor)
    fails = []
    eA, kA = _worst(np.abs(A_dev - ref["A"]), bar_A)
    er, kr = _worst(np.abs(rhs_dev - ref["rhs"])[1:], bar_r[1:])
    ep, kp = _worst(np.abs(prec_dev - ref["precond"])[1:], bar_p[1:])
    if not eA <= 1.0:
        fails.append(f"A[{kA[0]}, {kA[1]}] (frames {kA[0] // 6}, {kA[1] // 6}): {A_dev[kA]!r} against {ref['A'][kA]!r}, {eA:.3g} x its bar {bar_A[kA]:.3e}")
    if not er <= 1.0:
        fails.append(f"rhs of frame {kr[0] + 1} unknown {kr[1]}: {rhs_dev[1:][kr]!r} against {ref['rhs'][1:][kr]!r}, {er:.3g} x its bar {bar_r[1:][kr]:.3e}")
    if not ep <= 1.0:
        fails.append(f"precond of frame {kp[0] + 1} unknown {kp[1]}: {prec_dev[1:][kp]!r} against {ref['precond'][1:][kp]!r}, {ep:.3g} x its bar {bar_p[1:][kp]:.3e}")
    symmetric = bool(np.array_equal(A_dev, A_dev.T))
    if not symmetric and not np.all(np.abs(A_dev - A_dev.T) <= bar_A):
        fails.append("A differs from its transpose by more than the bar")
    if np.any(A_dev[:6] != 0) or np.any(A_dev[:, :6] != 0):
        fails.append("frame 0's rows and columns of A are not exact zeros")
    untouched = (ref["sp_A"] == 0) & (ref["n_A"] == 0)
    if np.any(A_dev[untouched] != 0):
        k = np.argwhere(untouched & (A_dev != 0))[0]
        fails.append(f"A[{k[0]}, {k[1]}] belongs to a block that no pair touches and is {A_dev[k[0], k[1]]!r}")
    if not sparse_on and np.any(prec_dev[1:] != 1.0):
        fails.append("sparse term off: precond is not exactly 1 on every active unknown")
    return dict(e_A=eA, e_rhs=er, e_prec=ep, symmetric=symmetric, fails=fails)


# ---- stage B -------------------------------------------------------------------------------------------------------------
def _dot(a, b, dtype, order):
    t = a * b
    if order == "numpy":
        return t.sum(dtype=dtype)
    return np.cumsum(t[::-1], dtype=dtype)[-1] if t.size else dtype(0)         # (cumsum adds sequentially in its dtype)


def _matvec(A, p, dtype, order):
    if order == "numpy":
        return A @ p
    return np.cumsum(A[:, ::-1] * p[::-1], axis=1, dtype=dtype)[:, -1] if p.size else np.zeros(0, dtype)


def pcg_ref(A, b, Minv, n_pcg, dtype=np.float64, order="numpy", decisions=None):
    """oracle_np.solve's PCG recurrences on the active 6 (N - 1) block of A [6N, 6N] ([trans, rot]) with b, Minv [N, 6] ((rot, trans), as
    traced), carried out in `dtype`; order: how a dot product and a row of the mat-vec are summed ("numpy": numpy's own reductions,
    "reversed": one term after the other, last term first).  decisions: {(step, "alpha" | "beta"): bool} forces the outcome of the named
    guards (pAp > 1e-6 / previous rz > 1e-6); the others are taken on the run's own numbers.
    Returns dict(delta [N, 6] (rot, trans), scalars [n_pcg, 4] = (pAp, alpha, rz_new, beta), rz0, decisions: every guard's outcome)."""
    dt = np.dtype(dtype).type
    N = np.asarray(b).reshape(-1, 6).shape[0]
    Aa = np.asarray(A)[6:, 6:].astype(dt)
    ba, Ma = to_trans_rot(b)[6:].astype(dt), to_trans_rot(Minv)[6:].astype(dt)
    eps = dt(GUARD)
    decisions = decisions or {}
    taken = {}
    d = np.zeros_like(ba); rr = ba.copy(); z = Ma * rr; p = z.copy()
    rz = rz0 = _dot(rr, z, dt, order)
    sc = np.zeros((n_pcg, 4))
    for li in range(n_pcg):
        Ap = _matvec(Aa, p, dt, order)
        pAp = _dot(p, Ap, dt, order)
        on = taken[(li, "alpha")] = bool(decisions.get((li, "alpha"), pAp > eps))
        alpha = rz / pAp if on else dt(0)
        d = d + alpha * p; rr = rr - alpha * Ap; z = Ma * rr
        rzn = _dot(z, rr, dt, order)
        on = taken[(li, "beta")] = bool(decisions.get((li, "beta"), rz > eps))
        beta = rzn / rz if on else dt(0)
        sc[li] = (pAp, alpha, rzn, beta)
        rz = rzn; p = z + beta * p
    delta = np.zeros((N, 6))
    delta[1:] = SW.to_rot_trans(d.astype(np.float64))
    return dict(delta=delta, scalars=sc, rz0=float(rz0), decisions=taken)


def _running_max(v):
    return np.maximum.accumulate(np.abs(np.asarray(v, np.float64)))


def _units(diff, scale):
    diff, scale = np.asarray(diff, np.float64), np.asarray(scale, np.float64)
    return np.where(diff == 0, 0.0, np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), np.inf))


def pcg_errors(scalars, delta, ref):
    """(e_pAp [n_pcg], e_rz [n_pcg], e_delta) of an implementation's scalars and delta against pcg_ref(float64)'s dict, in its units."""
    scalars, delta = np.asarray(scalars, np.float64), np.asarray(delta, np.float64)
    e_p = _units(np.abs(scalars[:, 0] - ref["scalars"][:, 0]), _running_max(ref["scalars"][:, 0]))
    e_r = _units(np.abs(scalars[:, 2] - ref["scalars"][:, 2]), _running_max(ref["scalars"][:, 2]))
    dmax = np.abs(ref["delta"]).max()
    e_d = float(_units(np.abs(delta - ref["delta"]), dmax).max())
    return e_p, e_r, e_d


def guard_margins(ref):
    """{(step, kind): |guard quantity - 1e-6| of the fp64 reference in the units its bar is stated in} -- a cell whose margin is inside the
    bar is BORDERLINE: a correct fp32 implementation may decide it either way."""
    sc = ref["scalars"]
    rm_p, rm_r = _running_max(sc[:, 0]), _running_max(sc[:, 2])
    out = {}
    for li in range(sc.shape[0]):
        out[(li, "alpha")] = float(_units(abs(sc[li, 0] - GUARD), rm_p[li]))
        q, s = (ref["rz0"], abs(ref["rz0"])) if li == 0 else (sc[li - 1, 2], rm_r[li - 1])
        out[(li, "beta")] = float(_units(abs(q - GUARD), s))
    return out


def _ulps(x, q):
    """|x - q| in ulps of the float32 nearest q"""
    return abs(float(x) - float(q)) / float(_ulp(q)) if np.isfinite(q) else np.inf


def compare_pcg(A_dev, rhs_dev, prec_dev, pcg_dev, delta_dev):
    """One traced PCG (scalars [n_pcg, 4], delta [N, 6]) against pcg_ref(float64) on the traced system.  Returns dict
      e = (pAp, rz, delta) worst errors, floor = the same for the two fp32 restatements, cell: where the worst errors sit,
      margins {(step, kind): margin} of every guard, forced [(step, kind)]: guards where the reference followed the device,
      fails: violations of the exact checks (decisions on the device's own numbers, quotients within 2 ulp, frame 0's delta)."""
    pcg_dev, delta_dev = np.asarray(pcg_dev, np.float64), np.asarray(delta_dev, np.float64)
    n_pcg = pcg_dev.shape[0]
    n_act = 6 * (delta_dev.shape[0] - 1)
    fails = []
    free = pcg_ref(A_dev, rhs_dev, prec_dev, n_pcg)
    rz0 = free["rz0"]
    g_dot = float(gamma(n_act + 2))                      # an fp32 dot product of n_act positive terms r M^-1 r, each two multiplies
    rz0_borderline = abs(rz0 - GUARD) <= g_dot * abs(rz0)
    dev_dec = {}
    for li in range(n_pcg):
        pAp, alpha, rzn, beta = pcg_dev[li]
        rz_prev = rz0 if li == 0 else pcg_dev[li - 1, 2]
        dev_dec[(li, "alpha")] = bool(pAp > GUARD)
        if (alpha == 0) != (pAp <= GUARD) and rz_prev != 0:
            fails.append(f"step {li}: alpha {alpha!r} with pAp {pAp!r}")
        if li == 0 and rz0_borderline:
            dev_dec[(li, "beta")] = bool(beta != 0)
        else:
            dev_dec[(li, "beta")] = bool(rz_prev > GUARD)
            if (beta == 0) != (rz_prev <= GUARD) and rzn != 0:
                fails.append(f"step {li}: beta {beta!r} with the previous rz {rz_prev!r}")
        slack = g_dot * 2.0 ** 24 if li == 0 else 0.0      # step 0's numerator / denominator rz0 is recomputed in fp64, not traced
        if alpha != 0 and not _ulps(alpha, rz_prev / pAp) <= 2.0 + slack:
            fails.append(f"step {li}: alpha {alpha!r} is {_ulps(alpha, rz_prev / pAp):.1f} ulp from rz / pAp = {rz_prev / pAp!r}")
        if beta != 0 and not _ulps(beta, rzn / rz_prev) <= 2.0 + slack:
            fails.append(f"step {li}: beta {beta!r} is {_ulps(beta, rzn / rz_prev):.1f} ulp from rz_new / rz = {rzn / rz_prev!r}")
    q0 = max([_ulps(pcg_dev[0, 1], rz0 / pcg_dev[0, 0])] * bool(pcg_dev[0, 1] != 0) + [_ulps(pcg_dev[0, 3], pcg_dev[0, 2] / rz0)] * bool(pcg_dev[0, 3] != 0) + [0.0])
    forced, ref = {}, free
    for _ in range(2 * n_pcg):
        diff = [c for c in sorted(dev_dec) if c not in forced and ref["decisions"][c] != dev_dec[c]]
        if not diff:
            break
        forced[diff[0]] = dev_dec[diff[0]]
        ref = pcg_ref(A_dev, rhs_dev, prec_dev, n_pcg, decisions=forced)
    margins = guard_margins(ref)
    if np.any(delta_dev[0] != 0):
        fails.append("delta of frame 0 is not exact zeros")
    e_p, e_r, e_d = pcg_errors(pcg_dev, delta_dev, ref)
    fl = np.zeros(3)
    for order in ORDERS:
        r32 = pcg_ref(A_dev, rhs_dev, prec_dev, n_pcg, np.float32, order, decisions=ref["decisions"])
        f_p, f_r, f_d = pcg_errors(r32["scalars"], r32["delta"], ref)
        fl = np.maximum(fl, (f_p.max(), f_r.max(), f_d))
    return dict(e=np.array([e_p.max(), e_r.max(), e_d]), floor=fl, cell=(int(np.argmax(e_p)), int(np.argmax(e_r))), margins=margins,
                forced=sorted(forced), fails=fails, ref=ref, step0_ulps=q0)


def pcg_verdict(results):
    """results: [(label, iterate, compare_pcg's dict)] of ONE case.  Returns dict(floor, bar, worst (pAp, rz, delta), borderline: the cells
    whose guard margin is inside the bar, fails).  Bar = FACTOR x the case's floor; a delta bar above DELTA_CAP fails the case as ill-chosen;
    at most one borderline cell per case and none at iterate 0; the reference may follow the device's decision in a borderline cell only."""
    floor = np.max([r["floor"] for _, _, r in results], 0)
    bar = FACTOR * floor
    worst = np.max([r["e"] for _, _, r in results], 0)
    fails = []
    if not bar[2] <= DELTA_CAP:
        fails.append(f"ill-chosen case: the delta bar {bar[2]:.3e} exceeds {DELTA_CAP:.0e}")
    borderline = []
    for label, it, r in results:
        fails += [f"{label} iterate {it}: {m}" for m in r["fails"]]
        for q, name in enumerate(("pAp", "rz_new", "delta")):
            if not r["e"][q] <= bar[q]:
                where = f" (step {r['cell'][q]})" if q < 2 else ""
                fails.append(f"{label} iterate {it}: {name}{where} is {r['e'][q]:.3e} from the fp64 PCG on the traced system, bar {bar[q]:.3e}")
        for cell, m in r["margins"].items():
            inside = m <= bar[0 if cell[1] == "alpha" else 1]
            if inside:
                borderline.append((label, it) + cell)
            if cell in r["forced"] and not inside:
                fails.append(f"{label} iterate {it}: the {cell[1]} guard of step {cell[0]} is decided against the fp64 reference, {m:.3e} from 1e-6 in the bar's units")
    if len(borderline) > 1 or any(c[1] == 0 for c in borderline):
        fails.append(f"ill-chosen case: borderline guards {borderline} (at most one per case, none at iterate 0)")
    return dict(floor=floor, bar=bar, worst=worst, borderline=borderline, fails=fails, step0_ulps=max(r["step0_ulps"] for _, _, r in results))


# ---- stage C -------------------------------------------------------------------------------------------------------------
def update_ref(delta, x_before):
    """x_k <- Log(Exp(delta_k) Exp(x_k)) for k >= 1 (delta, x_before [N, 6] in (rot, trans) order); frame 0 untouched.
    Returns (x_after [N, 6], T_after [N, 4, 4]) in float64."""
    delta, x = np.asarray(delta, np.float64), np.asarray(x_before, np.float64)
    rot, trans = SE.update(delta[:, :3], delta[:, 3:], x[:, :3], x[:, 3:])
    x_after = np.concatenate([rot, trans], 1)
    x_after[0] = x[0]
    return x_after, SE.pose_to_matrix(x_after[:, :3], x_after[:, 3:])


def check_update(oracle, x_after_dev, T_after_dev, delta_dev, x_before, T_before, stats=None):
    """Traced x_after [N, 6], T_after [N, 4, 4] of one iterate against update_ref(traced delta, x_before) under the A / B rule, and the exact
    claims: frame 0's x and T are the bits of the input, its delta is zero, every T_after ends in (0, 0, 0, 1).  Returns the failures."""
    x_after_dev, T_after_dev, delta_dev, x_before = (np.asarray(v, np.float32) for v in (x_after_dev, T_after_dev, delta_dev, x_before))
    stats = {} if stats is None else stats
    N = x_before.shape[0]
    fails = []
    if N > 1:
        t_x, _ = update_ref(delta_dev, x_before)
        o = [oracle.lie_update(delta_dev[k, :3], delta_dev[k, 3:], x_before[k, :3], x_before[k, 3:]) for k in range(1, N)]
        o_rot, o_trans = np.stack([v[0] for v in o]), np.stack([v[1] for v in o])
        lab = np.array(["frames"] * (N - 1))
        bad = _bound(stats, lab, "x_after.rot", x_after_dev[1:, :3], o_rot, t_x[1:, :3], np.linalg.norm(t_x[1:, :3], axis=1), A_FAST, B_FAST)
        bad += _bound(stats, lab, "x_after.trans", x_after_dev[1:, 3:], o_trans, t_x[1:, 3:], np.linalg.norm(t_x[1:, 3:], axis=1), A_FAST, B_FAST)
        t_T = SE.pose_to_matrix(x_after_dev[1:, :3].astype(np.float64), x_after_dev[1:, 3:].astype(np.float64))
        o_T = np.stack([oracle.pose_to_matrix(x_after_dev[k, :3], x_after_dev[k, 3:]) for k in range(1, N)])
        bad += _bound(stats, lab, "T_after.R", T_after_dev[1:, :3, :3], o_T[:, :3, :3], t_T[:, :3, :3], np.ones(N - 1), A_FAST, B_FAST)
        bad += _bound(stats, lab, "T_after.t", T_after_dev[1:, :3, 3], o_T[:, :3, 3], t_T[:, :3, 3], np.linalg.norm(t_T[:, :3, 3], axis=1), A_FAST, B_FAST)
        fails += [f"{name} of frame {i + 1}: {ratio:.3g} x (A e_oracle + B ulp)" for name, _, i, ratio in bad]
    if x_after_dev[0].tobytes() != x_before[0].tobytes():
        fails.append("x of frame 0 changed")
    if T_before is not None and T_after_dev[0].tobytes() != np.asarray(T_before, np.float32)[0].tobytes():
        fails.append("T of frame 0 changed")
    if np.any(delta_dev[0] != 0):
        fails.append("delta of frame 0 is not exact zeros")
    if not np.array_equal(T_after_dev[:, 3], np.tile(np.float32([0, 0, 0, 1]), (N, 1))):
        fails.append("a T_after does not end in (0, 0, 0, 1)")
    return fails


# ---- the cases of tests/test_gpu_solve_stages.py (their floors and caps are checked on the CPU by tests/test_solve_ref.py) ---------
SMALL_MAX, MID_MAX, SMALL_BLOCK = 21, 31, 1024       # kSmallMaxFrames, kMidMaxFrames = BTBA_MAX_FRAMES_LDS, kSmallBlock
CPU_MAX_FRAMES = 15                                  # oracle_np.solve takes 13 s at 15 frames and 50 s at 31: larger windows get their caps on the GPU


LDS_LIMIT = 160 * 1024                               # bytes of dynamic LDS a solve launch may ask for
SPARSE_VALS, DENSE_VALS, FRAME_SUMS = 44, 28, 48     # kSparseVals, kDenseVals, kFrameSums


def _r4(v):
    return (v + 3) & ~3


def small_cpl(N):
    na = 6 * (N - 1)
    return 4 if na <= 32 else 8 if na <= 64 else 12 if na <= 96 else 16


def small_solve_lds_floats(N, Pd):
    """SmallLayout<CPL>::fixed + the pair sums (btba_solve_small.hpp): every fixed region is sized for the instantiation's largest window."""
    cpl = small_cpl(N)
    NA = 8 * cpl
    NF = min(NA // 6 + 1, SMALL_MAX)
    NP = NF * (NF - 1) // 2
    lda = 4 * ((2 * cpl) | 1)
    fixed = NA * lda + 6 * lda + 2 * 16 * NF + _r4(6 * NF) + (NF - 1) * FRAME_SUMS + 2 * _r4(NP) + _r4(NF + 1) + 4 * NP
    return fixed + (N * (N - 1) // 2) * SPARSE_VALS + Pd * DENSE_VALS + 8 * SPARSE_VALS + 16


def mid_solve_lds_floats(N, Pd):
    """MidLayout::fixed + the pair sums (btba_solve_mid.hpp)."""
    NF = MID_MAX
    NP = NF * (NF - 1) // 2
    lv = 4 * 48 + 4
    fixed = 5 * lv + 2 * 16 * NF + _r4(6 * NF) + (NF - 1) * FRAME_SUMS + 288 + 2 * _r4(NP) + _r4(NF + 1) + _r4(2 * NP)
    return fixed + (N * (N - 1) // 2) * SPARSE_VALS + Pd * DENSE_VALS + 8 * SPARSE_VALS + 16


def general_solve_lds_floats(N, Pd):
    """SolveLayout(N, Pd, a_in_global = false).total (btba_solve_layout.hpp)."""
    n, P = 6 * N, N * (N - 1) // 2
    ld = 4 * (((n + 3) // 4) | 1)
    return n * ld + 6 * ld + 16 + 16 * N + 2 * Pd + (N + 1) + 2 * Pd + P + 288 + _r4(P) + _r4(n)


def selected_kernel(N, n_dense_pairs, solve_small=1):
    """The dispatch rule of btba_api.hip for a traced, non-atomic solve: which kernel turns the pair sums into the iterate.  The matrix moves
    to global memory when the general layout exceeds the LDS limit; k_solve_small and k_solve_mid are taken only while their own layouts,
    pair sums included, fit it (and k_solve_small's tables one trip of its 1 024 lanes, k_solve_mid at most one dense pair per canonical pair)."""
    P, Pd = N * (N - 1) // 2, n_dense_pairs
    a_global = 4 * general_solve_lds_floats(N, Pd) > LDS_LIMIT
    if solve_small and not a_global and N <= SMALL_MAX and 2 * Pd <= SMALL_BLOCK and 4 * small_solve_lds_floats(N, Pd) <= LDS_LIMIT:
        return "k_solve_small<%d>" % small_cpl(N)
    if solve_small and not a_global and SMALL_MAX < N <= MID_MAX and Pd <= P and 4 * mid_solve_lds_floats(N, Pd) <= LDS_LIMIT:
        return "k_solve_mid"
    return "k_system_solve[global,16-wave]" if a_global else "k_system_solve[lds,1-wave]"


def explicit_lists(K):
    """The PAIRS_EXPLICIT lists of (target, source), by name."""
    fwd = [(i, j) for i in range(K) for j in range(i + 1, K)]
    # Every ordered pair at 21 frames (Pd = 420) asks k_solve_small<16> for 168 416 bytes of LDS against the limit of 163 840 and goes to
    # k_system_solve: it cannot run on k_solve_small.  The largest list that does holds 379 pairs; at 21 frames the first list is therefore every
    # forward pair and the reverse of every pair at most nine frames apart (354 pairs, both orders of 144).
    both = [(i, j) for i in range(K) for j in range(K) if i != j and (K < SMALL_MAX or i < j or i - j <= 9)]
    return {
        "every_ordered_pair" if K < SMALL_MAX else "both_orders_up_to_9_apart": both,
        "reversed_only": [(j, i) for (i, j) in fwd],
        "frame_2_without_pair": [(i, j) for (i, j) in fwd if 2 not in (i, j)],
        "frame_0_source_only": [(j, 0) for j in range(1, K)] + [(i, j) for (i, j) in fwd if i > 0],
        "frame_0_target_only": [(0, j) for j in range(1, K)] + [(j, i) for (i, j) in fwd if i > 0],
        "one_pair": [(1, 2)],
    }


ITER_WEIGHTS = dict(sparse=(1.0, 0.5, 2.0, 0.25, 1.5, 0.75, 3.0), dense=(1.0, 0.5, 0.0, 2.0, 1.0, 0.0, 0.25))       # dense weight 0 in iterates 2 and 5
PARTIALS = ((1, 1), (4, 3), (5, 5), (8, 8), (16, 8))        # (sparse_chunks, dense_tiles): reduce_partials' identity, rounds of four, rounds of eight with a clamped tail


def _case(group, K, seeds, small=1, pairs=None, pairs_name=None, prm=None, iter_weights=None, no_corr_frame=None, partials=None):
    Pd = 0 if (prm or {}).get("weight_dense_depth", 1.0) == 0 else (len(pairs) if pairs is not None else K * (K - 1) // 2)
    kernel = selected_kernel(K, Pd, small)
    tag = pairs_name or (("chunks%d_tiles%d" % partials) if partials else None) or ("iter_weights" if iter_weights else None) \
        or ("no_corr_frame%d" % no_corr_frame if no_corr_frame is not None else None) or "-".join(f"{k}={v:g}" for k, v in (prm or {}).items()) or f"opt{small}"
    return dict(id=f"{group}-K{K}-{tag}-{kernel}", group=group, K=K, seeds=tuple(seeds), small=small, pairs=pairs, prm=dict(prm or {}), iter_weights=iter_weights,
                no_corr_frame=no_corr_frame, partials=partials, kernel=kernel)


# Seeds: 500 + 10 K + b, except where the fp64 reference alone misses a cap there (tests/test_solve_ref.py measures it on oracle_np's systems):
# K = 2 seed 521 has two borderline pAp guards (steps 4 of iterates 0 and 1), K = 3 seed 531 a delta bar of 1.04e-4.
SEEDS = {2: (520, 522), 3: (532, 533)}
# A frame without a correspondence keeps M^-1 = 1 while its diagonal block is the dense term's alone -- thousands at weight 1, which puts the
# delta bar at 1e-3 ... 1e-2 (measured on four seeds and frames); at a dense weight of 0.01 the block is of the order of 1 and the case meets its cap.
NO_CORR_DENSE_WEIGHT = 0.01


def _seeds(K, n=2):
    return list(SEEDS.get(K, [500 + 10 * K + b for b in range(n)]))[:n]


def cases():
    out = [_case("sizes", K, _seeds(K)) for K in (2, 3, 6, 7, 11, 12, 17, 18, 21, 22, 31)]
    out += [_case("sizes", K, _seeds(K), small=0) for K in (2, 21, 22, 31, 32, 40)]
    for K in (5, 21):
        out += [_case("lists", K, _seeds(K, 1), pairs=pl, pairs_name=name) for name, pl in explicit_lists(K).items()]
    assert all(c["kernel"].startswith("k_solve_small") for c in out if c["group"] == "lists")      # (the K = 24 list below: k_system_solve by fallback)
    out.append(_case("lists", 24, _seeds(24, 1), pairs=[(i, j) for i in range(24) for j in range(24) if i != j], pairs_name="every_ordered_pair"))
    for K in (7, 22):
        out += [_case("terms", K, _seeds(K, 1), prm=dict(weight_dense_depth=0.0)), _case("terms", K, _seeds(K, 1), prm=dict(weight_sparse=0.0)),
                _case("terms", K, _seeds(K, 1), prm=dict(weight_dense_depth=NO_CORR_DENSE_WEIGHT), no_corr_frame=K // 2), _case("terms", K, _seeds(K, 1), iter_weights=ITER_WEIGHTS)]
    for K in (4, 15):
        out += [_case("partials", K, _seeds(K, 1), partials=ct) for ct in PARTIALS]
    out.append(_case("batch", 6, [560, 561, 562]))
    assert len({c["id"] for c in out}) == len(out)
    return out


_window_cache = {}


def window(K, seed, no_corr_frame=None):
    """One instance: synthetic.make_problem(K, 40, seed, background=False, full_res=False), optionally without any correspondence of one frame."""
    key = (K, seed, no_corr_frame)
    if key not in _window_cache:
        from bundletrack_amd import synthetic as S
        pb = S.make_problem(K, 40, seed, background=False, full_res=False)
        corr = pb.corr
        if no_corr_frame is not None:
            corr = corr[(corr["imgIdx_i"] != no_corr_frame) & (corr["imgIdx_j"] != no_corr_frame)]
        _window_cache[key] = (pb, np.ascontiguousarray(corr, SW.ENTRYJ))
    return _window_cache[key]
