"""The product's small device functions, compiled as the product compiles them (tests/hip/btba_probe.hip), against exact references.

- SE(3) (btba_device.hpp), both flavours of division and square root: every output component within A e_oracle + B ulp(scale) of the
  float64 truth (tests/se3_ref.py), e_oracle being the CPU oracle's own error (the oracle is bit-exact with the reference).
- The bit-for-bit claims of the comments: sincosf = sinf / cosf, se3_sqrt(x / 4) = se3_sqrt(x) / 2, v_rcp_f32 / v_sqrt_f32 within 1 ulp,
  huber_weight = the oracle's, mat_inverse and the solve kernels' sixteen-lane inverse within a few ulps.
- The 3x3 approximate SVD and procrustes (btba_svd3.hpp): the device build equal to the host build, bit for bit, and to the
  reference's own procrustesKernel where oracle/_ref/libbtba_ref_ransac.so exists.
- The wave64 reductions: bit-exact against a float32 restatement of the documented DPP / permlane tree.
Worst observed numbers are printed per branch (run with -s)."""
import os

import numpy as np
import pytest

import device_probe
import se3_ref as R
from shared_checks import A_FAST, A_IEEE, B_FAST, B_IEEE, F32, FAST_VS_IEEE_ULPS, _bound, _ulp      # one copy, shared with test_gpu_solve_stages.py

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    import torch
    assert torch.cuda.is_available()
    return device_probe.load()


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda:0")


def _empty(*shape, dtype=None):
    import torch
    return torch.empty(*shape, dtype=dtype or torch.float32, device="cuda:0")


def _call(fn, *args):
    rc = fn(*[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args])
    assert rc == 0, f"{fn.__name__}: hipError {rc}"


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _axes(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ---- SE(3) inputs, labelled by branch ------------------------------------------------------------------------------
def _around(v, ks=(-4, -1, 0, 1, 4)):
    """the float32 v and its neighbours k ulps away"""
    b = int(np.array(v, F32).view(np.uint32))
    return [float(np.array(b + k, np.uint32).view(F32)) for k in ks]


def _se3_cases(seed=3):
    rng = np.random.default_rng(seed)
    groups = [
        ("zero", [0.0], False),
        ("denormal", [1e-40, 1e-30, 1e-20], True),
        ("theta2=1e-8", _around(1e-4), False),                     # exp's series thresholds on theta^2 (one axis: theta^2 = theta * theta)
        ("theta2=1e-6|theta=1e-3", _around(1e-3), False),          # ... and Log's theta > 1e-3
        ("theta=1e-5", _around(1e-5), False),                      # Log's theta > 1e-5
        ("cos=+1/sqrt2", _around(np.pi / 4), False),
        ("cos=-1/sqrt2", _around(3 * np.pi / 4), False),
        ("band", list(10.0 ** rng.uniform(-3, np.log10(3e-2), 200)), True),
        ("random", list(rng.uniform(0, np.pi, 300)), True),
        ("near_pi", list(np.pi - 10.0 ** rng.uniform(-7, -3, 100)), True),
        ("small", list(10.0 ** rng.uniform(-8, -3, 100)), True),
    ]
    labels, rot = [], []
    for name, thetas, random_axis in groups:
        for th in thetas:
            for rep in range(3 if not random_axis else 1):
                ax = _axes(rng, 1)[0] if random_axis else np.eye(3)[rep]
                rot.append(ax * th if random_axis else ax * F32(th))
                labels.append(name)
    for k in range(3):                                              # exactly pi about each axis
        rot.append(np.eye(3)[k] * F32(np.pi)); labels.append("pi")
    rot = np.asarray(rot, F32)
    trans = (_axes(rng, len(rot)) * 10.0 ** rng.uniform(-3, 1, (len(rot), 1))).astype(F32)
    return np.array(labels), rot, trans


def _print_stats(title, stats):
    print(f"\n{title}: worst |dev - truth| / (A e_oracle + B ulp)  [worst ulps of scale]")
    for (name, lab), (r, q) in sorted(stats.items()):
        print(f"  {name:28s} {lab:24s} {r:7.3f}  [{q:9.2f}]")


def _oracle_exp(oracle, rot, trans):
    return np.stack([oracle.pose_to_matrix(rot[k], trans[k]) for k in range(len(rot))])


def _oracle_log(oracle, M):
    out = [oracle.matrix_to_pose(M[k]) for k in range(len(M))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _run_se3(probe, fast, rot, trans, M):
    n = len(rot)
    x = _dev(np.concatenate([rot, trans], 1))
    Md, Rd = _dev(M.reshape(n, 16)), _dev(M[:, :3, :3].reshape(n, 9))
    oM, oR, ox, ow = _empty(n, 16), _empty(n, 9), _empty(n, 6), _empty(n, 3)
    _call(probe.probe_pose_to_matrix, fast, x, oM, n)
    _call(probe.probe_exp_rotation, fast, _dev(rot), oR, n)
    _call(probe.probe_matrix_to_pose, fast, Md, ox, n)
    _call(probe.probe_ln_rotation, fast, Rd, ow, n)
    return oM.cpu().numpy().reshape(n, 4, 4), oR.cpu().numpy().reshape(n, 3, 3), ox.cpu().numpy(), ow.cpu().numpy()


def test_se3_both_flavours_against_float64_truth(probe, oracle):
    labels, rot, trans = _se3_cases()
    n = len(rot)
    M = _oracle_exp(oracle, rot, trans)                             # Log's inputs: fp32 Exp outputs, as the solver's are
    for axis, k in enumerate(np.nonzero(labels == "pi")[0]):        # ... and the exact rotations by pi about each axis
        M[k, :3, :3] = np.diag(np.where(np.eye(3)[axis] > 0, 1.0, -1.0))
    r64, t64 = rot.astype(np.float64), trans.astype(np.float64)
    T_exp = R.pose_to_matrix(r64, t64)
    T_R = R.exp_rotation(r64)
    T_lr, T_lt = R.matrix_to_pose(M.astype(np.float64))
    T_w = R.ln_rotation(M[:, :3, :3].astype(np.float64))
    O_exp_true = _oracle_exp(oracle, rot, trans)
    O_R = _oracle_exp(oracle, rot, np.zeros_like(trans))[:, :3, :3]
    O_lr, O_lt = _oracle_log(oracle, M)
    M0 = M.copy(); M0[:, :3, 3] = 0
    O_w = _oracle_log(oracle, M0)[0]
    tscale = np.linalg.norm(T_exp[:, :3, 3], axis=1)
    outs, failures = {}, []
    for fast, A, B in ((0, A_IEEE, B_IEEE), (1, A_FAST, B_FAST)):
        stats = {}
        dM, dR, dx, dw = outs[fast] = _run_se3(probe, fast, rot, trans, M)
        fl = "fast" if fast else "ieee"
        failures += _bound(stats, labels, f"{fl} pose_to_matrix.R", dM[:, :3, :3], O_exp_true[:, :3, :3], T_exp[:, :3, :3], np.ones(n), A, B)
        failures += _bound(stats, labels, f"{fl} pose_to_matrix.t", dM[:, :3, 3], O_exp_true[:, :3, 3], T_exp[:, :3, 3], tscale, A, B)
        failures += _bound(stats, labels, f"{fl} exp_rotation", dR, O_R, T_R, np.ones(n), A, B)
        failures += _bound(stats, labels, f"{fl} matrix_to_pose.rot", dx[:, :3], O_lr, T_lr, np.linalg.norm(T_lr, axis=1), A, B)
        failures += _bound(stats, labels, f"{fl} matrix_to_pose.trans", dx[:, 3:], O_lt, T_lt, np.linalg.norm(T_lt, axis=1), A, B)
        failures += _bound(stats, labels, f"{fl} ln_rotation", dw, O_w, T_w, np.linalg.norm(T_w, axis=1), A, B)
        _print_stats(f"SE(3) {fl}", stats)
        for arr in (dM, dR, dx, dw):
            assert np.isfinite(arr).all()
        # the last row of Exp is the constant row
        assert np.array_equal(dM[:, 3], np.tile(F32([0, 0, 0, 1]), (n, 1)))
        # denormal angles: the identity rotation to 1 ulp
        den = labels == "denormal"
        assert np.abs(dM[den, :3, :3] - np.eye(3)).max() <= 2.0 ** -24 and np.abs(dR[den] - np.eye(3)).max() <= 2.0 ** -24
        assert np.abs(dw[den] - T_w[den]).max() <= 2.0 ** -24
    assert not failures, failures[:20]
    # fast against IEEE: a few ulps of scale outside the cancellation band
    worst = {}
    pairs = (("pose_to_matrix.R", outs[0][0][:, :3, :3], outs[1][0][:, :3, :3], np.ones(n)),
             ("pose_to_matrix.t", outs[0][0][:, :3, 3], outs[1][0][:, :3, 3], tscale),
             ("exp_rotation", outs[0][1], outs[1][1], np.ones(n)),
             ("matrix_to_pose.rot", outs[0][2][:, :3], outs[1][2][:, :3], np.linalg.norm(T_lr, axis=1)),
             ("matrix_to_pose.trans", outs[0][2][:, 3:], outs[1][2][:, 3:], np.linalg.norm(T_lt, axis=1)),
             ("ln_rotation", outs[0][3], outs[1][3], np.linalg.norm(T_w, axis=1)))
    bad = []
    for name, a, b, scale in pairs:
        u = _ulp(scale)
        while u.ndim < a.ndim:
            u = u[..., None]
        d = (np.abs(a.astype(np.float64) - b) / u).reshape(n, -1).max(1)
        for lab in np.unique(labels):
            worst[(name, lab)] = float(d[labels == lab].max())
        out_band = labels != "band"
        bad += [(name, labels[i], i, float(d[i])) for i in np.nonzero(out_band & ~(d <= FAST_VS_IEEE_ULPS))[0]]
    print("\nSE(3) |fast - ieee| in ulps of scale, worst per branch:")
    for (name, lab), v in sorted(worst.items()):
        print(f"  {name:28s} {lab:24s} {v:9.2f}")
    assert not bad, bad[:20]


def test_se3_nan_in_nan_out(probe):
    nan = np.nan
    rot = F32([[nan, 0, 0], [0.1, 0.2, 0.3], [1e-5, nan, 0]])
    trans = F32([[1, 2, 3], [nan, 0, 0], [0, 0, 0]])
    n = len(rot)
    M = np.zeros((n, 4, 4), F32)
    M[:] = np.eye(4)
    M[0, 0, 0] = nan                                                   # diagonal
    M[1, 1, 2] = nan                                                   # off-diagonal
    M[2, 0, 3] = nan                                                   # translation only
    for fast in (0, 1):
        dM, dR, dx, dw = _run_se3(probe, fast, rot, trans, M)
        assert np.isnan(dM[0, :3]).all() and np.isnan(dR[0]).all() and np.isnan(dR[2]).all() and np.isnan(dM[2, :3]).all()
        assert np.isnan(dM[1, :3, 3]).all() and np.isfinite(dM[1, :3, :3]).all()
        assert np.isnan(dx[0]).all() and np.isnan(dx[1]).all() and np.isnan(dw[0]).all() and np.isnan(dw[1]).all()
        assert np.isnan(dx[2, 3:]).all() and np.array_equal(dx[2, :3], F32([0, 0, 0]))


def test_update_composition(probe, oracle):
    """The solver's update Log(Exp(delta) Exp(x)) at its operating point: delta ~ N(0, 1e-4 ... 1e-2), x random; both flavours within the
    A / B bounds of the float64 truth, and the fast - IEEE difference (what the update phase's default flavour changes) printed."""
    rng = np.random.default_rng(5)
    n = 3000
    sig = 10.0 ** rng.uniform(-4, -2, (n, 1))
    d = (rng.normal(size=(n, 6)) * sig).astype(F32)
    th = np.concatenate([rng.uniform(0, np.pi * 0.999, n - 200), 10.0 ** rng.uniform(-6, -1, 200)])
    x = np.concatenate([_axes(rng, n) * th[:, None], _axes(rng, n) * 10.0 ** rng.uniform(-3, 1, (n, 1))], 1).astype(F32)
    t_rot, t_trans = R.update(d[:, :3].astype(np.float64), d[:, 3:].astype(np.float64), x[:, :3].astype(np.float64), x[:, 3:].astype(np.float64))
    o = [oracle.lie_update(d[k, :3], d[k, 3:], x[k, :3], x[k, 3:]) for k in range(n)]
    o_rot, o_trans = np.stack([v[0] for v in o]), np.stack([v[1] for v in o])
    labels = np.where(np.linalg.norm(t_rot, axis=1) < 3e-2, "theta<3e-2", "theta>=3e-2")
    dd, xd = _dev(d), _dev(x)
    out, failures = {}, []
    for fast, A, B in ((0, A_IEEE, B_IEEE), (1, A_FAST, B_FAST)):
        o_d = _empty(n, 6)
        _call(probe.probe_update, fast, dd, xd, o_d, n)
        out[fast] = o_d.cpu().numpy()
        stats = {}
        fl = "fast" if fast else "ieee"
        failures += _bound(stats, labels, f"{fl} update.rot", out[fast][:, :3], o_rot, t_rot, np.linalg.norm(t_rot, axis=1), A, B)
        failures += _bound(stats, labels, f"{fl} update.trans", out[fast][:, 3:], o_trans, t_trans, np.linalg.norm(t_trans, axis=1), A, B)
        _print_stats(f"update {fl}", stats)
    assert not failures, failures[:20]
    diff = np.abs(out[1].astype(np.float64) - out[0])
    u_r, u_t = _ulp(np.linalg.norm(t_rot, axis=1))[:, None], _ulp(np.linalg.norm(t_trans, axis=1))[:, None]
    print(f"update fast - ieee at the operating point: max |d rot| {diff[:, :3].max():.2e} ({(diff[:, :3] / u_r).max():.1f} ulps of |rot|), "
          f"max |d trans| {diff[:, 3:].max():.2e} ({(diff[:, 3:] / u_t).max():.1f} ulps of |trans|), "
          f"bit-identical in {np.all(out[1] == out[0], axis=1).mean() * 100:.1f} % of the frames")


# ---- exact claims -----------------------------------------------------------------------------------------------------
def _sweep(probe, which, lo=None, n=None, xs=None, n_bad=8):
    import torch
    stat = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    bad = _empty(n_bad)
    if xs is not None:
        xd = _dev(xs)
        _call(probe.probe_sweep, which, 0, len(xs), xd, stat, bad, n_bad)
    else:
        _call(probe.probe_sweep, which, int(lo), int(n), None, stat, bad, n_bad)
    s = stat.cpu().numpy().view(np.uint32)
    count = int(s[0])
    return count, float(s[1:2].view(F32)[0]), bad.cpu().numpy()[:min(count, n_bad)]


def _fbits(v):
    return int(np.array(v, F32).view(np.uint32))


def test_sincosf_equals_sinf_cosf_bit_for_bit(probe):
    lo, hi = _fbits(2.0 ** -4), _fbits(np.pi)
    cnt, _, bad = _sweep(probe, device_probe.SWEEP_SINCOS, lo, hi - lo + 1)
    assert cnt == 0, (cnt, bad)
    rng = np.random.default_rng(9)
    xs = (10.0 ** rng.uniform(-30, 4, 1_000_000) * rng.choice([-1.0, 1.0], 1_000_000)).astype(F32)
    cnt2, _, bad2 = _sweep(probe, device_probe.SWEEP_SINCOS, xs=xs)
    assert cnt2 == 0, (cnt2, bad2)
    print(f"sincosf = sinf / cosf on all {hi - lo + 1} floats in [2^-4, pi] and 1e6 arguments in +-[1e-30, 1e4]")


@pytest.mark.parametrize("fast", [0, 1])
def test_sqrt_commutes_with_scaling_by_four(probe, fast):
    """|-rot / 2| = theta / 2 in matrix_to_pose rests on se3_sqrt(x / 4) = se3_sqrt(x) / 2 (btba_device.hpp's comment)."""
    which = device_probe.SWEEP_SQRT_SCALE_FAST if fast else device_probe.SWEEP_SQRT_SCALE_IEEE
    cnt, _, bad = _sweep(probe, which, _fbits(1.0), 1 << 24)
    assert cnt == 0, (cnt, bad)
    rng = np.random.default_rng(10)
    xs = rng.integers(_fbits(2.0 ** -124), _fbits(np.finfo(F32).max), 1_000_000, dtype=np.uint32).view(F32)
    cnt2, _, bad2 = _sweep(probe, which, xs=xs)
    assert cnt2 == 0, (cnt2, bad2)


def test_fast_rcp_and_sqrt_within_one_ulp(probe):
    c1, e1, b1 = _sweep(probe, device_probe.SWEEP_RCP_ULP, _fbits(1.0), 1 << 23)
    c2, e2, b2 = _sweep(probe, device_probe.SWEEP_SQRT_ULP, _fbits(1.0), 1 << 24)
    print(f"v_rcp_f32 over [1, 2): worst {e1:.3f} ulp; v_sqrt_f32 over [1, 4): worst {e2:.3f} ulp")
    assert c1 == 0 and c2 == 0, (c1, b1, c2, b2)
    assert e1 > 0 and e2 > 0             # the sweeps measured something


def test_huber_weight_bit_exact(probe, oracle):
    e, dl = [], []
    for delta in (0.005, 0.02, 1.0):
        d2 = F32(delta) * F32(delta)
        vals = [0.0, 1e-45, 1e-40, 1.1754942e-38, 1e30, 1e-12, 3.0] + _around(d2, (-4, -3, -2, -1, 0, 1, 2, 3, 4))
        vals += list(10.0 ** np.random.default_rng(12).uniform(-20, 10, 200))
        e += vals
        dl += [delta] * len(vals)
    e, dl = F32(e), F32(dl)
    out = _empty(len(e))
    _call(probe.probe_huber_weight, _dev(e), _dev(dl), out, len(e))
    got = out.cpu().numpy()
    want = F32([oracle.huber_weight(float(a), float(b)) for a, b in zip(e, dl)])
    assert _same_bits(got, want).all(), [(float(a), float(b), g, w) for a, b, g, w in zip(e, dl, got, want) if g != w][:10]


def test_mat_inverse(probe, oracle):
    rng = np.random.default_rng(13)
    labels, rot, trans = _se3_cases(14)
    M = _oracle_exp(oracle, rot, trans)
    n = len(M)
    out = _empty(n, 16)
    _call(probe.probe_mat_inverse, _dev(M.reshape(n, 16)), out, n)
    got = out.cpu().numpy().reshape(n, 4, 4)
    want = np.stack([oracle.mat4_inverse(M[k]) for k in range(n)])
    scale = np.maximum(1.0, np.linalg.norm(trans, axis=1))[:, None, None]
    ulps = np.abs(got.astype(np.float64) - want) / _ulp(scale)
    print(f"mat_inverse on Exp outputs: worst {ulps.max():.2f} ulps of max(1, |t|) from the oracle")
    assert ulps.max() <= 4
    # general 4x4: the error relative to the condition number
    G = rng.normal(size=(2000, 4, 4))
    U, _, Vt = np.linalg.svd(rng.normal(size=(2000, 4, 4)))
    s = 10.0 ** -(rng.uniform(0, 4, (2000, 1)) * np.linspace(0, 1, 4))
    G[1000:] = (U * s[:, None, :] @ Vt)[1000:] * 10.0 ** rng.uniform(-3, 3, (2000, 1, 1))[1000:]
    G = G.astype(F32)
    out = _empty(len(G), 16)
    _call(probe.probe_mat_inverse, _dev(G.reshape(-1, 16)), out, len(G))
    got = out.cpu().numpy().reshape(-1, 4, 4).astype(np.float64)
    inv = np.linalg.inv(G.astype(np.float64))
    kappa = np.linalg.cond(G.astype(np.float64))
    rel = np.abs(got - inv).max((1, 2)) / (np.abs(inv).max((1, 2)) * kappa * 2.0 ** -24)
    print(f"mat_inverse on general 4x4 (cond up to {kappa.max():.1e}): worst max|err| / (cond eps max|inv|) = {rel.max():.2f}")
    assert rel.max() <= 64          # the CPU oracle (the same cofactor formula, no contraction) measures 29 on these inputs


INVERSE16_FAST_ULPS = 6.0           # twice the measured worst, 3.00 (the IEEE flavour measures 3.00 as well)


@pytest.fixture(scope="module")
def exp_inverse_cases(oracle):
    """test_mat_inverse's Exp-output cases: the matrices, the oracle's inverses, max(1, |t|)"""
    _, rot, trans = _se3_cases(14)
    M = _oracle_exp(oracle, rot, trans)
    want = np.stack([oracle.mat4_inverse(m) for m in M])
    return M, want, np.maximum(1.0, np.linalg.norm(trans, axis=1))[:, None, None]


@pytest.mark.parametrize("fast", [0, 1])
def test_inverse_on_sixteen_lanes(probe, exp_inverse_cases, fast):
    """The solve kernels' inverse (btba_solve_phases.hpp: one adjugate entry per lane, sixteen lanes per matrix) against the oracle's
    float4x4::getInverse.  IEEE flavour: test_mat_inverse's bar.  Fast flavour (the kernels' default): 1 / det is v_rcp_f32, 1 ulp off
    in every entry."""
    M, want, scale = exp_inverse_cases
    n = len(M)
    out = _empty(n, 16)
    _call(probe.probe_inverse16, fast, _dev(M.reshape(n, 16)), out, n)
    ulps = np.abs(out.cpu().numpy().reshape(n, 4, 4).astype(np.float64) - want) / _ulp(scale)
    print(f"inverse_on_sixteen_lanes<{'fast' if fast else 'ieee'}> on Exp outputs: worst {ulps.max():.2f} ulps of max(1, |t|) from the oracle")
    assert ulps.max() <= (INVERSE16_FAST_ULPS if fast else 4)


# ---- the 3x3 SVD: device build = host build -----------------------------------------------------------------------
def _rsqrt_inputs():
    rng = np.random.default_rng(11)                                # the inputs of test_oracle_ransac.py::test_rsqrt_is_correctly_rounded
    return np.concatenate([
        (rng.uniform(1.0, 4.0, 2_000_000) * 2.0 ** rng.integers(-30, 30, 2_000_000)).astype(F32),
        (np.arange(1, 4097, dtype=F32) ** 2),
        (1.0 / ((F32(1.0) + np.arange(1, 200001, 7, dtype=np.float64) * 2.0 ** -23 + 2.0 ** -24) ** 2)).astype(F32),
    ])


def test_rsqrt_device_equals_host(probe):
    H = device_probe.svd3_host()
    x = _rsqrt_inputs()
    xd = _dev(x)
    for refined, host in ((0, H.rsqrt_rn_host), (1, H.rsqrt_refined_host)):
        out = _empty(len(x))
        _call(probe.probe_rsqrt, refined, xd, out, len(x))
        got, want = out.cpu().numpy(), np.zeros_like(x)
        host(x.ctypes.data, len(x), want.ctypes.data)
        same = _same_bits(got, want)
        assert same.all(), (refined, int((~same).sum()), x[~same][:5])


def _svd_inputs(rng):
    n = 100_000
    A = rng.normal(size=(n, 3, 3)) * 10.0 ** rng.uniform(-6, 6, (n, 1, 1))
    m = 2000
    u, v, w = rng.normal(size=(m, 3)), rng.normal(size=(m, 3)), rng.normal(size=(m, 3))
    rank1 = u[:, :, None] * v[:, None, :]
    rank2 = rank1 + w[:, :, None] * rng.normal(size=(m, 3))[:, None, :]
    diag = np.stack([np.diag(d) for d in rng.normal(size=(m, 3))])
    Q = np.linalg.qr(rng.normal(size=(m, 3, 3)))[0]
    s = rng.uniform(0.1, 2, (m, 1)) * np.array([1.0, 1.0, 0.5])
    repeated = Q * s[:, None, :] @ np.swapaxes(Q, 1, 2)
    tiny = rng.normal(size=(m, 3, 3)) * 10.0 ** rng.uniform(-11, -5, (m, 1, 1))           # around sqrt(kTiny) / sqrt(kSmall) thresholds
    at_thr = np.tile(np.eye(3), (m, 1, 1)) + 0.0
    at_thr[:, 1, 0] = at_thr[:, 0, 1] = F32(2e-10) * (1 + rng.integers(-4, 5, m) * 2.0 ** -23)
    at_thr[:, 2, 0] = F32(1e-6) * (1 + rng.integers(-4, 5, m) * 2.0 ** -23)
    zero = np.zeros((4, 3, 3))
    return np.concatenate([A, rank1, rank2, diag, repeated, tiny, at_thr, zero]).astype(F32)


def test_svd_device_equals_host(probe):
    H = device_probe.svd3_host()
    A = _svd_inputs(np.random.default_rng(17))
    n = len(A)
    U, s, V = _empty(n, 9), _empty(n, 3), _empty(n, 9)
    _call(probe.probe_svd, _dev(A.reshape(n, 9)), U, s, V, n)
    hU, hs, hV = np.zeros((n, 9), F32), np.zeros((n, 3), F32), np.zeros((n, 9), F32)
    H.svd3_batch_host(A.ctypes.data, n, hU.ctypes.data, hs.ctypes.data, hV.ctypes.data)
    for name, d, h in (("U", U, hU), ("sigma", s, hs), ("V", V, hV)):
        same = _same_bits(d.cpu().numpy(), h).all(1)
        assert same.all(), (name, int((~same).sum()), np.nonzero(~same)[0][:10])


def _procrustes_inputs(rng):
    n3 = 100_000
    P = rng.uniform(-0.1, 0.1, (n3, 3, 3))
    Q = P @ np.linalg.qr(rng.normal(size=(n3, 3, 3)))[0] + rng.uniform(-0.1, 0.1, (n3, 1, 3)) + rng.normal(size=(n3, 3, 3)) * 1e-3
    col = slice(0, 2000)
    t = rng.uniform(-1, 1, (2000, 3, 1))
    P[col] = t * rng.normal(size=(2000, 1, 3)) + rng.normal(size=(2000, 1, 3))      # collinear
    coi = slice(2000, 3000)
    P[coi, 1] = P[coi, 0]                                                            # two coincident points
    P[3000:3100] = P[3000:3100, :1]                                                  # all three coincident
    sets_p, sets_q = list(P), list(Q)
    for k in range(2000):                                                            # n-point sets
        m = int(rng.integers(4, 300))
        p = rng.uniform(-0.1, 0.1, (m, 3))
        sets_p.append(p)
        sets_q.append(p @ np.linalg.qr(rng.normal(size=(3, 3)))[0].T + rng.normal(size=3) * 0.1 + rng.normal(size=(m, 3)) * 0.002)
    off = np.concatenate([[0], np.cumsum([len(p) for p in sets_p])]).astype(np.int32)
    pad = lambda s: np.concatenate([np.concatenate(s), np.ones((off[-1], 1))], 1).astype(F32)
    return pad(sets_p), pad(sets_q), off


def test_procrustes_device_equals_host_and_reference(probe):
    import torch
    from oracle import reference as REF
    H = device_probe.svd3_host()
    src, dst, off = _procrustes_inputs(np.random.default_rng(18))
    n = len(off) - 1
    pose, ok = _empty(n, 16), _empty(n, dtype=torch.int32)
    _call(probe.probe_procrustes, _dev(src), _dev(dst), _dev(off, np.int32), pose, ok, n)
    got, got_ok = pose.cpu().numpy(), ok.cpu().numpy()
    want, want_ok = np.zeros((n, 16), F32), np.zeros(n, np.int32)
    H.procrustes_batch_host(src.ctypes.data, dst.ctypes.data, off.ctypes.data, n, want.ctypes.data, want_ok.ctypes.data)
    same = _same_bits(got, want).all(1) & (got_ok == want_ok)
    assert same.all(), (int((~same).sum()), np.nonzero(~same)[0][:10])
    print(f"procrustes: {n} sets, device = host bit for bit; {int((got_ok == 0).sum())} 'R is not valid'")
    if not os.path.exists(REF.SO_RANSAC):
        return
    idx = np.random.default_rng(19).choice(n, 20_000, replace=False)
    idx = np.union1d(idx, np.arange(0, 3100, 7))
    mism = []
    for i in idx:
        r_ok, r_pose = REF.procrustes(src[off[i]:off[i + 1]], dst[off[i]:off[i + 1]])
        if int(r_ok) != got_ok[i] or (r_ok and not _same_bits(r_pose.reshape(16), got[i]).all()):
            mism.append(int(i))
    print(f"procrustes: device = the reference's procrustesKernel bit for bit on {len(idx) - len(mism)} of {len(idx)} sets")
    assert not mism, mism[:10]


# ---- wave64 reductions: a float32 restatement of the documented tree ------------------------------------------------
_LANE = np.arange(64)
_ROW = _LANE >> 4


def _dpp_add(v, src, rows):
    """v + update_dpp(old = 0, v, ...): lanes of rows outside the row mask receive old = 0"""
    moved = np.where(np.isin(_ROW, rows)[None, :], v[:, src], F32(0))
    return (v + moved).astype(F32)


def _row_butterfly(v):
    allr = (0, 1, 2, 3)
    v = _dpp_add(v, _LANE ^ 1, allr)                                   # quad_perm [1,0,3,2]
    v = _dpp_add(v, _LANE ^ 2, allr)                                   # quad_perm [2,3,0,1]
    v = _dpp_add(v, (_LANE & ~7) | (7 - (_LANE & 7)), allr)            # row_half_mirror
    v = _dpp_add(v, (_LANE & ~15) | (15 - (_LANE & 15)), allr)         # row_mirror
    return v


def restate_wave_sum(x):
    """[n, 64] -> [n, 64] after the six DPP steps of wave_sum_to_lane63"""
    v = _row_butterfly(np.asarray(x, F32))
    v = _dpp_add(v, np.maximum((_LANE & ~15) - 1, 0), (1, 3))          # row_bcast:15 -> rows 1, 3
    v = _dpp_add(v, np.full(64, 31), (2, 3))                           # row_bcast:31 -> rows 2, 3
    return v


def restate_fold(acc):
    """[n, NV, 64] -> [n, NV/4, 64]: permlane32_swap folds value k with k + NV/2, permlane16_swap k with k + NV/4, then the row butterfly;
    row r of q[k] ends with value k + r NV/4"""
    acc = np.asarray(acc, F32)
    n, nv, _ = acc.shape
    Q = nv // 4
    h = (acc[:, :, :32] + acc[:, :, 32:]).astype(F32)                # value j's halves: x[i] + x[i + 32]
    g = (h[:, :, :16] + h[:, :, 16:]).astype(F32)                    # then rows: h[i] + h[i + 16]
    q = np.zeros((n, Q, 64), F32)
    for k in range(Q):
        q[:, k] = np.concatenate([g[:, k + r * Q] for r in range(4)], 1)
        q[:, k] = _row_butterfly(q[:, k])
    return q


def _mixed(rng, shape):
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-8, 8, shape)).astype(F32)


def test_wave_sums_bit_exact(probe):
    rng = np.random.default_rng(20)
    n = 4096
    x = _mixed(rng, (n, 64))
    x[:64] = (rng.normal(size=(64, 64)) * 10.0 ** rng.uniform(-3, 3, (64, 1))).astype(F32)
    o63, oall = _empty(n, 64), _empty(n, 64)
    _call(probe.probe_wave_sum, _dev(x), o63, oall, n)
    o63, oall = o63.cpu().numpy(), oall.cpu().numpy()
    want = restate_wave_sum(x)[:, 63]
    assert _same_bits(o63[:, 63], want).all()                           # only lane 63 is the contract
    assert (_bits(oall) == _bits(oall[:, :1])).all() and _same_bits(oall[:, 0], want).all()
    seq = np.zeros(n, F32)
    for i in range(64):
        seq = (seq + x[:, i]).astype(F32)
    differ = (~_same_bits(seq, want)).mean()
    print(f"wave_sum_to_lane63: {n} waves bit-exact with the restated tree; a sequential sum differs on {differ * 100:.1f} % of them")
    assert differ > 0.5


@pytest.mark.parametrize("nv", [4, 8, 28, 44])
def test_wave_fold_sums_bit_exact_and_layout(probe, nv):
    rng = np.random.default_rng(21 + nv)
    n = 1024
    acc = _mixed(rng, (n, nv, 64))
    out = _empty(n, nv // 4, 64)
    _call(probe.probe_wave_fold, nv, _dev(acc), out, n)
    q = out.cpu().numpy()
    Q = nv // 4
    # the layout contract: every lane of row r of q[k] holds one value, the sum of value k + r NV/4 (by a restated wave tree of that value)
    rows = q.reshape(n, Q, 4, 16)
    assert (_bits(rows) == _bits(rows[..., :1])).all()
    want = restate_fold(acc)
    assert _same_bits(q, want).all(), int((~_same_bits(q, want)).sum())
    total = acc.astype(np.float64).sum(2)
    got_vals = np.stack([rows[:, k, r, 0] for r in range(4) for k in range(Q)], 1)       # value k + r Q at column k + r Q
    err = np.abs(got_vals - total) / np.abs(acc.astype(np.float64)).sum(2)
    assert err.max() < 64 * 2.0 ** -24                                  # ... and it is that value's sum, not another's
    seq = np.zeros((n, nv), F32)
    for i in range(64):
        seq = (seq + acc[:, :, i]).astype(F32)
    assert (~_same_bits(seq, got_vals)).mean() > 0.5


@pytest.mark.parametrize("nv", [28, 44])
def test_block_reduce_store_bit_exact(probe, nv):
    rng = np.random.default_rng(40 + nv)
    n = 512
    acc = _mixed(rng, (n, nv, 256))
    acc_d = _dev(acc)
    outs = []
    for mode in (0, 2):
        o = _empty(n, nv)
        _call(probe.probe_block_reduce, nv, mode, acc_d, o, n)
        outs.append(o.cpu().numpy())
    assert (_bits(outs[0]) == _bits(outs[1])).all()                    # mode 2 (agent-scope store) = mode 0
    per_wave = [restate_fold(acc[:, :, 64 * w: 64 * (w + 1)]) for w in range(4)]
    Q = nv // 4
    rec = [np.stack([p[:, j % Q, 16 * (j // Q)] for j in range(nv)], 1) for p in per_wave]      # lane 0 of row r of q[k] -> value k + r Q
    want = rec[0]
    for w in range(1, 4):
        want = (want + rec[w]).astype(F32)                              # wave order 0 ... 3
    assert _same_bits(outs[0], want).all(), int((~_same_bits(outs[0], want)).sum())
