"""Gate-aware fp64 references for depth pre-processing and normals (numpy only; test infrastructure).

The stage is  erode -> mean-gated bilateral filter -> the same filter again  (process_depth_tile, btba_image.hpp) and then
back-projection + finite-difference normals (depth_to_normals_pixel).  Each output value sits behind HARD decisions, so the
reference states, per decision, whether it is exact or can legitimately fall either way in fp32:

erode_ref            every decision compares fp32 values with fp32 constants (old <= 0.1f drops; d == -inf, d < 0.1f,
                     |d - old| > diff count, the subtraction being one fp32 operation) and one correctly rounded fp32 quotient
                     count / win against ratio.  All restated in fp32: the result is expected BIT FOR BIT.  Out-of-image
                     neighbours are not counted and the denominator stays the full window.  Note the asymmetry: the erode
                     drops old <= 0.1f (0.1f itself goes), the filter accepts c >= 0.1f (0.1f itself counts).

filter_pass_ref      fp64 on the given values.  With u = 2^-24, n = the number of valid taps, win = (2 rf + 1)^2:
  nvalid             c >= 0.1f on fp32 inputs is exact, never flagged.  (In the second pass of the chain the inputs carry the
                     first pass's bar; a tap within that bar of 0.1f flags the pixel.)
  gate               the kernel forms mean = fl(sum of n terms) / n and tests fl|c - mean| <= 0.01f, which accepts the same
                     floats as the double test < 0.01.  A sequential fp32 sum of n non-negative terms is off by at most
                     (n - 1) u sum, the quotient adds u |mean|, the subtraction u |c - mean| <= 2 u 0.01:
                         GATE MARGIN = n u mean + 2 u 0.01   (+ twice the largest input bar among the valid taps)
                     about 1.0e-6 for 25 taps at 0.7 m and 2.0e-6 for 49.  A pixel with a valid tap whose ||c - mean| - 0.01|
                     is inside the margin is BORDERLINE: flagged.
  underflow          a total weight below 2^-151 means every single weight is below half the smallest fp32 denormal (with a
                     factor 2 for exp's own error, ~1e-5 relative there): any fp32 evaluation gets sw = 0 and the pixel is 0,
                     exactly, not flagged.  A pixel whose total weight lies in [2^-151, FLT_MIN * win) is flagged UNDER: fp32
                     weights there are denormal, and an exp that flushes them leaves the pixel 0.  In the chain such a
                     pixel of pass 1 changes what pass 2 reads, so the band is walked as two whole-map references: "keep"
                     (denormal weights are kept: the pixel is inside its bar, which carries the denormal terms below) and
                     "flush" (weights below FLT_MIN are 0: a pixel whose weights all are stays 0).  An implementation has to
                     agree with one of the two everywhere.  Scenes that are not about underflow must have no band pixels.
  bar                first-order bound of the kernel's own sequence  sum += w c, sw += w, o = sum / sw  around the fp64 value:
                         (2 n_g + 3) u |o|                       n_g gated taps: product + n_g - 1 additions on each sum (all
                                                                  terms non-negative, so relative), one division
                       + eps_w * spread                          a weight's relative error moves o by at most that times
                                                                  spread = max c - min c over the gated taps (<= 0.02, which is
                                                                  why the stage is well conditioned); eps_w = the largest
                                                                  over the taps of  2^-23 (2 + 1.16 |x|) + 8 u |x|:  __expf's
                                                                  documented error at argument x, and the argument's own
                                                                  rounding (3 u on the spatial term, 7 u on the range term
                                                                  with 1 / (2 sr^2) multiplied, u on the difference)
                       + n_g 2^-149 (1 + |o|) / sw                absolute rounding of denormal weights and products
                       + min(2 n_g FLT_MIN / sw, 1) spread        weights below FLT_MIN that an exp may flush (a re-weighting
                                                                  stays inside the taps' range, hence the min)
                     The last two vanish unless sw is tiny.  FMA contraction only removes roundings.
  second pass        the chain hands pass 2 the pass-1 value with its bar b.  A convex combination passes on at most
                     max b over the gated taps; the weights move by  d x = |centre - c| / sr^2 * (b_centre + b_c)  and that
                     moves o by at most  max|centre - c| / sr^2 * (b_centre + max b) * spread.  With a gated centre
                     |centre - c| <= 0.02, so the gain on b is at most 2 * 0.02 * 0.02 / sr^2 = 8e-4 / sr^2: 8 at
                     sr = 0.01 and nothing at the tracker's 1e5.  The per-pixel value is used, not this ceiling.

process_ref          the chain.  The erode has no borderline pixels.  Pixels flagged in pass 1 (either way) contaminate the
                     pass-2 pixels within rf: those are flagged too.

backproject_ref      stage A of the normals, operation for operation in fp32 (contraction is off in the kernel):
                     ((Ki0 (x d) + Ki1 (y d)) + Ki2 d) + Ki3 d per row, zeros when !((double)d >= 0.1).  BIT FOR BIT.
normals_ref          stage B from those fp32 points, in fp64.  Validity (z >= 0.1f) and fl|z' - z| <= 0.02f are fp32 decisions
                     restated exactly, so the zero pattern is expected identical with no allowance.  Flagged: only pixels
                     whose orientation dot product is within its own rounding bound of 0, and pixels with l at 0.
                     Bar per component k of the unit normal, with n = xd x yd, n_k = a b - c d on fp32 differences (u each),
                     gamma = 4 u (three factors of 1 + u per product, one subtraction):
                         e_k = gamma (|a b| + |c d|) / l,  E = |e|_2 bounds the relative error of l from its components,
                         bar_k = e_k + |n_k / l| (E + 4 u)       4 u: the squares, two additions, sqrt and the division
                     It grows where the cross product cancels; it is not a constant.
                     Also returned: which difference scheme each axis took (CENTRAL, PLUS, MINUS, NONE; -1 = not evaluated).

check_filter / check_normals are the assertions of the GPU tests, applied to any implementation's output: the fp32 CPU
oracle (its worst error / bar is the measured floor), the device, and the planted faults of test_image_ref.py."""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24
C01 = float(F32(0.1))                       # the fp32 constant 0.1f
FLT_MIN = float(np.finfo(np.float32).tiny)
DEN_MIN = 2.0 ** -149
ZERO_SW = 2.0 ** -151                       # a total weight below this: every fp32 weight rounds (or flushes) to 0
STEP = 0.09                                 # the scene's box: see scene()
CENTRAL, PLUS, MINUS, NONE = 0, 1, 2, 3

TRACKER = dict(erode_radius=1, erode_diff=0.001, erode_ratio=0.8, bf_radius=2, sigma_d=2.0, sigma_r=100000.0)
GENERIC = dict(erode_radius=2, erode_diff=0.05, erode_ratio=0.5, bf_radius=3, sigma_d=1.5, sigma_r=0.01)


def _window(a, r, fill=0.0):
    """[(2r+1)^2, H, W] taps of a (x offset outer, y inner, as the kernels nest them), the same for the in-image mask, and
    the (dx, dy) list."""
    H, W = a.shape
    p = np.full((H + 2 * r, W + 2 * r), fill, a.dtype)
    p[r:r + H, r:r + W] = a
    m = np.zeros((H + 2 * r, W + 2 * r), bool)
    m[r:r + H, r:r + W] = True
    offs = [(dx, dy) for dx in range(-r, r + 1) for dy in range(-r, r + 1)]
    taps = np.stack([p[r + dy:r + dy + H, r + dx:r + dx + W] for dx, dy in offs])
    inim = np.stack([m[r + dy:r + dy + H, r + dx:r + dx + W] for dx, dy in offs])
    return taps, inim, offs


def dilate(mask, r):
    """mask OR-ed over the (2r+1)^2 window (in-image taps only)."""
    taps, inim, _ = _window(np.asarray(mask, bool), r, False)
    return (taps & inim).any(0)


def erode_ref(d32, re, diff, ratio, _fault=None):
    """erodeDepthMapDevice in fp32, exact.  _fault (planted faults only): 'in_image_denominator'."""
    d = np.ascontiguousarray(d32, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        taps, inim, _ = _window(d, re)
        bad = inim & ((taps == F32(-np.inf)) | (taps < F32(0.1)) | (np.abs(taps - d[None]) > F32(diff)))
        count = bad.sum(0)
        win = np.full(d.shape, (2 * re + 1) ** 2)
        if _fault == "in_image_denominator":
            win = inim.sum(0)
        frac = count.astype(F32) / win.astype(F32)
        keep = ~(d <= F32(0.1)) & ~(frac >= F32(ratio))
    return np.where(keep, d, F32(0.0)).astype(F32)


def filter_pass_ref(d, rf, sigma_d, sigma_r, bar_in=None, flag_in=None, under="flag", _fault=None):
    """One pass of gaussFilterDepthMapDevice in fp64.  d: fp32 values (or the fp64 values of a previous pass with their bar and
    flags).  Returns (value, flag, bar, under): fp64 [H,W], bool, fp64, bool.  under="flag": flag includes under.  "keep": an
    underflow-band pixel is an ordinary pixel (its bar carries the denormal terms).  "flush": the model of an exp that returns 0
    below FLT_MIN -- such weights are 0, so a pixel whose weights all are stays 0, exactly.
    _fault (planted faults only): 'gate_on_centre', 'no_range_term'."""
    d = np.asarray(d).astype(np.float64)
    H, W = d.shape
    sd, sr = float(F32(sigma_d)), float(F32(sigma_r))
    b_in = np.zeros((H, W)) if bar_in is None else np.asarray(bar_in, np.float64)
    win = (2 * rf + 1) ** 2
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        taps, inim, offs = _window(d, rf)
        tbar, _, _ = _window(b_in, rf)
        valid = inim & (taps >= C01)
        flag = (inim & (tbar > 0) & (np.abs(taps - C01) <= tbar)).any(0)           # a pass-2 validity decision inside its input's bar
        n = valid.sum(0)
        mean = np.where(valid, taps, 0.0).sum(0) / np.maximum(n, 1)
        vbar = np.where(valid, tbar, 0.0).max(0)
        ref_pt = d[None] if _fault == "gate_on_centre" else mean[None]
        dev = np.abs(taps - ref_pt)
        margin = n * U * mean + 2 * U * 0.01 + 2 * vbar
        gated = valid & (dev < 0.01)
        fin = np.isfinite(mean)
        flag |= (valid & fin[None] & (np.abs(dev - 0.01) <= margin[None])).any(0)
        r2 = np.array([dx * dx + dy * dy for dx, dy in offs], np.float64)[:, None, None]
        rng = (d[None] - taps) ** 2 / (2.0 * sr * sr)
        if _fault == "no_range_term":
            rng = np.zeros_like(rng)
        x = np.where(gated, -r2 / (2.0 * sd * sd) - rng, 0.0)
        w = np.where(gated, np.exp(x), 0.0)
        if under == "flush":
            w = np.where(w < FLT_MIN, 0.0, w)
        sw = w.sum(0)
        sm = (w * np.where(gated, taps, 0.0)).sum(0)
        live = sw >= ZERO_SW                                                         # NaN (a NaN centre) is not >=: the pixel stays 0
        sw1 = np.where(live, sw, 1.0)
        val = np.where(live, sm / sw1, 0.0)
        ng = gated.sum(0)
        cmax = np.where(gated, taps, -np.inf).max(0)
        cmin = np.where(gated, taps, np.inf).min(0)
        spread = np.where(ng > 0, cmax - cmin, 0.0)
        ax = np.where(gated, np.abs(x), 0.0)
        eps_w = (2.0 ** -23 * (2.0 + 1.16 * ax) + 8 * U * ax).max(0)
        bar = (2 * ng + 3) * U * np.abs(val) + eps_w * spread + ng * DEN_MIN * (1 + np.abs(val)) / sw1 + np.minimum(2 * ng * FLT_MIN / sw1, 1.0) * spread
        gbar = np.where(gated, tbar, 0.0).max(0)
        reach = np.where(gated, np.abs(d[None] - taps), 0.0).max(0)
        bar = bar + gbar + reach / (sr * sr) * (b_in + gbar) * spread
        bar = np.where(live, bar, 0.0)
        band = live & (sw < FLT_MIN * win)
    if under == "flag":
        flag |= band
    if flag_in is not None:
        flag |= dilate(flag_in, rf)
    return val, flag, bar, band


def process_ref(d32, erode_radius=1, erode_diff=0.001, erode_ratio=0.8, bf_radius=2, sigma_d=2.0, sigma_r=100000.0, under="flag", _fault=None):
    """Frame::processDepth.  Returns a dict: eroded (fp32, exact), pass1 / value (fp64), flag, bar, under (of the final pass),
    valid = value != 0; the excluded pixels are flag.  under: see filter_pass_ref; under1 = pass 1's band.
    _fault (planted faults only): 'one_pass' or one of the stages' faults."""
    e = erode_ref(d32, erode_radius, erode_diff, erode_ratio, _fault=_fault)
    v1, f1, b1, u1 = filter_pass_ref(e, bf_radius, sigma_d, sigma_r, under=under, _fault=_fault)
    if _fault == "one_pass":
        v2, f2, b2, u2 = v1, f1, b1, u1
    else:
        v2, f2, b2, u2 = filter_pass_ref(v1, bf_radius, sigma_d, sigma_r, bar_in=b1, flag_in=f1, under=under, _fault=_fault)
    return dict(eroded=e, pass1=v1, flag1=f1, under1=u1, value=v2, flag=f2, bar=b2, under=u2, valid=v2 != 0)


def tiled_process(d32, params, halo):
    """The chain computed tile by tile (32 x 8) from a window that reaches `halo` pixels past the tile, everything beyond it
    treated as outside the image: with halo = erode_radius + 2 bf_radius this is process_ref's value; with one less it is the
    planted fault 'short halo'."""
    d32 = np.ascontiguousarray(d32, F32)
    H, W = d32.shape
    out = np.zeros((H, W))
    for y0 in range(0, H, 8):
        for x0 in range(0, W, 32):
            ya, yb, xa, xb = max(y0 - halo, 0), min(y0 + 8 + halo, H), max(x0 - halo, 0), min(x0 + 32 + halo, W)
            v = process_ref(d32[ya:yb, xa:xb], **params)["value"]
            y1, x1 = min(y0 + 8, H), min(x0 + 32, W)
            out[y0:y1, x0:x1] = v[y0 - ya:y1 - ya, x0 - xa:x1 - xa]
    return out


def check_filter(got, ref, margin=1.0):
    """The GPU test's assertions on a processed depth map `got` against process_ref's dict.  Returns a dict of figures and
    `failures`, a list of strings (empty = pass):
      * got is finite everywhere;
      * outside flagged pixels the zero pattern is identical and |got - ref| <= margin * bar; flagged pixels are not compared."""
    got = np.asarray(got)
    val, bar, flag, under = ref["value"], ref["bar"], ref["flag"], ref["under"]
    fails = []
    if not np.isfinite(got).all():
        fails.append(f"{int((~np.isfinite(got)).sum())} non-finite outputs")
    g = np.where(np.isfinite(got), got, 0.0).astype(np.float64)
    clean = ~flag
    zp = clean & ((g == 0) != (val == 0))
    if zp.any():
        fails.append(f"{int(zp.sum())} zero-pattern mismatches outside flagged pixels, first at (y, x) = {tuple(np.argwhere(zp)[0])}")
    err = np.abs(g - val)
    cmp_ = clean & ~zp & (val != 0)
    ratio = np.where(cmp_, err / np.where(bar > 0, bar, 1.0), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > margin:
        y, x = np.unravel_index(int(ratio.argmax()), ratio.shape)
        fails.append(f"|got - ref| = {err[y, x]:.3e} is {worst:.2f} bars (bar {bar[y, x]:.3e}) at (y, x) = ({y}, {x})")
    return dict(failures=fails, worst=worst, excluded=int(flag.sum()), valid=int(ref["valid"].sum()), compared=int(cmp_.sum()),
                bar_max=float(bar[cmp_].max()) if cmp_.any() else 0.0, under=int(under.sum()), under_zero=int((under & (g == 0)).sum()))


# ---- normals ---------------------------------------------------------------------------------------------------------
def mat4_inverse_ref(K):
    """The generic cofactor inverse of the 4 x 4 embedding of K in fp32 (scaled_intrinsics, btba_host_common.hpp)."""
    K = np.asarray(K, F32).reshape(3, 3)
    m = np.zeros((4, 4), F32)
    m[:3, :3] = K
    m[3, 3] = 1
    adj = np.zeros((4, 4), F32)

    def minor(rr, cc):
        a = lambda i, j: m[rr[i], cc[j]]
        return F32(F32(F32(a(0, 0) * F32(F32(a(1, 1) * a(2, 2)) - F32(a(1, 2) * a(2, 1))))
                       - F32(a(0, 1) * F32(F32(a(1, 0) * a(2, 2)) - F32(a(1, 2) * a(2, 0)))))
                   + F32(a(0, 2) * F32(F32(a(1, 0) * a(2, 1)) - F32(a(1, 1) * a(2, 0)))))

    for r in range(4):
        for c in range(4):
            mn = minor([k for k in range(4) if k != r], [k for k in range(4) if k != c])
            adj[c, r] = -mn if (r + c) & 1 else mn
    det = F32(F32(F32(m[0, 0] * adj[0, 0]) + F32(m[0, 1] * adj[1, 0])) + F32(m[0, 2] * adj[2, 0])) + F32(m[0, 3] * adj[3, 0])
    return (adj * F32(F32(1.0) / F32(det))).astype(F32)


def backproject_ref(depth32, Kinv):
    """Stage A: [H,W,4] fp32 camera-space points (x, y, z, 1), zeros where !((double)d >= 0.1).  Exact."""
    d = np.ascontiguousarray(depth32, F32)
    H, W = d.shape
    Ki = np.asarray(Kinv, F32).reshape(16)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = d.astype(np.float64) >= 0.1
        vx = np.arange(W, dtype=F32)[None, :] * d
        vy = np.arange(H, dtype=F32)[:, None] * d
        out = np.zeros((H, W, 4), F32)
        for k, row in enumerate((0, 1, 3)):
            a = Ki[4 * row:4 * row + 4]
            out[..., k] = ((a[0] * vx + a[1] * vy) + a[2] * d) + a[3] * d
        out[..., 3] = 1
    out[~ok] = 0
    return out


def normals_ref(points32, depth32=None, _fault=None):
    """Stage B.  Returns a dict: normals [H,W,4] fp64, bar [H,W,3], flag [H,W] (orientation or l undecidable), sx / sy the scheme
    the (y +- 1) and (x +- 1) differences took, flips (orientation reversed), valid (a normal was written).
    _fault (planted faults only): 'opposite_neighbour', 'no_flip'."""
    P = np.ascontiguousarray(points32, F32)
    H, W = P.shape[:2]
    z = P[..., 2]
    if depth32 is not None:
        assert np.array_equal(z[np.asarray(depth32, np.float64) >= 0.1], np.asarray(depth32, F32)[np.asarray(depth32, np.float64) >= 0.1])
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = True
    with np.errstate(invalid="ignore"):
        live = inner & ~(z < F32(0.1))

    def shifted(dy, dx):
        out = np.zeros_like(P)
        ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
        xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
        out[yd, xd] = P[ys, xs]
        return out

    def near(Q):                                          # fp32: z' >= 0.1f and fl|z' - z| <= 0.02f
        with np.errstate(invalid="ignore"):
            return (Q[..., 2] >= F32(0.1)) & (np.abs(Q[..., 2] - z) <= F32(0.02))

    def scheme(Pl, Mi):
        p, m = near(Pl), near(Mi)
        s = np.where(p & m, CENTRAL, np.where(p, PLUS, np.where(m, MINUS, NONE)))
        C64, P64, M64 = P[..., :3].astype(np.float64), Pl[..., :3].astype(np.float64), Mi[..., :3].astype(np.float64)
        if _fault == "opposite_neighbour":
            P64, M64 = np.where((s == CENTRAL)[..., None], P64, M64), np.where((s == CENTRAL)[..., None], M64, P64)
        d = np.where((s == CENTRAL)[..., None], P64 - M64, np.where((s == PLUS)[..., None], P64 - C64, M64 - C64))
        return np.where(live, s, -1), d

    sx, xd = scheme(shifted(1, 0), shifted(-1, 0))        # PC, MC
    sy, yd = scheme(shifted(0, 1), shifted(0, -1))        # CP, CM
    ok = live & (sx != NONE) & (sy != NONE)
    g = 4 * U
    ab = np.stack([xd[..., 1] * yd[..., 2], xd[..., 2] * yd[..., 0], xd[..., 0] * yd[..., 1]], -1)
    cd = np.stack([xd[..., 2] * yd[..., 1], xd[..., 0] * yd[..., 2], xd[..., 1] * yd[..., 0]], -1)
    n = ab - cd
    l = np.sqrt((n * n).sum(-1))
    l0 = ok & ~(l > 1e-30)
    l1 = np.where(l > 1e-30, l, 1.0)[..., None]
    nh = n / l1
    e = g * (np.abs(ab) + np.abs(cd)) / l1
    bar = e + np.abs(nh) * (np.sqrt((e * e).sum(-1))[..., None] + 4 * U)
    C64 = P[..., :3].astype(np.float64)
    dot = -(nh * C64).sum(-1)
    dot_bar = (np.abs(nh) * np.abs(C64)).sum(-1) * 3 * U + (bar * np.abs(C64)).sum(-1)
    flips = ok & (dot < 0)
    if _fault != "no_flip":
        nh = np.where(flips[..., None], -nh, nh)
    valid = ok & ~l0
    out = np.zeros((H, W, 4))
    out[..., :3] = np.where(valid[..., None], nh, 0.0)
    flag = l0 | (ok & (np.abs(dot) <= dot_bar))
    return dict(normals=out, bar=np.where(valid[..., None], bar, 0.0), flag=flag, l_flag=l0, sx=sx, sy=sy, flips=flips, valid=valid)


def check_normals(got, ref, margin=1.0):
    """The GPU test's assertions on a normal map: the zero pattern identical everywhere (but where l is at 0), w = 0, and
    |got - ref| <= margin * bar per component outside flagged pixels."""
    got = np.asarray(got)
    fails = []
    if not np.isfinite(got).all():
        fails.append("non-finite normals")
    g = np.nan_to_num(got.astype(np.float64))
    if (g[..., 3] != 0).any():
        fails.append("w != 0")
    gz = (g[..., :3] != 0).any(-1)
    zp = (gz != ref["valid"]) & ~ref["l_flag"]
    if zp.any():
        fails.append(f"{int(zp.sum())} zero-pattern mismatches, first at (y, x) = {tuple(np.argwhere(zp)[0])}")
    cmp_ = ref["valid"] & ~ref["flag"] & ~zp
    err = np.abs(g[..., :3] - ref["normals"][..., :3])
    ratio = np.where(cmp_[..., None], err / np.where(ref["bar"] > 0, ref["bar"], 1.0), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > margin:
        y, x, k = np.unravel_index(int(ratio.argmax()), ratio.shape)
        fails.append(f"|got - ref| = {err[y, x, k]:.3e} is {worst:.2f} bars (bar {ref['bar'][y, x, k]:.3e}) at (y, x, k) = ({y}, {x}, {k})")
    return dict(failures=fails, worst=worst, excluded=int(ref["flag"].sum()), valid=int(ref["valid"].sum()), compared=int(cmp_.sum()),
                bar_max=float(ref["bar"][cmp_].max()) if cmp_.any() else 0.0, bar_min=float(ref["bar"][cmp_].min()) if cmp_.any() else 0.0)


# ---- inputs ----------------------------------------------------------------------------------------------------------
FILTER_SHAPES_SMALL = [(1, 1), (1, 9), (40, 1), (31, 7), (32, 8), (33, 9)]                    # (W, H)
FILTER_SHAPES_H5 = [(68, 20), (69, 21)]               # 32 x 8 tiles, halo 5: no INTERIOR workgroup / exactly one
FILTER_SHAPES_H8 = [(71, 23), (72, 24)]               # the same for halo 8
FILTER_SHAPE_BIG = (101, 37)
NORMALS_SHAPES = [(1, 1), (2, 2), (3, 3), (63, 3), (64, 4), (65, 5), (129, 6)]                # (W, H); the grid is 64 x 4
NORMALS_PHASES = 5


def interior_workgroups(W, H, h):
    """How many 32 x 8 workgroups have their whole LDS tile inside the image (k_process_depth's `interior`)."""
    return sum(1 for by in range((H + 7) // 8) for bx in range((W + 31) // 32)
               if bx * 32 - h >= 0 and by * 8 - h >= 0 and bx * 32 + 32 + h <= W and by * 8 + 8 + h <= H)


def plane(W, H, seed=0, noise=3e-4):
    """Slope ~1e-4 per pixel, a weak quadratic, uniform noise: nothing here is eroded or gated out."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = 0.69 + 1.0e-4 * xs + 0.7e-4 * ys + 2e-7 * (xs - W / 2) ** 2
    return (z + np.random.default_rng(seed).uniform(-noise, noise, size=z.shape)).astype(F32)


@functools.lru_cache(maxsize=None)
def scene(W, H, h, seed=0):
    """The constructed filter scene for halo h (the lattices are wider than any window of that chain): plane(), a box raised by
    0.073 (k * 0.073 / 25 and k * 0.073 / 49 stay >= 4e-4 from the 0.01 gate for every integer k), isolated holes, isolated
    +0.15 flyers (never gated) and +0.005 flyers (eroded at diff 0.001, gated when they survive: the probe that sees a short
    halo or a wrong erode denominator), at tile seams, at distance h and h + 1 from them and on the live rim; one block hole;
    dead rows and columns at the rim.  Read-only."""
    d = plane(W, H, seed).copy()
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rim = W >= 40 and H >= 16
    dead = (((ys < 2) & (H >= 36)) | (xs >= W - 3)) if rim else np.zeros((H, W), bool)      # dead rows only where the box stays clear of them
    box = np.zeros((H, W), bool)
    if H >= 36:
        box[H // 3:2 * H // 3, 6:6 + max(W // 6, 8)] = True               # corners: windows with 1 .. 6 box taps
    elif W >= 16:
        box[:, 6:6 + max(W // 6, 8)] = True                      # too low for corners clear of the rim: a band, edges only
    d[box] += F32(STEP)
    # no defect where a window could hold both sides of the step (there n has to stay the full window's, see above), none within
    # reach of the image's or the dead rim's edge but the ones placed there on purpose
    keep_off = dilate(box, h + 1) & dilate(~box, h + 1)
    inner = ~dilate(dead, h) & (xs >= h) & (xs < W - h) & (ys >= h) & (ys < H - h)
    # the small flyers first (an eroded flyer is a hole, which the filters carry 2 bf_radius = h, h - 1 or h - 2 far: those are the
    # distances at which a tile needs its whole halo to take the erode's decision on the flyer rightly), then the lattices around them
    small = [(64 - h, 5), (64 - h + 1, 11), (64 - h + 2, 19), (40, 16 - h), (46, 16 - h + 1), (52, 16 - h + 2), (63 + h, 15 + h), (31, 7), (32, 8),
             (0, H // 2), (0, H - 1), (W // 2, H - 1), (W // 2 + 5, 3)]
    smallm = np.zeros((H, W), bool)
    for x, y in small:
        if 0 <= x < W and 0 <= y < H and not keep_off[y, x] and not dead[y, x] and not dilate(smallm, 2)[y, x]:
            smallm[y, x] = True
    if h >= 7 and H >= 36:
        # a column of four at distance h - 2 from the seam x = 64: an erode of radius 2 takes each (21 or 22 of 25 differ) unless a tile
        # misses the column at distance h (16 or 17 of 25); four kept flyers move the tile's edge by more than a 7 x 7 window's bar
        smallm[26:30, 64 - h + 2] = True
    d[smallm] += F32(0.005)
    sp = h + 5
    clear = ~keep_off & ~dilate(smallm, 2)                     # (out of the small flyers' erode windows)
    holes = (xs % sp == 2) & (ys % sp == 1) & clear & ~dead
    big = (xs % sp == 2 + sp // 2) & (ys % sp == 1 + sp // 2) & clear & inner
    d[holes] = 0
    d[big] += F32(0.15)
    taken = holes | big | smallm
    if rim:
        blk = (ys >= H - 7) & (ys < H - 4) & (xs >= W - 16) & (xs < W - 12)
        if not (dilate(blk, h) & (box | taken)).any():
            d[blk] = 0
    d[dead] = 0
    d.setflags(write=False)
    return d


def intrinsics(W, H):
    return np.array([[120.0, 0.25, (W - 1) / 2.0], [0.0, 118.0, (H - 1) / 2.0], [0.0, 0.0, 1.0]], F32)


@functools.lru_cache(maxsize=None)
def normals_scene(W, H, phase=0):
    """A plane whose interior pixels at x = 1 (mod 3), y = 1 (mod 4) each get one of the 4 x 4 (scheme, scheme) combinations by
    spoiling the matching neighbours, with a hole or (alternating) a z step of 0.05 > 0.02; the combination walks with the
    pixel's index and `phase`.  Read-only."""
    d = plane(W, H, 100 + phase, noise=1e-4).copy()
    spoil = lambda x, y, k: d.__setitem__((y, x), F32(0.0) if k % 2 else d[y, x] + F32(0.05))
    i = 0
    for y in range(1, H - 1, 4):
        for x in range(1, W - 1, 3):
            c = (i * 7 + phase * 3 + W) % 16
            sx, sy = c // 4, c % 4
            k = i + phase
            if sx in (PLUS, NONE): spoil(x, y - 1, k)                # MC
            if sx in (MINUS, NONE): spoil(x, y + 1, k + 1)           # PC
            if sy in (PLUS, NONE): spoil(x - 1, y, k + 1)            # CM
            if sy in (MINUS, NONE): spoil(x + 1, y, k)               # CP
            i += 1
    d.setflags(write=False)
    return d


def scheme_census(refs):
    """{(sx, sy): pixels} over normals_ref dicts, for evaluated pixels."""
    out = {}
    for r in refs:
        m = r["sx"] >= 0
        for a, b in zip(r["sx"][m], r["sy"][m]):
            out[(int(a), int(b))] = out.get((int(a), int(b)), 0) + 1
    return out


# ---- the filter cases both test files walk -------------------------------------------------------------------------------------------------
PARAM_SETS = {
    "tracker": TRACKER,                                              # <1, 2>, unrolled: only as the full chain
    "generic": GENERIC,                                              # <-1, -1> from here on
    "radii_2_3": dict(TRACKER, erode_radius=2, bf_radius=3),
    "radii_1_3": dict(TRACKER, erode_radius=1, bf_radius=3),
    "filters_alone_r2": dict(TRACKER, erode_radius=0),               # the erode only zeroes !(d > 0.1f)
    "filters_alone_r3": dict(GENERIC, erode_radius=0),
    "erode_alone_r1": dict(TRACKER, bf_radius=0),                    # 1 x 1 filter windows: the passes are the identity
    "erode_alone_r2": dict(GENERIC, bf_radius=0, erode_diff=0.001),
}
UNDERFLOW = dict(TRACKER, sigma_r=0.05)
FILTER_SHAPES = FILTER_SHAPES_SMALL + FILTER_SHAPES_H5 + FILTER_SHAPES_H8 + [FILTER_SHAPE_BIG]
MIN_VALID = 200            # per case with at least 900 pixels; the shapes below that (1 x 1 .. 33 x 9) cannot hold 200 and keep the 5 % cap only


def halo(p):
    return p["erode_radius"] + 2 * p["bf_radius"]


@functools.lru_cache(maxsize=None)
def filter_case(name, W, H, codes=False):
    """(input, ref): the scene for that parameter set's halo as float32 metres, or as uint16 millimetre codes (the reference then
    runs on their decode), and process_ref of it."""
    import ingest_ref
    p = PARAM_SETS[name]
    d = scene(W, H, halo(p))
    if codes:
        c = ingest_ref.metres_to_codes(d)
        c.setflags(write=False)
        return c, process_ref(ingest_ref.decode_depth(c), **p)
    return d, process_ref(d, **p)


def cap_failures(ref, n_pixels):
    """The condition on a case's INPUT: excluded pixels are at most 5 % of its valid output pixels, and a case that can hold them
    keeps at least MIN_VALID valid output pixels."""
    valid, excl = int(ref["valid"].sum()), int(ref["flag"].sum())
    out = []
    if excl > 0.05 * valid:
        out.append(f"{excl} excluded pixels > 5 % of {valid} valid")
    if n_pixels >= 900 and valid < MIN_VALID:
        out.append(f"only {valid} valid output pixels")
    return out


IMPULSE_PARAMS = ("tracker", "radii_2_3", "filters_alone_r2")        # erodes whose decision on a small flyer a tile's halo can spoil


def impulse_positions(p, W=FILTER_SHAPE_BIG[0], H=FILTER_SHAPE_BIG[1]):
    """(x, y) of the defect: the four pixels around the tile corner (32, 8); at distance h (the outermost halo cell of the next
    tile) and h + 1 (just outside it) from the seams x = 64 and y = 16, from either side; and the same at 2 bf_radius and
    2 bf_radius + 1, which is how far the two filter passes carry a defect that the erode does not spread."""
    pos = [(31, 7), (32, 7), (31, 8), (32, 8)]
    for dist in sorted({halo(p), halo(p) + 1, 2 * p["bf_radius"], 2 * p["bf_radius"] + 1}):
        pos += [(64 - dist, 16 - dist), (63 + dist, 15 + dist)]
    assert all(0 <= x < W and 0 <= y < H for x, y in pos)
    return pos


def ramp(W=FILTER_SHAPE_BIG[0], H=FILTER_SHAPE_BIG[1]):
    """The impulse cases' flat surface: 4e-4 per pixel along x, 3e-4 along y, no noise -- steep enough that a tap taken away moves a
    filtered value by far more than its bar, flat enough that no erode here (diff 0.001) and no gate touches it."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return (0.69 + 4e-4 * xs + 3e-4 * ys).astype(F32)


def impulse_input(kind, x, y, W=FILTER_SHAPE_BIG[0], H=FILTER_SHAPE_BIG[1]):
    """ramp() with one defect: a hole, or a flyer of +0.005 (small enough to pass the mean gate where it survives the erode, so
    that its reach is the chain's full h)."""
    d = ramp(W, H)
    d[y, x] = 0 if kind == "hole" else d[y, x] + F32(0.005)
    return d


def support_ref(ref_defect, ref_flat):
    """(changed, same, ambiguous) of the reference: bit-equal values are `same` (the defect is out of that pixel's reach: an
    implementation's two outputs there are bit-equal too); a change beyond both bars is `changed` (its outputs must differ); in between
    (the outer ring, where two passes have thinned the change out) either may happen."""
    diff = np.abs(ref_defect["value"] - ref_flat["value"])
    same = ref_defect["value"] == ref_flat["value"]
    changed = diff > ref_defect["bar"] + ref_flat["bar"]
    return changed, same, ~same & ~changed


EDGE_VALUES = [("0.1f", F32(0.1)), ("0.1f+", np.nextafter(F32(0.1), F32(1))), ("0.1f-", np.nextafter(F32(0.1), F32(0))), ("0", F32(0.0)),
               ("-0", F32(-0.0)), ("denormal", F32(1e-41)), ("negative", F32(-0.5)), ("nan", F32(np.nan)), ("+inf", F32(np.inf)),
               ("-inf", F32(-np.inf)), ("1e30", F32(1e30))]
EDGE_SPACING = 9           # > the largest halo walked (8)


def edge_value_input():
    """One 45 x 36 plane with each special value once, on a lattice of spacing 9 from (4, 4).  Returns (map, {name: (x, y)})."""
    W, H = 4 * EDGE_SPACING + 9, 3 * EDGE_SPACING + 9
    d = plane(W, H, 11).copy()
    where = {}
    for i, (name, v) in enumerate(EDGE_VALUES):
        x, y = 4 + EDGE_SPACING * (i % 4), 4 + EDGE_SPACING * (i // 4)
        d[y, x] = v
        where[name] = (x, y)
    return d, where


def underflow_input(W=40, H=12):
    """A noise-free plane with holes at (8, 5) and (31, 6) -- either side of the seam x = 32 -- for sigma_r = 0.05: the hole centre sees
    c ~ 0.69, the weights' argument is ~ -95 and every weight is an fp32 denormal."""
    d = plane(W, H, 0, noise=0.0).copy()
    d[5, 8] = 0
    d[6, 31] = 0
    return d
