// The dead-block test of the dense block walk in SEPARABLE form: plain C++ without HIP, so the very arithmetic the kernel runs (dense_block_pinhole<2>
// in btba_kernels.hpp) is also compiled for the host and held to an fp64 per-pixel projection there (tests/cpp/hull_host.cpp).
//
// Is an 8 x 8 block of the source frame PROVABLY without a pixel that lands in the target image?  A block's pixels with a usable depth lie in the
// frustum segment spanned by the block's extreme rays and its depth range [zlo, zhi] (clipped to depth_min .. depth_max); the relative pose maps the
// segment to a convex polytope whose vertices are the 8 transformed corners.  A point q = d r + t of it, q.z > 0, projects left of the image by more
// than the margin m iff
//     fx q.x / q.z + cx < -0.5 - m   <=>   fx q.x + (cx + 0.5 + m) q.z < 0   <=>   d aL(r) + bL < 0,   aL(r) = fx r.x + cL r.z,  bL = fx t.x + cL t.z,
// a LINEAR form in d for a fixed ray, so over the depth range it peaks at one of the two ends; likewise for the other three image edges.  The block is
// outside iff one of the four forms keeps its sign over all 4 corner rays x 2 depths, and while every corner has q.z > 0 no pixel of the block can
// then pass the in-image test of SolverBundlingDenseUtil.h:91-94 (a ratio of affine functions is quasi-linear on a convex set where the denominator is
// positive).  The margin -- 0.01 pixel -- is three orders of magnitude above the rounding differences between this evaluation and the per-pixel one.
//
// SEPARABLE: the rotated ray of source pixel (x, y) is r(x, y) = colA[x] + rowB[y] (colA[x] = R[:, 0] lx(x), rowB[y] = R[:, 1] ly(y) + R[:, 2]) and the
// forms are linear in r, so aL(x, y) = aLc[x] + aLr[y].  The corners of a block are the product set {xa, xb} x {ya, yb}, hence
//     max over corners of aL = max(aLc[xa], aLc[xb]) + max(aLr[ya], aLr[yb])
// and the same for the minima of the R and B forms and of r.z.  The usable depths are positive (zlo >= depth_min > 0), so the maximum over corners AND
// depths of aL d is max(A zlo, A zhi) with A the corner maximum.  Per block COLUMN and block ROW one HullEntry of five numbers; a block's verdict is
// five adds, ten products, five min / max and the comparisons -- the same real-valued quantities as the corner-by-corner evaluation, rounded differently
// by a few ulp.
//
// NO CONTRACTION: every function below switches the fusing of a * b + c off, so that the device build (which would contract) and a host build for a
// target without FMA round every operation alike and give the same verdicts bit for bit, not only up to rounding.
//
// Kept exactly: a block whose clamped depth range is empty is dead; a corner at or behind the camera plane keeps the block; a NaN in the pose keeps
// the block (every comparison below is false for it, and an entry that met a NaN or an infinity is NaN as a whole).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define BTBA_HULL_FN __host__ __device__ inline
#elif defined(__GNUC__) && !defined(__clang__)
#define BTBA_HULL_FN __attribute__((optimize("fp-contract=off"))) inline      /* g++: no fused multiply-add in these functions, whatever the build's flags and target */
#else
#define BTBA_HULL_FN inline
#endif
#if defined(__clang__)
#define BTBA_HULL_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define BTBA_HULL_NO_CONTRACT
#endif

namespace btba_hull {

constexpr float kMargin = 0.01f;      // pixels

// The four edge forms' coefficients of r.z / t.z, from the intrinsics of the (cache-resolution) target image.
struct HullForms { float fx, fy, cL, cR, cT, cB; };

BTBA_HULL_FN HullForms hull_forms(float fx, float fy, float cx, float cy, int width, int height)
{
    BTBA_HULL_NO_CONTRACT
    HullForms F;
    F.fx = fx; F.fy = fy;
    F.cL = cx + 0.5f + kMargin; F.cR = cx - ((float)width - 0.5f + kMargin);
    F.cT = cy + 0.5f + kMargin; F.cB = cy - ((float)height - 0.5f + kMargin);
    return F;
}

// Extremes of the four forms and of r.z over the two extreme rays of one block column (row = false: r = R[:, 0] l) or block row (row = true:
// r = R[:, 1] l + R[:, 2]).
struct HullEntry { float lmax, rmin, tmax, bmin, zmin; };

// la, lb: the back-projection terms (pinhole_lut_entry) of the block column's first and last column resp. the block row's first and last row.
BTBA_HULL_FN HullEntry hull_entry(const float (&R)[9], const HullForms &F, bool row, float la, float lb)
{
    BTBA_HULL_NO_CONTRACT
    const float mx = row ? R[1] : R[0], my = row ? R[4] : R[3], mz = row ? R[7] : R[6];
    const float ox = row ? R[2] : 0.0f, oy = row ? R[5] : 0.0f, oz = row ? R[8] : 0.0f;
    const float ax = mx * la + ox, ay = my * la + oy, az = mz * la + oz;
    const float bx = mx * lb + ox, by = my * lb + oy, bz = mz * lb + oz;
    const float fa = F.fx * ax, fb = F.fx * bx, ga = F.fy * ay, gb = F.fy * by;
    const float La = fa + F.cL * az, Lb = fb + F.cL * bz, Ra = fa + F.cR * az, Rb = fb + F.cR * bz;
    const float Ta = ga + F.cT * az, Tb = gb + F.cT * bz, Ba = ga + F.cB * az, Bb = gb + F.cB * bz;
    // fmaxf / fminf drop a NaN operand: the poison puts it back (0 * finite = 0, 0 * NaN = 0 * inf = NaN), and a NaN entry keeps every block it belongs to
    const float poison = 0.0f * (((La + Lb) + (Ra + Rb)) + ((Ta + Tb) + (Ba + Bb)));
    HullEntry e;
    e.lmax = fmaxf(La, Lb) + poison; e.rmin = fminf(Ra, Rb) + poison;
    e.tmax = fmaxf(Ta, Tb) + poison; e.bmin = fminf(Ba, Bb) + poison;
    e.zmin = fminf(az, bz) + poison;
    return e;
}

// The translation's share of the four forms and of q.z.
struct HullBias { float bL, bR, bT, bB, tz; };

BTBA_HULL_FN HullBias hull_bias(const HullForms &F, const float (&t)[3])
{
    BTBA_HULL_NO_CONTRACT
    HullBias b;
    b.bL = F.fx * t[0] + F.cL * t[2]; b.bR = F.fx * t[0] + F.cR * t[2];
    b.bT = F.fy * t[1] + F.cT * t[2]; b.bB = F.fy * t[1] + F.cB * t[2];
    b.tz = t[2] + 0.0f * (t[0] + t[1]);      // a NaN or an infinity anywhere in t: NaN, and the verdict is `live`
    return b;
}

// The verdict for the block in block column `c` and block row `r` whose usable pixels have depths in [zlo, zhi] (k_block_ranges).  false: provably dead.
BTBA_HULL_FN bool hull_block_live(const HullEntry &c, const HullEntry &r, const HullBias &b, float zlo, float zhi, float depth_min, float depth_max)
{
    BTBA_HULL_NO_CONTRACT
    zlo = fmaxf(zlo, depth_min); zhi = fminf(zhi, depth_max);      // usable depths: depth_min < z < depth_max
    if (!(zlo <= zhi)) return false;                               // no usable depth at all
    const float L = c.lmax + r.lmax, Rr = c.rmin + r.rmin, T = c.tmax + r.tmax, B = c.bmin + r.bmin, Z = c.zmin + r.zmin;
    const float maxL = fmaxf(L * zlo, L * zhi), minR = fminf(Rr * zlo, Rr * zhi);
    const float maxT = fmaxf(T * zlo, T * zhi), minB = fminf(B * zlo, B * zhi);
    const float zq = fminf(Z * zlo, Z * zhi);
    const bool outside = (maxL + b.bL < 0.0f) | (minR + b.bR > 0.0f) | (maxT + b.bT < 0.0f) | (minB + b.bB > 0.0f);
    return !((zq + b.tz > 1e-3f) && outside);                      // a corner at or behind the camera plane, a NaN: the block stays
}

}      // namespace btba_hull
