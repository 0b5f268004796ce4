// The dead-block test of the dense block walk (bundletrack_amd/csrc/btba_hull.hpp) compiled for the HOST: the very arithmetic the kernel runs, held to
// fp64 references on random relative poses, intrinsics, caches and block depth ranges (tests/test_hull_host.py), and exported as hull_band_live() so
// that a GPU test can count the blocks the device must have kept (tests/test_gpu_sweep_setup.py builds this file as a shared library).
//   check 1  a block the header calls dead has no pixel, at any of 9 depths of its range, that an fp64 projection puts into the target image
//   check 2  the separable verdict equals the four-corner verdict of the forms in fp64, except where an fp64 form lies within 1e-4 of zero
//   check 3  a corner behind the camera keeps the block; a NaN pose keeps it; no ranges at all keep every block
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../../bundletrack_amd/csrc/btba_hull.hpp"

using namespace btba_hull;

// The live blocks of the band of block rows [r0, r1) of a width x height cache, as dense_block_pinhole<2> decides them: R, t the relative pose (source
// camera -> target camera), lut[0 .. width) the columns' and lut[width .. width + height) the rows' back-projection terms, ranges[2 * (by * bw + bx)] the
// blocks' (zlo, zhi) -- null: every block is live.  live_out (may be null): one byte per block of the band.
extern "C" int hull_band_live(const float *R9, const float *t3, float fx, float fy, float cx, float cy, int width, int height, const float *lut,
                              const float *ranges, float depth_min, float depth_max, int r0, int r1, unsigned char *live_out)
{
    const int bw = width / 8, bh = height / 8;
    float R[9], t[3];
    for (int k = 0; k < 9; k++) R[k] = R9[k];
    for (int k = 0; k < 3; k++) t[k] = t3[k];
    const HullForms F = hull_forms(fx, fy, cx, cy, width, height);
    const HullBias b = hull_bias(F, t);
    std::vector<HullEntry> col(bw), row(bh);
    for (int x = 0; x < bw; x++) col[x] = hull_entry(R, F, false, lut[8 * x], lut[8 * x + 7]);
    for (int y = 0; y < bh; y++) row[y] = hull_entry(R, F, true, lut[width + 8 * y], lut[width + 8 * y + 7]);
    int n = 0;
    for (int by = r0; by < r1; by++)
        for (int bx = 0; bx < bw; bx++) {
            const bool live = ranges ? hull_block_live(col[bx], row[by], b, ranges[2 * (by * bw + bx)], ranges[2 * (by * bw + bx) + 1], depth_min, depth_max) : true;
            if (live_out) live_out[(by - r0) * bw + bx] = live;
            n += live;
        }
    return n;
}

namespace {

struct Tally { long blocks = 0, dead = 0, dead_nonempty = 0, live = 0, pixels_checked = 0, violations = 0, exceptions = 0, mismatches = 0; };

void random_pose(std::mt19937_64 &g, float *R, float *t)
{
    std::uniform_real_distribution<double> U(-1.0, 1.0), A(0.0, 0.6), T(0.0, 0.3);
    double ax[3], n;
    do { for (double &a : ax) a = U(g); n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]); } while (n < 1e-3 || n > 1.0);
    for (double &a : ax) a /= n;
    const double th = A(g), c = std::cos(th), s = std::sin(th), v = 1.0 - c;
    const double M[9] = { c + ax[0] * ax[0] * v, ax[0] * ax[1] * v - ax[2] * s, ax[0] * ax[2] * v + ax[1] * s,
                          ax[1] * ax[0] * v + ax[2] * s, c + ax[1] * ax[1] * v, ax[1] * ax[2] * v - ax[0] * s,
                          ax[2] * ax[0] * v - ax[1] * s, ax[2] * ax[1] * v + ax[0] * s, c + ax[2] * ax[2] * v };
    for (int k = 0; k < 9; k++) R[k] = (float)M[k];
    double d[3];
    do { for (double &a : d) a = U(g); n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); } while (n < 1e-3 || n > 1.0);
    const double len = T(g);
    for (int k = 0; k < 3; k++) t[k] = (float)(d[k] / n * len);
}

struct Camera { int width, height; float fx, fy, cx, cy; std::vector<float> lut; };

// a cache of width x height sampled from a full-resolution image 4 times as large, intrinsics near the project's (focal length ~ 0.9 widths)
Camera random_camera(std::mt19937_64 &g, int width, int height)
{
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    Camera c;
    c.width = width; c.height = height;
    const double fxf = 4.0 * width * (0.9 + 0.1 * U(g)), fyf = fxf * (1.0 + 0.02 * U(g));
    const double cxf = 2.0 * width * (1.0 + 0.05 * U(g)), cyf = 2.0 * height * (1.0 + 0.05 * U(g));
    c.fx = (float)(fxf / 4.0); c.fy = (float)(fyf / 4.0); c.cx = (float)(cxf / 4.0); c.cy = (float)(cyf / 4.0);
    c.lut.resize(width + height);
    const float kix = (float)(1.0 / fxf), kiy = (float)(1.0 / fyf), kcx = (float)(-cxf / fxf), kcy = (float)(-cyf / fyf);
    for (int x = 0; x < width; x++) c.lut[x] = kix * (float)(unsigned)(x * 4.0f + 0.5f) + kcx;              // the cache builder's nearest-neighbour source pixel
    for (int y = 0; y < height; y++) c.lut[width + y] = kiy * (float)(unsigned)(y * 4.0f + 0.5f) + kcy;
    return c;
}

constexpr float kDepthMin = 0.1f, kDepthMax = 3.0f;

std::vector<float> random_ranges(std::mt19937_64 &g, int nblocks)
{
    std::uniform_real_distribution<double> Z(0.15, 2.5), W(0.0, 0.4), P(0.0, 1.0);
    std::vector<float> r(2 * nblocks);
    for (int k = 0; k < nblocks; k++) {
        const double p = P(g), z = Z(g);
        float lo, hi;
        if (p < 0.10) { lo = std::numeric_limits<float>::infinity(); hi = -lo; }      // no usable pixel: the range builder's empty range
        else if (p < 0.15) { lo = 0.0f; hi = 0.05f; }                                   // all depths below depth_min: empty after clamping
        else if (p < 0.30) { lo = hi = (float)z; }                                      // degenerate
        else if (p < 0.40) { lo = kDepthMin; hi = kDepthMax; }                          // full range
        else if (p < 0.45) { lo = 0.0f; hi = 10.0f; }                                   // wider than the usable depths: clamped to them
        else { lo = (float)z; hi = (float)(z + W(g)); }
        r[2 * k] = lo; r[2 * k + 1] = hi;
    }
    return r;
}

void check_scene(const Camera &c, const float *R, const float *t, const std::vector<float> &ranges, Tally &T)
{
    const int bw = c.width / 8, bh = c.height / 8;
    std::vector<unsigned char> live(bw * bh);
    hull_band_live(R, t, c.fx, c.fy, c.cx, c.cy, c.width, c.height, c.lut.data(), ranges.data(), kDepthMin, kDepthMax, 0, bh, live.data());
    const double m = 0.01;
    const double cL = (double)c.cx + 0.5 + m, cR = (double)c.cx - ((double)c.width - 0.5 + m), cT = (double)c.cy + 0.5 + m, cB = (double)c.cy - ((double)c.height - 0.5 + m);
    const double bL = (double)c.fx * t[0] + cL * t[2], bR = (double)c.fx * t[0] + cR * t[2], bT = (double)c.fy * t[1] + cT * t[2], bB = (double)c.fy * t[1] + cB * t[2];
    for (int by = 0; by < bh; by++)
        for (int bx = 0; bx < bw; bx++) {
            const int k = by * bw + bx;
            T.blocks++;
            const float zlo = std::fmax(ranges[2 * k], kDepthMin), zhi = std::fmin(ranges[2 * k + 1], kDepthMax);
            const bool nonempty = zlo <= zhi;
            if (!nonempty) {                                   // dead by definition, in both evaluations
                T.dead++;
                if (live[k]) T.mismatches++;
                continue;
            }
            // check 2: the four corners x two depths of today's formula, in fp64
            double maxL = -INFINITY, minR = INFINITY, maxT = -INFINITY, minB = INFINITY, zq = INFINITY;
            for (int corner = 0; corner < 4; corner++) {
                const double x = c.lut[8 * bx + ((corner & 1) ? 7 : 0)], y = c.lut[c.width + 8 * by + ((corner & 2) ? 7 : 0)];
                const double rx = (double)R[0] * x + (double)R[1] * y + R[2], ry = (double)R[3] * x + (double)R[4] * y + R[5], rz = (double)R[6] * x + (double)R[7] * y + R[8];
                const double aL = c.fx * rx + cL * rz, aR = c.fx * rx + cR * rz, aT = c.fy * ry + cT * rz, aB = c.fy * ry + cB * rz;
                for (const double d : { (double)zlo, (double)zhi }) {
                    maxL = std::fmax(maxL, aL * d); minR = std::fmin(minR, aR * d); maxT = std::fmax(maxT, aT * d); minB = std::fmin(minB, aB * d);
                    zq = std::fmin(zq, rz * d);
                }
            }
            const double forms[5] = { maxL + bL, minR + bR, maxT + bT, minB + bB, zq + t[2] - 1e-3 };
            bool near_zero = false;
            for (const double f : forms) near_zero |= std::fabs(f) < 1e-4;
            const bool outside = forms[0] < 0.0 || forms[1] > 0.0 || forms[2] < 0.0 || forms[3] > 0.0;
            const bool live64 = !(forms[4] > 0.0 && outside);
            if (near_zero) T.exceptions++;
            else if (live64 != (bool)live[k]) T.mismatches++;
            if (live[k]) { T.live++; continue; }
            // check 1: a dead block has no pixel in the target image, at either end of its range or 7 depths inside
            T.dead++; T.dead_nonempty++;
            for (int py = 0; py < 8; py++)
                for (int px = 0; px < 8; px++) {
                    const double x = c.lut[8 * bx + px], y = c.lut[c.width + 8 * by + py];
                    const double rx = (double)R[0] * x + (double)R[1] * y + R[2], ry = (double)R[3] * x + (double)R[4] * y + R[5], rz = (double)R[6] * x + (double)R[7] * y + R[8];
                    for (int s = 0; s <= 8; s++) {
                        const double d = (double)zlo + ((double)zhi - (double)zlo) * s / 8.0;
                        const double qx = rx * d + t[0], qy = ry * d + t[1], qz = rz * d + t[2];
                        const double u = c.fx * qx / qz + c.cx, v = c.fy * qy / qz + c.cy;
                        T.pixels_checked++;
                        // the in-image rule of the sweep (SolverBundlingDenseUtil.h:91-94 on the rounded coordinates); a dead block's points are in front of the camera
                        if (!(qz > 0.0) || (u > -0.5 && u < c.width - 0.5 && v > -0.5 && v < c.height - 0.5)) T.violations++;
                    }
                }
        }
}

}      // namespace

int main(int argc, char **argv)
{
    const int n_poses = argc > 1 ? std::atoi(argv[1]) : 400;
    std::mt19937_64 g(20261019);
    const int sizes[3][2] = { { 16, 16 }, { 24, 16 }, { 160, 120 } };
    Tally T;
    for (const auto &wh : sizes)
        for (int p = 0; p < (wh[0] == 160 ? n_poses / 8 : n_poses); p++) {
            const Camera c = random_camera(g, wh[0], wh[1]);
            float R[9], t[3];
            random_pose(g, R, t);
            check_scene(c, R, t, random_ranges(g, (wh[0] / 8) * (wh[1] / 8)), T);
        }
    std::printf("blocks %ld live %ld dead %ld (non-empty range: %ld) pixel-depth samples %ld violations %ld exceptions %ld mismatches %ld\n",
                T.blocks, T.live, T.dead, T.dead_nonempty, T.pixels_checked, T.violations, T.exceptions, T.mismatches);
    int bad = 0;
    if (T.violations) { std::printf("FAIL check 1: a dead block has a pixel in the target image\n"); bad = 1; }
    if (T.mismatches) { std::printf("FAIL check 2: separable and four-corner verdicts differ away from zero\n"); bad = 1; }
    if (1000 * T.exceptions >= T.blocks) { std::printf("FAIL check 2: too many near-zero exceptions\n"); bad = 1; }
    if (20 * T.dead_nonempty < T.blocks || 20 * T.live < T.blocks) { std::printf("FAIL: the cases do not exercise both verdicts\n"); bad = 1; }

    // check 3
    {
        const Camera c = random_camera(g, 24, 16);
        const int nbk = 3 * 2;
        std::vector<float> full(2 * nbk);
        for (int k = 0; k < nbk; k++) { full[2 * k] = 0.5f; full[2 * k + 1] = 1.0f; }
        const float I[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
        // far to the side AND behind the target camera: every form says `outside`, the sign of q.z forbids the conclusion
        const float behind[3] = { 50.0f, 0.0f, -2.0f }, side[3] = { 50.0f, 0.0f, 0.0f };
        const int n_behind = hull_band_live(I, behind, c.fx, c.fy, c.cx, c.cy, 24, 16, c.lut.data(), full.data(), kDepthMin, kDepthMax, 0, 2, nullptr);
        const int n_side = hull_band_live(I, side, c.fx, c.fy, c.cx, c.cy, 24, 16, c.lut.data(), full.data(), kDepthMin, kDepthMax, 0, 2, nullptr);
        // one corner at the camera plane: q.z = z - 0.5 with z in [0.5, 1]
        const float plane[3] = { 50.0f, 0.0f, -0.5f };
        const int n_plane = hull_band_live(I, plane, c.fx, c.fy, c.cx, c.cy, 24, 16, c.lut.data(), full.data(), kDepthMin, kDepthMax, 0, 2, nullptr);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        int n_nan = 0, n_cases = 0;
        for (int k = 0; k < 12; k++) {                         // a NaN in any single element of the pose, and in all of them
            float Rn[9], tn[3];
            for (int e = 0; e < 9; e++) Rn[e] = I[e];
            for (int e = 0; e < 3; e++) tn[e] = side[e];
            (k < 9 ? Rn[k] : tn[k - 9]) = nan;
            n_nan += hull_band_live(Rn, tn, c.fx, c.fy, c.cx, c.cy, 24, 16, c.lut.data(), full.data(), kDepthMin, kDepthMax, 0, 2, nullptr);
            n_cases++;
        }
        const float Rn[9] = { nan, nan, nan, nan, nan, nan, nan, nan, nan }, tn[3] = { nan, nan, nan };
        n_nan += hull_band_live(Rn, tn, c.fx, c.fy, c.cx, c.cy, 24, 16, c.lut.data(), full.data(), kDepthMin, kDepthMax, 0, 2, nullptr);
        n_cases++;
        const int n_none = hull_band_live(I, side, c.fx, c.fy, c.cx, c.cy, 24, 16, c.lut.data(), nullptr, kDepthMin, kDepthMax, 0, 2, nullptr);
        std::printf("check 3: behind %d/%d plane %d/%d side %d/%d nan %d/%d no-ranges %d/%d\n", n_behind, nbk, n_plane, nbk, n_side, nbk, n_nan, n_cases * nbk, n_none, nbk);
        if (n_behind != nbk || n_plane != nbk || n_side != 0 || n_nan != n_cases * nbk || n_none != nbk) { std::printf("FAIL check 3\n"); bad = 1; }
    }
    if (!bad) std::printf("ok\n");
    return bad;
}
