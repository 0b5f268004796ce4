// nocs_host.cpp -- CPU restatement of btba_nocs_errors (include/btba.h, "the NOCS evaluation"), for the tests.
// Written from the header's contract: fp64, no fma (built with -ffp-contract=off), sums left to right.  The (cos, sin) table of
// the symmetry steps comes from the caller, as the library's host side hands it to the kernel.
#include <cmath>
#include <cstdint>
#include <limits>

namespace {

struct Pose { double m[4][4]; };

Pose load(const double *p)
{
    Pose M;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) M.m[r][c] = p[4 * r + c];
    return M;
}

bool all_finite(const double *p)
{
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(p[k])) return false;
    return true;
}

void prepare(Pose &M, bool flip, bool normalize)
{
    if (flip)
        for (int r = 0; r < 2; r++)
            for (int c = 0; c < 4; c++) M.m[r][c] = -M.m[r][c];
    if (normalize)
        for (int c = 0; c < 3; c++) {
            double s = M.m[0][c] * M.m[0][c];
            for (int r = 1; r < 4; r++) s = s + M.m[r][c] * M.m[r][c];
            const double nrm = std::sqrt(s);
            for (int r = 0; r < 4; r++) M.m[r][c] = M.m[r][c] / nrm;
        }
}

bool bottom_row_ok(const Pose &M) { return M.m[3][0] == 0.0 && M.m[3][1] == 0.0 && M.m[3][2] == 0.0 && M.m[3][3] == 1.0; }

// benchmark.py:75-78 reduce the 3 x 8 corner array along axis 0: per corner the min and max over its three coordinates
struct Box { double lo[8], hi[8]; };

Box extent(const Pose &M, const double *corners)
{
    Box b{};
    for (int k = 0; k < 8; k++) {
        const double *q = corners + 3 * k;
        const double w = M.m[3][0] * q[0] + M.m[3][1] * q[1] + M.m[3][2] * q[2] + M.m[3][3];
        for (int r = 0; r < 3; r++) {
            const double p = (M.m[r][0] * q[0] + M.m[r][1] * q[1] + M.m[r][2] * q[2] + M.m[r][3]) / w;
            if (r == 0 || p < b.lo[k]) b.lo[k] = p;
            if (r == 0 || p > b.hi[k]) b.hi[k] = p;
        }
    }
    return b;
}

double volume(const Box &b)
{
    double v = b.hi[0] - b.lo[0];
    for (int k = 1; k < 8; k++) v = v * (b.hi[k] - b.lo[k]);
    return v;
}

double iou(const Pose &A, const Pose &B, const double *corners)
{
    const Box a = extent(A, corners), b = extent(B, corners);
    double e[8];
    bool apart = false;
    for (int k = 0; k < 8; k++) {
        const double lo = a.lo[k] > b.lo[k] ? a.lo[k] : b.lo[k];
        const double hi = a.hi[k] < b.hi[k] ? a.hi[k] : b.hi[k];
        e[k] = hi - lo;
        if (e[k] < 0.0) apart = true;
    }
    double inter = 0.0;
    if (!apart) {
        inter = e[0];
        for (int k = 1; k < 8; k++) inter = inter * e[k];
    }
    return inter / (volume(a) + volume(b) - inter);
}

void rotation(const Pose &M, double R[3][3])
{
    const double (*m)[4] = M.m;
    const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    const double s = std::cbrt(det);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[r][c] = m[r][c] / s;
}

}  // namespace

extern "C" __attribute__((visibility("default"))) void nocs_host(const double *boxes, int n, const int32_t *class_id, const int32_t *handle_visible,
                                                                  const int32_t *box_index, const double *poses_pred, const double *poses_gt,
                                                                  const double *table, int n_steps, int flip, int normalize, int clamp,
                                                                  double *theta_out, double *shift_out, double *iou_out)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int e = 0; e < n; e++) {
        const double *pp = poses_pred + 16 * (size_t)e, *pg = poses_gt + 16 * (size_t)e;
        if (!all_finite(pp) || !all_finite(pg)) {
            theta_out[e] = shift_out[e] = iou_out[e] = nan;
            continue;
        }
        Pose P = load(pp), G = load(pg);
        prepare(P, flip != 0, normalize != 0);
        prepare(G, false, normalize != 0);
        if (!bottom_row_ok(P) || !bottom_row_ok(G)) {
            theta_out[e] = shift_out[e] = 10000.0;
            iou_out[e] = nan;
            continue;
        }
        const int c = class_id[e];
        const bool sym = c == 1 || c == 2 || c == 4 || (c == 6 && handle_visible && handle_visible[e] == 0);
        const double *corners = boxes + 24 * (size_t)box_index[e];

        double R1[3][3], R2[3][3], a;
        rotation(P, R1);
        rotation(G, R2);
        if (sym) {
            const double d = R1[0][1] * R2[0][1] + R1[1][1] * R2[1][1] + R1[2][1] * R2[2][1];
            const double n1 = std::sqrt(R1[0][1] * R1[0][1] + R1[1][1] * R1[1][1] + R1[2][1] * R1[2][1]);
            const double n2 = std::sqrt(R2[0][1] * R2[0][1] + R2[1][1] * R2[1][1] + R2[2][1] * R2[2][1]);
            a = d / (n1 * n2);
        } else {
            double t[3];
            for (int r = 0; r < 3; r++) t[r] = R1[r][0] * R2[r][0] + R1[r][1] * R2[r][1] + R1[r][2] * R2[r][2];
            a = (t[0] + t[1] + t[2] - 1.0) / 2.0;
        }
        if (clamp) {
            if (a > 1.0) a = 1.0;
            else if (a < -1.0) a = -1.0;
        }
        theta_out[e] = std::acos(a) * (180.0 / M_PI);
        const double dx = P.m[0][3] - G.m[0][3], dy = P.m[1][3] - G.m[1][3], dz = P.m[2][3] - G.m[2][3];
        shift_out[e] = std::sqrt(dx * dx + dy * dy + dz * dz);

        if (sym) {
            double best = 0.0;
            for (int i = 0; i < n_steps; i++) {
                const double co = table[2 * i], si = table[2 * i + 1];
                Pose Gr = G;
                for (int r = 0; r < 4; r++) {
                    Gr.m[r][0] = G.m[r][0] * co + G.m[r][2] * -si;
                    Gr.m[r][2] = G.m[r][0] * si + G.m[r][2] * co;
                }
                const double x = iou(Gr, P, corners);
                if (x > best) best = x;
            }
            iou_out[e] = best;
        } else {
            iou_out[e] = iou(G, P, corners);
        }
    }
}
