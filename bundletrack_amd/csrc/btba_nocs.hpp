// btba_nocs.hpp -- the NOCS / 6-PACK evaluation per item (btba_nocs_errors, include/btba.h)
//   normalizeRotation, the z-180 flip        scripts/benchmark.py:59-63, 262-269
//   compute_3d_iou_new                       scripts/benchmark.py:65-118
//   compute_RT_degree_cm_symmetry            scripts/benchmark.py:120-159
// The reference scores one frame at a time in numpy: a 20-step symmetry maximum of its corner-extent IoU plus one rotation /
// translation error.  Here one launch scores any number of (predicted pose, ground-truth pose, class, box) items in fp64:
//   k_nocs_errors  one 32-lane half wave per item, two items per wave, eight per 256-thread workgroup.  Every lane forms the
//                  pre-processed poses itself (32 loads that the half wave shares through the cache; no broadcast).  Lane l <
//                  n_sym_steps takes symmetry step l: the ground-truth pose times the y rotation of the step, eight corner
//                  transforms per pose, the reference's min / max, one IoU; a non-symmetric item has lane 0 alone do this
//                  without a rotation.
//                  The symmetry maximum is an xor butterfly over the half wave (__shfl_xor, width 32) on values with NaN and
//                  everything not above 0 replaced by 0: a maximum of non-NaN values does not depend on the order, so it is
//                  the sequential "m = x if x > m" from m = 0.  Lane 31 computes theta and the shift; lane 0 stores.
// No LDS, no barrier, no atomics.  Nothing is contracted into an fma: every product and sum below is its own rounding, in the
// order written (include/btba.h states the same order).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace btba {

constexpr int kNocsThreads = 256;                     // four waves
constexpr int kNocsHalf = 32;                         // lanes per item
constexpr int kNocsItems = kNocsThreads / kNocsHalf;  // eight items per workgroup
constexpr int kNocsMaxSteps = 32;                     // one symmetry step per lane of the half wave
constexpr int kNocsPoseLane = 31;                     // the lane that computes theta and the shift
constexpr int kNocsChunkItems = 1 << 18;              // items per launch (bounds the host-form staging: 72 MB)

constexpr int kNocsFlip = 1, kNocsNormalize = 2, kNocsClamp = 4;   // k_nocs_errors' flags

// Pre-processing: rows 0 and 1 negated (the protocol's z-180 flip), then columns 0 .. 2 divided by their norm over all four rows.
__device__ __forceinline__ void nocs_prepare(double *M, bool flip, bool normalize)
{
#pragma clang fp contract(off)
    if (flip) {
#pragma unroll
        for (int k = 0; k < 8; k++) M[k] = -M[k];
    }
    if (normalize) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double nrm = sqrt(M[c] * M[c] + M[4 + c] * M[4 + c] + M[8 + c] * M[8 + c] + M[12 + c] * M[12 + c]);
#pragma unroll
            for (int r = 0; r < 4; r++) M[4 * r + c] /= nrm;
        }
    }
}

// The reference reduces its 3 x 8 corner array along axis 0 (benchmark.py:75-78): per CORNER the min and the max over the corner's
// three coordinates, eight values each.  Each corner is divided by its homogeneous coordinate first.
__device__ __forceinline__ void nocs_extent(const double *M, const double *__restrict__ box, double *lo, double *hi)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double x = box[3 * k], y = box[3 * k + 1], z = box[3 * k + 2];
        const double w = M[12] * x + M[13] * y + M[14] * z + M[15];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double p = (M[4 * r] * x + M[4 * r + 1] * y + M[4 * r + 2] * z + M[4 * r + 3]) / w;
            lo[k] = r == 0 || p < lo[k] ? p : lo[k];
            hi[k] = r == 0 || p > hi[k] ? p : hi[k];
        }
    }
}

// The reference's IoU of the corners under A and under B: eight "extents", one per corner.
__device__ __forceinline__ double nocs_iou(const double *A, const double *B, const double *__restrict__ box)
{
#pragma clang fp contract(off)
    double lo1[8], hi1[8], lo2[8], hi2[8];
    nocs_extent(A, box, lo1, hi1);
    nocs_extent(B, box, lo2, hi2);
    bool apart = false;
    double inter = 1.0, v1 = 1.0, v2 = 1.0;              // 1 * e_0 == e_0: the products run e_0 e_1 .. e_7 from the left
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const double lo = lo1[k] > lo2[k] ? lo1[k] : lo2[k], hi = hi1[k] < hi2[k] ? hi1[k] : hi2[k];
        const double e = hi - lo;
        apart |= e < 0.0;
        inter *= e;
        v1 *= hi1[k] - lo1[k];
        v2 *= hi2[k] - lo2[k];
    }
    if (apart) inter = 0.0;
    return inter / (v1 + v2 - inter);
}

// R = M[:3, :3] / cbrt(det M[:3, :3])
__device__ __forceinline__ void nocs_rotation(const double *M, double *R)
{
#pragma clang fp contract(off)
    const double det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) + M[2] * (M[4] * M[9] - M[5] * M[8]);
    const double s = cbrt(det);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[3 * r + c] = M[4 * r + c] / s;
}

// theta in degrees and the shift of the pre-processed poses P (prediction) and G (ground truth).
__device__ __forceinline__ void nocs_rt(const double *P, const double *G, bool sym, bool clamp, double &theta, double &shift)
{
#pragma clang fp contract(off)
    double R1[9], R2[9], a;
    nocs_rotation(P, R1);
    nocs_rotation(G, R2);
    if (sym) {
        const double d = R1[1] * R2[1] + R1[4] * R2[4] + R1[7] * R2[7];
        const double n1 = sqrt(R1[1] * R1[1] + R1[4] * R1[4] + R1[7] * R1[7]), n2 = sqrt(R2[1] * R2[1] + R2[4] * R2[4] + R2[7] * R2[7]);
        a = d / (n1 * n2);
    } else {
        const double t0 = R1[0] * R2[0] + R1[1] * R2[1] + R1[2] * R2[2], t1 = R1[3] * R2[3] + R1[4] * R2[4] + R1[5] * R2[5],
                     t2 = R1[6] * R2[6] + R1[7] * R2[7] + R1[8] * R2[8];
        a = (t0 + t1 + t2 - 1.0) / 2.0;
    }
    if (clamp) a = a > 1.0 ? 1.0 : (a < -1.0 ? -1.0 : a);        // a NaN stays a NaN
    theta = acos(a) * (180.0 / 3.14159265358979323846);
    const double dx = P[3] - G[3], dy = P[7] - G[7], dz = P[11] - G[11];
    shift = sqrt(dx * dx + dy * dy + dz * dz);
}

// meta[e] = box_index << 1 | rotation-symmetric.  table: (cos, sin) of step i at [2 i], [2 i + 1].
__global__ void __launch_bounds__(kNocsThreads) k_nocs_errors(int n, const int32_t *__restrict__ meta, const double *__restrict__ boxes,
                                                              const double *__restrict__ poses_pred, const double *__restrict__ poses_gt,
                                                              const double *__restrict__ table, int n_steps, int flags,
                                                              double *__restrict__ theta_out, double *__restrict__ shift_out,
                                                              double *__restrict__ iou_out)
{
    const int e = blockIdx.x * kNocsItems + threadIdx.x / kNocsHalf;
    if (e >= n) return;                                  // a whole half wave: the shuffles below stay inside the half
    const int l = threadIdx.x % kNocsHalf;
    const int m = meta[e];
    const bool sym = m & 1;
    const double *box = boxes + 24 * (size_t)(m >> 1);

    double P[16], G[16];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        P[k] = poses_pred[16 * (size_t)e + k];
        G[k] = poses_gt[16 * (size_t)e + k];
        finite &= __builtin_isfinite(P[k]) & __builtin_isfinite(G[k]);
    }
    nocs_prepare(P, flags & kNocsFlip, flags & kNocsNormalize);
    nocs_prepare(G, false, flags & kNocsNormalize);
    const bool rows_ok = P[12] == 0.0 && P[13] == 0.0 && P[14] == 0.0 && P[15] == 1.0 &&
                         G[12] == 0.0 && G[13] == 0.0 && G[14] == 0.0 && G[15] == 1.0;

    double x = 0.0;                                      // this lane's IoU
    if (l < (sym ? n_steps : 1)) {
        if (sym) {
#pragma clang fp contract(off)
            const double c = table[2 * l], s = table[2 * l + 1];
            double Gr[16];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                Gr[4 * r] = G[4 * r] * c + G[4 * r + 2] * -s;
                Gr[4 * r + 1] = G[4 * r + 1];
                Gr[4 * r + 2] = G[4 * r] * s + G[4 * r + 2] * c;
                Gr[4 * r + 3] = G[4 * r + 3];
            }
            x = nocs_iou(Gr, P, box);
        } else {
            x = nocs_iou(G, P, box);
        }
    }
    double best = x > 0.0 ? x : 0.0;                     // NaN and everything not above the initial 0 are never taken
#pragma unroll
    for (int d = kNocsHalf / 2; d >= 1; d >>= 1) best = fmax(best, __shfl_xor(best, d, kNocsHalf));
    const double single = __shfl(x, 0, kNocsHalf);

    double theta = 0.0, shift = 0.0;
    if (l == kNocsPoseLane) nocs_rt(P, G, sym, flags & kNocsClamp, theta, shift);
    theta = __shfl(theta, kNocsPoseLane, kNocsHalf);
    shift = __shfl(shift, kNocsPoseLane, kNocsHalf);

    if (l == 0) {
        const double nan = __builtin_nan("");
        double iou = sym ? best : single;
        if (!finite) theta = shift = iou = nan;
        else if (!rows_ok) { theta = shift = 10000.0; iou = nan; }
        theta_out[e] = theta;
        shift_out[e] = shift;
        iou_out[e] = iou;
    }
}

}  // namespace btba
