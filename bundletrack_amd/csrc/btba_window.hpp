// btba_window.hpp -- window assembly between the tracker's findCorres and the solver (btba_marshal_windows,
// btba_procrustes_pairs, include/btba.h)
//   Bundler::optimizeGPU's marshalling          src/Bundler.cpp:286-347
//   SiftManager::procrustesByCorrespondence     src/FeatureManager.cpp:523-557
//   Utils::solveRigidTransformBetweenPoints     src/Utils.cpp:180-214
// The reference does both on the host, one pair at a time.  Here the btba_match records a chain leaves on the device become the
// solver's device input without leaving it:
//   k_window_marshal   grid (ceil(longest segment / 256), P, windows): workgroup (t, p, w) owns records [256 t, 256 t + 256) of pair
//                      p's segment.  It sums the window's segment counts before p (the pair's place in the pair-major array), reads
//                      its records' bytes -- one contiguous range of up to 10 240 bytes -- as aligned 16-byte pieces into LDS, and
//                      every lane writes its record as EntryJ (two 16-byte stores) and, optionally, as the three float2 planes of
//                      the 24-byte layout.  A pure transcode: 40 B read, 32 B (+ 24 B) written per match, no atomics.
//   k_kabsch_moments   one workgroup of 256 per pair: model-frame points in the matcher's fp32 arithmetic, their sums and then the
//                      centred 3 x 3 moment matrix in fp64, each in the fixed order of btba_pose_errors (256 slots, then a tree).
//   k_kabsch_solve     one workgroup of 256 per pair: lane 0 turns the moments into the rotation (Horn's quaternion method, below)
//                      and the translation in fp64 and rounds them once to fp32; all lanes then sum the residual for err.
// The wave reductions of btba_device.hpp are fp32 butterflies whose order differs from the slot / tree order the contract fixes, so
// the fp64 sums go through the LDS tree of k_eval_reduce instead.
//
// Rotation (kabsch_rotation).  With S = sum (a - m1)(b - m2)^T, tr(R S) = q^T N q for the unit quaternion q = (w, x, y, z) of R, where
//   N = [ Sxx+Syy+Szz   Syz-Szy       Szx-Sxz       Sxy-Syx     ]
//       [ Syz-Szy       Sxx-Syy-Szz   Sxy+Syx       Szx+Sxz     ]
//       [ Szx-Sxz       Sxy+Syx      -Sxx+Syy-Szz   Syz+Szy     ]
//       [ Sxy-Syx       Szx+Sxz       Syz+Szy      -Sxx-Syy+Szz ]      (Horn 1987; Sxy = S[0][1])
// so the maximiser over PROPER rotations is the eigenvector of N's largest eigenvalue: no reflection case exists.  N is diagonalised
// by cyclic Jacobi in fp64: sweeps over (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a rotation is skipped (and the entry set to
// zero) when |N_pq| <= 2^-62 * (sum of |N_ij| of the initial matrix); the loop ends after the first sweep that skipped all six, or
// after 16 sweeps.  t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (N_qq - N_pp) / (2 N_pq), c = 1 / sqrt(t^2 + 1), s = t c.
// The eigenvector of the largest diagonal entry (the lowest index among equals) is normalised and expanded to R.
// Rank-deficient S: the eigenvector is still a unit vector, so R is a finite proper rotation -- ONE of the maximisers when the
// largest eigenvalue is repeated (collinear points: the rotation about the line is free); S = 0 (all points equal) gives N = 0, no
// rotation is applied, the first unit vector wins and R is the identity.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "btba_device.hpp"

namespace btba {

constexpr int kWinThreads = 256;                      // k_window_marshal: records per workgroup
constexpr int kWinRecBytes = 40;                      // sizeof(btba_match)
constexpr int kWinPieces = kWinThreads * kWinRecBytes / 16 + 1;    // 16-byte pieces that cover 256 records at either alignment
constexpr int kKabschThreads = 256;                   // the 256 slots of the fixed summation order
constexpr int kKabschMinPoints = 5;                   // countInlierCorres < 5 -> identity (FeatureManager.cpp:527)

struct KabschRec { uint32_t off; int32_t n; };        // a pair's records: [off, off + n) of the match array

// segs: uint32 [windows][P][2] = (first record, count).  n_records: records in `rec` (a segment that leaves it is not read and its
// entries are not written); corr_stride: entries per window in corr / corr24 (an entry at or beyond it is not written).
__global__ void __launch_bounds__(kWinThreads) k_window_marshal(int n_frames, int n_pairs, const uint32_t *__restrict__ segs,
                                                                const unsigned char *__restrict__ rec, unsigned long long n_records,
                                                                unsigned long long corr_stride, uint4 *__restrict__ corr,
                                                                uint32_t *__restrict__ pair_offsets, float2 *__restrict__ corr24)
{
    __shared__ uint4 stage[kWinPieces];
    __shared__ uint32_t wave_sum[kWinThreads / 64];
    const int p = blockIdx.y, w = blockIdx.z, tid = threadIdx.x;
    const uint2 *sg = reinterpret_cast<const uint2 *>(segs) + (size_t)w * n_pairs;
    const uint2 me = sg[p];
    const uint32_t first = blockIdx.x * (uint32_t)kWinThreads;
    if (first >= me.y && blockIdx.x != 0) return;                      // (uniform over the workgroup)

    // the pair's place: the window's counts before p (integers: any order gives the same sum)
    uint32_t s = 0;
    for (int q = tid; q < p; q += kWinThreads) s += sg[q].y;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = s;
    __syncthreads();
    const uint32_t seg0 = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    if (blockIdx.x == 0 && tid == 0) {
        uint32_t *po = pair_offsets + (size_t)w * (n_pairs + 1);
        po[p] = seg0;
        if (p == n_pairs - 1) po[n_pairs] = seg0 + me.y;
    }
    if (first >= me.y || (unsigned long long)me.x + me.y > n_records) return;

    // bytes [b0, b1) of the record array -> LDS as aligned 16-byte pieces; a piece that sticks out of the range (records start on
    // 8-byte boundaries) is read as its inner 8 bytes, so nothing outside the workgroup's own records is touched
    const uint32_t cnt = min((uint32_t)kWinThreads, me.y - first);
    const size_t b0 = ((size_t)me.x + first) * kWinRecBytes, b1 = b0 + (size_t)cnt * kWinRecBytes;
    const size_t a0 = b0 & ~(size_t)15;
    const int pieces = (int)((b1 - a0 + 15) >> 4);
    for (int i = tid; i < pieces; i += kWinThreads) {
        const size_t at = a0 + 16 * (size_t)i;
        uint4 v;
        if (at >= b0 && at + 16 <= b1) v = *reinterpret_cast<const uint4 *>(rec + at);
        else {
            const uint2 h = *reinterpret_cast<const uint2 *>(rec + (at >= b0 ? at : at + 8));
            v = at >= b0 ? make_uint4(h.x, h.y, 0u, 0u) : make_uint4(0u, 0u, h.x, h.y);
        }
        stage[i] = v;
    }
    __syncthreads();
    if ((uint32_t)tid >= cnt) return;
    const unsigned long long e = (unsigned long long)seg0 + first + tid;          // entry within the window
    if (e >= corr_stride) return;
    // the record's ptA_cam (bytes 16 .. 27) and ptB_cam (28 .. 39) as three 8-byte LDS reads
    const uint2 *r = reinterpret_cast<const uint2 *>(reinterpret_cast<const unsigned char *>(stage) + (b0 - a0) + (size_t)tid * kWinRecBytes + 16);
    const uint2 q0 = r[0], q1 = r[1], q2 = r[2];                                  // (A.x, A.y) (A.z, B.x) (B.y, B.z)
    int fi, fj;
    pair_from_index(p, n_frames, fi, fj);
    const size_t E = (size_t)w * corr_stride + e;
    // EntryJ{imgIdx_i = i, imgIdx_j = j, pos_i = ptB_cam, pos_j = ptA_cam} (Bundler.cpp:311-316)
    corr[2 * E] = make_uint4((uint32_t)fi, (uint32_t)fj, q1.y, q2.x);
    corr[2 * E + 1] = make_uint4(q2.y, q0.x, q0.y, q1.x);
    if (corr24) {
        float2 *o = corr24 + corr24_index(E);
        o[0] = make_float2(__uint_as_float(q1.y), __uint_as_float(q2.x));
        o[64] = make_float2(__uint_as_float(q2.y), __uint_as_float(q0.x));
        o[128] = make_float2(__uint_as_float(q0.y), __uint_as_float(q1.x));
    }
}

// a_k = TA ptA_cam, b_k = TB ptB_cam of record i: P_r = ((T_r0 x + T_r1 y) + T_r2 z) + T_r3, fp32, nothing contracted
__device__ __forceinline__ void kabsch_points(const unsigned char *__restrict__ rec, size_t i, const float *__restrict__ TA,
                                              const float *__restrict__ TB, float (&a)[3], float (&b)[3])
{
#pragma clang fp contract(off)
    const float2 *r = reinterpret_cast<const float2 *>(rec + i * kWinRecBytes + 16);
    const float2 q0 = r[0], q1 = r[1], q2 = r[2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a[k] = ((TA[4 * k] * q0.x + TA[4 * k + 1] * q0.y) + TA[4 * k + 2] * q1.x) + TA[4 * k + 3];
        b[k] = ((TB[4 * k] * q1.y + TB[4 * k + 1] * q2.x) + TB[4 * k + 2] * q2.y) + TB[4 * k + 3];
    }
}

// acc[v][l] over l: s = 128, 64, .., 1: acc[l] += acc[l + s] for l < s (the tree of btba_pose_errors); the totals land in acc[v][0]
template <int NV>
__device__ __forceinline__ void kabsch_tree(double (*acc)[kKabschThreads], int l)
{
#pragma unroll
    for (int s = kKabschThreads / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (l < s) {
#pragma unroll
            for (int v = 0; v < NV; v++) acc[v][l] += acc[v][l + s];
        }
    }
    __syncthreads();
}

// mom[pair][16] = n, m1[3], m2[3], S[9] row-major; n alone (and zeros) for a pair of fewer than 5 records
__global__ void __launch_bounds__(kKabschThreads) k_kabsch_moments(const KabschRec *__restrict__ R, const unsigned char *__restrict__ rec,
                                                                   const float *__restrict__ posesA, const float *__restrict__ posesB,
                                                                   double *__restrict__ mom)
{
#pragma clang fp contract(off)
    __shared__ double acc[9][kKabschThreads];
    const int e = blockIdx.x, l = threadIdx.x;
    const KabschRec r = R[e];
    double *out = mom + 16 * (size_t)e;
    if (r.n < kKabschMinPoints) {
        if (l < 16) out[l] = l == 0 ? (double)r.n : 0.0;
        return;
    }
    const float *TA = posesA + 16 * (size_t)e, *TB = posesB + 16 * (size_t)e;
    double sum[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int i = l; i < r.n; i += kKabschThreads) {
        float a[3], b[3];
        kabsch_points(rec, (size_t)r.off + i, TA, TB, a, b);
#pragma unroll
        for (int k = 0; k < 3; k++) { sum[k] += (double)a[k]; sum[3 + k] += (double)b[k]; }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k][l] = sum[k];
    kabsch_tree<6>(acc, l);
    double m[6];
#pragma unroll
    for (int k = 0; k < 6; k++) m[k] = acc[k][0] / (double)r.n;
    __syncthreads();                                   // every lane has read the sums before the slots are reused
    double S[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int i = l; i < r.n; i += kKabschThreads) {
        float a[3], b[3];
        kabsch_points(rec, (size_t)r.off + i, TA, TB, a, b);
        const double da[3] = { (double)a[0] - m[0], (double)a[1] - m[1], (double)a[2] - m[2] };
        const double db[3] = { (double)b[0] - m[3], (double)b[1] - m[4], (double)b[2] - m[5] };
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
#pragma unroll
            for (int c = 0; c < 3; c++) S[3 * rr + c] += da[rr] * db[c];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) acc[k][l] = S[k];
    kabsch_tree<9>(acc, l);
    if (l == 0) {
        out[0] = (double)r.n;
#pragma unroll
        for (int k = 0; k < 6; k++) out[1 + k] = m[k];
#pragma unroll
        for (int k = 0; k < 9; k++) out[7 + k] = acc[k][0];
    }
}

// the proper rotation that maximises tr(R S) (the header's algorithm), row-major
__device__ __forceinline__ void kabsch_rotation(const double *__restrict__ S, double (&R)[9])
{
#pragma clang fp contract(off)
    double A[4][4], V[4][4];
    A[0][0] = (S[0] + S[4]) + S[8];
    A[1][1] = (S[0] - S[4]) - S[8];
    A[2][2] = (S[4] - S[0]) - S[8];
    A[3][3] = (S[8] - S[0]) - S[4];
    A[0][1] = A[1][0] = S[5] - S[7];
    A[0][2] = A[2][0] = S[6] - S[2];
    A[0][3] = A[3][0] = S[1] - S[3];
    A[1][2] = A[2][1] = S[1] + S[3];
    A[1][3] = A[3][1] = S[6] + S[2];
    A[2][3] = A[3][2] = S[5] + S[7];
    double norm = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) { norm += fabs(A[r][c]); V[r][c] = (r == c) ? 1.0 : 0.0; }
    const double tiny = norm * 0x1p-62;
    for (int sweep = 0; sweep < 16; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[p][q];
                const bool go = fabs(apq) > tiny;
                rotated |= go;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * (go ? apq : 1.0));
                double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                t = go ? t : 0.0;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                A[p][p] -= t * apq; A[q][q] += t * apq; A[p][q] = A[q][p] = 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (r != p && r != q) {
                        const double arp = A[r][p], arq = A[r][q];
                        A[r][p] = A[p][r] = c * arp - s * arq;
                        A[r][q] = A[q][r] = s * arp + c * arq;
                    }
                    const double vrp = V[r][p], vrq = V[r][q];
                    V[r][p] = c * vrp - s * vrq;
                    V[r][q] = s * vrp + c * vrq;
                }
            }
        if (!rotated) break;
    }
    double l1 = A[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; k++) {
        const bool better = A[k][k] > l1;
        qw = better ? V[0][k] : qw; qx = better ? V[1][k] : qx; qy = better ? V[2][k] : qy; qz = better ? V[3][k] : qz;
        l1 = better ? A[k][k] : l1;
    }
    const double inv = 1.0 / sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    qw *= inv; qx *= inv; qy *= inv; qz *= inv;
    R[0] = 1.0 - 2.0 * (qy * qy + qz * qz); R[1] = 2.0 * (qx * qy - qw * qz); R[2] = 2.0 * (qx * qz + qw * qy);
    R[3] = 2.0 * (qx * qy + qw * qz); R[4] = 1.0 - 2.0 * (qx * qx + qz * qz); R[5] = 2.0 * (qy * qz - qw * qx);
    R[6] = 2.0 * (qx * qz - qw * qy); R[7] = 2.0 * (qy * qz + qw * qx); R[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
}

// pose_out[pair][16] row-major 4 x 4 (R | t; 0 0 0 1), err_out[pair] = sqrt(sum |R a + t - b|^2) / n
__global__ void __launch_bounds__(kKabschThreads) k_kabsch_solve(const KabschRec *__restrict__ Rc, const unsigned char *__restrict__ rec,
                                                                 const float *__restrict__ posesA, const float *__restrict__ posesB,
                                                                 const double *__restrict__ mom, float *__restrict__ pose_out,
                                                                 float *__restrict__ err_out)
{
#pragma clang fp contract(off)
    __shared__ double acc[1][kKabschThreads];
    __shared__ double Rt[12];
    __shared__ int ok;
    const int e = blockIdx.x, l = threadIdx.x;
    const KabschRec r = Rc[e];
    float *P = pose_out + 16 * (size_t)e;
    if (l == 0) {
        const double *M = mom + 16 * (size_t)e;
        bool good = r.n >= kKabschMinPoints;
#pragma unroll
        for (int k = 0; k < 16; k++) good &= (bool)__builtin_isfinite(M[k]);
        float out[12];
        if (good) {
            double R[9];
            kabsch_rotation(M + 7, R);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double t = M[4 + k] - ((R[3 * k] * M[1] + R[3 * k + 1] * M[2]) + R[3 * k + 2] * M[3]);      // t = m2 - R m1
                Rt[3 * k] = R[3 * k]; Rt[3 * k + 1] = R[3 * k + 1]; Rt[3 * k + 2] = R[3 * k + 2]; Rt[9 + k] = t;
                out[4 * k] = (float)R[3 * k]; out[4 * k + 1] = (float)R[3 * k + 1]; out[4 * k + 2] = (float)R[3 * k + 2]; out[4 * k + 3] = (float)t;
            }
#pragma unroll
            for (int k = 0; k < 12; k++) good &= (bool)__builtin_isfinite(out[k]);
        }
#pragma unroll
        for (int k = 0; k < 12; k++) P[k] = good ? out[k] : ((k % 5) == 0 ? 1.0f : 0.0f);
        P[12] = 0.0f; P[13] = 0.0f; P[14] = 0.0f; P[15] = 1.0f;
        if (!good) err_out[e] = 0.0f;
        ok = good ? 1 : 0;
    }
    __syncthreads();
    if (!ok) return;
    const float *TA = posesA + 16 * (size_t)e, *TB = posesB + 16 * (size_t)e;
    double s2 = 0.0;
    for (int i = l; i < r.n; i += kKabschThreads) {
        float a[3], b[3];
        kabsch_points(rec, (size_t)r.off + i, TA, TB, a, b);
        double d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double d = ((((Rt[3 * k] * (double)a[0] + Rt[3 * k + 1] * (double)a[1]) + Rt[3 * k + 2] * (double)a[2]) + Rt[9 + k]) - (double)b[k]);
            d2 += d * d;
        }
        s2 += d2;
    }
    acc[0][l] = s2;
    kabsch_tree<1>(acc, l);
    if (l == 0) err_out[e] = (float)(sqrt(acc[0][0]) / (double)r.n);
}

}  // namespace btba
