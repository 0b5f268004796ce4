// btba_marginals.hpp -- pose covariances: the batched fp64 inverse of the solver's matrix (btba_pose_covariances), and the kernel that
// lifts that matrix out of a trace record in the public order of the unknowns (btba_linearize_batch_zn_aux).
//
// k_pose_covariances: ONE workgroup per instance.  The fp32 matrix H (na x na, na = 6 (N - 1) <= 180, the unknowns in the public (rot, trans)
// order) is widened to fp64 into the packed lower triangle in LDS (btba_marginals_layout.hpp) and goes through three phases in place:
//   1  Cholesky H = L L^T, left-looking: lane i owns row i; column j is one dot product per lane over the finished columns, one division by
//      sqrt(d_j) and ONE barrier.  Lane i keeps its running pivot d_i = H_ii - sum_k L_ik^2 in a register and hands it over through LDS when
//      its turn comes, so no lane recomputes it.
//   2  L^-1 in place, columns from the last to the first: M_ij = -(sum_{k = j+1 .. i} M_ik L_kj) / L_jj.  The column of L a step is about to
//      overwrite is copied out one step ahead (double-buffered), so this phase too has one barrier per column.
//   3  Sigma = M^T M, entry (a, b) = sum_{k >= a} M_ka M_kb for a >= b, every entry by one lane, written to both triangles (and to the frame's
//      6 x 6 block): the outputs are symmetric, and blocks equal the diagonal blocks of the full matrix, bit for bit.
// All arithmetic is IEEE fp64: fma(), `/` and sqrt() (correctly rounded; no reciprocal or rsq estimate is used as a result), no atomics, no
// cross-lane sums.  Every sum runs in an order fixed by its bounds alone (dot4 below; phase 3: ascending k), so an instance's bits do not
// depend on its position in the batch or on the batch size.
// LDS: row i of the packed triangle starts at double i (i + 1) / 2, and the triangular numbers are a permutation modulo 32 over any aligned
// run of 32 lanes -- the 32 lanes of a ds_read_b64 / ds_write_b64 group that read entry k of their own rows hit 32 different 8-byte
// bank pairs (64 banks of 4 bytes), conflict-free without padding; row j, which every lane reads in phase 1, is a broadcast.
// Cost: fp64 FMA issues at half the fp32 vector rate on gfx950; the two triangular phases are latency-bound chains (na^2 / 2 dependent FMAs each,
// cut in four by dot4), their 2 na <= 360 barriers (three waves waiting on LDS) are small beside that; phase 3 carries the bulk of the
// arithmetic (na^3 / 6 FMAs) on all four waves without a barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "btba_marginals_layout.hpp"

namespace btba {

struct MarginalsArgs {
    int n_frames;
    int64_t info_stride;            // floats per instance of info
    const float *info;              // [B][>= na * na]: the lower triangle is read
    double *cov_blocks;             // [B][N][6][6]
    double *cov_full;               // nullptr or [B][na][na]
    double *pivot_ratio;            // nullptr or [B]
    int32_t *status;                // [B]
};

// sum_{k = lo .. hi - 1} a[k] b[k]: four interleaved FMA chains (k - lo modulo 4), joined as (s0 + s1) + (s2 + s3)
__device__ inline double dot4(const double *a, const double *b, int lo, int hi)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int k = lo;
    for (; k + 4 <= hi; k += 4) {
        s0 = fma(a[k], b[k], s0);
        s1 = fma(a[k + 1], b[k + 1], s1);
        s2 = fma(a[k + 2], b[k + 2], s2);
        s3 = fma(a[k + 3], b[k + 3], s3);
    }
    if (k < hi) s0 = fma(a[k], b[k], s0);
    if (k + 1 < hi) s1 = fma(a[k + 1], b[k + 1], s1);
    if (k + 2 < hi) s2 = fma(a[k + 2], b[k + 2], s2);
    return (s0 + s1) + (s2 + s3);
}

__global__ __launch_bounds__(kMarginalsBlock) void k_pose_covariances(MarginalsArgs S)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char marginals_lds[];
    const MarginalsLayout lay(S.n_frames);
    const int na = lay.na, N = S.n_frames, tid = (int)threadIdx.x;
    const size_t b = blockIdx.x;
    double *tri = reinterpret_cast<double *>(marginals_lds + lay.tri);
    double *col = reinterpret_cast<double *>(marginals_lds + lay.col);
    double *pivot = reinterpret_cast<double *>(marginals_lds + lay.pivot);
    double *diag = reinterpret_cast<double *>(marginals_lds + lay.diag);
    const float *H = S.info + b * (size_t)S.info_stride;
    const int ntri = na * (na + 1) / 2;

    for (int e = tid; e < na * na; e += kMarginalsBlock) {
        const int i = e / na, j = e - i * na;
        if (j <= i) tri[marginals_tri_index(i, j)] = (double)H[e];
    }
    const int i = tid;
    const bool row = i < na;
    double *ri = tri + marginals_tri_index(row ? i : 0, 0);
    double dd = row ? (double)H[(size_t)i * na + i] : 0.0;      // lane i's running pivot
    if (row) diag[i] = dd;
    if (i == 0) pivot[0] = dd;
    __syncthreads();

    // ---- phase 1: H = L L^T
    int fail = 0;
    for (int j = 0; j < na; j++) {
        const double d = pivot[j];                              // every lane reads the same word: the branch is uniform
        if (!(d > 0.0) || !isfinite(d)) { fail = 1 + j; break; }
        const double ljj = sqrt(d);
        if (row && i > j) {
            const double l = (ri[j] - dot4(ri, tri + marginals_tri_index(j, 0), 0, j)) / ljj;
            ri[j] = l;
            dd = fma(-l, l, dd);
            if (i == j + 1) pivot[j + 1] = dd;
        } else if (i == j) {
            ri[j] = ljj;
        }
        __syncthreads();
    }

    double *full = S.cov_full ? S.cov_full + b * (size_t)na * na : nullptr;
    double *blocks = S.cov_blocks + b * (size_t)N * 36;
    if (fail) {                                                 // all of this instance's covariances: quiet NaN
        const double qnan = __longlong_as_double(0x7FF8000000000000ll);
        if (full) for (int e = tid; e < na * na; e += kMarginalsBlock) full[e] = qnan;
        for (int e = tid; e < N * 36; e += kMarginalsBlock) blocks[e] = qnan;
        if (tid == 0) {
            S.status[b] = fail;
            if (S.pivot_ratio) S.pivot_ratio[b] = 0.0;
        }
        return;
    }

    // ---- phase 2: M = L^-1 in place
    if (i == na - 1) col[((na - 1) & 1) * na + i] = ri[na - 1];
    __syncthreads();
    for (int j = na - 1; j >= 0; j--) {
        const double *x = col + (j & 1) * na;                   // x[k] = L[k][j], k >= j
        double m = 0.0;
        if (row && i == j) m = 1.0 / x[j];
        else if (row && i > j) m = -dot4(ri, x, j + 1, i + 1) / x[j];
        if (row && j > 0 && i >= j - 1) col[((j - 1) & 1) * na + i] = ri[j - 1];
        if (row && i >= j) ri[j] = m;
        __syncthreads();
    }

    // ---- phase 3: Sigma = M^T M
    if (tid < 36) blocks[tid] = 0.0;                            // frame 0 is fixed
    for (int e = tid; e < ntri; e += kMarginalsBlock) {
        int a = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
        while (a * (a + 1) / 2 > e) a--;
        while ((a + 1) * (a + 2) / 2 <= e) a++;
        const int c = e - a * (a + 1) / 2;                      // entry (a, c), c <= a
        const bool in_block = a / 6 == c / 6;
        if (!full && !in_block) continue;
        size_t idx = marginals_tri_index(a, 0);
        double s = tri[idx + a] * tri[idx + c];
        for (int k = a + 1; k < na; k++) {
            idx += (size_t)k;
            s = fma(tri[idx + a], tri[idx + c], s);
        }
        if (full) { full[(size_t)a * na + c] = s; full[(size_t)c * na + a] = s; }
        if (in_block) {
            double *blk = blocks + (size_t)(a / 6 + 1) * 36;
            blk[(a % 6) * 6 + c % 6] = s;
            blk[(c % 6) * 6 + a % 6] = s;
        }
    }
    if (tid == 0) {
        S.status[b] = 0;
        if (S.pivot_ratio) {
            double r = pivot[0] / diag[0];
            for (int j = 1; j < na; j++) r = fmin(r, pivot[j] / diag[j]);
            S.pivot_ratio[b] = r;
        }
    }
}

// The solver's system out of a one-iterate trace record (btba_trace_layout): A without frame 0's rows and columns, each frame's halves swapped
// from the internal [trans, rot] to the public (rot, trans) order, and the right-hand side of frames 1 .. N - 1 (traced in the public order).
__global__ void k_gather_system(int n_frames, const float *trace, int64_t record_floats, int64_t off_A, int64_t off_rhs, float *info, float *rhs)
{
    const int na = 6 * (n_frames - 1), n = 6 * n_frames;
    const size_t b = blockIdx.y;
    const float *tr = trace + b * (size_t)record_floats;
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= na * na) return;
    const int r = e / na, c = e - r * na;
    const int ir = 6 + 6 * (r / 6) + (r % 6 < 3 ? r % 6 + 3 : r % 6 - 3), ic = 6 + 6 * (c / 6) + (c % 6 < 3 ? c % 6 + 3 : c % 6 - 3);
    info[b * (size_t)na * na + e] = tr[off_A + (size_t)ir * n + ic];
    if (rhs && e < na) rhs[b * (size_t)na + e] = tr[off_rhs + 6 + e];
}

}  // namespace btba
