// btba_match.hpp -- descriptor matching with the tracker's geometric gate (btba_match_pairs, include/btba.h)
//   SiftManager::findCorresbyNN / findCorresbyNNMultiPair   src/FeatureManager.cpp:247-288, 370-437
//   SiftManager::pruneMatches / collectMutualMatches        src/FeatureManager.cpp:290-368
// The reference runs OpenCV's CUDA brute-force kNN matcher per pair and direction, downloads the neighbour lists, and
// gates them on the host.  Here every pair of a call, both directions, goes through five launches:
//   k_match_norms   squared descriptor norms of every keypoint (one fmaf chain each)
//   k_match_topk    one workgroup per (pair, direction, 64 query rows): streams the train descriptors through LDS in
//                   64-column tiles, 4 x 4 fmaf-chained dot products per thread, row top-8 in registers (lists split
//                   over four column quarters, merged at the end)
//   k_match_select  one workgroup per pair: the gate, first passing neighbour per query, ordered prefix count
//   k_match_offsets one workgroup: exclusive scan of the pair counts
//   k_match_pack    the records and the model-frame points at their packed positions
// The distance is recomputed for B -> A instead of keeping column lists: d2 is symmetric bit for bit (fmaf(a, b, c) ==
// fmaf(b, a, c), na + nb == nb + na), so both directions rank the same numbers.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>

#include "../../include/btba.h"
#include "btba_device.hpp"
#include "btba_image.hpp"

namespace btba {

constexpr int kMatchKMax = 8;          // top-k lists are always 8 long in registers; the first k are reported
constexpr int kMatchRows = 64, kMatchCols = 64, kMatchDK = 32;
constexpr int kMatchMaxKpts = 8192, kMatchMaxD = 512;

struct MatchFrame {
    const float *desc;                 // [n][D]
    const float2 *kpts;                // [n] (x, y) full-resolution pixels
    const float *depth;                // [H * W]
    const float4 *normal;              // [H * W]
    int n, norm_off, pad0, pad1;
    float pose[12];                    // rows 0..2 of the row-major camera -> model matrix
};
struct MatchPair { int a, b, qbase, pad; float max_dist, cos_max, pad1, pad2; };   // queries of the pair: A's rows, then (mutual) B's rows, from qbase
struct MatchCand { float d2; int idx; };
struct MatchDims { int W, H, D, k, mutual; float min_z; Mat4 Kinv; };

__device__ __forceinline__ bool cand_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

// sorted insertion into the register list (bd, bi) by (d2, index); every index is compile-time after unrolling
__device__ __forceinline__ void topk_insert(float (&bd)[kMatchKMax], int (&bi)[kMatchKMax], float d, int i)
{
    if (!cand_less(d, i, bd[kMatchKMax - 1], bi[kMatchKMax - 1])) return;
#pragma unroll
    for (int m = kMatchKMax - 1; m > 0; m--) {
        const bool above = cand_less(d, i, bd[m - 1], bi[m - 1]);      // the candidate goes above slot m - 1: slot m takes its entry
        const bool here = cand_less(d, i, bd[m], bi[m]);
        bd[m] = above ? bd[m - 1] : (here ? d : bd[m]);
        bi[m] = above ? bi[m - 1] : (here ? i : bi[m]);
    }
    if (cand_less(d, i, bd[0], bi[0])) { bd[0] = d; bi[0] = i; }
}

// grid (ceil(max n / 256), n_frames)
__global__ void __launch_bounds__(256) k_match_norms(const MatchFrame *__restrict__ F, int D, float *__restrict__ norms)
{
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F[f].n) return;
    const float4 *row = reinterpret_cast<const float4 *>(F[f].desc + (size_t)i * D);
    float s = 0.0f;
    for (int k = 0; k < D / 4; k++) {
        const float4 v = row[k];
        s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
    }
    norms[F[f].norm_off + i] = s;
}

// grid (n_pairs, ceil(max n / 64), 1 + mutual) x 256.  Thread (tr, tc) = (tid / 16, tid % 16) owns rows tr + 16 i and columns
// tc + 16 j of a 64 x 64 tile.  Descriptors beyond D are zero-filled to a multiple of kMatchDK: fmaf(0, 0, acc) changes at most
// the sign of a zero accumulator, which the d2 formula cannot see (fmaf(-2, +-0, s) == s for s != 0, and a zero d2 becomes +0).
__global__ void __launch_bounds__(256) k_match_topk(MatchDims M, const MatchFrame *__restrict__ F, const MatchPair *__restrict__ P,
                                                    const float *__restrict__ norms, MatchCand *__restrict__ cand)
{
    __shared__ float qs[kMatchDK][kMatchRows];
    __shared__ float ts[kMatchDK][kMatchCols];
    __shared__ float lds_d[kMatchRows * (kMatchCols + 1)];
    __shared__ int lds_i[3 * kMatchRows * kMatchKMax];
    const int p = blockIdx.x, row0 = blockIdx.y * kMatchRows, dir = blockIdx.z;
    const MatchPair pr = P[p];
    const int fq = dir ? pr.b : pr.a, ft = dir ? pr.a : pr.b;
    const int nq = F[fq].n, nt = F[ft].n, D = M.D;
    if (row0 >= nq) return;
    const float *__restrict__ qd = F[fq].desc;
    const float *__restrict__ td = F[ft].desc;
    const float *qn = norms + F[fq].norm_off, *tn = norms + F[ft].norm_off;
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15, lrow = tid & 63, quarter = tid >> 6;
    float bd[kMatchKMax];
    int bi[kMatchKMax];
#pragma unroll
    for (int m = 0; m < kMatchKMax; m++) { bd[m] = __builtin_inff(); bi[m] = INT_MAX; }
    float qnorm[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { const int r = row0 + tr + 16 * i; qnorm[i] = r < nq ? qn[r] : 0.0f; }
    for (int col0 = 0; col0 < nt; col0 += kMatchCols) {
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = 0.0f;
        for (int kc = 0; kc < D; kc += kMatchDK) {
#pragma unroll
            for (int l = tid; l < kMatchRows * kMatchDK / 4; l += 256) {
                const int r = l >> 3, k4 = (l & 7) * 4;
                float4 vq = make_float4(0.f, 0.f, 0.f, 0.f), vt = vq;
                if (row0 + r < nq && kc + k4 < D) vq = *reinterpret_cast<const float4 *>(qd + (size_t)(row0 + r) * D + kc + k4);
                if (col0 + r < nt && kc + k4 < D) vt = *reinterpret_cast<const float4 *>(td + (size_t)(col0 + r) * D + kc + k4);
                qs[k4][r] = vq.x; qs[k4 + 1][r] = vq.y; qs[k4 + 2][r] = vq.z; qs[k4 + 3][r] = vq.w;
                ts[k4][r] = vt.x; ts[k4 + 1][r] = vt.y; ts[k4 + 2][r] = vt.z; ts[k4 + 3][r] = vt.w;
            }
            __syncthreads();
#pragma unroll 8
            for (int kk = 0; kk < kMatchDK; kk++) {
                float a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; i++) { a[i] = qs[kk][tr + 16 * i]; b[i] = ts[kk][tc + 16 * i]; }
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = col0 + tc + 16 * j;
            const float tnorm = c < nt ? tn[c] : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float x = fmaf(-2.0f, acc[i][j], qnorm[i] + tnorm);
                lds_d[(tr + 16 * i) * (kMatchCols + 1) + tc + 16 * j] = x > 0.0f ? x : 0.0f;
            }
        }
        __syncthreads();
        if (row0 + lrow < nq)
            for (int c = 0; c < 16; c++) {
                const int col = quarter * 16 + c;
                if (col0 + col < nt) topk_insert(bd, bi, lds_d[lrow * (kMatchCols + 1) + col], col0 + col);
            }
        __syncthreads();
    }
    // the four column quarters' lists of a row -> one (quarters 1..3 hand theirs over through LDS)
    if (quarter > 0)
#pragma unroll
        for (int m = 0; m < kMatchKMax; m++) {
            lds_d[((quarter - 1) * kMatchRows + lrow) * kMatchKMax + m] = bd[m];
            lds_i[((quarter - 1) * kMatchRows + lrow) * kMatchKMax + m] = bi[m];
        }
    __syncthreads();
    if (quarter == 0 && row0 + lrow < nq) {
        for (int o = 0; o < 3 * kMatchKMax; o++) {
            const int s = ((o / kMatchKMax) * kMatchRows + lrow) * kMatchKMax + o % kMatchKMax;
            topk_insert(bd, bi, lds_d[s], lds_i[s]);
        }
        const int q = (dir ? F[pr.a].n : 0) + row0 + lrow;
        MatchCand *out = cand + (size_t)(pr.qbase + q) * M.k;
#pragma unroll
        for (int m = 0; m < kMatchKMax; m++)
            if (m < M.k) out[m] = MatchCand{ bd[m], bi[m] };
    }
}

// the reference's pixel lookup: rounded keypoint inside the image, camera-space point with z >= min_z
__device__ __forceinline__ bool match_pixel(const MatchDims &M, const MatchFrame &f, float2 kp, float3 &pt, float3 &nrm)
{
    const float u = roundf(kp.x), v = roundf(kp.y);
    if (!(u >= 0.0f && u < (float)M.W && v >= 0.0f && v < (float)M.H)) return false;
    const int x = (int)u, y = (int)v;
    const size_t o = (size_t)y * M.W + x;
    pt = backproject(M.Kinv.m, x, y, f.depth[o]);
    if (pt.z < M.min_z) return false;
    const float4 n = f.normal[o];
    nrm = make_float3(n.x, n.y, n.z);
    return true;
}

__device__ __forceinline__ float3 match_model_point(const float *T, float3 p)
{
#pragma clang fp contract(off)
    return make_float3(T[0] * p.x + T[1] * p.y + T[2] * p.z + T[3], T[4] * p.x + T[5] * p.y + T[6] * p.z + T[7],
                       T[8] * p.x + T[9] * p.y + T[10] * p.z + T[11]);
}

__device__ __forceinline__ float3 match_model_normal(const float *T, float3 n)
{
#pragma clang fp contract(off)
    float3 r = make_float3(T[0] * n.x + T[1] * n.y + T[2] * n.z, T[4] * n.x + T[5] * n.y + T[6] * n.z, T[8] * n.x + T[9] * n.y + T[10] * n.z);
    const float z = r.x * r.x + r.y * r.y + r.z * r.z;          // Eigen's normalized(): unchanged when the squared norm is 0
    if (z > 0.0f) { const float s = sqrtf(z); r = make_float3(r.x / s, r.y / s, r.z / s); }
    return r;
}

// the gate of one query: slot of the first passing neighbour in its candidate list, or -1
__device__ __forceinline__ int match_gate(const MatchDims &M, const MatchFrame *__restrict__ F, const MatchPair &pr, const MatchCand *__restrict__ cand, int q)
{
#pragma clang fp contract(off)
    const int nA = F[pr.a].n, dir = q >= nA ? 1 : 0;
    const int fq = dir ? pr.b : pr.a, ft = dir ? pr.a : pr.b, row = dir ? q - nA : q;
    const int nc = min(M.k, F[ft].n);
    float3 pq, nq;
    if (nc == 0 || !match_pixel(M, F[fq], F[fq].kpts[row], pq, nq)) return -1;
    const float3 PQ = match_model_point(F[fq].pose, pq), NQ = match_model_normal(F[fq].pose, nq);
    const MatchCand *c = cand + (size_t)(pr.qbase + q) * M.k;
    for (int m = 0; m < nc; m++) {
        float3 pt, nt;
        if (!match_pixel(M, F[ft], F[ft].kpts[c[m].idx], pt, nt)) continue;
        const float3 PT = match_model_point(F[ft].pose, pt), NT = match_model_normal(F[ft].pose, nt);
        const float dx = PQ.x - PT.x, dy = PQ.y - PT.y, dz = PQ.z - PT.z;
        if (sqrtf(dx * dx + dy * dy + dz * dz) > pr.max_dist) continue;
        if (NQ.x * NT.x + NQ.y * NT.y + NQ.z * NT.z < pr.cos_max) continue;
        return m;
    }
    return -1;
}

// grid n_pairs x 256: gate every query of the pair, ordered positions of the kept ones, the pair's count
__global__ void __launch_bounds__(256) k_match_select(MatchDims M, const MatchFrame *__restrict__ F, const MatchPair *__restrict__ P,
                                                      const MatchCand *__restrict__ cand, int *__restrict__ sel, int *__restrict__ pos, int *__restrict__ counts)
{
    __shared__ int wsum[4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MatchPair pr = P[p];
    const int nqt = F[pr.a].n + (M.mutual ? F[pr.b].n : 0);
    int running = 0;
    for (int base = 0; base < nqt; base += 256) {
        const int q = base + tid;
        const int slot = q < nqt ? match_gate(M, F, pr, cand, q) : -1;
        const unsigned long long bal = __ballot(slot >= 0);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int off = running;
        for (int w = 0; w < wave; w++) off += wsum[w];
        if (q < nqt) { sel[pr.qbase + q] = slot; pos[pr.qbase + q] = off + before; }
        running += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) counts[p] = running;
}

// one workgroup of 256: offs = exclusive scan of counts
__global__ void __launch_bounds__(256) k_match_offsets(int n_pairs, const int *__restrict__ counts, int *__restrict__ offs)
{
    __shared__ int s[256];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < n_pairs; base += 256) {
        const int v = base + tid < n_pairs ? counts[base + tid] : 0;
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int add = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        if (base + tid < n_pairs) offs[base + tid] = carry + s[tid] - v;
        carry += s[255];
        __syncthreads();
    }
}

// grid (n_pairs, ceil(max queries / 256)) x 256
__global__ void __launch_bounds__(256) k_match_pack(MatchDims M, const MatchFrame *__restrict__ F, const MatchPair *__restrict__ P,
                                                    const MatchCand *__restrict__ cand, const int *__restrict__ sel, const int *__restrict__ pos,
                                                    const int *__restrict__ offs, btba_match *__restrict__ out, float4 *__restrict__ ptsA, float4 *__restrict__ ptsB)
{
    const int p = blockIdx.x, q = blockIdx.y * 256 + threadIdx.x;
    const MatchPair pr = P[p];
    const int nA = F[pr.a].n, nqt = nA + (M.mutual ? F[pr.b].n : 0);
    if (q >= nqt) return;
    const int slot = sel[pr.qbase + q];
    if (slot < 0) return;
    const int dir = q >= nA ? 1 : 0, row = dir ? q - nA : q;
    const MatchCand c = cand[(size_t)(pr.qbase + q) * M.k + slot];
    const int ia = dir ? c.idx : row, ib = dir ? row : c.idx;
    float3 pa, pb, na, nb;
    match_pixel(M, F[pr.a], F[pr.a].kpts[ia], pa, na);          // passed the gate: both lookups succeed
    match_pixel(M, F[pr.b], F[pr.b].kpts[ib], pb, nb);
    const size_t o = (size_t)offs[p] + pos[pr.qbase + q];
    btba_match &r = out[o];
    r.idx_a = ia; r.idx_b = ib; r.dist = sqrtf(c.d2); r.dir = dir;
    r.ptA_cam[0] = pa.x; r.ptA_cam[1] = pa.y; r.ptA_cam[2] = pa.z;
    r.ptB_cam[0] = pb.x; r.ptB_cam[1] = pb.y; r.ptB_cam[2] = pb.z;
    if (ptsA) { const float3 P3 = match_model_point(F[pr.a].pose, pa); ptsA[o] = make_float4(P3.x, P3.y, P3.z, 1.0f); }
    if (ptsB) { const float3 P3 = match_model_point(F[pr.b].pose, pb); ptsB[o] = make_float4(P3.x, P3.y, P3.z, 1.0f); }
}

}  // namespace btba
