// btba_eval.hpp -- pose accuracy: ADD and ADD-S per evaluation (btba_pose_errors, include/btba.h)
//   add / adi              scripts/Utils.py:69-95
//   eval_all               scripts/eval_ycbineoat.py:86-163
// The reference transforms the model with open3d and answers ADD-S with a cKDTree, one frame at a time on the CPU.  Here a
// call evaluates any number of (model, predicted pose, ground-truth pose) triples in two launches per chunk:
//   k_eval_nn      one workgroup per (evaluation, 1024 queries, candidate split): every lane keeps 8 ground-truth points
//                  q_i = G x_i in registers as four packed pairs; the predicted points c_j = P x_j are transformed into LDS
//                  256 at a time and read back as broadcasts (every lane reads the same float4).  Per (query, candidate):
//                  3 subtracts, 1 multiply, 2 fmaf as v_pk_*_f32 over two queries, and half a v_min3_f32.  The per-point
//                  minimum of d2 goes out as its uint bit pattern: a plain store, or atomicMin when the candidates of an
//                  evaluation are split over workgroups (d2 >= +0, so the uint order is the float order and the result does
//                  not depend on the split).
//   k_eval_reduce  one workgroup per evaluation: add_i recomputed with the same arithmetic, sqrtf of the stored minima,
//                  both summed in fp64 in the fixed slot / tree order, divided by N.
// The exact distance d2 = |q - c|^2 is used, not |q|^2 + |c|^2 - 2 q.c: that expansion cancels at millimetre distances on
// decimetre objects and would break the bit-exact contract.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace btba {

constexpr int kEvalThreads = 128;                     // k_eval_nn: two waves
constexpr int kEvalQPL = 8;                           // queries per lane (four packed pairs)
constexpr int kEvalQTile = kEvalThreads * kEvalQPL;   // 1024 queries per workgroup
constexpr int kEvalCTile = 256;                       // candidates per LDS tile, two per thread; also the split granularity
constexpr int kEvalRedThreads = 256;                  // k_eval_reduce: the 256 slots of the fixed summation order
constexpr int64_t kEvalScratchPoints = 16 << 20;      // per-point minima of one chunk: 64 MB
constexpr int kEvalChunkEvals = 65536;                // evaluations per chunk (bounds the tables)

struct EvalRec { const float *pts; int n, off; };     // model points, N, offset of the evaluation's minima in the chunk

typedef float evf2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool eval_pose_finite(const float *__restrict__ P, const float *__restrict__ G)
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 16; k++) ok &= __builtin_isfinite(P[k]) & __builtin_isfinite(G[k]);     // one test, no branch per entry
    return ok;
}

// p_r = fmaf(T_r2, z, fmaf(T_r1, y, fmaf(T_r0, x, T_r3)))
__device__ __forceinline__ float4 eval_xform(const float *__restrict__ T, const float *__restrict__ x)
{
    const float px = x[0], py = x[1], pz = x[2];
    return make_float4(fmaf(T[2], pz, fmaf(T[1], py, fmaf(T[0], px, T[3]))),
                       fmaf(T[6], pz, fmaf(T[5], py, fmaf(T[4], px, T[7]))),
                       fmaf(T[10], pz, fmaf(T[9], py, fmaf(T[8], px, T[11]))), 0.0f);
}

// d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)), d = a - b
__device__ __forceinline__ float eval_d2(float4 a, float4 b)
{
#pragma clang fp contract(off)
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// The same d2 for two queries at once (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: per lane the bits of the scalar chain).
__device__ __forceinline__ evf2 eval_d2x2(evf2 qx, evf2 qy, evf2 qz, float4 c)
{
#pragma clang fp contract(off)
    const evf2 dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
    return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
}

// grid (evaluations of the chunk, query tiles, candidate splits).  mins: the chunk's per-point minima, 0xffffffff-filled
// beforehand when split != 0.
__global__ void __launch_bounds__(kEvalThreads) k_eval_nn(const EvalRec *__restrict__ R, const float *__restrict__ poses_pred,
                                                          const float *__restrict__ poses_gt, int cand_per_split, int split,
                                                          unsigned *__restrict__ mins)
{
    __shared__ float4 tile[kEvalCTile];
    const int e = blockIdx.x;
    const EvalRec r = R[e];
    const int q0 = blockIdx.y * kEvalQTile, j0 = blockIdx.z * cand_per_split;
    if (q0 >= r.n || j0 >= r.n) return;
    const float *P = poses_pred + 16 * (size_t)e, *G = poses_gt + 16 * (size_t)e;
    if (!eval_pose_finite(P, G)) return;
    const int j1 = min(r.n, j0 + cand_per_split);
    const int tid = threadIdx.x;

    // query s of this lane: q0 + s * kEvalThreads + tid; pair k holds s = 2k (x) and s = 2k + 1 (y).  Lanes past N take the
    // last point (a valid duplicate) and store nothing.
    evf2 qx[kEvalQPL / 2], qy[kEvalQPL / 2], qz[kEvalQPL / 2];
    float m[kEvalQPL];
#pragma unroll
    for (int k = 0; k < kEvalQPL / 2; k++) {
        const int ia = min(q0 + (2 * k) * kEvalThreads + tid, r.n - 1), ib = min(q0 + (2 * k + 1) * kEvalThreads + tid, r.n - 1);
        const float4 a = eval_xform(G, r.pts + 3 * (size_t)ia), b = eval_xform(G, r.pts + 3 * (size_t)ib);
        qx[k] = evf2{ a.x, b.x }; qy[k] = evf2{ a.y, b.y }; qz[k] = evf2{ a.z, b.z };
        m[2 * k] = m[2 * k + 1] = __builtin_inff();
    }

    for (int t0 = j0; t0 < j1; t0 += kEvalCTile) {
        const int cnt = min(kEvalCTile, j1 - t0);
        __syncthreads();                                   // the previous tile is consumed
        for (int c = tid; c < kEvalCTile; c += kEvalThreads)   // pad with the tile's last candidate: min is idempotent
            tile[c] = eval_xform(P, r.pts + 3 * (size_t)(t0 + min(c, cnt - 1)));
        __syncthreads();
        const int cnt2 = (cnt + 1) & ~1;
#pragma unroll 2
        for (int c = 0; c < cnt2; c += 2) {
            const float4 ca = tile[c], cb = tile[c + 1];
#pragma unroll
            for (int k = 0; k < kEvalQPL / 2; k++) {
                const evf2 da = eval_d2x2(qx[k], qy[k], qz[k], ca), db = eval_d2x2(qx[k], qy[k], qz[k], cb);
                m[2 * k] = fminf(m[2 * k], fminf(da.x, db.x));
                m[2 * k + 1] = fminf(m[2 * k + 1], fminf(da.y, db.y));
            }
        }
    }

    unsigned *out = mins + r.off;
#pragma unroll
    for (int s = 0; s < kEvalQPL; s++) {
        const int i = q0 + s * kEvalThreads + tid;
        if (i < r.n) {
            const unsigned bits = __float_as_uint(m[s]);
            if (split) atomicMin(out + i, bits);
            else out[i] = bits;
        }
    }
}

// grid (evaluations of the chunk): ADD and ADD-S of each.
__global__ void __launch_bounds__(kEvalRedThreads) k_eval_reduce(const EvalRec *__restrict__ R, const float *__restrict__ poses_pred,
                                                                 const float *__restrict__ poses_gt, const unsigned *__restrict__ mins,
                                                                 float *__restrict__ add_out, float *__restrict__ adds_out)
{
    __shared__ double acc_a[kEvalRedThreads], acc_s[kEvalRedThreads];
    const int e = blockIdx.x, l = threadIdx.x;
    const EvalRec r = R[e];
    const float *P = poses_pred + 16 * (size_t)e, *G = poses_gt + 16 * (size_t)e;
    if (!eval_pose_finite(P, G)) {
        if (l == 0) add_out[e] = adds_out[e] = __builtin_nanf("");
        return;
    }
    const unsigned *mn = mins + r.off;
    double sa = 0.0, ss = 0.0;
    for (int i = l; i < r.n; i += kEvalRedThreads) {
        const float4 q = eval_xform(G, r.pts + 3 * (size_t)i), c = eval_xform(P, r.pts + 3 * (size_t)i);
        sa += (double)sqrtf(eval_d2(q, c));
        ss += (double)sqrtf(__uint_as_float(mn[i]));
    }
    acc_a[l] = sa;
    acc_s[l] = ss;
#pragma unroll
    for (int s = kEvalRedThreads / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (l < s) { acc_a[l] += acc_a[l + s]; acc_s[l] += acc_s[l + s]; }
    }
    if (l == 0) {
        add_out[e] = (float)(acc_a[0] / (double)r.n);
        adds_out[e] = (float)(acc_s[0] / (double)r.n);
    }
}

}  // namespace btba
