// btba_solve_small.hpp -- k_solve_small: the per-instance system solve of tracker-sized windows (N <= 21 frames), round 5.
//
// Replaces k_system_solve (btba_kernels.hpp) wherever the window fits; what it computes is the same Gauss-Newton step
//   reduce the sweep partials -> A = w_s JsT Js + JdT Jd, b -> 5 x Jacobi-PCG -> x <- Log(Exp(delta) Exp(x)), T, T^-1
// of SolverBundling.cu:575-651 (PCGInit), :692-818 (PCGStep / epsilon guards), :805-815 + :890-897 (update, matrices) and
// SolverBundlingDenseUtil.h:349-385 (dense blocks), with the SAME sums but NOT in k_system_solve's order: round 4's verdict asked
// for the kernel to become shorter instead of hidden, and dropped the "same bits as round 1" rule for it (gate: the parity suite
// and the decision traces against the oracle / the reference).
//
// What bounds a kernel like this (profiles/r05/solve_small.json): ONE workgroup per instance on one compute unit, a chain of short
// dependent phases (k_system_solve: 44 k cycles = reduce 10.6 k + assemble 11.2 k + PCG 13.5 k + update 7.9 k, profiles/r03/
// system_solve_experiments.json).  Measured while writing this kernel:
//   * a wave ALONE on its SIMD retires one instruction per ~10-12 cycles (dependent issue + LDS round trips it cannot hide): phases
//     with work for everybody run on all 16 waves (4 per SIMD: one instruction per 4 cycles per SIMD), whatever their set-up costs --
//     a 256-thread version of this kernel took 35 k cycles against 24 k -- and only the truly serial chains run on one wave;
//   * every vector instruction that all 16 waves execute costs 16 cycles of the compute unit: per-lane set-up and index arithmetic
//     are what the throughput phases consist of, so they are cut to the bone (descriptors from the host's table, compile-time LDS
//     offsets, 24-bit multiplies, no 64-bit address arithmetic, no divisions);
//   * hipcc sinks a load into the conditional block that uses it and then waits for every load in turn (first version: eight
//     serial fabric round trips in the reduce phase): loads and stores are UNCONDITIONAL here -- dead slots repeat the last live one;
//   * a cold instruction cache is NOT what bounds it (the body run twice: the second pass is no faster).
//
// Every phase that k_solve_mid (btba_solve_mid.hpp) runs too lives in btba_solve_phases.hpp; this file keeps the layout and the assembly.
//   reduce     (reduce_partials) 16-byte loads -> 16-byte LDS stores; source index = destination index when there is one partial per sum
//              (every chip-filling batch): ONE fabric round trip; up to eight partials of two slots per lane in flight otherwise.
//   assemble   a lane keeps ONE (row, column) of the 6 x 6 block pattern for its lifetime and walks pairs -- no per-entry decode
//              (e / 36, pair_index, tri21).  Diagonal blocks: the sparse blocks are LINEAR in the pair's moment sums, so a frame's 20
//              sparse and 27 dense sums over its pairs are formed first (frame_sums: 20 (N - 1) lanes with one sparse sum each, 7 (N - 1)
//              lanes with four dense sums each, loads batched) and expanded once, instead of expanding every pair's block and summing 36
//              entries x 14 pairs.
//   PCG        (pcg) the matrix is read from LDS ONCE into registers -- eight lanes per row, CPL columns each, 8 rows per wave -- and a
//              step is: packed FMAs against p (broadcast reads), three DPP adds, A p through LDS, a barrier, the two dot products
//              and vector updates on ONE wave alone on its SIMD, a barrier.  alpha and beta by v_rcp_f32 (1 ulp; the reference is
//              built with -use_fast_math), guards as they stand.
//   update     (update_poses, invert_poses) one lane per frame for Exp / Log; the generic cofactor inverse (float4x4::getInverse, ~300
//              instructions of the chain) on sixteen lanes per frame: one adjugate entry each, the same six products per entry.
//
// LDS-resident; frame 0 (fixed) has no rows or columns here.
#pragma once
#include "btba_solve_phases.hpp"

namespace btba {

constexpr int kSmallMaxFrames = 21;      // 6 (N - 1) <= 128 unknowns: two vector entries per lane of the wave that runs the PCG's serial part, 16 waves x 8 matrix rows;
                                         // every per-window table of the kernel fits one trip of its 1 024 lanes (2 Pd <= 2 N (N - 1) = 840 adjacency entries)

__host__ __device__ constexpr int small_lda(int cpl) { return 4 * ((2 * cpl) | 1); }      // row length 8 CPL, padded to an odd multiple of 4 floats: 16-byte rows, conflict-free 16-byte reads down a column of rows
// columns per lane the PCG is compiled for (eight lanes per matrix row): the smallest instantiation with 8 CPL >= 6 (N - 1)
__host__ inline int small_cpl(int n_frames) { const int na = 6 * (n_frames - 1); return na <= 32 ? 4 : na <= 64 ? 8 : na <= 96 ? 12 : 16; }

// LDS layout of k_solve_small<CPL>, in floats: every region is sized for the LARGEST window of the instantiation, so that every address
// in the kernel is a compile-time offset (plus an index); only the dense pair sums, at the end, have a run-time size.
template <int CPL>
struct SmallLayout {
    static constexpr int NA = 8 * CPL;                                       // unknowns (rows / columns) provided for
    static constexpr int NF = (NA / 6 + 1) < kSmallMaxFrames ? (NA / 6 + 1) : kSmallMaxFrames;      // frames
    static constexpr int NP = NF * (NF - 1) / 2;                             // canonical pairs
    static constexpr int lda = small_lda(CPL);
    static constexpr int oA = 0;                                             // [NA][lda] system matrix (frame 0 has no rows / columns); columns na .. 8 CPL - 1 zero
    static constexpr int op = oA + NA * lda;                                 // p (zero beyond na)
    static constexpr int oAp = op + lda;                                     // A p, two buffers
    static constexpr int ob = oAp + 2 * lda, oM = ob + lda, od = oM + lda;   // right-hand side, Jacobi preconditioner, delta
    static constexpr int oT = od + lda;                                      // this iterate's T [N][16]
    static constexpr int oE = oT + 16 * NF;                                  // the next iterate's T (input of the sixteen-lane inverse)
    static constexpr int ox = oE + 16 * NF;                                  // this iterate's x
    static constexpr int oF = ox + round4(6 * NF);                           // frame sums [(N - 1)][48]
    static constexpr int opij = oF + (NF - 1) * kFrameSums;                  // ints: canonical pair -> (i << 8 | j)
    static constexpr int ocross = opij + round4(NP);                         // ints: canonical pair -> dense pair with its cross block
    static constexpr int oadjoff = ocross + round4(NP);                      // ints: N + 1
    static constexpr int oadj = oadjoff + round4(NF + 1);                    // ints: 2 Pd <= 4 NP (an explicit list may name every ordered pair)
    static constexpr int ops = oadj + 4 * NP;                                // reduced sparse pair sums [P][44] ...
    static constexpr int fixed = ops;                                        // ... and behind them the dense ones [Pd][28] (model frame: dense_epilogue): at ops + P * 44
};
__host__ inline size_t small_solve_lds_floats(int N, int Pd, int cpl)
{
    const size_t fixed = cpl == 4 ? SmallLayout<4>::fixed : cpl == 8 ? SmallLayout<8>::fixed : cpl == 12 ? SmallLayout<12>::fixed : SmallLayout<16>::fixed;
    return fixed + (size_t)(N * (N - 1) / 2) * kSparseVals + (size_t)Pd * kDenseVals + 8 * kSparseVals + 16;      // (+ eight records of slack: the frame sums' unconditional loads run past the last pair)
}

template <int CPL>
__global__ void __launch_bounds__(kSmallBlock) k_solve_small(const SmallSolveArgs S)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using L = SmallLayout<CPL>;
    constexpr unsigned nthr = kSmallBlock;
    constexpr int lda = L::lda;
    const unsigned tid = threadIdx.x, b = blockIdx.x;
    const int N = S.n_frames, P = S.n_pairs, Pd = S.n_dense_pairs, na = 6 * (N - 1);
    float *A = lds + L::oA, *vp = lds + L::op, *vAp = lds + L::oAp, *vb = lds + L::ob, *vM = lds + L::oM, *vd = lds + L::od;
    float *vT = lds + L::oT, *vE = lds + L::oE, *x_l = lds + L::ox, *F = lds + L::oF;
    int *pair_ij_l = reinterpret_cast<int *>(lds + L::opij), *cross_l = reinterpret_cast<int *>(lds + L::ocross);
    int *adj_off_l = reinterpret_cast<int *>(lds + L::oadjoff), *adj_l = reinterpret_cast<int *>(lds + L::oadj);
    float *ps = lds + L::ops, *pd = ps + __umul24(P, kSparseVals);

    float *tr = S.trace ? S.trace + (size_t)b * (size_t)S.trace_instance + (size_t)S.iter * S.trace_record : nullptr;
    const long long clk0 = tr ? (long long)clock64() : 0;

    // ---- phase 1: everything this solve reads from global memory, issued at once, loads and stores unconditional (btba_solve_phases.hpp)
    // thread constants.  Entry role: lanes 0 .. 1007 keep one (row r, column c) of the 6 x 6 block pattern ([trans, rot] order) and one of 28
    // pair groups; the two descriptors of that entry -- value = c1 rec[i1] + c2 rec[i2] -- come from the host's table
    const unsigned grp = tid / 36u, rc = tid - 36u * grp, r6 = rc / 6u, c6 = rc - 6u * r6;
    const int4 lut_d = *reinterpret_cast<const int4 *>(S.entry_lut + 4 * rc), lut_x = *reinterpret_cast<const int4 *>(S.entry_lut + 4 * (36 + rc));
    const StagedTables st(S, tid, b, N, P, Pd);
    reduce_partials<2>(S, tid, b, P, Pd, ps, pd);
    st.store(tid, N, P, Pd, vT, x_l, pair_ij_l, cross_l, adj_off_l, adj_l);
    // zero what the assembly does not write and the PCG reads: the matrix columns na .. 8 CPL - 1 and p beyond na
    {
        const int padc = 8 * CPL - na;
        if (padc > 0) for (int e = (int)tid; e < na * padc; e += nthr) { const int row = e / padc, q = e - row * padc; A[row * lda + na + q] = 0.0f; }
        if (tid < (unsigned)(lda - na)) vp[na + tid] = 0.0f;
    }
    BTBA_SOLVE_STAMP(0);
    __syncthreads();
    BTBA_SOLVE_STAMP(1);

    const float w_s = S.use_sparse ? S.w_sparse : 0.0f;
    const unsigned t21 = tri21((int)r6, (int)c6);
    // ---- phase 2a: off-diagonal blocks.  Lane (group g, entry rc) walks the canonical pairs (N - 1) + g, + 28, ... (the pairs with i >= 1):
    //   A_ij[r][c] = -(w_s (J_i^T J_j)[r][c] + S_dense[r][c]),  A_ji = A_ij^T     (SolverBundlingDenseUtil.h:349-385; FlipJtJ keeps the (target lower) listing)
    if (tid < 1008u) {
        const unsigned xi1 = lut_x.x & 255, xi2 = lut_x.y;
        const float xc1 = __int_as_float(lut_x.z), xc2 = __int_as_float(lut_x.w);
        constexpr int kU = 4;                                                // pairs per lane and batch: their table entries, then their sums, are read together
        for (int p0 = (N - 1) + (int)grp; p0 < P; p0 += 28 * kU) {
            int pij[kU], dq[kU];
#pragma unroll
            for (int u = 0; u < kU; u++) { const int p = min(p0 + 28 * u, P - 1); pij[u] = pair_ij_l[p]; dq[u] = cross_l[p]; }      // (a dead slot repeats pair P - 1: the same values to the same places)
            float m1[kU], m2[kU], sd[kU];
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const float *rec = ps + __umul24(min(p0 + 28 * u, P - 1), kSparseVals);
                m1[u] = rec[xi1]; m2[u] = rec[xi2];
                sd[u] = Pd ? pd[__umul24(max(dq[u], 0), kDenseVals) + t21] : 0.0f;       // (no dense pair for this canonical pair: pair 0's value, dropped below)
            }
#pragma unroll
            for (int u = 0; u < kU; u++) {
                const unsigned i = (pij[u] >> 8) - 1, j = (pij[u] & 255) - 1;
                const float v = -(w_s * (xc1 * m1[u] + xc2 * m2[u])) - (dq[u] >= 0 ? sd[u] : 0.0f);
                A[__umul24(6u * i + r6, lda) + 6u * j + c6] = v;
                A[__umul24(6u * j + c6, lda) + 6u * i + r6] = v;
            }
        }
    }
    // ---- phase 2b: frame sums (dense ones on lanes 576 ..: behind the 400 sparse lanes of a 21-frame window)
    frame_sums<576u>(tid, N, P, Pd, ps, pd, adj_off_l, adj_l, F);
    __syncthreads();
    BTBA_SOLVE_STAMP(2);

    // ---- phase 2c: diagonal blocks, right-hand side, Jacobi diagonal from the frame sums
    if (tid < 36u * (N - 1)) {
        const unsigned i1 = lut_d.x & 255, i2 = lut_d.y;                     // indices into (n, s[3], -, M[6]) of endpoint i -> frame sums 0, 1..3, 4..9
        const unsigned di1 = i1 < 4 ? i1 : i1 - 3, di2 = i2 < 4 ? i2 : i2 - 3;
        const float dc1 = __int_as_float(lut_d.z), dc2 = __int_as_float(lut_d.w);
        const float *Fk = F + __umul24(grp, kFrameSums);                     // frame grp + 1
        float v = w_s * (dc1 * Fk[di1] + dc2 * Fk[di2]);
        if (Pd) v += Fk[20 + t21];
        A[__umul24(6u * grp + r6, lda) + 6u * grp + c6] = v;
    }
    rhs_precond_p0(tid, 36u * (N - 1), na, w_s, Pd, F, vb, vM, vp);
    __syncthreads();
    BTBA_SOLVE_STAMP(3);
    if (tr) {
        trace_system(S, tr, tid, N, Pd, vb, vM, pd);
        const int n = 6 * N;
        for (int e = (int)tid; e < n * n; e += nthr) { const int row = e / n, col = e - row * n; tr[S.tr_A + e] = (row < 6 || col < 6) ? 0.0f : A[(row - 6) * lda + col - 6]; }
    }
    BTBA_SOLVE_STAMP(4);

    // ---- phase 3: the PCG on the matrix rows in registers: 8 rows x 8 lanes per wave (~3 waves per SIMD own rows)
    {
        const PcgRows<8> R(tid, na);
        f2 Ar[CPL / 2];
        if (R.pw) {
            const float4 *src = reinterpret_cast<const float4 *>(A + min(R.a_row, na - 1) * lda + R.h * CPL);
#pragma unroll
            for (int k = 0; k < CPL / 4; k++) { const float4 v = src[k]; Ar[2 * k] = (f2){ v.x, v.y }; Ar[2 * k + 1] = (f2){ v.z, v.w }; }
        }
        pcg<CPL, 8>(S, tr, tid, na, R, Ar, vp, vAp, vb, vM, vd);
    }
    __syncthreads();
    BTBA_SOLVE_STAMP(5);

    // ---- phase 4: the update, one lane per frame, and the inverse of the new T on sixteen lanes per frame
    update_poses<BTBA_SOLVE_FAST_SE3>(S, tr, tid, b, N, x_l, vd, vT, vE);
    BTBA_SOLVE_STAMP(6);
    __syncthreads();
    invert_poses<BTBA_SOLVE_FAST_SE3>(S, tid, b, N, vE);
    BTBA_SOLVE_STAMP(7);
}

}  // namespace btba
