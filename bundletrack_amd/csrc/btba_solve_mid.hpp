// btba_solve_mid.hpp -- k_solve_mid: the per-instance system solve of windows of 22 ... 31 frames in ONE launch (round 6).
//
// BASELINE configs[3] (K = 30 keyframes) ran rounds 1-4's three-launch path until now -- k_big_reduce + k_big_assemble + k_system_solve,
// 5.0 + 11.4 + 20.7 us per Gauss-Newton iteration at c4 x 32 (profiles/r05/bench_c4x32_r05_kernel_stats.csv) -- because k_solve_small
// (btba_solve_small.hpp) keeps the 6 (N - 1) square system matrix in LDS next to the reduced pair sums, which stops fitting one compute
// unit's 160 KB at 22 frames.  The same Gauss-Newton step
//   reduce the sweep partials -> A = w_s JsT Js + JdT Jd, b -> 5 x Jacobi-PCG -> x <- Log(Exp(delta) Exp(x)), T, T^-1
// (SolverBundling.cu:575-651, 692-818, 805-815, 890-897; SolverBundlingDenseUtil.h:349-385) with the matrix NEVER in LDS:
//
//   reduce     as k_solve_small: the pair sums (sparse [P][44], dense [Pd][28]: 125 KB at K = 30) land in LDS, one fabric round trip
//   frame sums as k_solve_small: a frame's 20 sparse and 27 dense sums over its pairs, formed first, expanded once
//   assemble   GATHER, into registers: four lanes own a matrix row, 48 columns (8 frame blocks) each, and form their 48 entries from
//              the pair sums in LDS -- cross blocks from the pair's record through the 36-entry descriptor table (transposed below the
//              diagonal), the diagonal block from the frame sums.  k_solve_small scatters the same values into an LDS matrix and then
//              loads its rows into registers for the PCG; here the rows are born there.
//   PCG        as k_solve_small, four lanes per row: a step = 24 packed FMAs per lane against p (12 broadcast 16-byte LDS reads), two DPP
//              adds, A p through LDS, a barrier, the dot products and vector updates on wave 0 alone (three entries per lane: <= 192
//              unknowns), a barrier
//   update     as k_solve_small: one lane per frame for Exp / Log, sixteen lanes per frame for the generic cofactor inverse
// Everything "as k_solve_small" is that kernel's code: btba_solve_phases.hpp.
//
// The same sums as k_system_solve / k_solve_small, in another order (the gate is the parity suite: c4 per iterate against the oracle and
// against the reference's own solver, tests/test_gpu_fullsize.py, test_gpu_vs_reference.py; this kernel against k_system_solve,
// tests/test_gpu_parity.py).
#pragma once
#include "btba_solve_phases.hpp"

namespace btba {

constexpr int kMidMaxFrames = 31;        // BTBA_MAX_FRAMES_LDS: 6 (N - 1) <= 180 unknowns, P <= 465 pairs: pair sums + tables <= 160 KB of LDS
constexpr int kMidCPL = 48;              // matrix columns per lane, four lanes per row: 192 columns
constexpr int kMidNA = 4 * kMidCPL;

struct MidLayout {
    static constexpr int NF = kMidMaxFrames, NP = NF * (NF - 1) / 2;
    static constexpr int lv = kMidNA + 4;                                    // a vector: 192 entries + a 16-byte pad
    static constexpr int op = 0, oAp = op + lv, ob = oAp + lv, oM = ob + lv, od = oM + lv;
    static constexpr int oT = od + lv;                                       // this iterate's T [N][16]
    static constexpr int oE = oT + 16 * NF;                                  // the next iterate's T
    static constexpr int ox = oE + 16 * NF;                                  // this iterate's x
    static constexpr int oF = ox + round4(6 * NF);                           // frame sums [(N - 1)][48]
    static constexpr int olut = oF + (NF - 1) * kFrameSums;                  // ints: the 72 entry descriptors (36 diagonal-block, 36 cross-block)
    static constexpr int opij = olut + 288;                                  // ints: canonical pair -> (i << 8 | j)
    static constexpr int ocross = opij + round4(NP);                         // ints: canonical pair -> dense pair with its cross block
    static constexpr int oadjoff = ocross + round4(NP);                      // ints: N + 1
    static constexpr int oadj = oadjoff + round4(NF + 1);                    // ints: 2 Pd <= 2 NP (the host sends explicit lists with more dense pairs to k_system_solve)
    static constexpr int ops = oadj + round4(2 * NP);                        // reduced sparse pair sums [P][44], behind them the dense ones [Pd][28]
    static constexpr int fixed = ops;
};
__host__ inline size_t mid_solve_lds_floats(int N, int Pd)
{
    return (size_t)MidLayout::fixed + (size_t)(N * (N - 1) / 2) * kSparseVals + (size_t)Pd * kDenseVals + 8 * kSparseVals + 16;      // (+ slack: the frame sums' unconditional loads run past the last pair)
}

__global__ void __launch_bounds__(kSmallBlock) k_solve_mid(const SmallSolveArgs S)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using L = MidLayout;
    constexpr unsigned nthr = kSmallBlock;
    const unsigned tid = threadIdx.x, b = blockIdx.x;
    const int N = S.n_frames, P = S.n_pairs, Pd = S.n_dense_pairs, na = 6 * (N - 1);
    float *vp = lds + L::op, *vAp = lds + L::oAp, *vb = lds + L::ob, *vM = lds + L::oM, *vd = lds + L::od;
    float *vT = lds + L::oT, *vE = lds + L::oE, *x_l = lds + L::ox, *F = lds + L::oF;
    int *lut_l = reinterpret_cast<int *>(lds + L::olut);
    int *pair_ij_l = reinterpret_cast<int *>(lds + L::opij), *cross_l = reinterpret_cast<int *>(lds + L::ocross);
    int *adj_off_l = reinterpret_cast<int *>(lds + L::oadjoff), *adj_l = reinterpret_cast<int *>(lds + L::oadj);
    float *ps = lds + L::ops, *pd = ps + __umul24(P, kSparseVals);

    float *tr = S.trace ? S.trace + (size_t)b * (size_t)S.trace_instance + (size_t)S.iter * S.trace_record : nullptr;
    const long long clk0 = tr ? (long long)clock64() : 0;

    // ---- phase 1: everything this solve reads from global memory, issued at once, loads and stores unconditional (btba_solve_phases.hpp).
    // Four slots per lane in flight when there is one partial per sum (K = 30: 7 830 slots)
    const StagedTables st(S, tid, b, N, P, Pd);
    const int st_lut = S.entry_lut[min(tid, 287u)];
    reduce_partials<4>(S, tid, b, P, Pd, ps, pd);
    st.store(tid, N, P, Pd, vT, x_l, pair_ij_l, cross_l, adj_off_l, adj_l);
    lut_l[min(tid, 287u)] = st_lut;
    if (tid < (unsigned)(L::lv - na)) vp[na + tid] = 0.0f;                   // p beyond na: the padded columns multiply zeros
    BTBA_SOLVE_STAMP(0);
    __syncthreads();
    BTBA_SOLVE_STAMP(1);

    const float w_s = S.use_sparse ? S.w_sparse : 0.0f;
    // ---- phase 2b: frame sums (dense ones on lanes 640 ..: behind the 600 sparse lanes of a 31-frame window)
    frame_sums<640u>(tid, N, P, Pd, ps, pd, adj_off_l, adj_l, F);
    __syncthreads();
    BTBA_SOLVE_STAMP(2);

    // ---- phase 2c: the matrix rows, gathered into registers.  Lane (row a_row, quarter h) owns columns 48 h .. 48 h + 47 = the 6 x 6 blocks of column
    // frames 8 h .. 8 h + 7 (frame indices without the fixed frame 0).  Entry (r, c) of the block (row frame i, column frame j):
    //   i <  j   -(w_s (J_i^T J_j)[r][c] + S_dense[r][c])        from the canonical pair (i, j)'s record, descriptor (r, c)
    //   i >  j   the transpose: pair (j, i)'s entry (c, r)        (SolverBundlingDenseUtil.h:349-385; FlipJtJ mirrors the kept triangle)
    //   i == j   w_s (diagonal block of the frame's sparse sums) + the frame's dense S                                  (frame sums)
    // Right-hand side, Jacobi diagonal and p_0 on the lanes behind the row lanes.
    const PcgRows<4> R(tid, na);                                             // 16 rows per wave
    f2 Ar[kMidCPL / 2];
    if (R.pw) {
        const int a_c = min(R.a_row, na - 1);
        const int i1 = a_c / 6, r = a_c - 6 * i1;
        unsigned t21r[6];
#pragma unroll
        for (int c = 0; c < 6; c++) t21r[c] = (unsigned)tri21(r, c);
        const int4 *lut4 = reinterpret_cast<const int4 *>(lut_l);
#pragma unroll
        for (int jj = 0; jj < 8; jj++) {
            const int jf = 8 * R.h + jj;
            const bool col_live = jf < N - 1;
            const int jc = min(jf, N - 2);
            float v[6];
            if (jc == i1) {
                const float *Fk = F + __umul24((unsigned)i1, kFrameSums);
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    const int4 d = lut4[6 * r + c];
                    const unsigned q1 = d.x & 255, q2 = d.y;                // indices into (n, s[3], -, M[6]) of endpoint i -> frame sums 0, 1..3, 4..9
                    const unsigned di1 = q1 < 4 ? q1 : q1 - 3, di2 = q2 < 4 ? q2 : q2 - 3;
                    float e = w_s * (__int_as_float(d.z) * Fk[di1] + __int_as_float(d.w) * Fk[di2]);
                    if (Pd) e += Fk[20 + t21r[c]];
                    v[c] = e;
                }
            } else {
                const bool upper = i1 < jc;
                const int lo = upper ? i1 : jc, hi = upper ? jc : i1;       // canonical pair (lo + 1, hi + 1)
                const int p = (lo + 1) * N - ((lo + 1) * (lo + 2)) / 2 + (hi - lo - 1);
                const int dq = cross_l[p];
                const float *rec = ps + __umul24((unsigned)p, kSparseVals);
                const float *sdp = pd + __umul24((unsigned)max(dq, 0), kDenseVals);
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    const int4 d = lut4[36 + (upper ? 6 * r + c : 6 * c + r)];
                    const float m1 = rec[d.x & 255], m2 = rec[d.y];
                    const float sd = Pd ? sdp[t21r[c]] : 0.0f;
                    v[c] = -(w_s * (__int_as_float(d.z) * m1 + __int_as_float(d.w) * m2)) - (dq >= 0 ? sd : 0.0f);
                }
            }
#pragma unroll
            for (int c = 0; c < 6; c += 2) Ar[3 * jj + c / 2] = col_live ? (f2){ v[c], v[c + 1] } : (f2){ 0.f, 0.f };
        }
    }
    rhs_precond_p0(tid, 64u * ((unsigned)(na + 15) >> 4), na, w_s, Pd, F, vb, vM, vp);      // on the lanes behind the row waves
    __syncthreads();
    BTBA_SOLVE_STAMP(3);
    if (tr) {
        trace_system(S, tr, tid, N, Pd, vb, vM, pd);
        const int n = 6 * N;
        for (int e = (int)tid; e < n * n; e += nthr) { const int row = e / n, col = e - row * n; if (row < 6 || col < 6) tr[S.tr_A + e] = 0.0f; }
        if (R.row_live) {
#pragma unroll
            for (int k = 0; k < kMidCPL / 2; k++) {
                const int col = kMidCPL * R.h + 2 * k;
                if (col < na) tr[S.tr_A + (size_t)(R.a_row + 6) * n + col + 6] = Ar[k].x;
                if (col + 1 < na) tr[S.tr_A + (size_t)(R.a_row + 6) * n + col + 7] = Ar[k].y;
            }
        }
    }
    BTBA_SOLVE_STAMP(4);

    pcg<kMidCPL, 4>(S, tr, tid, na, R, Ar, vp, vAp, vb, vM, vd);
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
