// btba_solve_phases.hpp -- the phases that k_solve_small (btba_solve_small.hpp) and k_solve_mid (btba_solve_mid.hpp) share.
//
// Both kernels run one workgroup of 1 024 lanes per instance through
//   reduce the sweep partials -> frame sums -> (their own assembly) -> right-hand side, Jacobi diagonal -> PCG -> update -> T^-1
// and differ in where the system matrix lives.  What does not depend on that is here, once, as forced-inline functions over the
// calling kernel's LDS pointers: a template constant where the two differ (slots in flight, first lane of a role, columns per lane,
// lanes per row), no run-time argument that the kernels did not have.  The measurements that shaped each phase are in
// btba_solve_small.hpp's header; tests/hip/btba_probe.hip runs update_frame and inverse_on_sixteen_lanes from here as the kernels do.
#pragma once
#include "btba_kernels.hpp"

#ifndef BTBA_SOLVE_FAST_SE3
#define BTBA_SOLVE_FAST_SE3 true     // the update phase's divisions and square roots as x * v_rcp_f32(y) / v_sqrt_f32 (btba_device.hpp: se3_div, se3_sqrt); false = IEEE, rounds 5's kernel
#endif

// clock stamp `slot` of the trace record, by lane 0 (uses the kernel's S, tr, tid and clk0)
#define BTBA_SOLVE_STAMP(slot) do { if (tr && tid == 0) tr[S.tr_clk + (slot)] = (float)((long long)clock64() - clk0); } while (0)

namespace btba {

constexpr int kSmallBlock = 1024;
constexpr int kFrameSums = 48;           // floats per frame of the frame-sum table (20 sparse + 27 dense used)

typedef float f2 __attribute__((ext_vector_type(2)));
typedef btba_f4v v4;                     // (the native vector type: one global_load_dwordx4 / ds_write_b128 each)

struct SmallSolveArgs {
    int n_frames, n_pairs, n_dense_pairs;        // N, P = N (N - 1) / 2, dense pairs in THIS iteration (0: dense term off)
    int sparse_chunks, dense_tiles, n_pcg, use_sparse;
    float w_sparse;
    unsigned sp_stride, dp_stride;               // floats per instance in the sweep partials
    int pose_stride, x_stride;
    int iter;
    const float *sparse_partials, *dense_partials;
    const int *adj_off, *adj, *cross, *pair_ij;  // dense adjacency (frame -> (pair << 1 | is_source)), canonical pair -> dense pair carrying its cross block (-1: none), canonical pair -> (i << 8 | j)
    const int *entry_lut;                        // 72 x 4 ints: sparse_entry_descriptor of the 36 diagonal-block and the 36 cross-block entries
    float *x, *T, *Tinv, *poses_out, *trace;
    int64_t trace_record, tr_x, tr_T, tr_rhs, tr_prec, tr_pcg, tr_delta, tr_dpair, tr_A, tr_clk, trace_instance;      // trace_instance: floats per instance (n_gn records)
};

__host__ __device__ constexpr int round4(int v) { return (v + 3) & ~3; }

// ---- phase 1: everything a solve reads from global memory, issued at once (every load is a fabric-latency miss: the sweeps of other
// XCDs wrote the partials, the previous launch the poses).  Loads and stores WITHOUT conditions around them (btba_solve_small.hpp's
// header): a dead slot repeats the last live one.
//
// The small per-window tables: one trip of the 1 024 lanes covers every window of either kernel.  Construct BEFORE reduce_partials, store()
// after it: the loads are then in flight under the reduce loop, where a load-then-store helper would wait for each in turn.
struct StagedTables {
    float T, x;
    int pij, cross, ao, adj;
    __device__ __forceinline__ StagedTables(const SmallSolveArgs &S, unsigned tid, unsigned b, int N, int P, int Pd)
    {
        const float *T_in = S.T + __umul24(b, (unsigned)S.pose_stride), *x_in = S.x + __umul24(b, (unsigned)S.x_stride);
        T = T_in[min(tid, 16u * N - 1u)];
        x = x_in[min(tid, 6u * N - 1u)];
        pij = S.pair_ij[min(tid, (unsigned)P - 1u)];
        cross = Pd ? S.cross[min(tid, (unsigned)P - 1u)] : -1;
        ao = Pd ? S.adj_off[min(tid, (unsigned)N)] : 0;
        adj = Pd ? S.adj[min(tid, 2u * Pd - 1u)] : 0;
    }
    __device__ __forceinline__ void store(unsigned tid, int N, int P, int Pd, float *vT, float *x_l, int *pair_ij_l, int *cross_l, int *adj_off_l, int *adj_l) const
    {
        vT[min(tid, 16u * N - 1u)] = T;
        x_l[min(tid, 6u * N - 1u)] = x;
        pair_ij_l[min(tid, (unsigned)P - 1u)] = pij; cross_l[min(tid, (unsigned)P - 1u)] = cross;
        if (Pd) { adj_off_l[min(tid, (unsigned)N)] = ao; adj_l[min(tid, 2u * Pd - 1u)] = adj; }
    }
};

// The sweep partials -> the reduced pair sums in LDS: sparse [P][44] at ps (zeros when the sparse term is off: read with weight 0), dense
// [Pd][28] at pd.  16-byte loads -> 16-byte LDS stores; SLOTS of them per lane in flight when there is one partial per sum.
template <int SLOTS>
__device__ __forceinline__ void reduce_partials(const SmallSolveArgs &S, unsigned tid, unsigned b, int P, int Pd, float *ps, float *pd)
{
    constexpr unsigned nthr = kSmallBlock;
    const v4 *sp4 = reinterpret_cast<const v4 *>(S.sparse_partials + (size_t)b * S.sp_stride);
    const v4 *dp4 = reinterpret_cast<const v4 *>(S.dense_partials + (size_t)b * S.dp_stride);
    constexpr int kS4 = kSparseVals / 4, kD4 = kDenseVals / 4;
    const int ns4 = S.use_sparse ? P * kS4 : 0, nd4 = Pd * kD4, n4 = ns4 + nd4;
    v4 *ps4 = reinterpret_cast<v4 *>(ps), *pd4 = reinterpret_cast<v4 *>(pd);
    if (S.sparse_chunks == 1 && S.dense_tiles == 1) {
        // one partial per sum (every chip-filling batch): the reduced arrays ARE the partial arrays -- source index = destination index, ONE fabric round trip
        for (int e0 = (int)tid; e0 < n4; e0 += SLOTS * nthr) {
            int e_[SLOTS]; v4 f_[SLOTS];
#pragma unroll
            for (int u = 0; u < SLOTS; u++) { e_[u] = u ? min(e0 + u * (int)nthr, n4 - 1) : e0; f_[u] = *(e_[u] < ns4 ? sp4 + e_[u] : dp4 + (e_[u] - ns4)); }
#pragma unroll
            for (int u = 0; u < SLOTS; u++) *(e_[u] < ns4 ? ps4 + e_[u] : pd4 + (e_[u] - ns4)) = f_[u];
        }
    } else {
        // several partials per sum (small batches: up to 16 chunks / 8 tiles): two slots per lane, four or eight partials of each in flight; sums in partial order
        const int max_parts = max(S.sparse_chunks, S.dense_tiles);
        for (int e0 = (int)tid; e0 < n4; e0 += 2 * nthr) {
            const v4 *src[2]; int per[2], parts[2], e_[2];
            v4 acc[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int e = min(e0 + u * (int)nthr, n4 - 1);
                const bool sp = e < ns4;
                const int q = sp ? e : e - ns4, rec = sp ? q / kS4 : q / kD4;
                e_[u] = e; per[u] = sp ? kS4 : kD4; parts[u] = sp ? S.sparse_chunks : S.dense_tiles;
                src[u] = (sp ? sp4 : dp4) + __umul24(__umul24(rec, parts[u]), per[u]) + (q - rec * per[u]);
                acc[u] = (v4){ 0.f, 0.f, 0.f, 0.f };
            }
            // rounds of four partials per slot while that covers the sums (a single tracker window: 4 chunks x 3 tiles -- eight-wide rounds would issue
            // as many clamped repeats as loads), of eight beyond (8 tiles at B = 1 on full frames)
            auto round = [&](auto width_c, int c0) {
                constexpr int kW = decltype(width_c)::value;
                v4 g[2][kW];
#pragma unroll
                for (int u = 0; u < 2; u++)
#pragma unroll
                    for (int c = 0; c < kW; c++) g[u][c] = src[u][__umul24(c0 + c < parts[u] ? c0 + c : 0, per[u])];
#pragma unroll
                for (int u = 0; u < 2; u++)
#pragma unroll
                    for (int c = 0; c < kW; c++) { const bool live = c0 + c < parts[u]; acc[u] += (v4){ live ? g[u][c].x : 0.0f, live ? g[u][c].y : 0.0f, live ? g[u][c].z : 0.0f, live ? g[u][c].w : 0.0f }; }      // (a dead partial adds an exact zero -- a select, as everywhere in these kernels: a non-finite partial 0 must not leak through 0 x inf)
            };
            if (max_parts <= 4) round(std::integral_constant<int, 4>{}, 0);
            else for (int c0 = 0; c0 < max_parts; c0 += 8) round(std::integral_constant<int, 8>{}, c0);
#pragma unroll
            for (int u = 0; u < 2; u++) *(e_[u] < ns4 ? ps4 + e_[u] : pd4 + (e_[u] - ns4)) = acc[u];
        }
    }
    if (!S.use_sparse) for (int e = (int)tid; e < P * kS4; e += nthr) ps4[e] = (v4){ 0.f, 0.f, 0.f, 0.f };
}

// ---- phase 2b: frame sums.  Sum v of frame k over the frame's pairs in ascending partner order: (m, k) for m < k -- canonical index
// k - 1, then + (N - m - 2) per step -- and (k, m) for m > k: consecutive indices from k N - k (k + 1) / 2.
//   sparse (record slots of btba_kernels.hpp): 0 n | 1..3 s | 4..9 M | 10..12 rhs trans | 13..15 rhs rot | 16 prec trans | 17..19 prec rot
//   dense: 20 + (0..20 S upper triangle, 21..26 g)
// (sparse sums: one per lane on lanes 0 .. 20 (N - 1) - 1; dense sums: four per lane -- a 16-byte slot of the 28-float record -- on lanes
// DENSE_LANE0 .. DENSE_LANE0 + 7 (N - 1) - 1, behind the sparse lanes of the kernel's largest window: a wave runs one of the two loops, the
// heavy waves sit on different SIMDs)
template <unsigned DENSE_LANE0>
__device__ __forceinline__ void frame_sums(unsigned tid, int N, int P, int Pd, const float *ps, const float *pd, const int *adj_off_l, const int *adj_l, float *F)
{
    if (tid < 20u * (N - 1)) {
        const unsigned fk1 = tid / 20u, fv = tid - 20u * fk1;                // frame fk1 + 1
        const int fk = (int)fk1 + 1;
        // record slot when the frame is the pair's i / j end
        unsigned off_i, off_j;
        float sg_i = 1.0f;
        if (fv == 0) { off_i = off_j = 0; }
        else if (fv < 4) { off_i = fv; off_j = fv + 3; }
        else if (fv < 10) { off_i = fv + 3; off_j = fv + 9; }
        else if (fv < 13) { off_i = off_j = fv + 18; sg_i = -1.0f; }
        else if (fv < 16) { off_i = fv + 18; off_j = fv + 21; sg_i = -1.0f; }
        else if (fv == 16) { off_i = off_j = 37; }
        else { off_i = fv + 21; off_j = fv + 24; }
        // partner slot q = 0 .. N - 2: m = q (q < k: the frame is the j end of pair (m, k)) or q + 1 (the i end of pair (k, m)).  BOTH candidates are
        // loaded for every slot -- the j one along the running index, the i one at a fixed stride (an immediate offset) -- and one is selected:
        // eight instructions per term instead of fourteen.  Slots beyond the frame's pairs read a live address (or the slack behind the records)
        // and are dropped by the select.
        const unsigned lim = __umul24((unsigned)P - 1u, kSparseVals) + off_j;
        unsigned aj = __umul24((unsigned)fk - 1u, kSparseVals) + off_j;      // pair (0, k)
        const float *pi = ps + __umul24((unsigned)(fk * N - fk * (fk + 1) / 2 - fk), kSparseVals) + off_i;      // pair (k, q + 1) at + 44 q
        int stride = kSparseVals * (N - 2);
        float acc_j = 0.0f, acc_i = 0.0f;
        for (int q0 = 0; q0 < N - 1; q0 += 8) {
            float vj[8], vi[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { vj[u] = ps[min(aj, lim)]; vi[u] = pi[kSparseVals * (q0 + u)]; aj += stride; stride -= kSparseVals; }
#pragma unroll
            for (int u = 0; u < 8; u++) { const int q = q0 + u; acc_j += (q < fk) ? vj[u] : 0.0f; acc_i += (q >= fk && q < N - 1) ? vi[u] : 0.0f; }
        }
        F[__umul24(fk1, kFrameSums) + fv] = acc_j + sg_i * acc_i;
    } else if (tid >= DENSE_LANE0 && tid < DENSE_LANE0 + 7u * (N - 1)) {
        const unsigned t = tid - DENSE_LANE0, fk1 = t / 7u, sl = t - 7u * fk1;      // slot sl of frame fk1 + 1: record floats 4 sl .. 4 sl + 3 (S: 0 .. 20, g: 21 .. 26, count: 27)
        v4 acc = (v4){ 0.f, 0.f, 0.f, 0.f };
        if (Pd) {
            const int qa = adj_off_l[fk1 + 1], qb = adj_off_l[fk1 + 2];
            const v4 *pd4s = reinterpret_cast<const v4 *>(pd) + sl;
            for (int q0 = qa; q0 < qb; q0 += 8) {
                int a[8];
                v4 v[8];
#pragma unroll
                for (int u = 0; u < 8; u++) a[u] = adj_l[min(q0 + u, qb - 1)];
#pragma unroll
                for (int u = 0; u < 8; u++) v[u] = pd4s[__umul24(a[u] >> 1, kDenseVals / 4)];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    // g: + for the source frame (row_j = a), - for the target frame (row_i = -a); S: + for both.  (a dead slot repeats the last entry with weight 0)
                    const float live = q0 + u < qb ? 1.0f : 0.0f, sg = (a[u] & 1) ? live : -live;
                    const float wx = sl == 6u ? sg : live, wr = sl >= 5u ? sg : live;
                    acc.x += wx * v[u].x; acc.y += wr * v[u].y; acc.z += wr * v[u].z; acc.w += wr * v[u].w;
                }
            }
        }
        *reinterpret_cast<v4 *>(F + __umul24(fk1, kFrameSums) + 20u + 4u * sl) = acc;
    }
}

// ---- right-hand side, Jacobi diagonal and p_0 from the frame sums, unknown a on lane lane0 + a
__device__ __forceinline__ void rhs_precond_p0(unsigned tid, unsigned lane0, int na, float w_s, int Pd, const float *F, float *vb, float *vM, float *vp)
{
    if (tid >= lane0 && tid < lane0 + (unsigned)na) {
        const unsigned a = tid - lane0, k1 = a / 6u, r = a - 6u * k1;
        const float *Fk = F + __umul24(k1, kFrameSums);
        // b = -J^T r: sparse part weighted (SolverBundlingEquationsLie.h:60-137), dense part from the sweep's g;  M^-1 = 1 / diag of the UNWEIGHTED sparse J^T J (Lie.h:107-108)
        const float rhs = w_s * Fk[10 + r] - (Pd ? Fk[41 + r] : 0.0f);
        const float md = Fk[r < 3 ? 16 : 14 + r];
        const float minv = (md > kEps) ? 1.0f / md : 1.0f;
        vb[a] = rhs;
        vM[a] = minv;
        vp[a] = minv * rhs;                                                  // p_0 = M^-1 r_0
    }
}

// ---- trace: right-hand side and preconditioner in trace order -- (rot, trans) per frame; internal [trans, rot]; frame 0's entries are
// zero -- and the reduced dense pair sums.  (The matrix is dumped by each kernel from where it keeps it.)
__device__ __forceinline__ void trace_system(const SmallSolveArgs &S, float *tr, unsigned tid, int N, int Pd, const float *vb, const float *vM, const float *pd)
{
    constexpr unsigned nthr = kSmallBlock;
    const int n = 6 * N;
    for (int e = (int)tid; e < n; e += nthr) {
        const int k = e / 6, r = e % 6, o = k * 6 + (r < 3 ? r + 3 : r - 3);
        tr[S.tr_rhs + o] = k ? vb[e - 6] : 0.0f;
        tr[S.tr_prec + o] = k ? vM[e - 6] : 0.0f;
    }
    for (int e = (int)tid; e < Pd * kDenseVals; e += nthr) tr[S.tr_dpair + e] = pd[e];
}

// ---- phase 3: Jacobi-preconditioned CG (SolverBundling.cu:575-818; the absolute epsilon guards of :746-818 as they stand).
// The matrix sits in registers: LPR lanes own a row, CPL columns each, 64 / LPR rows per wave.  A step = the matrix-vector product on every
// wave that owns rows (packed FMAs against p -- broadcast 16-byte LDS reads --, log2 LPR DPP adds, A p through LDS), a barrier, the two dot
// products and the vector updates on wave 0 ALONE (a chain of ~60 dependent instructions: a wave that shares its SIMD with others running
// the same chain retires it slower -- eleven waves doing it redundantly measured 8.2 k cycles for the five steps, three waves 7.3 k), a
// barrier.  alpha and beta by v_rcp_f32 (1 ulp; the reference is built with -use_fast_math).
template <int LPR>
struct PcgRows {                             // which matrix row part a lane owns
    static constexpr int rows_per_wave = 64 / LPR;
    int wave, lane, a_row, h;                // row a_row, columns CPL h .. CPL h + CPL - 1
    bool pw, row_live;                       // the wave owns rows; the row exists
    __device__ __forceinline__ PcgRows(unsigned tid, int na)
    {
        wave = (int)(tid >> 6); lane = (int)(tid & 63u);
        pw = wave < (int)((unsigned)(na + rows_per_wave - 1) / rows_per_wave);
        a_row = rows_per_wave * wave + lane / LPR; h = lane & (LPR - 1);
        row_live = pw && a_row < na;
    }
};

// Ar: the lane's CPL matrix entries (lanes of R.pw waves).  Reads b (vb), M^-1 (vM) and p_0 (vp, zero beyond na); leaves delta in vd.
template <int CPL, int LPR>
__device__ __forceinline__ void pcg(const SmallSolveArgs &S, float *tr, unsigned tid, int na, const PcgRows<LPR> &R, const f2 (&Ar)[CPL / 2],
                                    float *vp, float *vAp, const float *vb, const float *vM, float *vd)
{
    static_assert(LPR == 4 || LPR == 8, "a row's lanes fold inside a DPP row half");
    constexpr int NV = LPR * CPL > 128 ? 3 : 2;      // vector entries per lane of wave 0 (two at least: every k_solve_small keeps the widest one's serial part)
    const int lane = R.lane;
    float r_[NV], m_[NV], p_[NV], d_[NV];
    float rz = 0.0f;
    if (R.wave == 0) {
        float part = 0.0f;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int idx = lane + 64 * j;
            const bool live = idx < na;
            r_[j] = live ? vb[idx] : 0.0f; m_[j] = live ? vM[idx] : 0.0f; d_[j] = 0.0f;
            p_[j] = m_[j] * r_[j];                                          // (= what rhs_precond_p0 stored in vp)
            part += r_[j] * p_[j];
        }
        rz = wave_sum_all(part);
    }
    for (int li = 0; li < S.n_pcg; li++) {
        if (R.pw) {
            const float4 *p4 = reinterpret_cast<const float4 *>(vp + R.h * CPL);
            f2 qa = (f2){ 0.f, 0.f }, qb = qa, qc = qa, qd = qa;
#pragma unroll
            for (int k = 0; k < CPL / 4; k++) {
                const float4 pc = p4[k];
                if (k & 1) { qc = __builtin_elementwise_fma(Ar[2 * k], (f2){ pc.x, pc.y }, qc); qd = __builtin_elementwise_fma(Ar[2 * k + 1], (f2){ pc.z, pc.w }, qd); }
                else { qa = __builtin_elementwise_fma(Ar[2 * k], (f2){ pc.x, pc.y }, qa); qb = __builtin_elementwise_fma(Ar[2 * k + 1], (f2){ pc.z, pc.w }, qb); }
            }
            if (CPL > 4) { qa += qc; qb += qd; }
            float s = (qa.x + qa.y) + (qb.x + qb.y);
            s = dpp_add<0xB1, 0xf>(s);                                      // + the row's other lanes: quad_perm [1,0,3,2],
            s = dpp_add<0x4E, 0xf>(s);                                      //   quad_perm [2,3,0,1],
            if (LPR > 4) s = dpp_add<0x141, 0xf>(s);                        //   row_half_mirror
            if (R.h == 0 && R.row_live) vAp[R.a_row] = s;
        }
        __syncthreads();
        if (R.wave == 0) {
            float ap_[NV], z_[NV];
            float part = 0.0f;
#pragma unroll
            for (int j = 0; j < NV; j++) { const int idx = lane + 64 * j; ap_[j] = idx < na ? vAp[idx] : 0.0f; part += p_[j] * ap_[j]; }
            const float pAp = wave_sum_all(part);
            const float alpha = (pAp > kEps) ? rz * __builtin_amdgcn_rcpf(pAp) : 0.0f;
            part = 0.0f;
#pragma unroll
            for (int j = 0; j < NV; j++) {
                d_[j] = d_[j] + alpha * p_[j];
                r_[j] = r_[j] - alpha * ap_[j];
                z_[j] = m_[j] * r_[j];
                part += z_[j] * r_[j];
            }
            const float rz_new = wave_sum_all(part);
            const float beta = (rz > kEps) ? rz_new * __builtin_amdgcn_rcpf(rz) : 0.0f;
            if (tr && tid == 0) { float *sc = tr + S.tr_pcg + 4 * li; sc[0] = pAp; sc[1] = alpha; sc[2] = rz_new; sc[3] = beta; }
            rz = rz_new;
#pragma unroll
            for (int j = 0; j < NV; j++) { p_[j] = z_[j] + beta * p_[j]; if (lane + 64 * j < na) vp[lane + 64 * j] = p_[j]; }
        }
        __syncthreads();
    }
    if (R.wave == 0) {
#pragma unroll
        for (int j = 0; j < NV; j++) if (lane + 64 * j < na) vd[lane + 64 * j] = d_[j];
    }
}

// ---- phase 4: x_k <- Log(Exp(delta_k) Exp(x_k)), the next iterate's T (SolverBundling.cu:805-815, 890-897).
// One frame: (rot, trans) hold x_k and receive the update; dk = the frame's delta ([trans, rot], as the PCG leaves it), Tk = Exp(x_k) in LDS.
// A frame that does not move (frame 0) keeps its x.  Returns Exp of the result.
template <bool FAST>
__device__ __forceinline__ Mat4 update_frame(bool moves, const float *dk, const float *Tk, float (&rot)[3], float (&trans)[3])
{
    if (moves) {
        const float dW[3] = { dk[3], dk[4], dk[5] }, dT[3] = { dk[0], dk[1], dk[2] };
        const Mat4 U = pose_to_matrix<FAST>(dW, dT);
        Mat4 C = load_mat4(Tk);                                             // = Exp(x_k), from the previous launch: a pose_to_matrix result,
        C.m[12] = 0.0f; C.m[13] = 0.0f; C.m[14] = 0.0f; C.m[15] = 1.0f;       // whose last row is these constants (the product's dead terms fold away, same bits)
        matrix_to_pose<FAST>(mat_mul(U, C), rot, trans);
    }
    return pose_to_matrix<FAST>(rot, trans);
}

// One lane per frame: x and T to global memory (and the caller's matrices on the last iterate), T to vE for the inverse, the trace.
template <bool FAST>
__device__ __forceinline__ void update_poses(const SmallSolveArgs &S, float *tr, unsigned tid, unsigned b, int N, const float *x_l, const float *vd, const float *vT, float *vE)
{
    if (tid < (unsigned)N) {
        const int k = (int)tid;
        float *xk = S.x + __umul24(b, (unsigned)S.x_stride) + 6 * k;
        const float *xl = x_l + 6 * k;
        float rot[3] = { xl[0], xl[1], xl[2] }, trans[3] = { xl[3], xl[4], xl[5] };
        const Mat4 E = update_frame<FAST>(k > 0, vd + 6 * (k - 1), vT + 16 * k, rot, trans);
        if (k > 0) { xk[0] = rot[0]; xk[1] = rot[1]; xk[2] = rot[2]; xk[3] = trans[0]; xk[4] = trans[1]; xk[5] = trans[2]; }
        store_mat4(S.T + __umul24(b, (unsigned)S.pose_stride) + 16 * k, E);
        if (S.poses_out) store_mat4(S.poses_out + 16 * (b * N + k), E);      // last iterate: convertPosesToMatricesCU (SBA.cpp:115)
        store_mat4(vE + 16 * k, E);
        if (tr) {
            for (int q = 0; q < 3; q++) { tr[S.tr_x + 6 * k + q] = rot[q]; tr[S.tr_x + 6 * k + 3 + q] = trans[q]; }
            for (int q = 0; q < 16; q++) tr[S.tr_T + 16 * k + q] = E.m[q];
            for (int q = 0; q < 3; q++) { tr[S.tr_delta + 6 * k + q] = k ? vd[6 * (k - 1) + 3 + q] : 0.0f; tr[S.tr_delta + 6 * k + 3 + q] = k ? vd[6 * (k - 1) + q] : 0.0f; }
        }
    }
}

// ---- the generic cofactor inverse (float4x4::getInverse, cuda_SimpleMatrixUtil.h:978-1104; btba_device.hpp: mat_inverse: ~300 instructions
// of a one-lane chain) on sixteen lanes per matrix: lane e = 4 R + C of an aligned group of sixteen forms adjugate entry (R, C) = cofactor of
// element (C, R) from the same six triple products; the determinant is the first row against the adjugate's first column (lanes 0, 4, 8,
// 12 of the group).  m: the matrix, in LDS; returns entry e of its inverse.  All sixteen lanes of a group call it together.
template <bool FAST>
__device__ __forceinline__ float inverse_on_sixteen_lanes(const float *m, unsigned tid)
{
    const unsigned e = tid & 15u, R = e >> 2, Cc = e & 3u;
    const int r0 = (Cc == 0) ? 1 : 0, r1 = (Cc <= 1) ? 2 : 1, r2 = (Cc <= 2) ? 3 : 2;
    const int c0 = (R == 0) ? 1 : 0, c1 = (R <= 1) ? 2 : 1, c2 = (R <= 2) ? 3 : 2;
    const float m00 = m[4 * r0 + c0], m01 = m[4 * r0 + c1], m02 = m[4 * r0 + c2];
    const float m10 = m[4 * r1 + c0], m11 = m[4 * r1 + c1], m12 = m[4 * r1 + c2];
    const float m20 = m[4 * r2 + c0], m21 = m[4 * r2 + c1], m22 = m[4 * r2 + c2];
    const float t1 = m00 * m11 * m22, t2 = m00 * m12 * m21, t3 = m10 * m01 * m22, t4 = m10 * m02 * m21, t5 = m20 * m01 * m12, t6 = m20 * m02 * m11;
    const float even = ((((t1 - t2) - t3) + t4) + t5) - t6;
    const float adj = ((R + Cc) & 1) ? -even : even;
    const int g0 = (int)(tid & 63u) & ~15;
    const float a0 = __shfl(adj, g0, 64), a4 = __shfl(adj, g0 + 4, 64), a8 = __shfl(adj, g0 + 8, 64), a12 = __shfl(adj, g0 + 12, 64);
    const float det = m[0] * a0 + m[1] * a4 + m[2] * a8 + m[3] * a12;
    const float rdet = se3_div<FAST>(1.0f, det);
    return adj * rdet;
}

// T^-1 of the next iterate's poses (vE), sixteen lanes per frame
template <bool FAST>
__device__ __forceinline__ void invert_poses(const SmallSolveArgs &S, unsigned tid, unsigned b, int N, const float *vE)
{
    if (tid < 16u * N) S.Tinv[__umul24(b, (unsigned)S.pose_stride) + tid] = inverse_on_sixteen_lanes<FAST>(vE + 16 * (tid >> 4), tid);
}

}  // namespace btba
