// btba_solve_general.hpp -- the general system solve: k_system_solve, with k_big_reduce and k_big_assemble in front of it on larger windows.
// It runs windows of 32 to 85 frames, the atomic reduction mode, explicit dense pair lists with more than P pairs, and every
// window when BTBA_OPT_SOLVE_SMALL = 0.  One workgroup of kSolveBlock threads per instance walks
//   reduce the sweep partials -> assemble A, b, M^-1 -> PCG -> update x, T, T^-1
// each step a forced-inline function over one SolveCtx; the LDS layout is btba_solve_layout.hpp's, shared with the host.
// The order of every sum in here is pinned: the decision traces (BTBA_FLAG_TRACE) are compared bit for bit across builds,
// tests/test_gpu_solve_stages.py holds each stage to its fp64 reference, and test_small_solve_kernel_agrees_with_the_legacy_kernel holds
// k_solve_small to this kernel.
#pragma once
#include "btba_kernels.hpp"
#include "btba_solve_layout.hpp"

namespace btba {

static_assert(kLayoutSparseVals == kSparseVals, "btba_solve_layout.hpp carries the sparse record's length");

// Linear form of a sparse 6x6 block entry ([trans, rot] order; J_k = [ I | -[w_k]x ]) from a pair's 44 moment sums:
//   diagonal block of endpoint e (0 = i, 1 = j):  [[ n I, -[s]x ], [ [s]x, tr(M) I - M ]]
//   cross block J_i^T J_j (row on frame i, column on frame j):  [[ n I, -[s_j]x ], [ [s_i]x, tr(Mij) I - Mij^T ]]
// value = c1 rec[i1 + e es] + c2 rec[i2 + e es].
// Returned as int4 (i1 | es << 8, i2, bits(c1), bits(c2)); es = record offset per endpoint (0 for n and cross blocks).
// (c1, c2 are 0 or +-1; the table is built once per window size on the host, btba_api.hip: solve_tables)
__host__ __device__ inline void sparse_entry_descriptor(bool cross, int r, int c, int out[4])
{
    const int br = r / 3, bc = c / 3, rr = r % 3, cc = c % 3;
    int i1 = 0, i2 = 0, es = 0;
    int c1 = 0, c2 = 0;                                                // signs
    const int k = 3 - rr - cc;
    const int sgn = ((cc - rr + 3) % 3 == 1) ? -1 : 1;                 // skew(v, rr, cc) = sgn v[k] for rr != cc
    if (br == 0 && bc == 0) { if (rr == cc) { i1 = 0; c1 = 1; } }
    else if (br == 0 && bc == 1) { if (rr != cc) { i1 = (cross ? 4 : 1) + k; c1 = -sgn; es = cross ? 0 : 3; } }
    else if (br == 1 && bc == 0) { if (rr != cc) { i1 = 1 + k; c1 = sgn; es = cross ? 0 : 3; } }
    else if (rr == cc) {                                               // tr(M) - M_rr = the other two diagonal entries
        const int a = (rr + 1) % 3, b = (rr + 2) % 3;
        const int dg[3] = { 0, 3, 5 };
        i1 = cross ? 19 + 4 * a : 7 + dg[a]; i2 = cross ? 19 + 4 * b : 7 + dg[b]; c1 = 1; c2 = 1; es = cross ? 0 : 6;
    } else {
        const int lo = rr < cc ? rr : cc, hi = rr < cc ? cc : rr;
        i1 = cross ? 19 + cc * 3 + rr : 7 + lo * 3 - lo * (lo - 1) / 2 + (hi - lo); c1 = -1; es = cross ? 0 : 6;
    }
    const int one = 0x3F800000, minus_one = (int)0xBF800000u;          // fp32 bit patterns of +-1
    out[0] = i1 | (es << 8); out[1] = i2;
    out[2] = c1 > 0 ? one : c1 < 0 ? minus_one : 0; out[3] = c2 > 0 ? one : c2 < 0 ? minus_one : 0;
}

__device__ __forceinline__ float block_sum(float v, float *scratch)
{
    // all threads must call; returns the workgroup total to every thread
    const float s = wave_sum_to_lane63(v);
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 63) scratch[threadIdx.x >> 6] = s;
    __syncthreads();
    float t = scratch[0];
    for (int w = 1; w < nw; w++) t += scratch[w];
    return t;
}

// ---- the assembly formulas, once: the workgroup (assemble, below) and k_big_assemble call them with their own slice counts and their
// own homes of the pair sums (ps: sparse [P][44], pd: dense [Pd][28]) and tables (LDS there, global memory here) ----------------------

// Off-diagonal entry rc = 6 r + c of canonical pair p (i < j):  A_ij = -(ws Ji^T Jj + S_dense).  The dense part is the value the caller
// fetched from the dense pair listed as (target i, source j) for this canonical pair, if there is one.
__device__ __forceinline__ float off_diag_entry(const SolveDims &D, const int *entry_lut, const float *ps, int p, int rc, bool has_dense, float dense_value)
{
    float v = 0.0f;
    if (D.use_sparse) {
        const int *dl = entry_lut + 4 * (36 + rc);
        const int4 d = make_int4(dl[0], dl[1], dl[2], dl[3]);
        const float *rec = ps + (size_t)p * kSparseVals;
        v = -D.w_sparse * (__int_as_float(d.z) * rec[d.x & 255] + __int_as_float(d.w) * rec[d.y & 255]);
    }
    if (has_dense) v -= dense_value;
    return v;
}

// Sum of the dense pair sums `off` of adjacency entries [qa, qb) of a frame, signed by the frame's role in the pair when `by_role`
// (source frame: row_j = a;  target frame: row_i = -a), in adjacency order.
__device__ __forceinline__ float dense_adj_sum(const int *adj, const float *pd, int qa, int qb, int off, bool by_role)
{
    float acc = 0.0f;
    for (int q = qa; q < qb; q++) {
        const int a = adj[q];
        const float v = pd[(size_t)(a >> 1) * kDenseVals + off];
        acc += by_role ? ((a & 1) ? v : -v) : v;
    }
    return acc;
}

// Slice s of PARTS of diagonal-block entry rc of frame k >= 1: the frame's partners m in [N s / PARTS, N (s + 1) / PARTS) and the same
// share of its dense adjacency, each in fixed order.  The caller adds the PARTS slices with its shuffle tree.
template <int PARTS>
__device__ __forceinline__ float diag_entry_slice(const SolveDims &D, int N, int k, int rc, int s, const int *entry_lut, const float *ps, const float *pd,
                                                  const int *adj_off, const int *adj)
{
    float v = 0.0f;
    if (D.use_sparse) {
        const int *dl = entry_lut + 4 * rc;
        const int4 d = make_int4(dl[0], dl[1], dl[2], dl[3]);
        const int es = d.x >> 8;
        const float c1 = __int_as_float(d.z), c2 = __int_as_float(d.w);
        float acc = 0.0f;
        for (int m = (N * s) / PARTS; m < (N * (s + 1)) / PARTS; m++) {
            if (m == k) continue;
            const int i = m < k ? m : k, j = m < k ? k : m;
            const float *rec = ps + (size_t)pair_index(i, j, N) * kSparseVals + (k == i ? 0 : es);
            acc += c1 * rec[d.x & 255] + c2 * rec[d.y & 255];
        }
        v = D.w_sparse * acc;
    }
    if (D.use_dense) {
        const int q0 = adj_off[k], nq = adj_off[k + 1] - q0;
        v += dense_adj_sum(adj, pd, q0 + (nq * s) / PARTS, q0 + (nq * (s + 1)) / PARTS, tri21(rc / 6, rc % 6), false);
    }
    return v;
}

// Slice s of PARTS of the right-hand side (rhs) and of the Jacobi diagonal (md) of unknown r of frame k >= 1
template <int PARTS>
__device__ __forceinline__ void rhs_jacobi_slice(const SolveDims &D, int N, int k, int r, int s, const float *ps, const float *pd, const int *adj_off, const int *adj,
                                                 float &rhs, float &md)
{
    if (D.use_sparse) {
        const int o_i = (r < 3) ? 28 + r : 31 + r - 3, o_j = (r < 3) ? 28 + r : 34 + r - 3;       // rhs slots of the i / j end
        const int p_i = (r < 3) ? 37 : 38 + r - 3, p_j = (r < 3) ? 37 : 41 + r - 3;              // preconditioner slots
        for (int m = (N * s) / PARTS; m < (N * (s + 1)) / PARTS; m++) {
            if (m == k) continue;
            const int i = m < k ? m : k, j = m < k ? k : m;
            const float *rec = ps + (size_t)pair_index(i, j, N) * kSparseVals;
            const bool is_i = (k == i);
            const float g = rec[is_i ? o_i : o_j];
            rhs += is_i ? -g : g;
            md += rec[is_i ? p_i : p_j];
        }
        rhs *= D.w_sparse;
    }
    if (D.use_dense) {
        const int q0 = adj_off[k], nq = adj_off[k + 1] - q0;
        rhs -= dense_adj_sum(adj, pd, q0 + (nq * s) / PARTS, q0 + (nq * (s + 1)) / PARTS, 21 + r, true);
    }
}
// M^-1 of an unknown from the summed Jacobi diagonal (frame 0 stays fixed)
__device__ __forceinline__ float jacobi_inverse(int k, float md) { return (k > 0) ? ((md > kEps) ? 1.0f / md : 1.0f) : 0.0f; }

// What the assembly does not write and the PCG reads: frame 0's rows (entries 0 .. 6 ld - 1 of A[n][ld]) and, in each of the other n - 6
// rows, frame 0's columns and the pad columns n .. ld - 1 that the 16-byte mat-vec chunks read: zero_fill_rest entries, entry e at
// offset zero_fill_rest_index(e).
__host__ __device__ inline unsigned zero_fill_rest(unsigned n, unsigned ld) { return (n - 6u) * (6u + ld - n); }
__device__ __forceinline__ int zero_fill_rest_index(int e, int n, int ld)
{
    const int row = 6 + e / (6 + ld - n), q = e % (6 + ld - n);
    return row * ld + (q < 6 ? q : n + q - 6);
}

// ---- large windows (matrix in a global scratch): reduction and assembly on MANY workgroups -------------------------------
// Above BTBA_MAX_FRAMES_LDS frames k_system_solve used to do everything on one workgroup; at N = 85 (3 570 pairs, a 510 x 510
// system) 118 k of its 989 k cycles went into reducing the sweep partials and 562 k into the assembly -- chains of dependent
// global-memory reads walked by one CU (scripts/sys_clocks_big.py).  Both are embarrassingly parallel over pairs / matrix entries:
//   k_big_reduce    one thread per reduced value: pair sums = sum over chunks / tiles of the sweep partials, in partial order
//   k_big_assemble  one thread per off-diagonal entry, EIGHT lanes per diagonal entry / per unknown of the right-hand side (each sums an
//                   eighth of the frame's pairs in fixed order, fixed shuffle tree), plus the zero-fill of what nobody writes
// k_system_solve then starts at the PCG (D.pre_assembled).  The formulas are the ones above; the sums over a frame's pairs are grouped
// in eighths instead of the workgroup's halves / quarters.  System layout per instance: A[n][ld], rhs[ld], prec[ld].
__global__ void __launch_bounds__(256) k_big_reduce(SolveDims D, float *sparse_partials, float *dense_partials,       // (not const: accumulators in BTBA_REDUCE_ATOMIC mode, cleared here)
                                                    float *__restrict__ pairsum_global)
{
    const int b = blockIdx.y;
    const size_t ns = (size_t)D.n_pairs * kSparseVals, nd = (size_t)D.n_dense_pairs * kDenseVals;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ns + nd) return;
    float *out = pairsum_global + (size_t)b * (ns + nd);
    float s = 0.0f;
    if (e < ns) {
        if (D.use_sparse) {
            const size_t p = e / kSparseVals, v = e - p * kSparseVals;
            float *q = sparse_partials + (size_t)b * D.sp_stride + (p * D.sparse_chunks) * kSparseVals + v;
            for (int c = 0; c < D.sparse_chunks; c++) s += q[(size_t)c * kSparseVals];
            if (D.atomic_sums) q[0] = 0.0f;
        }
    } else if (D.use_dense) {
        const size_t ed = e - ns, p = ed / kDenseVals, v = ed - p * kDenseVals;
        float *q = dense_partials + (size_t)b * D.dp_stride + (p * D.dense_tiles) * kDenseVals + v;
        for (int c = 0; c < D.dense_tiles; c++) s += q[(size_t)c * kDenseVals];
        if (D.atomic_sums) q[0] = 0.0f;
    }
    out[e] = s;
}

// task segments of k_big_assemble, each padded to a multiple of 64 threads
struct BigTasks { unsigned off_diag, diag, rhs, zero, total; };
__host__ __device__ inline BigTasks big_tasks(int N, int P, int ld)
{
    const unsigned n = 6u * (unsigned)N;
    auto pad = [](unsigned x) { return (x + 63u) & ~63u; };
    BigTasks t;
    t.off_diag = pad((unsigned)P * 36u);
    t.diag = pad((unsigned)(N - 1) * 36u * 8u);
    t.rhs = pad(n * 8u);
    t.zero = pad(6u * (unsigned)ld + zero_fill_rest(n, (unsigned)ld));
    t.total = t.off_diag + t.diag + t.rhs + t.zero;
    return t;
}

__global__ void __launch_bounds__(256) k_big_assemble(SolveDims D, const float *__restrict__ pairsum_global, const int2 *__restrict__ dense_pairs,
                                                      const int *__restrict__ adj_off, const int *__restrict__ adj, const int *__restrict__ solve_tab,
                                                      float *__restrict__ A_scratch)
{
    const int b = blockIdx.y;
    const int N = D.n_frames, n = 6 * N, ld = solve_row_floats(N);
    const BigTasks K = big_tasks(N, D.n_pairs, ld);
    unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= K.total) return;
    float *A = A_scratch + (size_t)b * (size_t)(n + 2) * ld, *rhs_out = A + (size_t)n * ld, *prec_out = rhs_out + ld;
    const float *ps = pairsum_global + (size_t)b * ((size_t)D.n_pairs * kSparseVals + (size_t)D.n_dense_pairs * kDenseVals);
    const float *pd = ps + (size_t)D.n_pairs * kSparseVals;
    const int *pair_ij = solve_tab, *entry_lut = solve_tab + D.n_pairs;
    const int n_adj = D.use_dense ? 2 * D.n_dense_pairs : 0;
    const int *cross_tab = adj + n_adj;
    if (t < K.off_diag) {                                  // ---- off-diagonal entries, one canonical pair (i < j) each
        if (t >= (unsigned)D.n_pairs * 36u) return;
        const int p = (int)(t / 36u), rc = (int)(t - 36u * (unsigned)p), r = rc / 6, c = rc - 6 * r;
        const int pij = pair_ij[p], i = pij >> 8, j = pij & 255;
        if (i == 0) return;
        const int dp = D.use_dense ? cross_tab[p] : -1;
        const float v = off_diag_entry(D, entry_lut, ps, p, rc, dp >= 0, dp >= 0 ? pd[(size_t)dp * kDenseVals + tri21(r, c)] : 0.0f);
        A[(size_t)(6 * i + r) * ld + 6 * j + c] = v;
        A[(size_t)(6 * j + c) * ld + 6 * i + r] = v;
        return;
    }
    t -= K.off_diag;
    if (t < K.diag) {                                      // ---- diagonal blocks: 8 lanes per (frame k >= 1, entry)
        const unsigned e = t >> 3, sub = t & 7u;
        const bool live = e < (unsigned)(N - 1) * 36u;
        const int k = live ? 1 + (int)(e / 36u) : 1, rc = live ? (int)(e % 36u) : 0;
        float v = live ? diag_entry_slice<8>(D, N, k, rc, (int)sub, entry_lut, ps, pd, adj_off, adj) : 0.0f;
        v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
        if (live && sub == 0) A[(size_t)(6 * k + rc / 6) * ld + 6 * k + rc % 6] = v;
        return;
    }
    t -= K.diag;
    if (t < K.rhs) {                                       // ---- right-hand side and Jacobi diagonal: 8 lanes per unknown
        const unsigned e = t >> 3, sub = t & 7u;
        const bool live = e < (unsigned)n;
        const int k = live ? (int)e / 6 : 0, r = live ? (int)e % 6 : 0;
        float rhs = 0.0f, md = 0.0f;
        if (live && k > 0) rhs_jacobi_slice<8>(D, N, k, r, (int)sub, ps, pd, adj_off, adj, rhs, md);
        rhs += __shfl_xor(rhs, 1, 64); md += __shfl_xor(md, 1, 64);
        rhs += __shfl_xor(rhs, 2, 64); md += __shfl_xor(md, 2, 64);
        rhs += __shfl_xor(rhs, 4, 64); md += __shfl_xor(md, 4, 64);
        if (live && sub == 0) {
            rhs_out[e] = rhs;
            prec_out[e] = jacobi_inverse(k, md);
        }
        return;
    }
    t -= K.rhs;
    if (t < 6u * ld) A[t] = 0.0f;                          // ---- what nobody writes
    else if (t - 6u * ld < zero_fill_rest((unsigned)n, (unsigned)ld)) A[zero_fill_rest_index((int)(t - 6u * ld), n, ld)] = 0.0f;
}

// What one instance's system solve reads and writes, every pointer already at THIS instance.  x, T and T^-1 are updated in place.
struct SolveIO {
    float *sparse_partials, *dense_partials;            // this iteration's sweep partials (not const: in BTBA_REDUCE_ATOMIC mode they are accumulators that the solve clears)
    float *x, *T, *Tinv;                                // this iterate on entry, the next one on return (T^-1 is only written)
    float *poses_out;                                   // last iteration: the caller's pose buffer (or nullptr)
    float *pairsum_global;                              // reduced pair sums when they are not staged in LDS
    float *A_scratch;                                   // A_GLOBAL / pre_assembled: A[n][ld], rhs[ld], prec[ld]
    float *trace;                                       // this instance's trace records (or nullptr)
};

// What every phase of one solve works on: the dimensions, the calling lane, and the workgroup's pointers -- into the dynamic LDS (each
// from the offset of the same name in SolveLayout, which says what the region holds), into global memory where a variant keeps something there.
struct SolveCtx {
    const SolveDims &D;
    const SolveIO io;                           // (by value: a reference kept in here reaches the optimiser as a pointer in memory, and the address spaces of what it points to are inferred too late)
    int tid, N, n, ld;
    float *tr;                                  // this iteration's trace record (or nullptr)
    long long clk0;
    float *A;                                   // the matrix: LDS, or the global scratch (A_GLOBAL); global layout per instance: A[n][ld], rhs[ld], prec[ld]
    float *vb, *vM, *vp, *vAp, *vd, *scratch, *vT, *x_l;
    int *dense_pairs_l, *adj_off_l, *adj_l, *pair_ij_l, *cross_l, *entry_lut;
    // reduced pair sums, sparse [P][44] and model-frame dense (S, g, count) [Pd][28]: in LDS when they fit (address space known at compile
    // time -> ds_* instructions, not flat_*), otherwise in an L2-resident global scratch (K = 30)
    float *ps, *pd;
    __device__ __forceinline__ SolveCtx(const SolveDims &D_, const SolveIO &io_, int tid_, float *tr_, float *lds, const SolveLayout &L, bool a_in_global, float *ps_, float *pd_)
        : D(D_), io(io_), tid(tid_), N(D_.n_frames), n(6 * D_.n_frames), ld(L.ld), tr(tr_), clk0(tr_ ? (long long)clock64() : 0),
          A(a_in_global ? io_.A_scratch : lds + L.A), vb(lds + L.vb), vM(lds + L.vM), vp(lds + L.vp), vAp(lds + L.vAp), vd(lds + L.vd),
          scratch(lds + L.scratch), vT(lds + L.vT), x_l(lds + L.x),
          dense_pairs_l(reinterpret_cast<int *>(lds + L.dense_pairs)), adj_off_l(reinterpret_cast<int *>(lds + L.adj_off)), adj_l(reinterpret_cast<int *>(lds + L.adj)),
          pair_ij_l(reinterpret_cast<int *>(lds + L.pair_ij)), cross_l(reinterpret_cast<int *>(lds + L.cross)), entry_lut(reinterpret_cast<int *>(lds + L.entry_lut)),
          ps(ps_), pd(pd_) {}
};

// clock stamp `slot` of the trace record, by lane 0
__device__ __forceinline__ void trace_stamp(const SolveCtx &C, int slot)
{
    if (C.tr && C.tid == 0) C.tr[C.D.tr_clk + slot] = (float)((long long)clock64() - C.clk0);
}

// ---- a pre-assembled system (larger windows): k_big_reduce + k_big_assemble have built A, the right-hand side and the Jacobi diagonal
// in the global scratch; a matrix that fits LDS is loaded back for the one-wave PCG (coalesced, once)
template <bool A_IN_GLOBAL>
__device__ __forceinline__ void load_pre_assembled(const SolveCtx &C)
{
    const int tid = C.tid, N = C.N, n = C.n, ld = C.ld;
    const float *Ag = C.io.A_scratch;
    const float *rhs_g = Ag + (size_t)n * ld, *prec_g = rhs_g + ld;
    if (!A_IN_GLOBAL) {
        const float4 *src = reinterpret_cast<const float4 *>(Ag);
        float4 *dst = reinterpret_cast<float4 *>(C.A);
        for (int e = tid; e < (n * ld) / 4; e += kSolveBlock) dst[e] = src[e];
    }
    for (int e = tid; e < 16 * N; e += kSolveBlock) C.vT[e] = C.io.T[e];
    for (int e = tid; e < 6 * N; e += kSolveBlock) C.x_l[e] = C.io.x[e];
    for (int e = tid; e < n; e += kSolveBlock) { C.vb[e] = rhs_g[e]; C.vM[e] = prec_g[e]; C.vd[e] = 0.0f; }
    for (int e = n + tid; e < ld; e += kSolveBlock) C.vp[e] = 0.0f;
    __syncthreads();
}

// ---- staging of this iterate's T and of the pair tables into LDS.  Every one of these global loads is a fabric-latency
// miss (~2 k cycles; written by the previous launch / the host), and a load -> LDS-store loop per array serialises
// them behind s_waitcnt (measured: 7.7 k cycles for four tiny arrays).  So: the first trip of all the arrays is
// loaded into registers by stage_load, the partial sums' loads are issued behind them (reduce_partials_general), and stage_store
// runs after the reduction -- the staging latency hides behind the first round of partial loads.
struct GeneralStaged { float T, x; int2 dp; int ao, adj, pij, lut, cross; };
struct SolveTables {                                           // the window's tables in global memory (host: solve_enqueue)
    const int2 *dense_pairs; const int *adj_off, *adj, *solve_tab;
    __device__ __forceinline__ const int *cross_tab(const SolveDims &D) const { return adj + (D.use_dense ? 2 * D.n_dense_pairs : 0); }      // behind the adjacency
};
__device__ __forceinline__ GeneralStaged stage_load(const SolveCtx &C, const SolveTables &G)
{
    const SolveDims &D = C.D;
    const int tid = C.tid, N = C.N, n_dp = D.n_dense_pairs, n_adj = D.use_dense ? 2 * D.n_dense_pairs : 0, n_ao = D.use_dense ? N + 1 : 0;
    GeneralStaged S;
    S.T = tid < 16 * N ? C.io.T[tid] : 0.0f;
    S.x = tid < 6 * N ? C.io.x[tid] : 0.0f;
    S.dp = tid < n_dp ? G.dense_pairs[tid] : make_int2(0, 0);
    S.ao = tid < n_ao ? G.adj_off[tid] : 0;
    S.adj = tid < n_adj ? G.adj[tid] : 0;
    // canonical pair -> (i << 8 | j) and the 72 entry descriptors: constant per window size, tabulated by the host
    S.pij = tid < D.n_pairs ? G.solve_tab[tid] : 0;
    S.lut = tid < 288 ? G.solve_tab[D.n_pairs + tid] : 0;
    S.cross = (D.use_dense && tid < D.n_pairs) ? G.cross_tab(D)[tid] : -1;
    return S;
}
// the staged values: first trip from the registers loaded above, the rest (windows beyond 64 frames / 1 024 pairs) by loops
__device__ __forceinline__ void stage_store(const SolveCtx &C, const SolveTables &G, const GeneralStaged &S)
{
    const SolveDims &D = C.D;
    const int tid = C.tid, N = C.N, n_dp = D.n_dense_pairs, n_adj = D.use_dense ? 2 * D.n_dense_pairs : 0, n_ao = D.use_dense ? N + 1 : 0;
    const int *cross_tab = G.cross_tab(D);
    if (tid < 16 * N) C.vT[tid] = S.T;
    if (tid < 6 * N) C.x_l[tid] = S.x;
    for (int e = tid + kSolveBlock; e < 6 * N; e += kSolveBlock) C.x_l[e] = C.io.x[e];
    if (tid < D.n_pairs) C.pair_ij_l[tid] = S.pij;
    if (tid < 288) C.entry_lut[tid] = S.lut;
    for (int e = tid + kSolveBlock; e < 288; e += kSolveBlock) C.entry_lut[e] = G.solve_tab[D.n_pairs + e];
    if (tid < D.n_pairs) C.cross_l[tid] = S.cross;
    for (int e = tid + kSolveBlock; e < D.n_pairs; e += kSolveBlock) { C.pair_ij_l[e] = G.solve_tab[e]; C.cross_l[e] = D.use_dense ? cross_tab[e] : -1; }
    if (tid < n_dp) { C.dense_pairs_l[2 * tid] = S.dp.x; C.dense_pairs_l[2 * tid + 1] = S.dp.y; }
    if (tid < n_ao) C.adj_off_l[tid] = S.ao;
    for (int e = tid + kSolveBlock; e < n_ao; e += kSolveBlock) C.adj_off_l[e] = G.adj_off[e];
    if (tid < n_adj) C.adj_l[tid] = S.adj;
    for (int e = tid + kSolveBlock; e < 16 * N; e += kSolveBlock) C.vT[e] = C.io.T[e];
    for (int e = tid + kSolveBlock; e < n_dp; e += kSolveBlock) { const int2 ij = G.dense_pairs[e]; C.dense_pairs_l[2 * e] = ij.x; C.dense_pairs_l[2 * e + 1] = ij.y; }
    for (int e = tid + kSolveBlock; e < n_adj; e += kSolveBlock) C.adj_l[e] = G.adj[e];
}

// ---- phase A: fixed-order reduction of the sweep partials.
// The scalar scheme: ITEMS sums per lane per trip, up to eight partials of each in flight (24-40 loads issued before the first add): the
// partials were written by other XCDs' workgroups, every load comes from the fabric side of this XCD's L2 at ~1-2 k
// cycles, so the phase costs (number of dependent load rounds) x (that latency) -- 6 rounds at B = 1 (10 tiles,
// 5 chunks) instead of the 14 of a 2-item x 4-partial scheme.  Sums in partial order (fixed), whatever the grouping.
template <int VALS, int ITEMS>
__device__ __forceinline__ void reduce_partials_scalar(const SolveCtx &C, float *src, float *dst, int n_items_pairs, int parts)
{
    const SolveDims &D = C.D;
    const int tid = C.tid;
    const int total = n_items_pairs * VALS;
    for (int e0 = tid; e0 < total; e0 += ITEMS * kSolveBlock) {
        float *q[ITEMS];
        float sum[ITEMS];
        bool own[ITEMS];                                              // dead slots re-read the lane's first item (and must not clear it twice)
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const int e = e0 + i * kSolveBlock;
            const int ec = e < total ? e : e0;
            own[i] = e < total;
            q[i] = src + (size_t)(ec / VALS) * parts * VALS + (ec % VALS);
            sum[i] = 0.0f;
        }
        int c = 0;
        auto round = [&](auto width_c) {
            constexpr int width = decltype(width_c)::value;
            float v[ITEMS][width];
#pragma unroll
            for (int i = 0; i < ITEMS; i++)
#pragma unroll
                for (int u = 0; u < width; u++) v[i][u] = q[i][(size_t)(c + u) * VALS];
#pragma unroll
            for (int i = 0; i < ITEMS; i++)
#pragma unroll
                for (int u = 0; u < width; u++) sum[i] += v[i][u];
            if (D.atomic_sums) {                    // the records are accumulators: leave them empty for the next iteration's sweeps
#pragma unroll
                for (int i = 0; i < ITEMS; i++)
#pragma unroll
                    for (int u = 0; u < width; u++) if (own[i]) q[i][(size_t)(c + u) * VALS] = 0.0f;
            }
            c += width;
        };
        while (c + 8 <= parts) round(std::integral_constant<int, 8>{});
        if (c + 4 <= parts) round(std::integral_constant<int, 4>{});
        if (c + 2 <= parts) round(std::integral_constant<int, 2>{});
        if (c < parts) round(std::integral_constant<int, 1>{});
#pragma unroll
        for (int i = 0; i < ITEMS; i++) { const int e = e0 + i * kSolveBlock; if (e < total) dst[e] = sum[i]; }
    }
}

__device__ __forceinline__ void reduce_partials_general(const SolveCtx &C)
{
    const SolveDims &D = C.D;
    const int tid = C.tid;
    float *ps = C.ps, *pd = C.pd;
    // items per lane per trip: one trip covers the c3 window (105 pairs: 4 620 sparse / 2 940 dense sums over 1 024 lanes).  (Reducing both kinds at
    // the same time on disjoint groups of waves -- one round of fabric-latency loads instead of two -- measured 0.5 us SLOWER per launch, r03 call 39.)
    // Batches big enough to fill the chip run with one or two partials per sum (pick_chunks, pick_tiles): 16-byte loads then, and ALL of a lane's loads --
    // sparse and dense records -- issued before the first add: ONE round of fabric latency instead of the two (sparse, then dense) of the scalar
    // scheme.  The same sums: 0 + first (+ second).  See DESIGN.md 4.3.
    if (!D.use_sparse) for (int e = tid; e < D.n_pairs * kSparseVals; e += kSolveBlock) ps[e] = 0.0f;       // (read with weight 0)
    if (D.sparse_chunks <= 2 && D.dense_tiles <= 2 && !D.atomic_sums) {
        constexpr int kS4 = kSparseVals / 4, kD4 = kDenseVals / 4;          // 15 frames = 1 155 + 735 sums of four, 1.85 per lane: a lane holds two per pass
        const int ns4 = D.use_sparse ? D.n_pairs * kS4 : 0, nd4 = D.use_dense ? D.n_dense_pairs * kD4 : 0;
        for (int e0 = tid; e0 < ns4 + nd4; e0 += 2 * kSolveBlock) {
            float4 v0[2], v1[2];
            bool two[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int e = min(e0 + u * kSolveBlock, ns4 + nd4 - 1);
                const bool sp = e < ns4;
                const int q = sp ? e : e - ns4, per = sp ? kS4 : kD4, parts = sp ? D.sparse_chunks : D.dense_tiles;
                const int rec = q / per, k = q - rec * per;
                const float4 *src = reinterpret_cast<const float4 *>(sp ? C.io.sparse_partials : C.io.dense_partials) + ((size_t)rec * parts) * per + k;
                two[u] = parts > 1;
                v0[u] = src[0];
                v1[u] = src[two[u] ? per : 0];
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int e = e0 + u * kSolveBlock;
                if (e >= ns4 + nd4) continue;
                float4 sum = make_float4(0.0f + v0[u].x, 0.0f + v0[u].y, 0.0f + v0[u].z, 0.0f + v0[u].w);
                if (two[u]) { sum.x += v1[u].x; sum.y += v1[u].y; sum.z += v1[u].z; sum.w += v1[u].w; }
                // (four scalar stores: the LDS copy of the pair sums is not 16-byte aligned; two branches, not a selected pointer: ps and pd
                // may live in different address spaces, and a select between them sends this compiler's backend into an illegal instruction)
                auto put = [&](auto *dst) { dst[0] = sum.x; dst[1] = sum.y; dst[2] = sum.z; dst[3] = sum.w; };
                if (e >= ns4) put(pd + 4 * (size_t)(e - ns4));
                else put(ps + 4 * (size_t)e);
            }
        }
    } else {
        if (D.use_sparse) reduce_partials_scalar<kSparseVals, 5>(C, C.io.sparse_partials, ps, D.n_pairs, D.sparse_chunks);
        if (D.use_dense) reduce_partials_scalar<kDenseVals, 3>(C, C.io.dense_partials, pd, D.n_dense_pairs, D.dense_tiles);
    }
}

// ---- phase B: the system from the reduced pair sums, by the workgroup (tables and sparse sums in LDS)
__device__ __forceinline__ void assemble(const SolveCtx &C)
{
    const SolveDims &D = C.D;
    const int tid = C.tid, N = C.N, n = C.n, ld = C.ld;
    float *A = C.A;
    const float *ps = C.ps, *pd = C.pd;
    // Phase B1: off-diagonal 6x6 blocks, one canonical pair (i<j) each: A_ij = -(ws Ji^T Jj + S_dense).  The dense part comes from the
    // dense pair listed as (target i, source j) for this canonical pair, if any (cross_l; a pair listed the other way round is erased
    // by the reference's FlipJtJ, duplicates of a pair in an explicit list are not supported -- documented): ONE pass, no
    // read-modify-write, no barrier before the diagonal blocks.
    for (int e = tid; e < D.n_pairs * 36; e += kSolveBlock) {
        const int p = e / 36, rc = e - 36 * p, r = rc / 6, c = rc - 6 * r;
        const int pij = C.pair_ij_l[p];
        const int i = pij >> 8, j = pij & 255;
        if (i == 0) continue;
        const int dp = C.cross_l[p];
        const float v = off_diag_entry(D, C.entry_lut, ps, p, rc, dp >= 0, dp >= 0 ? pd[(size_t)dp * kDenseVals + tri21(r, c)] : 0.0f);
        A[(6 * i + r) * ld + 6 * j + c] = v;
        A[(6 * j + c) * ld + 6 * i + r] = v;
    }
    // Phase B2: diagonal blocks: TWO lanes per (frame k >= 1, entry), each sums half of the frame's pairs in fixed order
    for (int t = tid; t < 2 * (N - 1) * 36; t += kSolveBlock) {
        const int e = t >> 1, half = t & 1;
        const int k = 1 + e / 36, rc = e % 36;
        float v = diag_entry_slice<2>(D, N, k, rc, half, C.entry_lut, ps, pd, C.adj_off_l, C.adj_l);
        v += __shfl_xor(v, 1, 64);                       // partner lane = same entry, other half (t and t^1 share a wave)
        if (!half) A[(6 * k + rc / 6) * ld + 6 * k + rc % 6] = v;
    }
    // right-hand side and Jacobi diagonal: FOUR lanes per unknown, each sums a quarter of the frame's pairs
    for (int t = tid; t < 4 * n; t += kSolveBlock) {
        const int e = t >> 2, part = t & 3;
        const int k = e / 6, r = e % 6;
        float rhs = 0.0f, md = 0.0f;
        if (k > 0) rhs_jacobi_slice<4>(D, N, k, r, part, ps, pd, C.adj_off_l, C.adj_l, rhs, md);
        rhs += __shfl_xor(rhs, 1, 64); md += __shfl_xor(md, 1, 64);        // the four lanes of an unknown sit in one wave
        rhs += __shfl_xor(rhs, 2, 64); md += __shfl_xor(md, 2, 64);
        if (part == 0) {
            C.vb[e] = rhs;
            C.vM[e] = jacobi_inverse(k, md);
            C.vd[e] = 0.0f;
        }
    }
    for (int e = n + tid; e < ld; e += kSolveBlock) C.vp[e] = 0.0f;      // pad of p: read by the 16-byte mat-vec chunks
    __syncthreads();
}

// ---- trace: right-hand side and preconditioner in trace order -- (rot, trans); internal [trans, rot] -- and the matrix
__device__ __forceinline__ void trace_general_system(const SolveCtx &C)
{
    const SolveDims &D = C.D;
    const int n = C.n;
    float *tr = C.tr;
    for (int e = C.tid; e < n; e += kSolveBlock) {
        const int k = e / 6, r = e % 6;           // trace order (rot, trans); internal [trans, rot]
        const int o = k * 6 + (r < 3 ? r + 3 : r - 3);
        tr[D.tr_rhs + o] = C.vb[e];
        tr[D.tr_prec + o] = C.vM[e];
    }
    for (int e = C.tid; e < n * n; e += kSolveBlock) tr[D.tr_A + e] = C.A[(e / n) * C.ld + (e % n)];
}

// ---- phase C: Jacobi-preconditioned CG, SolverBundling.cu:575-818 (frame 0 entries stay 0).
//
// A_GLOBAL, large windows (n up to 510): all 16 waves, one row per thread.  A is symmetric, so thread `row` walks COLUMN `row`
// (A[k ld + row]: neighbouring threads read neighbouring addresses), p and the other vectors stay in LDS, the two dot
// products per step are workgroup sums.  Same recurrences and epsilon guards as the single-wave version below.
__device__ __forceinline__ void pcg_block(const SolveCtx &C)
{
    const SolveDims &D = C.D;
    const int tid = C.tid, n = C.n, ld = C.ld;
    const float *A = C.A;
    float *vp = C.vp, *tr = C.tr;
    const int row = tid;
    const bool live = row < n;
    float r_ = live ? C.vb[row] : 0.0f, m_ = live ? C.vM[row] : 0.0f, d_ = 0.0f;
    float p_ = m_ * r_;
    if (live) vp[row] = p_;
    float rz = block_sum(r_ * p_, C.scratch);          // (contains the barrier that makes vp visible)
    for (int li = 0; li < D.n_pcg; li++) {
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        if (live) {
            int k = 0;
            for (; k + 4 <= n; k += 4) {
                a0 += A[(size_t)k * ld + row] * vp[k]; a1 += A[(size_t)(k + 1) * ld + row] * vp[k + 1];
                a2 += A[(size_t)(k + 2) * ld + row] * vp[k + 2]; a3 += A[(size_t)(k + 3) * ld + row] * vp[k + 3];
            }
            for (; k < n; k++) a0 += A[(size_t)k * ld + row] * vp[k];
        }
        const float ap = (a0 + a1) + (a2 + a3);
        const float pAp = block_sum(live ? p_ * ap : 0.0f, C.scratch);
        const float alpha = (pAp > kEps) ? rz / pAp : 0.0f;
        d_ = d_ + alpha * p_;
        r_ = r_ - alpha * (live ? ap : 0.0f);
        const float z_ = m_ * r_;
        const float rz_new = block_sum(z_ * r_, C.scratch);
        const float beta = (rz > kEps) ? rz_new / rz : 0.0f;
        if (tr && tid == 0) { float *sc = tr + D.tr_pcg + 4 * li; sc[0] = pAp; sc[1] = alpha; sc[2] = rz_new; sc[3] = beta; }
        rz = rz_new;
        p_ = z_ + beta * p_;
        __syncthreads();                             // every thread has finished reading the old p
        if (live) vp[row] = p_;
        __syncthreads();
    }
    if (live) C.vd[row] = d_;
}

// The matrix-vector product of a one-wave PCG step on the LDS-resident matrix: rows lane + 64 j of A p into ap_[j].
template <int ROWS>
__device__ __forceinline__ void wave_matvec(const SolveCtx &C, int lane, float (&ap_)[ROWS])
{
    const int n = C.n, ld = C.ld;
    const float *A = C.A;
    const float4 *a0 = reinterpret_cast<const float4 *>(A + (size_t)min(lane, n - 1) * ld), *a1 = reinterpret_cast<const float4 *>(A + (size_t)min(lane + 64, n - 1) * ld);
    const float4 *a2 = reinterpret_cast<const float4 *>(A + (size_t)min(lane + 128, n - 1) * ld), *a3 = reinterpret_cast<const float4 *>(A + (size_t)min(lane + 192, n - 1) * ld);
    const float4 *p4 = reinterpret_cast<const float4 *>(C.vp);
    const int nq = ld >> 2;                       // 16-byte chunks per row (pad columns hold zeros)
    // four independent partial sums per row (x, y, z, w lanes of the 16-byte chunks): the single wave has no other
    // work to hide FMA latency behind, so a 92-long dependent chain per row was the critical path of this phase
    // ... as PACKED fp32 FMAs (v_pk_fma_f32, two lanes of a chunk per instruction): this wave is alone on its SIMD, so it is
    // bound by the one-instruction-per-four-cycles issue rate, where a packed FMA costs what a plain one does
    // (profiles/r02/valu_calibration.md) -- half the instructions for the same fused multiply-adds, bit for bit
    typedef float f2 __attribute__((ext_vector_type(2)));
    auto lo = [](const float4 &v) { return (f2){ v.x, v.y }; };
    auto hi = [](const float4 &v) { return (f2){ v.z, v.w }; };
    f2 q0a = (f2){ 0.f, 0.f }, q0b = q0a, q1a = q0a, q1b = q0a, q2a = q0a, q2b = q0a, q3a = q0a, q3b = q0a;
    if (ROWS == 2) {
_Pragma("unroll 8")
        for (int c = 0; c < nq; c++) {
            const float4 pc = p4[c], r0 = a0[c], r1 = a1[c];
            q0a = __builtin_elementwise_fma(lo(r0), lo(pc), q0a); q0b = __builtin_elementwise_fma(hi(r0), hi(pc), q0b);
            q1a = __builtin_elementwise_fma(lo(r1), lo(pc), q1a); q1b = __builtin_elementwise_fma(hi(r1), hi(pc), q1b);
        }
    } else {
_Pragma("unroll 4")
        for (int c = 0; c < nq; c++) {
            const float4 pc = p4[c], r0 = a0[c], r1 = a1[c], r2 = a2[c], r3 = a3[c];
            q0a = __builtin_elementwise_fma(lo(r0), lo(pc), q0a); q0b = __builtin_elementwise_fma(hi(r0), hi(pc), q0b);
            q1a = __builtin_elementwise_fma(lo(r1), lo(pc), q1a); q1b = __builtin_elementwise_fma(hi(r1), hi(pc), q1b);
            q2a = __builtin_elementwise_fma(lo(r2), lo(pc), q2a); q2b = __builtin_elementwise_fma(hi(r2), hi(pc), q2b);
            q3a = __builtin_elementwise_fma(lo(r3), lo(pc), q3a); q3b = __builtin_elementwise_fma(hi(r3), hi(pc), q3b);
        }
    }
    ap_[0] = (q0a.x + q0a.y) + (q0b.x + q0b.y); ap_[1] = (q1a.x + q1a.y) + (q1b.x + q1b.y);
    if (ROWS == 4) { ap_[ROWS - 2] = (q2a.x + q2a.y) + (q2b.x + q2b.y); ap_[ROWS - 1] = (q3a.x + q3a.y) + (q3b.x + q3b.y); }
}

// ONE wave runs the PCG: <= 186 unknowns = <= 3 rows per lane (4 provisioned), vectors live in registers, the two dot products per
// step are DPP wave sums, only p travels through LDS.  No workgroup barrier inside the iteration (the
// 16-wave version spent ~6 k cycles per step in barriers; this one ~1 k).
// ROWS per lane: 2 up to 128 unknowns (windows of <= 21 frames: every tracker-size window), 4 up to 186 (N <= BTBA_MAX_FRAMES_LDS = 31).
// One wave alone on its SIMD pays ~8 cycles per instruction, so the two dead rows of a 4-row loop cost real time (the sums only
// ever add their exact zeros: same bits either way).
// Wave 0 alone calls.  The `w0` tests below restate that: the compiler does not carry the caller's `tid < 64` into the loop, and lays the
// scalar control flow out with a few instructions more without them.
template <int ROWS>
__device__ __forceinline__ void pcg_wave(const SolveCtx &C)
{
    const SolveDims &D = C.D;
    const int tid = C.tid, n = C.n;
    // the caller's choice of ROWS: rows 0 and 1 of a lane of the 4-row version are always live.  NOT a mere hint: without it the compiler contracts one
    // multiply-add of the 4-row version differently, and traced windows of 24 and 31 frames lose bit equality with the traces of earlier builds
    __builtin_assume(n > 64 * (ROWS - 2));
    float *vp = C.vp, *tr = C.tr;
    const int lane = tid & 63;
    float r_[ROWS], m_[ROWS], p_[ROWS], d_[ROWS];
    const bool w0 = tid < 64;
    float part = 0.0f, rz = 0.0f;
    if (w0) {
#pragma unroll
        for (int j = 0; j < ROWS; j++) {
            const int row = lane + 64 * j;
            const bool live = row < n;
            r_[j] = live ? C.vb[row] : 0.0f; m_[j] = live ? C.vM[row] : 0.0f; d_[j] = 0.0f;
            p_[j] = m_[j] * r_[j];
            part += r_[j] * p_[j];
            if (live) vp[row] = p_[j];
        }
        rz = wave_sum_all(part);
    }
    for (int li = 0; li < D.n_pcg; li++) {
        float ap_[ROWS];
#pragma unroll
        for (int j = 0; j < ROWS; j++) ap_[j] = 0.0f;
        wave_matvec<ROWS>(C, lane, ap_);
        if (!w0) continue;
        part = 0.0f;
#pragma unroll
        for (int j = 0; j < ROWS; j++) part += (lane + 64 * j < n) ? p_[j] * ap_[j] : 0.0f;
        const float pAp = wave_sum_all(part);
        const float alpha = (pAp > kEps) ? rz / pAp : 0.0f;
        float z_[ROWS];
        part = 0.0f;
#pragma unroll
        for (int j = 0; j < ROWS; j++) {
            const bool live = lane + 64 * j < n;
            d_[j] = d_[j] + alpha * p_[j];
            r_[j] = r_[j] - alpha * (live ? ap_[j] : 0.0f);
            z_[j] = m_[j] * r_[j];
            part += z_[j] * r_[j];
        }
        const float rz_new = wave_sum_all(part);
        const float beta = (rz > kEps) ? rz_new / rz : 0.0f;
        if (tr && lane == 0) { float *sc = tr + D.tr_pcg + 4 * li; sc[0] = pAp; sc[1] = alpha; sc[2] = rz_new; sc[3] = beta; }
        rz = rz_new;
#pragma unroll
        for (int j = 0; j < ROWS; j++) {
            p_[j] = z_[j] + beta * p_[j];
            if (lane + 64 * j < n) vp[lane + 64 * j] = p_[j];
        }
    }
    if (w0) {
#pragma unroll
        for (int j = 0; j < ROWS; j++) if (lane + 64 * j < n) C.vd[lane + 64 * j] = d_[j];
    }
}

// ---- phase D: x_k <- Log(Exp(delta_k) Exp(x_k)); next iterate's T, T^-1  (SolverBundling.cu:805-815, 890-897)
__device__ __forceinline__ void update_general(const SolveCtx &C)
{
    const SolveDims &D = C.D;
    const SolveIO &io = C.io;
    const float *vd = C.vd;
    float *tr = C.tr;
    for (int k = C.tid; k < C.N; k += kSolveBlock) {
        float *xk = io.x + 6 * k;
        const float *xl = C.x_l + 6 * k;
        float rot[3] = { xl[0], xl[1], xl[2] }, trans[3] = { xl[3], xl[4], xl[5] };
        if (k > 0) {
            const float dW[3] = { vd[6 * k + 3], vd[6 * k + 4], vd[6 * k + 5] }, dT[3] = { vd[6 * k], vd[6 * k + 1], vd[6 * k + 2] };
            const Mat4 U = pose_to_matrix(dW, dT);
            const Mat4 Ck = load_mat4(C.vT + 16 * k);      // = Exp(x_k): this iterate's T, computed from the same x_k by the previous launch
            matrix_to_pose(mat_mul(U, Ck), rot, trans);
        }
        if (k > 0) { xk[0] = rot[0]; xk[1] = rot[1]; xk[2] = rot[2]; xk[3] = trans[0]; xk[4] = trans[1]; xk[5] = trans[2]; }      // (frame 0 keeps its x)
        const Mat4 E = pose_to_matrix(rot, trans);
        store_mat4(io.T + 16 * k, E);
        if (io.poses_out) store_mat4(io.poses_out + 16 * k, E);      // last iterate: convertPosesToMatricesCU (SBA.cpp:115), no separate copy
        store_mat4(io.Tinv + 16 * k, mat_inverse(E));
        if (tr) {
            for (int q = 0; q < 3; q++) { tr[D.tr_x + 6 * k + q] = rot[q]; tr[D.tr_x + 6 * k + 3 + q] = trans[q]; }
            for (int q = 0; q < 16; q++) tr[D.tr_T + 16 * k + q] = E.m[q];
            for (int q = 0; q < 3; q++) { tr[D.tr_delta + 6 * k + q] = vd[6 * k + 3 + q]; tr[D.tr_delta + 6 * k + 3 + q] = vd[6 * k + q]; }
        }
    }
}

// The system solve of ONE instance by the calling workgroup of kSolveBlock threads (all of them must call; dynamic LDS: SolveLayout, plus
// (optionally) the reduced pair sums behind it): one-wave PCG on the LDS-resident matrix, or the 16-wave PCG of A_GLOBAL -- windows of more than
// BTBA_MAX_FRAMES_LDS frames, whose matrix does not fit the CU's LDS and lives in an L2-resident global scratch.
template <bool LDS_PAIRS, bool A_GLOBAL>
__device__ __forceinline__ void system_solve_body(const SolveDims &D, int iter, const int tid, float *lds, const SolveIO &io,
                                                  const int2 *__restrict__ dense_pairs, const int *__restrict__ adj_off, const int *__restrict__ adj,
                                                  const int *__restrict__ solve_tab)
{
    const int N = D.n_frames, n = 6 * N;
    const SolveLayout L(N, D.n_dense_pairs, A_GLOBAL);
    float *tr = (D.trace_on && io.trace) ? io.trace + (size_t)iter * D.trace_record : nullptr;
    float *ps = LDS_PAIRS ? lds + L.total : io.pairsum_global;
    const SolveCtx C(D, io, tid, tr, lds, L, A_GLOBAL, ps, ps + (size_t)D.n_pairs * kSparseVals);

    if (D.pre_assembled) load_pre_assembled<A_GLOBAL>(C);
    else {
        const SolveTables G = { dense_pairs, adj_off, adj, solve_tab };
        const GeneralStaged staged = stage_load(C, G);
        trace_stamp(C, 6);
        reduce_partials_general(C);
        trace_stamp(C, 7);
        stage_store(C, G, staged);
        // zero what the assembly does not write; every other entry is assigned by phase B (all canonical pairs with i >= 1, all diagonal blocks k >= 1)
        for (int e = tid; e < 6 * L.ld; e += kSolveBlock) C.A[e] = 0.0f;
        for (int e = tid; e < (n - 6) * (6 + L.ld - n); e += kSolveBlock) C.A[zero_fill_rest_index(e, n, L.ld)] = 0.0f;
        __syncthreads();
        trace_stamp(C, 0);
        // (the camera-frame -> model-frame congruence of the dense pair sums is done by the sweep workgroups: dense_epilogue)
        if (tr && D.use_dense) for (int e = tid; e < D.n_dense_pairs * kDenseVals; e += kSolveBlock) tr[D.tr_dpair + e] = C.pd[e];
        trace_stamp(C, 1);
        assemble(C);
    }
    trace_stamp(C, 2);
    if (tr) trace_general_system(C);
    trace_stamp(C, 5);
    if (A_GLOBAL) pcg_block(C);
    else if (tid < 64) { if (n <= 128) pcg_wave<2>(C); else pcg_wave<4>(C); }
    __syncthreads();
    trace_stamp(C, 3);
    update_general(C);
    trace_stamp(C, 4);
}

// grid (B) x kSolveBlock: one workgroup per instance, x / T / T^-1 updated in place.
template <bool LDS_PAIRS, bool A_GLOBAL = false>
__global__ void __launch_bounds__(kSolveBlock) k_system_solve(SolveDims D, int iter,
                                                        float *sparse_partials, float *dense_partials,
                                                        const int2 *__restrict__ dense_pairs, const int *__restrict__ adj_off, const int *__restrict__ adj,
                                                        float *__restrict__ x, float *__restrict__ T, float *__restrict__ Tinv,
                                                        float *__restrict__ pairsum_global, float *__restrict__ trace, float *__restrict__ A_scratch = nullptr,
                                                        float *__restrict__ poses_out = nullptr, const int *__restrict__ solve_tab = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const size_t b = blockIdx.x;
    const int N = D.n_frames, n = 6 * N, ld = solve_row_floats(N);
    SolveIO io;
    io.sparse_partials = sparse_partials + b * D.sp_stride; io.dense_partials = dense_partials + b * D.dp_stride;
    io.x = x + b * D.x_stride;
    io.T = T + b * D.pose_stride; io.Tinv = Tinv + b * D.pose_stride;
    io.poses_out = poses_out ? poses_out + 16 * b * N : nullptr;
    io.pairsum_global = pairsum_global ? pairsum_global + b * ((size_t)D.n_pairs * kSparseVals + (size_t)D.n_dense_pairs * kDenseVals) : nullptr;
    io.A_scratch = A_scratch ? A_scratch + b * (size_t)(n + 2) * ld : nullptr;
    io.trace = trace ? trace + b * (size_t)D.n_gn * D.trace_record : nullptr;
    system_solve_body<LDS_PAIRS, A_GLOBAL>(D, iter, (int)threadIdx.x, lds, io, dense_pairs, adj_off, adj, solve_tab);
}

}  // namespace btba
