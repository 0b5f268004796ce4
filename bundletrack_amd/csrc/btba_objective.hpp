// btba_objective.hpp -- the objective report (btba_objective_batch_zn_aux): the cost the Gauss-Newton loop descends, evaluated at given poses.
//
// Three sweeps and a fold, all on the matrices k_prepare makes of the caller's poses:
//   k_objective_sparse          grid (chunks, P, B): chunk c of pair p's correspondence segment, r = T_i pos_i - T_j pos_j from the sparse sweep's entry decode
//   k_objective_dense_pinhole   grid (tiles * Pd, B): 1 024 source pixels of a dense pair; the set-up phases of dense_block_pinhole<0> and, per pixel, pinhole_pixel's stages
//   k_objective_dense_general   the same for a K with skew or a projective last row: dense_block_zn's item set-up and pixel stages
//   k_objective_fold            grid (B): tiles and chunks in index order into the pair records, the pair records in index order into the instance's totals
// Every residual and accept test is fp32 and the sweeps' own device function (btba_kernels.hpp), called, not written again: the sweep accumulates Jacobian
// sums behind it, these kernels fp64 cost.  Everything behind it is IEEE fp64 with contraction off (a product of two fp32 values is exact in
// fp64, so e = r.r and res^2 carry only the roundings of their additions).  No hull cull, no block lists, no valid-pixel lists: every pixel of the source
// frame is walked -- this runs once per solve, not once per iterate.  No atomics: a lane sums its trips in ascending index order, a wave folds by a
// butterfly (xor 1, 2, 4, 8, 16, 32: the wave reductions of btba_device.hpp are fp32 and sum onto lane 63; this is their fp64 counterpart with the result
// in every lane), the four waves are added in wave order, tiles / chunks / pairs in index order.  All of these orders follow from the cache size, the
// segment lengths and the window size: an instance gives the same bytes at any batch position and in any batch size.
// This header needs the sweeps' device functions and is therefore included by the ONE unit that includes btba_kernels.hpp (btba_api.hip: that header
// defines kernels, two units with it would not link); the entry point's own unit, btba_api_objective.hip, reaches the launches through objective_enqueue.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/btba.h"
#include "btba_kernels.hpp"
#include "btba_objective_layout.hpp"

namespace btba {

static_assert(sizeof(btba_objective_pair) == kObjectiveRecordBytes, "a partial record is a btba_objective_pair");
static_assert(kObjectiveBlock == kBlock, "the sweeps' set-up phases (pinhole tables, zn_item_setup) fill their tables with kBlock lanes");

// what one lane, then one wave, then one workgroup has seen
struct ObjectiveAcc {
    double sq, rho, mx;             // sum_sq, sum_rho, max_abs (-1: nothing seen)
    int cnt, out, idx;              // count, n_outlier, worst (INT32_MAX: nothing seen)
};
__device__ __forceinline__ ObjectiveAcc objective_acc_empty() { return ObjectiveAcc{ 0.0, 0.0, -1.0, 0, 0, 0x7FFFFFFF }; }

// the Huber constants in fp64: delta is the fp32 parameter widened, its square exact
struct ObjectiveHuber { double delta, delta2; };
__device__ __forceinline__ ObjectiveHuber objective_huber(float robust_delta) { const double d = (double)robust_delta; return ObjectiveHuber{ d, d * d }; }

// rho(e) of huberLoss (SolverBundlingUtil.h:24-40): e inside the knee, 2 delta sqrt(e) - delta^2 beyond it
__device__ __forceinline__ double objective_rho(const ObjectiveHuber &h, double e)
{
#pragma clang fp contract(off)
    return e <= h.delta2 ? e : 2.0 * h.delta * sqrt(e) - h.delta2;
}

// one sparse entry: r in fp32; e = (rx^2 + ry^2) + rz^2
__device__ __forceinline__ void objective_add_sparse(ObjectiveAcc &a, const ObjectiveHuber &h, float rx, float ry, float rz, int index)
{
#pragma clang fp contract(off)
    const double x = (double)rx, y = (double)ry, z = (double)rz;
    const double e = (x * x + y * y) + z * z;
    a.sq += e;
    a.rho += objective_rho(h, e);
    a.cnt += 1;
    a.out += e > h.delta2 ? 1 : 0;
    const double m = (double)fmaxf(fmaxf(fabsf(rx), fabsf(ry)), fabsf(rz));
    if (m > a.mx) { a.mx = m; a.idx = index; }      // (a lane's indices ascend: the first to reach the maximum keeps it)
}

// one accepted dense pixel: res in fp32; the weighted square is w res^2 with w = min(1, delta / |res|)
__device__ __forceinline__ void objective_add_dense(ObjectiveAcc &a, const ObjectiveHuber &h, float res, int index)
{
#pragma clang fp contract(off)
    const double r = fabs((double)res), e = r * r;
    const double w = e <= h.delta2 ? 1.0 : h.delta / r;
    a.sq += w * e;
    a.rho += objective_rho(h, e);
    a.cnt += 1;
    a.out += e > h.delta2 ? 1 : 0;
    if (r > a.mx) { a.mx = r; a.idx = index; }
}

// the larger maximum, the lower index on ties
__device__ __forceinline__ void objective_take_max(double &mx, int &idx, double o_mx, int o_idx)
{
    const bool take = (o_mx > mx) | ((o_mx == mx) & (o_idx < idx));
    mx = take ? o_mx : mx; idx = take ? o_idx : idx;
}

// wave butterfly: every lane ends with the wave's record
__device__ __forceinline__ ObjectiveAcc objective_wave_fold(ObjectiveAcc a)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        a.sq += __shfl_xor(a.sq, m, 64);
        a.rho += __shfl_xor(a.rho, m, 64);
        a.cnt += __shfl_xor(a.cnt, m, 64);
        a.out += __shfl_xor(a.out, m, 64);
        const double o_mx = __shfl_xor(a.mx, m, 64);
        const int o_idx = __shfl_xor(a.idx, m, 64);
        objective_take_max(a.mx, a.idx, o_mx, o_idx);
    }
    return a;
}

// the workgroup's record: waves through LDS, added in wave order by thread 0
__device__ __forceinline__ void objective_block_store(const ObjectiveAcc &lane_acc, ObjectiveAcc *red, btba_objective_pair *out)
{
#pragma clang fp contract(off)
    const unsigned tid = threadIdx.x;
    const ObjectiveAcc w = objective_wave_fold(lane_acc);
    if ((tid & 63u) == 0u) red[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
        ObjectiveAcc s = red[0];
        for (int k = 1; k < kObjectiveBlock / 64; k++) {
            s.sq += red[k].sq; s.rho += red[k].rho; s.cnt += red[k].cnt; s.out += red[k].out;
            objective_take_max(s.mx, s.idx, red[k].mx, red[k].idx);
        }
        btba_objective_pair r;
        r.sum_sq = s.sq; r.sum_rho = s.rho; r.max_abs = s.cnt > 0 ? s.mx : 0.0;
        r.count = s.cnt; r.n_outlier = s.out; r.worst = s.cnt > 0 ? s.idx : -1; r.reserved = 0;
        *out = r;
    }
}

// ---- sparse: grid (chunks, P, B) ----------------------------------------------------------------------------------------------------
// corr: EntryJ (two float4 per entry) or, with D.corr24, the 24-byte records in their three-plane groups of 64 (corr24_index); an entry whose
// first word is 0xFFFFFFFF is invalid and skipped, as the sparse sweep skips it.  The index a record reports counts from the segment's start.
__global__ void __launch_bounds__(kObjectiveBlock) k_objective_sparse(SolveDims D, ObjectiveLayout lay, const float4 *__restrict__ corr, const uint32_t *__restrict__ pair_offsets,
                                                                      const float *__restrict__ T, btba_objective_pair *__restrict__ partials)
{
    __shared__ ObjectiveAcc red[kObjectiveBlock / 64];
    const int chunk = blockIdx.x, p = blockIdx.y, b = blockIdx.z;
    const unsigned tid = threadIdx.x;
    int fi, fj;
    pair_from_index(p, D.n_frames, fi, fj);
    const uint32_t *off = pair_offsets + (size_t)b * (D.n_pairs + 1);
    const uint32_t seg0 = off[p], len = off[p + 1] - seg0;
    const uint32_t lo = objective_chunk_lo(len, chunk), hi = objective_chunk_hi(len, chunk);
    const float *Tb = T + (size_t)b * (size_t)D.pose_stride;
    const Mat4 Ti = load_mat4(Tb + 16 * fi), Tj = load_mat4(Tb + 16 * fj);
    const ObjectiveHuber h = objective_huber(D.robust_delta);
    ObjectiveAcc acc = objective_acc_empty();
    const size_t e_base = (size_t)b * (size_t)D.corr_stride + seg0;
    for (uint32_t e = lo + tid; e < hi; e += kObjectiveBlock) {
        SparseEntry E;
        if (D.corr24) {
            const float2 *q = reinterpret_cast<const float2 *>(corr) + corr24_index(e_base + e);
            E = sparse_entry_c24(q[0], q[64], q[128]);
        } else E = sparse_entry_j(corr[2 * (e_base + e)], corr[2 * (e_base + e) + 1]);
        if (!E.valid) continue;
        float wix, wiy, wiz, wjx, wjy, wjz;
        xform_point(Ti, E.pix, E.piy, E.piz, wix, wiy, wiz);
        xform_point(Tj, E.pjx, E.pjy, E.pjz, wjx, wjy, wjz);
        objective_add_sparse(acc, h, wix - wjx, wiy - wjy, wiz - wjz, (int)e);
    }
    objective_block_store(acc, red, partials + lay.sparse_record(D.n_pairs, b, p, chunk));
}

// ---- dense, pinhole K: grid (tiles * Pd, B) -------------------------------------------------------------------------------------------
// One source pixel through the stages pinhole_pixel runs (btba_kernels.hpp), the single tests AND-ed per lane.  Returns whether the solver accepts it; res = (c_i - q) . n_i.
__device__ __forceinline__ bool objective_pinhole_pixel(const PinholeCtx &C, const float4 &zs, unsigned ox, unsigned oy, float &res)
{
    const PinholeProj P = pinhole_project(C, zs, ox, oy);
    if (!(P.src_ok & P.in_u & P.in_v)) return false;
    const float3 nq = pinhole_rotate_normal(C, zs);
    const PinholeTaps K = pinhole_taps(C, P);
    float4 z00, z10, z01, z11;
    pinhole_gather(C, K, z00, z10, z01, z11);
    const PinholeBlend B = pinhole_blend(C, P, K, z00, z10, z01, z11, nq);
    res = -pinhole_residual(B);                             // pinhole_pixel keeps (q - c_i) . n_i and puts the sign right once per workgroup
    return B.ciz_ok & B.dn_ok & B.dist_ok;
}

// D: the solve's dimensions with dense_tiles = 1 (the set-up phases then see one band, which the strip walk ignores); blockIdx.x = tile + tiles * work position
__global__ void __launch_bounds__(kObjectiveBlock) k_objective_dense_pinhole(SolveDims D, ObjectiveLayout lay, const float4 *__restrict__ zn, const float *__restrict__ T,
                                                                             const float *__restrict__ Tinv, btba_objective_pair *__restrict__ partials)
{
    __shared__ ObjectiveAcc red[kObjectiveBlock / 64];
    extern __shared__ __attribute__((aligned(16))) float objective_lds[];      // SweepLayout(Wd, Hd, 0, kSweepLdsStrips)
    const int tile = (int)(blockIdx.x % (unsigned)lay.tiles), q = (int)(blockIdx.x / (unsigned)lay.tiles), b = blockIdx.y;
    PinholeCtx C;
    (void)pinhole_item_and_poses<0>(D, C, q, T, Tinv, 0, b);
    pinhole_fill_tables<0>(D, C, objective_lds);
    (void)pinhole_live_blocks<0>(D, C);                   // (the barrier behind the tables)
    pinhole_walk_constants(D, C, zn);
    const ObjectiveHuber h = objective_huber(D.robust_delta);
    ObjectiveAcc acc = objective_acc_empty();
    const int lo = objective_tile_lo(D.npix, tile), hi = objective_tile_hi(D.npix, tile);
    for (int s = lo + (int)threadIdx.x; s < hi; s += kObjectiveBlock) {
        const int py = s / D.width, px = s - py * D.width;
        float res;
        // 16-byte entries of the ray tables: the column's, and the row's behind all columns
        if (objective_pinhole_pixel(C, C.zn_s[s], 16u * (unsigned)px, 16u * (unsigned)(D.width + py), res)) objective_add_dense(acc, h, res, s);
    }
    objective_block_store(acc, red, partials + lay.dense_record(D.n_dense_pairs, b, C.p, tile));
}

// ---- dense, general K -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kObjectiveBlock) k_objective_dense_general(SolveDims D, ObjectiveLayout lay, const float4 *__restrict__ zn, const float *__restrict__ T,
                                                                             const float *__restrict__ Tinv, btba_objective_pair *__restrict__ partials)
{
    __shared__ ObjectiveAcc red[kObjectiveBlock / 64];
    extern __shared__ __attribute__((aligned(16))) float objective_lds[];      // SweepLayout(Wd, Hd, 0, kSweepLdsGeneralK): (Wd + Hd) floats
    const int tile = (int)(blockIdx.x % (unsigned)lay.tiles), q = (int)(blockIdx.x / (unsigned)lay.tiles), b = blockIdx.y;
    const int4 item = D.dense_work[q];                    // (target, source, dense pair, -)
    const ZnItem I = zn_item_setup(D, zn, T, Tinv, item.x, item.y, b, objective_lds);
    const ObjectiveHuber h = objective_huber(D.robust_delta);
    ObjectiveAcc acc = objective_acc_empty();
    const int lo = objective_tile_lo(D.npix, tile), hi = objective_tile_hi(D.npix, tile);
    for (int s = lo + (int)threadIdx.x; s < hi; s += kObjectiveBlock) {
        const int py = s / D.width, px = s - py * D.width;
        const PixelGeom g = zn_pixel_geom(D, I, px, py, I.zn_s[s]);
        if (!g.valid) continue;
        const PixelBlend B = zn_pixel_blend(D, I, g);
        if (B.ok) objective_add_dense(acc, h, B.res, s);
    }
    objective_block_store(acc, red, partials + lay.dense_record(D.n_dense_pairs, b, item.z, tile));
}

// ---- fold: grid (B) ---------------------------------------------------------------------------------------------------------------
struct ObjectiveFoldArgs {
    int Pd_out, Pd, P_out, P;       // pair records the caller's arrays hold per instance; pairs the sweeps evaluated (0: that term is absent, its records are empty)
    float w_sparse, w_dense;
    const btba_objective_pair *dense_partials, *sparse_partials;
    btba_objective_pair *dense_folded, *sparse_folded;      // scratch [B][Pd], [B][P]: record 0 of every pair's run of partials, overwritten in place
    btba_objective_pair *dense_out, *sparse_out;            // nullptr, or the caller's arrays
    btba_objective_total *total;
};

// n partial records in index order -> one record
__device__ __forceinline__ btba_objective_pair objective_fold_run(const btba_objective_pair *r, int n)
{
#pragma clang fp contract(off)
    btba_objective_pair s;
    s.sum_sq = 0.0; s.sum_rho = 0.0; s.max_abs = 0.0; s.count = 0; s.n_outlier = 0; s.worst = -1; s.reserved = 0;
    for (int k = 0; k < n; k++) {
        s.sum_sq += r[k].sum_sq; s.sum_rho += r[k].sum_rho; s.count += r[k].count; s.n_outlier += r[k].n_outlier;
        if (r[k].worst >= 0 && (s.worst < 0 || r[k].max_abs > s.max_abs)) { s.max_abs = r[k].max_abs; s.worst = r[k].worst; }      // (indices ascend with k: the first maximum keeps it)
    }
    return s;
}

// sum of n pair records in index order by one wave: 64 records per coalesced round, added lane by lane
__device__ __forceinline__ void objective_sum_pairs(const btba_objective_pair *rec, int stride, int n, double &rho, double &sq, long long &count)
{
#pragma clang fp contract(off)
    const int lane = (int)(threadIdx.x & 63u);
    rho = 0.0; sq = 0.0; count = 0;
    for (int base = 0; base < n; base += 64) {
        const int k = base + lane;
        const double my_rho = k < n ? rec[(size_t)k * stride].sum_rho : 0.0, my_sq = k < n ? rec[(size_t)k * stride].sum_sq : 0.0;
        const int my_cnt = k < n ? rec[(size_t)k * stride].count : 0;
        const int m = min(64, n - base);
        for (int l = 0; l < m; l++) { rho += __shfl(my_rho, l, 64); sq += __shfl(my_sq, l, 64); count += __shfl(my_cnt, l, 64); }
    }
}

__global__ void __launch_bounds__(kObjectiveBlock) k_objective_fold(ObjectiveFoldArgs A, ObjectiveLayout lay)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x, tid = (int)threadIdx.x;
    btba_objective_pair empty;
    empty.sum_sq = 0.0; empty.sum_rho = 0.0; empty.max_abs = 0.0; empty.count = 0; empty.n_outlier = 0; empty.worst = -1; empty.reserved = 0;
    // pair records: a thread folds the run of partials of its pairs and leaves the result in the run's first record
    for (int p = tid; p < A.Pd; p += kObjectiveBlock) {
        const size_t at = lay.dense_record(A.Pd, b, p, 0);
        const btba_objective_pair s = objective_fold_run(A.dense_partials + at, lay.tiles);
        A.dense_folded[at] = s;
        if (A.dense_out) A.dense_out[(size_t)b * A.Pd_out + p] = s;
    }
    for (int p = tid; p < A.P; p += kObjectiveBlock) {
        const size_t at = lay.sparse_record(A.P, b, p, 0);
        const btba_objective_pair s = objective_fold_run(A.sparse_partials + at, lay.chunks);
        A.sparse_folded[at] = s;
        if (A.sparse_out) A.sparse_out[(size_t)b * A.P_out + p] = s;
    }
    // a term the call does not evaluate: empty records
    if (A.dense_out) for (int p = A.Pd + tid; p < A.Pd_out; p += kObjectiveBlock) A.dense_out[(size_t)b * A.Pd_out + p] = empty;
    if (A.sparse_out) for (int p = A.P + tid; p < A.P_out; p += kObjectiveBlock) A.sparse_out[(size_t)b * A.P_out + p] = empty;
    __threadfence_block();
    __syncthreads();
    if (tid < 64) {
        double s_rho, s_sq, d_rho, d_sq;
        long long n_s, n_d;
        objective_sum_pairs(A.sparse_folded + (A.P ? lay.sparse_record(A.P, b, 0, 0) : 0), lay.chunks, A.P, s_rho, s_sq, n_s);
        objective_sum_pairs(A.dense_folded + (A.Pd ? lay.dense_record(A.Pd, b, 0, 0) : 0), lay.tiles, A.Pd, d_rho, d_sq, n_d);
        if (tid == 0) {
            btba_objective_total t;
            const double ws = (double)A.w_sparse * s_rho, wd = (double)A.w_dense * d_rho;
            t.objective = ws + wd;
            t.sparse_rho = s_rho; t.dense_rho = d_rho; t.sparse_sq = s_sq; t.dense_wsq = d_sq;
            t.n_sparse = n_s; t.n_dense = n_d; t.n_residuals = 3 * n_s + n_d;
            A.total[b] = t;
        }
    }
}

}  // namespace btba
