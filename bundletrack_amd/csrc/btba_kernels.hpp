// btba_kernels.hpp -- the gfx950 kernels of the bundle-adjustment hot path.
//
// One Gauss-Newton iteration = three launches (reference: 37 launches, 11 memsets, one blocking
// D2H copy and a cudaMalloc/cudaFree pair):
//
//   sparse_sweep  (A11/A12)  one pass over EntryJ[]: per frame pair the Huber-weighted right-hand
//                            side, the Jacobi preconditioner diagonal AND the moment sums from
//                            which the *unweighted* sparse J^T J blocks follow in closed form.
//                            Replaces PCGInit_Kernel1 (one thread per frame!) and the 5 x
//                            (PCGStep_Kernel0 + PCGStep_Kernel1a) matrix-free passes.
//   dense_sweep   (A10)      the point-to-plane Jacobian sweep: per (pair, pixel) projective
//                            association, bilinear target lookup, residual, Huber weight and the
//                            closed-form row a = [-n_w ; n_w x w]; since row_i = -row_j only
//                            S = sum w a a^T (21) and g = sum w a res (6) are reduced per pair.
//                            Replaces BuildDenseSystem_Kernel + FlipJtJ_Kernel (and drops the dead
//                            FindDenseCorrespondences_Kernel twin pass).
//   system_solve  (A11-A13)  one workgroup per instance: fixed-order reduction of the partials,
//                            assembly of the 6N x 6N normal matrix in LDS, Jacobi-PCG entirely in
//                            LDS, SE(3) update, next iterate's T and T^-1.
//
// This file holds what all of them share (SolveDims, the frame caches) and the sweeps; the system solves are in
// btba_solve_general.hpp (k_system_solve, k_big_reduce, k_big_assemble), btba_solve_small.hpp and btba_solve_mid.hpp.  The dynamic-LDS
// layout of a dense item on the compact cache is btba_sweep_layout.hpp (shared with the host).
//
// Summation is deterministic (fixed DPP tree inside a wave, fixed order across waves, tiles and
// pairs); the reference uses float atomics (SURVEY.md section 5 "race detection").
#pragma once
#ifndef BTBA_FUSED_WAVES
#define BTBA_FUSED_WAVES 6      // waves per SIMD the fused sweep is compiled for (80 VGPRs)
#endif
#if defined(BTBA_REFERENCE_ORDER) && !defined(BTBA_EXACT_DIV)
#define BTBA_EXACT_DIV 1        // the reference-order experiment build (tests/tools/reference_order_experiment.py) divides and takes roots exactly, like the oracle
#endif
#include <type_traits>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "btba_device.hpp"
#include "btba_hull.hpp"
#include "btba_sweep_layout.hpp"

namespace btba {

constexpr int kBlock = 256;          // 4 waves (sweeps)
constexpr int kSolveBlock = 1024;    // 16 waves: the per-instance solve is latency-bound serial phases, so go wide
constexpr int kSparseVals = 44;      // per-pair sparse partial record
constexpr int kDenseVals = 28;       // per-pair dense partial record: S(21) g(6) count(1)
constexpr float kEps = 0.000001f;    // FLOAT_EPSILON, SolverUtil.h:10
constexpr int kRedFloats = 4 * kSparseVals + 8;   // LDS scratch of a sweep workgroup: 4 waves x 44 sparse sums, or 4 x 28 dense sums + their total (28) + M (36)

// sparse record layout
//  0      n (valid count)
//  1..3   sum w_i           4..6   sum w_j
//  7..12  sum w_i w_i^T (xx xy xz yy yz zz)     13..18 same for w_j
//  19..27 sum w_i w_j^T (row-major 3x3)
//  28..30 sum rho r         31..33 sum rho (w_i x r)      34..36 sum rho (w_j x r)
//  37     sum rho
//  38..40 sum rho (wy^2+wz^2, wx^2+wz^2, wx^2+wy^2) at w_i     41..43 same at w_j

struct SolveDims {
    int n_frames;        // N
    int n_pairs;         // P = N(N-1)/2 canonical correspondence pairs
    int n_dense_pairs;   // Pd
    int npix, width, height;
    int sparse_chunks;   // workgroups per correspondence segment
    int dense_tiles;     // workgroups per dense pair
    int n_pcg;
    int use_sparse, use_dense;
    float fx, fy, cx, cy;
    float robust_delta, dist_thresh, normal_thresh, depth_min, depth_max;
    float dist2_thresh;  // dist_thresh^2 (fp32 product, formed once on the host)
    float wm1, hm1, wm2, hm2;     // (float)(width - 1), (height - 1), (width - 2), (height - 2): the dense sweep's clamp bounds -- from the host, so that they arrive in SCALAR registers
    float w_sparse, w_dense;
    int64_t corr_stride; // EntryJ per instance block
    int trace_on;
    int64_t trace_record; // floats per (instance, iteration) record
    int64_t tr_x, tr_T, tr_rhs, tr_prec, tr_pcg, tr_delta, tr_dpair, tr_A, tr_clk;
    int n_gn;
    int pairsum_in_lds;  // 1: stage reduced pair sums in LDS, 0: in global scratch
    int pre_assembled;   // large windows: k_big_reduce + k_big_assemble have built the system, k_system_solve only solves and updates
    int walk_blocks;     // pinhole sweep on the compact cache: waves walk 8 x 8 pixel blocks (width and height multiples of 8)
    const int4 *dense_work;       // work position q -> (target, source, dense pair, -): the order the sweeps work the pairs off, heaviest first
    int work_formula;             // 1 / 2: the table is the closed form "all pairs by ascending |i - j|, then ascending i" with target = lower / higher
                                  // frame -- the pinhole sweeps then compute their item instead of loading it (one memory round trip less)
    const float2 *block_ranges;   // per (cache slot, 8 x 8 block): [min, max] valid depth (k_block_ranges); nullptr: no block is skipped
    int sparse_tail_256; // fused sweep: share (in 1/256) of the sparse items placed at the END of each XCD's item sequence instead of interleaved
    int tile_major;      // dense work order inside an instance: 1 = (tile, pair) -- all pairs' band t of the images together -- 0 = (pair, tile)
    int *order_flag;     // non-null: the sparse sweep ORs 1 into it when an entry does not belong to the pair of its segment
    int atomic_sums;     // BTBA_REDUCE_ATOMIC: sweep workgroups ADD their sums into one record per pair (float atomics) instead of storing one record
                         // per (pair, chunk / tile); k_system_solve reads those records (chunks = tiles = 1 on its side) and clears them for the next iteration
    int corr24;          // the correspondences are 24-byte (pos_i, pos_j) records (k_pack_corr24) instead of EntryJ
    int64_t corr_entry0; // 24-byte layout: entry index of this launch's first instance in the array
    const uint32_t *pair_lens;   // non-null: [B][P] segment lengths (segments not back to back: the keyed pool); else offsets[p + 1] - offsets[p]
    // compact (z, nx, ny, nz) frame cache: how a cached pixel maps back to camera space -- the arithmetic of k_build_cache
    float zn_ki[16];     // full-resolution intrinsicsInv (4x4 embedding, generic cofactor inverse)
    float zn_scale_w, zn_scale_h;   // (W-1)/(Wd-1), (H-1)/(Hd-1) of the nearest-neighbour resample
    int zn_simple;       // 1: zero skew and affine last row (ki[1]=ki[3]=ki[4]=ki[7]=ki[12]=ki[13]=ki[14]=0)
    // persistent frame cache: frame f of the solve lives in pool slot frame_slot[f] (nullptr: slot == f, contiguous cache)
    const int *frame_slot;
    // floats per INSTANCE in the pose arrays (T, Tinv: 16 N), the state array (x: 6 N) and the sweep partials: the instances lie back to back.
    // (the two pose strides arrive as kernel arguments although they follow from N: computed in the kernels they measured +0.5 % on the fused
    // sweep at c3 x 32, profiles/chain_removal/ab.json)
    int pose_stride, x_stride;
    unsigned sp_stride, dp_stride;      // (32-bit: an instance's partials are a few MB at most; 64-bit strides cost the short masked / sparse items ~100 scalar instructions)
    float2 *corr24_out;  // non-null (EntryJ sweeps only): the sweep also WRITES every entry it reads as a 24-byte record (corr24_index layout, entry index counted from
                         // corr_entry0 + b * corr_stride): the first iteration of a solve re-lays the caller's fresh EntryJ array out for the iterations that follow
    unsigned long long *live_blocks;   // non-null (BTBA_OPT_COUNT_LIVE, bench.py's roofline.executed): every block-walk workgroup adds the number of 8 x 8 blocks it walks
    int corr_nt_from;    // instances b >= corr_nt_from read their correspondences with NON-TEMPORAL loads: once a batch's frames + correspondences exceed the memory-side
                         // cache, the read-once stream otherwise evicts the frames the dense items re-read every iteration (btba_api.hip: corr_nt_auto); what still fits
                         // beside the frames -- the first instances' correspondences -- stays cached, and below the limit plain loads are faster for everything
};

__device__ __forceinline__ size_t frame_slot_of(const SolveDims &D, size_t f) { return D.frame_slot ? (size_t)D.frame_slot[f] : f; }

__device__ __forceinline__ int pair_index(int i, int j, int n) { return i * n - i * (i + 1) / 2 + (j - i - 1); }

__device__ __forceinline__ Mat4 mat4_rows(const float4 &a, const float4 &b, const float4 &c, const float4 &d)
{
    Mat4 m;
    m.m[0] = a.x; m.m[1] = a.y; m.m[2] = a.z; m.m[3] = a.w;
    m.m[4] = b.x; m.m[5] = b.y; m.m[6] = b.z; m.m[7] = b.w;
    m.m[8] = c.x; m.m[9] = c.y; m.m[10] = c.z; m.m[11] = c.w;
    m.m[12] = d.x; m.m[13] = d.y; m.m[14] = d.z; m.m[15] = d.w;
    return m;
}
__device__ __forceinline__ Mat4 load_mat4(const float *p)
{
    const float4 *q = reinterpret_cast<const float4 *>(p);
    return mat4_rows(q[0], q[1], q[2], q[3]);
}
// the same through a constant-address-space pointer (wave-uniform address: four s_load_dwordx4)
__device__ __forceinline__ Mat4 load_mat4_uniform(const float *p)
{
    return mat4_rows(ld_const_f4(p), ld_const_f4(p + 4), ld_const_f4(p + 8), ld_const_f4(p + 12));
}
__device__ __forceinline__ void store_mat4(float *p, const Mat4 &m)
{
    float4 *q = reinterpret_cast<float4 *>(p);
    q[0] = make_float4(m.m[0], m.m[1], m.m[2], m.m[3]);
    q[1] = make_float4(m.m[4], m.m[5], m.m[6], m.m[7]);
    q[2] = make_float4(m.m[8], m.m[9], m.m[10], m.m[11]);
    q[3] = make_float4(m.m[12], m.m[13], m.m[14], m.m[15]);
}

// The compiler forgets where a pose came from.  A kernel that takes Log and then Exp of its result otherwise shares subexpressions between the two
// (|rot|^2 and what hangs on it) and contracts them into other fused multiply-adds than a kernel that starts from the stored pose: the first
// iterate's T then differed from k_poses_to_matrices' Exp of the stored x by an ulp in all entries of about one frame in seventeen
// (tests/test_gpu_solve_stages.py found it: the assembly of iterate 0, fed the seam's matrices, was 4 x its bar out in that frame's blocks).
// With it, the assembly of iterate 0 meets its bars from btba_matrices_to_poses / btba_poses_to_matrices' (x, T, Tinv) of the same matrices
// (0.03 ... 0.74 of them).  No test compares the bits: the first T is not in the trace record, and how two kernels contract the same
// expressions is the compiler's choice.
__device__ __forceinline__ void se3_opaque(float (&rot)[3], float (&trans)[3])
{
    asm volatile("" : "+v"(rot[0]), "+v"(rot[1]), "+v"(rot[2]), "+v"(trans[0]), "+v"(trans[1]), "+v"(trans[2]));
}

// ---- prepare: Log of the input matrices, then Exp and inverse (SBA.cu:71-79, SolverBundling.cu:890-897)
// keep_T (developer / experiment builds only, tests/tools/reference_order_experiment.py): the incoming matrix IS the first iterate's T -- no Exp(Log(.)) through
// the device's libm in between --, so that an experiment can start this path and the oracle from bit-identical matrices
__global__ void __launch_bounds__(64) k_prepare(int total, const float *__restrict__ poses, float *__restrict__ x, float *__restrict__ T, float *__restrict__ Tinv, int keep_T = 0)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const Mat4 M = load_mat4(poses + 16 * (size_t)idx);
    float rot[3], trans[3];
    matrix_to_pose(M, rot, trans);
    if (x) { float *o = x + 6 * (size_t)idx; o[0] = rot[0]; o[1] = rot[1]; o[2] = rot[2]; o[3] = trans[0]; o[4] = trans[1]; o[5] = trans[2]; }
    if (T || Tinv) {
        se3_opaque(rot, trans);
        Mat4 E = pose_to_matrix(rot, trans);
#if defined(BTBA_DEV_EXPERIMENTS) || defined(BTBA_REFERENCE_ORDER)
        if (keep_T) E = M;
#endif
        if (T) store_mat4(T + 16 * (size_t)idx, E);
        if (Tinv) store_mat4(Tinv + 16 * (size_t)idx, mat_inverse(E));
    }
}

__global__ void __launch_bounds__(64) k_poses_to_matrices(int total, const float *__restrict__ x, float *__restrict__ T, float *__restrict__ Tinv)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const float *o = x + 6 * (size_t)idx;
    const float rot[3] = { o[0], o[1], o[2] }, trans[3] = { o[3], o[4], o[5] };
    const Mat4 E = pose_to_matrix(rot, trans);
    if (T) store_mat4(T + 16 * (size_t)idx, E);
    if (Tinv) store_mat4(Tinv + 16 * (size_t)idx, mat_inverse(E));
}

// ---- frame cache (A3): CUDACache::storeFrame as ONE launch for all frames --------------------
// grid (ceil(npix/256), n_frames).  Reads only the full-res pixels the nearest-neighbour
// resample picks (CUDAImageUtil.cu:57-61) instead of converting the whole 640x480 image first.
__global__ void __launch_bounds__(kBlock) k_build_cache(int W, int H, int Wd, int Hd, Mat4 Kinv,
                                                       const float *const *__restrict__ depth, const float *const *__restrict__ normals,
                                                       float4 *__restrict__ campos_out, float4 *__restrict__ normals_out, int *__restrict__ n_valid)
{
#pragma clang fp contract(off)   // plain IEEE mul/add: the cache is bit-identical to the CPU oracle's
    const int f = blockIdx.y;
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    const int npix = Wd * Hd;
    int valid = 0;
    if (o < npix) {
        const int x = o % Wd, y = o / Wd;
        const float scaleW = (float)(W - 1) / (float)(Wd - 1);
        const float scaleH = (float)(H - 1) / (float)(Hd - 1);
        const unsigned xi = (unsigned)(x * scaleW + 0.5f);
        const unsigned yi = (unsigned)(y * scaleH + 0.5f);
        if (xi < (unsigned)W && yi < (unsigned)H) {
            const size_t s = (size_t)yi * W + xi;
            const float d = depth[f][s];
            float4 cp = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((double)d >= 0.1) {
                // intrinsicsInv * (x d, y d, d, d); output (x, y, w, 1)  (CUDAImageUtil.cu:310-327)
                const float vx = (float)xi * d, vy = (float)yi * d;
                cp.x = Kinv.m[0] * vx + Kinv.m[1] * vy + Kinv.m[2] * d + Kinv.m[3] * d;
                cp.y = Kinv.m[4] * vx + Kinv.m[5] * vy + Kinv.m[6] * d + Kinv.m[7] * d;
                cp.z = Kinv.m[12] * vx + Kinv.m[13] * vy + Kinv.m[14] * d + Kinv.m[15] * d;
                cp.w = 1.0f;
                valid = 1;
            }
            campos_out[(size_t)f * npix + o] = cp;
            normals_out[(size_t)f * npix + o] = reinterpret_cast<const float4 *>(normals[f])[s];
        }
    }
    if (n_valid) {
        const unsigned long long b = __ballot(valid);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&n_valid[f], __popcll(b));
    }
}

// ---- compact frame cache ("ZN": float4 = depth z, normal x, y, z; 16 B per pixel instead of 32) -----------
// camPos is a pure function of (full-res pixel, depth): CUDAImageUtil.cu:310-327 computes
// intrinsicsInv * (x d, y d, d, d).  Storing only d and re-evaluating that expression with the SAME fp32
// operations (no contraction) where it is consumed gives bit-identical camera-space points while halving the
// bytes and the load instructions of the dense sweep (one 16-byte load per tap instead of two).
// Camera-space point of a cached pixel from its depth.  General intrinsics: the cache builder's arithmetic, term by
// term (cx, cy = (float) full-resolution column / row of the cached pixel).  (Zero skew and an affine last row -- every
// pinhole K -- take dense_block_pinhole instead: x = K^-1[0][0] (xi d) + K^-1[0][2] d = d (K^-1[0][0] xi + K^-1[0][2]) with the
// bracket tabulated per column / row, pinhole_lut_entry: three multiplies per point instead of nine operations; differs from the
// builder's rounding sequence by at most 1 ulp per coordinate.)
__device__ __forceinline__ float3 zn_backproject(const float *ki, float cx, float cy, float d)
{
#pragma clang fp contract(off)
    // (double)d >= 0.1  <=>  d >= 0.1f  (0.1f is the smallest float above 0.1); below it the reference stores zeros,
    // and with d := 0 every product below is an exact zero as well, so one select replaces three.
    d = (d >= 0.1f) ? d : 0.0f;
    const float vx = cx * d, vy = cy * d;
    return make_float3(ki[0] * vx + ki[1] * vy + ki[2] * d + ki[3] * d, ki[4] * vx + ki[5] * vy + ki[6] * d + ki[7] * d,
                       ki[12] * vx + ki[13] * vy + ki[14] * d + ki[15] * d);
}
__device__ __forceinline__ unsigned zn_src_coord(int c, float scale)
{
#pragma clang fp contract(off)
    return (unsigned)(c * scale + 0.5f);          // CUDAImageUtil.cu:60-61
}

// grid (ceil(npix/256), n_frames): CUDACache::storeFrame for all frames, compact output.
__global__ void __launch_bounds__(kBlock) k_build_cache_zn(int W, int H, int Wd, int Hd, const float *const *__restrict__ depth, const float *const *__restrict__ normals,
                                                          float4 *__restrict__ zn_out, int *__restrict__ n_valid, const int *__restrict__ out_slot)
{
#pragma clang fp contract(off)
    const int f = blockIdx.y;
    const int fo = out_slot ? out_slot[f] : f;        // where frame f is stored (persistent cache: a pool slot)
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    const int npix = Wd * Hd;
    int valid = 0;
    if (o < npix) {
        const int x = o % Wd, y = o / Wd;
        const float scaleW = (float)(W - 1) / (float)(Wd - 1);
        const float scaleH = (float)(H - 1) / (float)(Hd - 1);
        const unsigned xi = (unsigned)(x * scaleW + 0.5f);
        const unsigned yi = (unsigned)(y * scaleH + 0.5f);
        if (xi < (unsigned)W && yi < (unsigned)H) {
            const size_t s = (size_t)yi * W + xi;
            const float d = depth[f][s];
            const float4 nr = reinterpret_cast<const float4 *>(normals[f])[s];
            valid = ((double)d >= 0.1) ? 1 : 0;
            // GATED depth: 0 where the reference's camPos is (0, 0, 0, 0) (CUDAImageUtil.cu:310-327: d < 0.1, and NaN fails the
            // comparison too), so that the sweep blends exactly what the reference blends without re-testing every tap
            zn_out[(size_t)fo * npix + o] = make_float4(valid ? d : 0.0f, nr.x, nr.y, nr.z);
        }
    }
    if (n_valid) {
        const unsigned long long b = __ballot(valid);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(&n_valid[fo], __popcll(b));
    }
}

// float4 camPos + float4 normal caches -> compact cache (for callers that already hold the reference layout;
// camPos.xy are dropped and later recomputed from z, so the input must come from the standard formula)
__global__ void __launch_bounds__(kBlock) k_pack_zn(size_t total, const float4 *__restrict__ campos, const float4 *__restrict__ normals, float4 *__restrict__ zn)
{
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= total) return;
    const float4 c = campos[o], nr = normals[o];
    zn[o] = make_float4(c.z, nr.x, nr.y, nr.z);
}

// ---- sparse sweep -----------------------------------------------------------------------------
// grid (sparse_chunks, P, B).  Workgroup (c, p, b) owns slice c of pair p's contiguous correspondence segment, 44 register
// accumulators per lane.  Two device layouts of a correspondence:
//   EntryJ (32 B, the wire format, SIFTImageManager.h:44-59): two coalesced 16-byte loads; the frame indices are checked against the
//            segment's pair on the fly (order_flag) -- what a call that uploads the caller's array runs on;
//   C24    (24 B: pos_i, pos_j; invalid <=> first word 0xFFFFFFFF): the indices are implied by the segment, so device-RESIDENT
//            correspondences (batches, the keyed pool) drop them -- a quarter of the stream that bounds the masked / feature-only launches
//            (k_pack_corr24 converts and checks the order once).  Stored in groups of 64 entries as three planes of float2 --
//            (pos_i.x, pos_i.y)[64], (pos_i.z, pos_j.x)[64], (pos_j.y, pos_j.z)[64] -- so that each of a wave's three 8-byte loads covers 512
//            contiguous bytes: plain 24-byte records, three loads at stride 24, touch every cache line three times and measured SLOWER than
//            EntryJ on the masked launch although they move a quarter less (52.0 vs 49.9 us, gpurun_out/r03_13).
// the loaded words of one correspondence -> (valid, pos_i, pos_j): the one statement of both layouts (the sweep below, the objective report)
struct SparseEntry { bool valid; float pix, piy, piz, pjx, pjy, pjz; };
// EntryJ: q0 = (imgIdx_i, imgIdx_j, pos_i.x, pos_i.y)  q1 = (pos_i.z, pos_j.x, pos_j.y, pos_j.z); invalid <=> imgIdx_i = 0xFFFFFFFF (EntryJ::isValid)
__device__ __forceinline__ SparseEntry sparse_entry_j(const float4 &q0, const float4 &q1) { return SparseEntry{ __float_as_uint(q0.x) != 0xFFFFFFFFu, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w }; }
// C24: the three planes' words of the entry
__device__ __forceinline__ SparseEntry sparse_entry_c24(const float2 &q0, const float2 &q1, const float2 &q2) { return SparseEntry{ __float_as_uint(q0.x) != 0xFFFFFFFFu, q0.x, q0.y, q1.x, q1.y, q2.x, q2.y }; }

template <bool C24, bool NT>
__device__ __forceinline__ void sparse_block_impl(const SolveDims &D, const float4 *__restrict__ corr, const uint32_t *__restrict__ pair_offsets,
                                                  const float *__restrict__ T, float *__restrict__ partials, int chunk, int p, int b, float *red)
{
    const unsigned tid = item_tid();
    int fi, fj;
    pair_from_index(p, D.n_frames, fi, fj);
    const auto off = as_const(pair_offsets + (size_t)b * (D.n_pairs + 1));
    const uint32_t seg0 = off[p];
    const uint32_t len = D.pair_lens ? as_const(D.pair_lens)[(size_t)b * D.n_pairs + p] : off[p + 1] - seg0;       // (pool segments are not back to back)
    const uint32_t per = (len + D.sparse_chunks - 1) / D.sparse_chunks;
    const uint32_t lo = seg0 + min(len, per * chunk), hi = seg0 + min(len, per * (chunk + 1));
    const float *Tb = T + (unsigned)b * (unsigned)D.pose_stride;
    const Mat4 Ti = load_mat4_uniform(Tb + 16 * fi);
    const Mat4 Tj = load_mat4_uniform(Tb + 16 * fj);
    float acc[kSparseVals];
#pragma unroll
    for (int k = 0; k < kSparseVals; k++) acc[k] = 0.0f;

    const float delta2 = D.robust_delta * D.robust_delta;
    int n_valid = 0;                                  // valid entries of this WAVE (scalar register); joins the record as acc[0] behind the loop
    // One correspondence.  all_valid (wave-uniform): every entry of the wave's trip is valid -- in real windows almost every trip -- and nothing is masked.
    // Otherwise an invalid / out-of-range slot contributes exact zeros (its payload may be anything, even NaN) through the selects in the two blocks behind
    // wave-uniform branches; with every entry valid those selects return their first operand, so both ways are the same arithmetic and the same bits.
    // (The empty asm keeps each block a branch: speculated, its selects would run on every trip again.)
    auto accumulate = [&](const bool all_valid, bool valid, const SparseEntry &E) {
        float wix, wiy, wiz, wjx, wjy, wjz;
        xform_point(Ti, E.pix, E.piy, E.piz, wix, wiy, wiz);
        xform_point(Tj, E.pjx, E.pjy, E.pjz, wjx, wjy, wjz);
        if (!all_valid) {
            asm volatile("");
            wix = valid ? wix : 0.0f; wiy = valid ? wiy : 0.0f; wiz = valid ? wiz : 0.0f;
            wjx = valid ? wjx : 0.0f; wjy = valid ? wjy : 0.0f; wjz = valid ? wjz : 0.0f;
        }
        const float rx = wix - wjx, ry = wiy - wjy, rz = wiz - wjz;
        const float e2 = rx * rx + ry * ry + rz * rz;
#ifdef BTBA_EXACT_DIV
        float rho = (e2 <= delta2) ? 1.0f : D.robust_delta / sqrtf(e2);
#else
        float rho = (e2 <= delta2) ? 1.0f : D.robust_delta * __builtin_amdgcn_rsqf(e2);
#endif
        if (!all_valid) {
            asm volatile("");
            rho = valid ? rho : 0.0f;                 // (a masked slot has e2 = 0: rho was 1)
        }
        acc[1] += wix; acc[2] += wiy; acc[3] += wiz;
        acc[4] += wjx; acc[5] += wjy; acc[6] += wjz;
        acc[7] += wix * wix; acc[8] += wix * wiy; acc[9] += wix * wiz; acc[10] += wiy * wiy; acc[11] += wiy * wiz; acc[12] += wiz * wiz;
        acc[13] += wjx * wjx; acc[14] += wjx * wjy; acc[15] += wjx * wjz; acc[16] += wjy * wjy; acc[17] += wjy * wjz; acc[18] += wjz * wjz;
        acc[19] += wix * wjx; acc[20] += wix * wjy; acc[21] += wix * wjz;
        acc[22] += wiy * wjx; acc[23] += wiy * wjy; acc[24] += wiy * wjz;
        acc[25] += wiz * wjx; acc[26] += wiz * wjy; acc[27] += wiz * wjz;
        acc[28] += rho * rx; acc[29] += rho * ry; acc[30] += rho * rz;
        acc[31] += rho * (wiy * rz - wiz * ry); acc[32] += rho * (wiz * rx - wix * rz); acc[33] += rho * (wix * ry - wiy * rx);
        acc[34] += rho * (wjy * rz - wjz * ry); acc[35] += rho * (wjz * rx - wjx * rz); acc[36] += rho * (wjx * ry - wjy * rx);
        acc[37] += rho;
        acc[38] += rho * (wiy * wiy + wiz * wiz); acc[39] += rho * (wix * wix + wiz * wiz); acc[40] += rho * (wix * wix + wiy * wiy);
        acc[41] += rho * (wjy * wjy + wjz * wjz); acc[42] += rho * (wjx * wjx + wjz * wjz); acc[43] += rho * (wjx * wjx + wjy * wjy);
    };
    // One trip's two correspondences.  The count is a popcount of the two valid masks (the ballots of single comparisons, AND-ed in scalar registers).
    auto accumulate_pair = [&](const SparseEntry &A, bool live_b, const SparseEntry &B) {
        const unsigned long long ma = __builtin_amdgcn_ballot_w64(A.valid), mb = __builtin_amdgcn_ballot_w64(live_b) & __builtin_amdgcn_ballot_w64(B.valid);
        n_valid += __popcll(ma) + __popcll(mb);
        const bool all_valid = (ma & mb) == ~0ull;
        accumulate(all_valid, A.valid, A);
        accumulate(all_valid, live_b && B.valid, B);
    };
    // two correspondences per lane per trip (entries e and e + 256: every load instruction of a wave covers consecutive entries), all of
    // their loads in flight together
    if (C24) {
        const float2 *cb = reinterpret_cast<const float2 *>(corr);
        const size_t e_base = (size_t)D.corr_entry0 + (size_t)b * (size_t)D.corr_stride;
        // (three and four entries per lane per trip -- more bytes in flight -- measured slower everywhere: the registers they hold push the
        // fused kernel into spills, gpurun_out/r03_16)
        for (uint32_t e = lo + tid; e < hi; e += 2 * kBlock) {
            const uint32_t e2 = e + kBlock;
            const bool live2 = e2 < hi;
            const float2 *qa = cb + corr24_index(e_base + e), *qb = cb + corr24_index(e_base + (live2 ? e2 : e));
            const float2 a0 = ld_stream_f2<NT>(qa), a1 = ld_stream_f2<NT>(qa + 64), a2 = ld_stream_f2<NT>(qa + 128), b0 = ld_stream_f2<NT>(qb), b1 = ld_stream_f2<NT>(qb + 64), b2 = ld_stream_f2<NT>(qb + 128);
            accumulate_pair(sparse_entry_c24(a0, a1, a2), live2, sparse_entry_c24(b0, b1, b2));
        }
    } else {
        const float4 *cb = corr + 2 * (size_t)b * D.corr_stride;
        bool misplaced = false;                       // an entry whose (imgIdx_i, imgIdx_j) is not this segment's pair
        float2 *const c24 = D.corr24_out;             // (wave-uniform) the re-layout of the first iteration: k_pack_corr24_batch's records, written as the entries pass by
        const size_t e_out = (size_t)D.corr_entry0 + (size_t)b * (size_t)D.corr_stride;
        // the entry's order check and re-layout (its sums: accumulate_pair)
        auto entry = [&](const float4 &q0, const float4 &q1, bool live, uint32_t e) {
            const bool valid = live && sparse_entry_j(q0, q1).valid;
            misplaced |= valid & ((__float_as_uint(q0.x) != (uint32_t)fi) | (__float_as_uint(q0.y) != (uint32_t)fj));
            if (c24 && live) {
                float2 *o = c24 + corr24_index(e_out + e);
                o[0] = make_float2(valid ? q0.z : __uint_as_float(0xFFFFFFFFu), q0.w);
                o[64] = make_float2(q1.x, q1.y);
                o[128] = make_float2(q1.z, q1.w);
            }
        };
        for (uint32_t e = lo + tid; e < hi; e += 2 * kBlock) {
            const uint32_t e2 = e + kBlock;
            const bool live2 = e2 < hi;
            const uint32_t e2c = live2 ? e2 : e;
            const float4 a0 = ld_stream_f4<NT>(cb + 2 * (size_t)e), a1 = ld_stream_f4<NT>(cb + 2 * (size_t)e + 1), b0 = ld_stream_f4<NT>(cb + 2 * (size_t)e2c), b1 = ld_stream_f4<NT>(cb + 2 * (size_t)e2c + 1);
            entry(a0, a1, true, e);
            entry(b0, b1, live2, e2c);
            accumulate_pair(sparse_entry_j(a0, a1), live2, sparse_entry_j(b0, b1));
        }
        if (D.order_flag && misplaced) atomicOr(D.order_flag, 1);
    }
    acc[0] = (tid & 63u) == 0u ? (float)n_valid : 0.0f;         // an integer far below 2^24: the float the per-lane counts summed to
    float *out = partials + ((unsigned)b * D.sp_stride + (unsigned)(D.atomic_sums ? p : p * D.sparse_chunks + chunk) * (unsigned)kSparseVals);
    block_reduce_store<kSparseVals, 4>(acc, red, out, D.atomic_sums ? 1 : 0);
}
__device__ __forceinline__ void sparse_block(const SolveDims &D, const float4 *__restrict__ corr, const uint32_t *__restrict__ pair_offsets,
                                             const float *__restrict__ T, float *__restrict__ partials, int chunk, int p, int b, float *red)
{
    // (four instances of one loop; the choice is uniform over the workgroup)
    if (D.corr24) { if (b >= D.corr_nt_from) sparse_block_impl<true, true>(D, corr, pair_offsets, T, partials, chunk, p, b, red); else sparse_block_impl<true, false>(D, corr, pair_offsets, T, partials, chunk, p, b, red); }
    else { if (b >= D.corr_nt_from) sparse_block_impl<false, true>(D, corr, pair_offsets, T, partials, chunk, p, b, red); else sparse_block_impl<false, false>(D, corr, pair_offsets, T, partials, chunk, p, b, red); }
}

// EntryJ segments -> 24-byte correspondences, in place in the entry index space (entry e of the input is entry e of the output).
// grid (ceil(longest segment / 256), n_segments); seg[s] = (source offset, destination offset, length, i << 16 | j), offsets in entries.
// A valid entry that does not carry (i, j) raises the order flag (the array was not pair-major: the caller falls back to bucketing).
__global__ void __launch_bounds__(256) k_pack_corr24(const uint4 *__restrict__ seg, const uint4 *__restrict__ src, float2 *__restrict__ dst, int *__restrict__ order_flag)
{
    const uint4 d = seg[blockIdx.y];
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= d.z) return;
    const uint4 a = src[2 * (size_t)(d.x + e)], b = src[2 * (size_t)(d.x + e) + 1];
    const bool valid = a.x != 0xFFFFFFFFu;
    if (valid && ((a.x != (d.w >> 16)) | (a.y != (d.w & 0xFFFFu)))) atomicOr(order_flag, 1);
    float2 *o = dst + corr24_index((size_t)(d.y + e));
    o[0] = make_float2(valid ? __uint_as_float(a.z) : __uint_as_float(0xFFFFFFFFu), __uint_as_float(a.w));
    o[64] = make_float2(__uint_as_float(b.x), __uint_as_float(b.y));
    o[128] = make_float2(__uint_as_float(b.z), __uint_as_float(b.w));
}
// the same for a batch of pair-major instances described by their offset tables: grid (ceil(longest segment / 256), P, B)
__global__ void __launch_bounds__(256) k_pack_corr24_batch(int n_frames, int n_pairs, int64_t corr_stride, const uint32_t *__restrict__ pair_offsets,
                                                          const uint4 *__restrict__ src, float2 *__restrict__ dst, int *__restrict__ order_flag)
{
    const int p = blockIdx.y, b = blockIdx.z;
    const uint32_t *off = pair_offsets + (size_t)b * (n_pairs + 1);
    const uint32_t seg0 = off[p], len = off[p + 1] - seg0, e = blockIdx.x * 256u + threadIdx.x;
    if (e >= len) return;
    int fi, fj;
    pair_from_index(p, n_frames, fi, fj);
    const size_t at = (size_t)b * (size_t)corr_stride + seg0 + e;
    const uint4 a = src[2 * at], q = src[2 * at + 1];
    const bool valid = a.x != 0xFFFFFFFFu;
    if (order_flag && valid && ((a.x != (uint32_t)fi) | (a.y != (uint32_t)fj))) atomicOr(order_flag, 1);
    float2 *o = dst + corr24_index(at);
    o[0] = make_float2(valid ? __uint_as_float(a.z) : __uint_as_float(0xFFFFFFFFu), __uint_as_float(a.w));
    o[64] = make_float2(__uint_as_float(q.x), __uint_as_float(q.y));
    o[128] = make_float2(__uint_as_float(q.z), __uint_as_float(q.w));
}

// grid (sparse_chunks, P, B).  Workgroup (c, p, b) owns slice c of pair p's contiguous EntryJ segment.
__global__ void __launch_bounds__(kBlock) k_sparse_sweep(SolveDims D, const float4 *__restrict__ corr, const uint32_t *__restrict__ pair_offsets,
                                                        const float *__restrict__ T, float *__restrict__ partials)
{
    __shared__ float red[kRedFloats];
    sparse_block(D, corr, pair_offsets, T, partials, blockIdx.x, blockIdx.y, blockIdx.z, red);
}

// ---- dense sweep ------------------------------------------------------------------------------
// The reference is built with nvcc -use_fast_math (CMakeLists.txt:7): its divisions, sqrt and rsqrt are the
// approximate hardware forms.  v_rcp_f32 / v_rsq_f32 (1 ulp) are the CDNA counterparts; an IEEE division
// costs ~10 VALU instructions and this kernel had ~25 of them per pixel.
// -DBTBA_EXACT_DIV (an EXPERIMENT build, tests/tools/exact_div_experiment.py -- never the product): IEEE division and square root instead, to measure
// how much of the difference between this path's accept decisions and the oracle's the 1-ulp forms explain (profiles/r04/exact_div_experiment.json).
#ifdef BTBA_EXACT_DIV
__device__ __forceinline__ float fast_rcp(float x) { return 1.0f / x; }
__device__ __forceinline__ float fast_rsq(float x) { return 1.0f / sqrtf(x); }
#else
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fast_rsq(float x) { return __builtin_amdgcn_rsqf(x); }
#endif

// XCD-aware remap of a 1-D grid: the dispatcher places block L on XCD L % 8 (observed, used for speed only),
// so logical work item L' = (contiguous range per XCD) keeps one instance's frames in ONE XCD's L2 instead of
// replicating them into all eight.
__device__ __forceinline__ unsigned xcd_remap(unsigned L, unsigned n)
{
    const unsigned q = n >> 3, r = n & 7u, xcd = L & 7u, slot = L >> 3;
    return xcd < r ? xcd * (q + 1) + slot : r * (q + 1) + (xcd - r) * q + slot;
}

// ---- per-pixel work of the dense sweep, branch-free so that all ten loads of a pixel are independent and
// in flight together.  The kernel is VALU-bound (PMC: VALU pipe ~87 % busy at 283 instructions per pixel),
// so the per-pixel arithmetic is kept minimal:
//   * the Jacobian row is accumulated in the TARGET CAMERA frame, a' = [-n_i ; n_i x q]; the model-frame row
//     of the reference is a = M a' with the constant per-pair 6x6  M = [[R_i, 0], [[t_i]x R_i, R_i]]
//     (n_w = R_i n_i, w = R_i q + t_i  =>  n_w x w = R_i (n_i x q) + [t_i]x R_i (-n_i)), so
//     S = M S' M^T and g = M g' are applied once per pair in k_system_solve instead of 18 FMAs per pixel;
//   * one set of bilinear tap coefficients serves camPos and normals (same taps, same in-image tests);
//   * the -inf sentinel tests of ICPUtil.h:96-102 are dropped: the cache never contains -inf (invalid data is
//     zeros and is blended in -- SURVEY.md appendix A.4 step 4; the reference notes the test never fires);
//   * the w lanes are not fetched: camPos.w is never used and normal.w is 0 by the wire format (Frame.h:75).
struct DenseCtx {
    Mat4 Tij;
    const float4 *cam_t, *nrm_t;
    float fx, fy, cx, cy, depth_min, depth_max, normal_thresh, dist2_thresh, delta, delta2, w_dense;
    int W, H;
};

struct PixelGeom {                  // stage 1: everything that does not need the target taps
    float qx, qy, qz, nqx, nqy, nqz;
    float c00, c10, c01, c11;       // final bilinear coefficients (row/column renormalisation folded in)
    int i00, i10, i01, i11;
    int xa, xb, ya, yb;             // clamped tap columns / rows (compact cache: needed to back-project the taps)
    bool valid;
};

__device__ __forceinline__ PixelGeom pixel_geom(const DenseCtx &C, const float4 &cs, const float4 &ns)
{
    PixelGeom g;
    g.valid = (cs.z > C.depth_min && cs.z < C.depth_max);
    const Mat4 &M = C.Tij;
    g.nqx = M.m[0] * ns.x + M.m[1] * ns.y + M.m[2] * ns.z;
    g.nqy = M.m[4] * ns.x + M.m[5] * ns.y + M.m[6] * ns.z;
    g.nqz = M.m[8] * ns.x + M.m[9] * ns.y + M.m[10] * ns.z;
    xform_point(M, cs.x, cs.y, cs.z, g.qx, g.qy, g.qz);
    const float rqz = fast_rcp(g.qz);
    float u = g.qx * C.fx * rqz + C.cx, v = g.qy * C.fy * rqz + C.cy;
    // in-image test of the rounded coordinates (SolverBundlingDenseUtil.h:91-94) without rounding them:
    // 0 <= (int)roundf(u) < W  <=>  -0.5 < u < W - 0.5  (round half away from zero; W - 0.5 is exact in fp32).
    // NaN / inf coordinates of rejected pixels fail the comparisons, so nothing non-finite reaches the int conversions.
    g.valid = g.valid && (u > -0.5f) && (u < (float)C.W - 0.5f) && (v > -0.5f) && (v < (float)C.H - 0.5f);
    u = g.valid ? u : 0.0f; v = g.valid ? v : 0.0f;
    // bilinear taps (ICPUtil.h:83-110): out-of-image taps get weight 0, weights renormalised per row, then per column
    const float fx0 = floorf(u), fy0 = floorf(v);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float alpha = u - fx0, beta = v - fy0;
    const bool okx0 = (unsigned)x0 < (unsigned)C.W, okx1 = (unsigned)(x0 + 1) < (unsigned)C.W;
    const bool oky0 = (unsigned)y0 < (unsigned)C.H, oky1 = (unsigned)(y0 + 1) < (unsigned)C.H;
    const int xa = min(max(x0, 0), C.W - 1), xb = min(max(x0 + 1, 0), C.W - 1);
    const int ya = min(max(y0, 0), C.H - 1), yb = min(max(y0 + 1, 0), C.H - 1);
    g.i00 = ya * C.W + xa; g.i10 = ya * C.W + xb; g.i01 = yb * C.W + xa; g.i11 = yb * C.W + xb;
    g.xa = xa; g.xb = xb; g.ya = ya; g.yb = yb;
    const float a0 = okx0 ? 1.0f - alpha : 0.0f, a1 = okx1 ? alpha : 0.0f;
    const float wr = a0 + a1;                                   // same for both rows
    const float b0 = (oky0 && wr > 0.0f) ? 1.0f - beta : 0.0f, b1 = (oky1 && wr > 0.0f) ? beta : 0.0f;
    const float ww = b0 + b1;
    const float k = (ww > 0.0f) ? fast_rcp(wr) * fast_rcp(ww) : 0.0f;
    const float k0 = k * b0, k1 = k * b1;
    g.c00 = k0 * a0; g.c10 = k0 * a1; g.c01 = k1 * a0; g.c11 = k1 * a1;
    return g;
}

// stage 2: blend of the target taps, the gates and the residual.  ok contains g.valid; nothing here is masked yet.
struct PixelBlend { float nix, niy, niz, dx, dy, dz, res; bool ok; };
__device__ __forceinline__ PixelBlend pixel_blend(const DenseCtx &C, const PixelGeom &g, const float4 &c00, const float4 &c10, const float4 &c01, const float4 &c11,
                                                  const float4 &n00, const float4 &n10, const float4 &n01, const float4 &n11)
{
    PixelBlend B;
    const float cix = g.c00 * c00.x + g.c10 * c10.x + g.c01 * c01.x + g.c11 * c11.x;
    const float ciy = g.c00 * c00.y + g.c10 * c10.y + g.c01 * c01.y + g.c11 * c11.y;
    const float ciz = g.c00 * c00.z + g.c10 * c10.z + g.c01 * c01.z + g.c11 * c11.z;
    B.nix = g.c00 * n00.x + g.c10 * n10.x + g.c01 * n01.x + g.c11 * n11.x;
    B.niy = g.c00 * n00.y + g.c10 * n10.y + g.c01 * n01.y + g.c11 * n11.y;
    B.niz = g.c00 * n00.z + g.c10 * n10.z + g.c01 * n01.z + g.c11 * n11.z;
    B.dx = g.qx - cix; B.dy = g.qy - ciy; B.dz = g.qz - ciz;
    const float dist2 = B.dx * B.dx + B.dy * B.dy + B.dz * B.dz;
    const float dn = g.nqx * B.nix + g.nqy * B.niy + g.nqz * B.niz;
    // `&`, not `&&`: short-circuit evaluation turns into nested exec-mask branches with a block of zeroing moves on each
    B.ok = g.valid & (ciz > C.depth_min) & (ciz < C.depth_max) & (dn >= C.normal_thresh) & (dist2 <= C.dist2_thresh);
    B.res = -(B.dx * B.nix + B.dy * B.niy + B.dz * B.niz);
    return B;
}
// stage 3: the pixel's row, weight and residual into the lane's sums
__device__ __forceinline__ void pixel_sums(const DenseCtx &C, const PixelGeom &g, const PixelBlend &B, float (&acc)[kDenseVals])
{
    // rejected pixels contribute exact zeros.  Bit masks, not `ok ? x : 0`: the compiler turns a run of such selects into
    // an exec-mask branch with a block of zeroing moves on the other path; AND-ing with 0 / ~0 stays straight-line and is
    // NaN-safe (0 * NaN would poison the sums if a target normal were not finite; q is finite whenever the poses are)
    const unsigned keep = B.ok ? 0xFFFFFFFFu : 0u;
    auto masked = [keep](float x) { return __uint_as_float(__float_as_uint(x) & keep); };
    const float res = masked(B.res);
    const float e = res * res;
    const float wgt = masked(C.w_dense * ((e <= C.delta2) ? 1.0f : C.delta * fast_rsq(e)));
    // camera-frame row a' = [-n_i ; n_i x q]
    const float mx = masked(B.nix), my = masked(B.niy), mz = masked(B.niz);
    const float a[6] = { -mx, -my, -mz, my * g.qz - mz * g.qy, mz * g.qx - mx * g.qz, mx * g.qy - my * g.qx };
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; r++) {
        const float wa = wgt * a[r];
#pragma unroll
        for (int c = r; c < 6; c++) acc[k++] += wa * a[c];
        acc[21 + r] += wa * res;
    }
    acc[27] += masked(1.0f);
}

__device__ __forceinline__ void pixel_accumulate(const DenseCtx &C, const PixelGeom &g, const float4 &c00, const float4 &c10, const float4 &c01, const float4 &c11,
                                                 const float4 &n00, const float4 &n10, const float4 &n01, const float4 &n11, float (&acc)[kDenseVals])
{ pixel_sums(C, g, pixel_blend(C, g, c00, c10, c01, c11, n00, n10, n01, n11), acc); }

#ifdef BTBA_REFERENCE_ORDER
// ---- TEST-ONLY build (-DBTBA_REFERENCE_ORDER, never the product; speed irrelevant): one pixel of the dense term evaluated in the REFERENCE's order --
// findDenseCorr (SolverBundlingDenseUtil.h:78-110): float4x4 * float3 / float4 as cuda_SimpleMatrixUtil.h:923-942 multiplies them, cameraToDepth with a
// division, the in-image test on the ROUNDED coordinates, bilinearInterpolationFloat4 (ICPUtil.h:83-110) with its weights renormalised per row and
// then per column, the distance as a square root against the threshold -- fused multiply-add contraction off, IEEE division and square root.  It is the
// oracle's find_dense_corr (oracle/btba_oracle.c) statement by statement.  What it is for: round 4's verdict asked whether the ORDER of the per-pixel
// arithmetic is what makes this path's accept decisions differ from the oracle's on identical inputs; with this pixel they must not differ at all
// (profiles/r05/reference_order_experiment.json).
__device__ __attribute__((noinline)) bool bilinear4_reference(float x, float y, const float4 *__restrict__ img, int W, int H, float out[4])
{
#pragma clang fp contract(off)
    const int p00x = (int)floorf(x), p00y = (int)floorf(y);
    const int p01x = p00x, p01y = p00y + 1, p10x = p00x + 1, p10y = p00y, p11x = p00x + 1, p11y = p00y + 1;
    const float alpha = x - (float)p00x, beta = y - (float)p00y;
    const float MINF = -INFINITY;
    float s0[4] = { 0.f, 0.f, 0.f, 0.f }, w0 = 0.0f;
    if ((unsigned)p00x < (unsigned)W && (unsigned)p00y < (unsigned)H) { const float4 q = img[(size_t)p00y * W + p00x]; const float v[4] = { q.x, q.y, q.z, q.w }; if (v[0] != MINF) { for (int k = 0; k < 4; k++) s0[k] += (1.0f - alpha) * v[k]; w0 += (1.0f - alpha); } }
    if ((unsigned)p10x < (unsigned)W && (unsigned)p10y < (unsigned)H) { const float4 q = img[(size_t)p10y * W + p10x]; const float v[4] = { q.x, q.y, q.z, q.w }; if (v[0] != MINF) { for (int k = 0; k < 4; k++) s0[k] += alpha * v[k]; w0 += alpha; } }
    float s1[4] = { 0.f, 0.f, 0.f, 0.f }, w1 = 0.0f;
    if ((unsigned)p01x < (unsigned)W && (unsigned)p01y < (unsigned)H) { const float4 q = img[(size_t)p01y * W + p01x]; const float v[4] = { q.x, q.y, q.z, q.w }; if (v[0] != MINF) { for (int k = 0; k < 4; k++) s1[k] += (1.0f - alpha) * v[k]; w1 += (1.0f - alpha); } }
    if ((unsigned)p11x < (unsigned)W && (unsigned)p11y < (unsigned)H) { const float4 q = img[(size_t)p11y * W + p11x]; const float v[4] = { q.x, q.y, q.z, q.w }; if (v[0] != MINF) { for (int k = 0; k < 4; k++) s1[k] += alpha * v[k]; w1 += alpha; } }
    float ss[4] = { 0.f, 0.f, 0.f, 0.f }, ww = 0.0f;
    if (w0 > 0.0f) { for (int k = 0; k < 4; k++) ss[k] += (1.0f - beta) * (s0[k] / w0); ww += (1.0f - beta); }
    if (w1 > 0.0f) { for (int k = 0; k < 4; k++) ss[k] += beta * (s1[k] / w1); ww += beta; }
    if (ww > 0.0f) { for (int k = 0; k < 4; k++) out[k] = ss[k] / ww; return true; }
    out[0] = out[1] = out[2] = out[3] = MINF;
    return false;
}

__device__ __attribute__((noinline)) void pixel_reference_order(const DenseCtx &C, float dist_thresh, const float4 &cs, const float4 &ns, float (&acc)[kDenseVals])
{
#pragma clang fp contract(off)
    const float *T = C.Tij.m;
    bool ok = (cs.z > C.depth_min && cs.z < C.depth_max) && (ns.x != -INFINITY);
    float q[3] = { 0.f, 0.f, 0.f }, ci[4] = { 0.f, 0.f, 0.f, 0.f }, ni[4] = { 0.f, 0.f, 0.f, 0.f };
    if (ok) {
        const float nt[4] = { T[0] * ns.x + T[1] * ns.y + T[2] * ns.z + T[3] * ns.w, T[4] * ns.x + T[5] * ns.y + T[6] * ns.z + T[7] * ns.w,
                              T[8] * ns.x + T[9] * ns.y + T[10] * ns.z + T[11] * ns.w, T[12] * ns.x + T[13] * ns.y + T[14] * ns.z + T[15] * ns.w };
        q[0] = T[0] * cs.x + T[1] * cs.y + T[2] * cs.z + T[3] * 1.0f;
        q[1] = T[4] * cs.x + T[5] * cs.y + T[6] * cs.z + T[7] * 1.0f;
        q[2] = T[8] * cs.x + T[9] * cs.y + T[10] * cs.z + T[11] * 1.0f;
        const float u = q[0] * C.fx / q[2] + C.cx, v = q[1] * C.fy / q[2] + C.cy;      // cameraToDepth, CUDACameraUtil.h:9-14
        const int sx = (int)roundf(u), sy = (int)roundf(v);
        ok = sx >= 0 && sy >= 0 && sx < C.W && sy < C.H;
        if (ok) {
            bilinear4_reference(u, v, C.cam_t, C.W, C.H, ci);
            ok = ci[2] > C.depth_min && ci[2] < C.depth_max;
        }
        if (ok) {
            bilinear4_reference(u, v, C.nrm_t, C.W, C.H, ni);
            ok = ni[0] != -INFINITY;
        }
        if (ok) {
            const float d[3] = { q[0] - ci[0], q[1] - ci[1], q[2] - ci[2] };
            const float dist = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            const float dNormal = nt[0] * ni[0] + nt[1] * ni[1] + nt[2] * ni[2] + nt[3] * ni[3];
            ok = dNormal >= C.normal_thresh && dist <= dist_thresh;
        }
    }
    if (!ok) return;
    // the accepted pixel's contribution: the product's row and residual (pixel_accumulate) from these points
    const float dx = q[0] - ci[0], dy = q[1] - ci[1], dz = q[2] - ci[2];
    const float res = -(dx * ni[0] + dy * ni[1] + dz * ni[2]);
    const float e = res * res;
    const float wgt = C.w_dense * ((e <= C.delta2) ? 1.0f : C.delta / sqrtf(e));
    const float a[6] = { -ni[0], -ni[1], -ni[2], ni[1] * q[2] - ni[2] * q[1], ni[2] * q[0] - ni[0] * q[2], ni[0] * q[1] - ni[1] * q[0] };
    int k = 0;
    for (int r = 0; r < 6; r++) {
        const float wa = wgt * a[r];
        for (int c = r; c < 6; c++) acc[k++] += wa * a[c];
        acc[21 + r] += wa * res;
    }
    acc[27] += 1.0f;
}
#endif

// index of (r, c), r <= c, in the 21-entry upper-triangle row-major packing of a symmetric 6x6
__device__ __forceinline__ int tri21(int r, int c) { if (r > c) { const int t = r; r = c; c = t; } return r * 6 - r * (r - 1) / 2 + (c - r); }

// Epilogue of a dense workgroup: fixed-order reduction of the 28 per-lane sums over the workgroup, then the camera-frame ->
// model-frame congruence S = M S' M^T, g = M g' with M = [[R_i, 0], [[t_i]x R_i, R_i]] of the TARGET frame's pose of this iterate
// (see pixel_accumulate), then one 112-byte record per workgroup.  The congruence is linear, so applying it per tile and summing
// the tiles in k_system_solve equals applying it to the sum; doing it here (27 lanes, ~40 FMAs each, once per workgroup) takes it
// off the single-workgroup critical path of k_system_solve (it was 8.4 k of its 55 k cycles).
// M of the congruence (6 x 6, from the target frame's pose), staged in LDS by 36 threads at the START of a dense workgroup: its global
// loads are then off the tail of the workgroup (the epilogue used to wait a memory round trip for them)
// In two halves -- the entry of thread `tid` from the pose, and its store -- so that an item can issue the load with its other prologue loads and store
// behind whatever it does meanwhile (dense_block_pinhole: the table fill); dense_block and dense_block_zn call them back to back.
__device__ __forceinline__ float dense_M_load(unsigned tid, const float *__restrict__ T_target)
{
    float v = 0.0f;
    if (tid >= 64 && tid < 64 + 36) {
        const int e = (int)tid - 64, r = e / 6, c = e % 6;
        if (r < 3) v = (c < 3) ? T_target[4 * r + c] : 0.0f;
        else {
            const int q = r - 3, qa = (q + 1) % 3, qb = (q + 2) % 3;     // ([t]x R)[q][c] = t[qa] R[qb][c] - t[qb] R[qa][c]
            v = (c < 3) ? T_target[4 * qa + 3] * T_target[4 * qb + c] - T_target[4 * qb + 3] * T_target[4 * qa + c] : T_target[4 * q + (c - 3)];
        }
    }
    return v;
}
__device__ __forceinline__ void dense_M_store(unsigned tid, float *red, float v)
{
    if (tid >= 64 && tid < 64 + 36) red[4 * kDenseVals + kDenseVals + 4 + ((int)tid - 64)] = v;
}

// FLIPPED: the sums were accumulated with a+ = D a, res+ = -res (dense_block_pinhole): S = D S+ D negates the nine entries that couple a
// translation row with a rotation row, g = -D g+ negates the three rotation entries -- exact.
// mode: 0 store the record, 1 add it to the record with float atomics (BTBA_REDUCE_ATOMIC)
__device__ __forceinline__ void store_sum(float *p, float v, int mode)
{
    if (mode == 1) unsafeAtomicAdd(p, v);
    else *p = v;
}
template <bool FLIPPED = false>
__device__ __forceinline__ void dense_epilogue(float (&acc)[kDenseVals], float *red, float *out, int mode = 0)
{
    const unsigned tid = item_tid();
    wave_fold_store<kDenseVals>(acc, red + (tid >> 6) * kDenseVals);
    __syncthreads();
    float *Sp = red + 4 * kDenseVals;                    // the workgroup's camera-frame sums (28) ...
    float *Mt = Sp + kDenseVals + 4;                     // ... and M (36)
    if (tid < kDenseVals) {
        float s = red[tid];
#pragma unroll
        for (int w = 1; w < 4; w++) s += red[w * kDenseVals + tid];
        if (FLIPPED) {
            // upper-triangle packing (tri21): row r < 3 holds columns r .. 5 from r * 6 - r (r - 1) / 2 on; its columns 3 .. 5 are the mixed entries
            const bool mixed = (tid >= 3 && tid < 6) || (tid >= 8 && tid < 11) || (tid >= 12 && tid < 15);
            if (mixed || (tid >= 24 && tid < 27)) s = -s;
        }
        Sp[tid] = s;
    }
    __syncthreads();
    const int idx = (int)tid;
    if (idx < 21) {
        int r = 0, rem = idx;
        while (rem >= 6 - r) { rem -= 6 - r; r++; }
        const int c = r + rem;
        float S[21];
#pragma unroll
        for (int k2 = 0; k2 < 21; k2++) S[k2] = Sp[k2];
        float Mr[6], Mc[6];
#pragma unroll
        for (int l = 0; l < 6; l++) { Mr[l] = Mt[6 * r + l]; Mc[l] = Mt[6 * c + l]; }
        float a = 0.0f;
#pragma unroll
        for (int k2 = 0; k2 < 6; k2++) {
            float u = 0.0f;                                   // u = (S' Mc^T)[k2]
#pragma unroll
            for (int l = 0; l < 6; l++) u += S[tri21(k2, l)] * Mc[l];
            a += Mr[k2] * u;
        }
        store_sum(out + idx, a, mode);
    } else if (idx < 27) {
        const int r = idx - 21;
        float a = 0.0f;
#pragma unroll
        for (int k2 = 0; k2 < 6; k2++) a += Mt[6 * r + k2] * Sp[21 + k2];
        store_sum(out + idx, a, mode);
    } else if (idx == 27) {
        store_sum(out + 27, Sp[27], mode);
    }
}

// where the workgroup of (dense pair p, tile, instance b) puts its record, and how (store_sum's mode)
__device__ __forceinline__ float *dense_record_out(const SolveDims &D, float *__restrict__ partials, int p, int tile, int b) { return partials + ((unsigned)b * D.dp_stride + (unsigned)(D.atomic_sums ? p : p * D.dense_tiles + tile) * (unsigned)kDenseVals); }
__device__ __forceinline__ int dense_record_mode(const SolveDims &D) { return D.atomic_sums ? 1 : 0; }

// (tile, pair, instance) of position L of the dense grids: tile fastest, then pair, then instance
__device__ __forceinline__ void dense_grid_decode(const SolveDims &D, unsigned L, int &tile, int &p, int &b)
{
    tile = (int)(L % (unsigned)D.dense_tiles);
    p = (int)((L / (unsigned)D.dense_tiles) % (unsigned)D.n_dense_pairs);
    b = (int)(L / ((unsigned)D.dense_tiles * (unsigned)D.n_dense_pairs));
}

// the context of pixel_geom / pixel_accumulate for target fi, source fj of the instance whose poses start at T + pb
__device__ __forceinline__ DenseCtx dense_ctx(const SolveDims &D, const float *__restrict__ T, const float *__restrict__ Tinv, unsigned pb, int fi, int fj, const float4 *cam_t, const float4 *nrm_t)
{
    DenseCtx C;
    C.Tij = mat_mul(load_mat4(Tinv + pb + 16 * fi), load_mat4(T + pb + 16 * fj));      // source camera -> target camera
    C.cam_t = cam_t; C.nrm_t = nrm_t;
    C.fx = D.fx; C.fy = D.fy; C.cx = D.cx; C.cy = D.cy; C.depth_min = D.depth_min; C.depth_max = D.depth_max;
    C.normal_thresh = D.normal_thresh; C.dist2_thresh = D.dist_thresh * D.dist_thresh;
    C.delta = D.robust_delta; C.delta2 = D.robust_delta * D.robust_delta; C.w_dense = D.w_dense;
    C.W = D.width; C.H = D.height;
    return C;
}

// 1-D grid of dense_tiles * Pd * B workgroups (XCD-remapped).  Lane = consecutive source pixel (coalesced
// float4 loads of the source camPos / normal); two pixels per lane per trip, sixteen target-tap gathers in
// flight; the taps stay in L1/L2 because neighbouring source pixels project to neighbouring target pixels.
__device__ __forceinline__ void dense_block(const SolveDims &D, const float4 *__restrict__ campos, const float4 *__restrict__ normals,
                                            const int2 ij, const float *__restrict__ T, const float *__restrict__ Tinv,
                                            float *__restrict__ partials, int tile, int p, int b, float *red)
{
    const int fi = ij.x, fj = ij.y;                       // fi = target, fj = source
    const size_t fb = (size_t)b * D.n_frames;
    const unsigned pb = (unsigned)b * (unsigned)D.pose_stride;
    dense_M_store(threadIdx.x, red, dense_M_load(threadIdx.x, T + pb + 16 * fi));
    const DenseCtx C = dense_ctx(D, T, Tinv, pb, fi, fj, campos + (fb + fi) * (size_t)D.npix, normals + (fb + fi) * (size_t)D.npix);
    const float4 *cam_s = campos + (fb + fj) * (size_t)D.npix, *nrm_s = normals + (fb + fj) * (size_t)D.npix;
    const int per = (D.npix + D.dense_tiles - 1) / D.dense_tiles;
    const int lo = min(D.npix, per * tile), hi = min(D.npix, per * (tile + 1));
    float acc[kDenseVals];
#pragma unroll
    for (int k = 0; k < kDenseVals; k++) acc[k] = 0.0f;

    {
        int s = lo + (int)threadIdx.x;
        float4 cs_n = make_float4(0.f, 0.f, 0.f, 0.f), ns_n = cs_n;
        if (s < hi) { cs_n = cam_s[s]; ns_n = nrm_s[s]; }
        for (; s < hi; s += kBlock) {
            const float4 cs = cs_n, ns = ns_n;
            if (s + kBlock < hi) { cs_n = cam_s[s + kBlock]; ns_n = nrm_s[s + kBlock]; }      // next pixel's stream loads
#ifdef BTBA_REFERENCE_ORDER
            pixel_reference_order(C, D.dist_thresh, cs, ns, acc);
            continue;
#endif
            const PixelGeom g = pixel_geom(C, cs, ns);
            // a wave whose 64 source pixels are all rejected (masked scenes: ~95 % of the image) skips the gathers
            if (__builtin_amdgcn_ballot_w64(g.valid) == 0ull) continue;
            const float4 c00 = C.cam_t[g.i00], c10 = C.cam_t[g.i10], c01 = C.cam_t[g.i01], c11 = C.cam_t[g.i11];
            const float4 n00 = C.nrm_t[g.i00], n10 = C.nrm_t[g.i10], n01 = C.nrm_t[g.i01], n11 = C.nrm_t[g.i11];
            pixel_accumulate(C, g, c00, c10, c01, c11, n00, n10, n01, n11, acc);
        }
    }
    dense_epilogue(acc, red, dense_record_out(D, partials, p, tile, b), dense_record_mode(D));
}

// ---- per-block depth ranges of the compact cache ------------------------------------------------------------------
// [min, max] of the valid (gated: non-zero) depths per 8 x 8 pixel block of a cached frame; an empty block gets (+inf, -inf).
// Part of the frame cache: built once per frame (pool slot), not per solve.  One wave per block, lane = pixel, butterfly min / max;
// grid (blocks / 4, frames): one load per lane and no loop -- a single memory round trip deep.
__global__ void __launch_bounds__(kBlock) k_block_ranges(int width, int height, const float4 *__restrict__ zn, const int *__restrict__ slots, float2 *__restrict__ ranges)
{
    const int slot = slots ? slots[blockIdx.y] : (int)blockIdx.y;
    const int bw = width >> 3, nblk = bw * (height >> 3);
    const int lane = (int)threadIdx.x & 63, blk = (int)blockIdx.x * (kBlock / 64) + ((int)threadIdx.x >> 6);
    if (blk >= nblk) return;
    const int by = blk / bw, bx = blk - by * bw;
    const float d = zn[(size_t)slot * width * height + (size_t)((by * 8 + (lane >> 3)) * width + bx * 8 + (lane & 7))].x;
    const bool ok = d > 0.0f;                              // gated depth: 0 where invalid; NaN compares false
    float lo = ok ? d : INFINITY, hi = ok ? d : -INFINITY;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { lo = fminf(lo, __shfl_xor(lo, m)); hi = fmaxf(hi, __shfl_xor(hi, m)); }
    if (lane == 0) ranges[(size_t)slot * nblk + blk] = make_float2(lo, hi);
}

// Ordered list of the pixels of every frame that carry a depth (>= 0.1 m, the cache builder's validity rule).
// grid (B * K) x 1024.  The dense sweep walks this list instead of all Wd x Hd source pixels: a tracker's frames
// are masked to the object (~5 % of the image, src/Frame.cpp:342-358), so 95 % of the source stream disappears.
// Deterministic order (ascending pixel index).
constexpr int kListTrips = 32;        // ballots a wave keeps in scalar registers: frames up to 16 * 64 * 32 = 32 768 cached pixels
__global__ void __launch_bounds__(1024) k_valid_lists(int npix, const float4 *__restrict__ zn, uint32_t *__restrict__ lists, int *__restrict__ counts,
                                                     const int *__restrict__ slots)
{
    // one workgroup of 16 waves per frame; wave w owns the contiguous segment [w seg, (w+1) seg) and reads it in
    // coalesced 64-pixel trips, all loads in flight at once; the per-trip ballots stay in SGPRs, so after the 16
    // wave totals have been exchanged through LDS the lists are written without reading the frame again.
    __shared__ int wave_tot[16];
    const int f = slots ? slots[blockIdx.x] : (int)blockIdx.x;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const float4 *z = zn + (size_t)f * npix;
    uint32_t *out = lists + (size_t)f * npix;
    const int seg = (((npix + 15) / 16) + 63) & ~63, trips = seg / 64;
    const int s_wave = wave * seg;
    int total = 0;
    if (trips <= kListTrips) {
        unsigned long long m[kListTrips];
#pragma unroll
        for (int k = 0; k < kListTrips; k++) {
            const int s = s_wave + k * 64 + lane;
            const bool v = (k < trips) && (s < npix) && (z[min(s, npix - 1)].x >= 0.1f);      // (double)d >= 0.1  <=>  d >= 0.1f
            m[k] = __builtin_amdgcn_ballot_w64(v);
        }
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < kListTrips; k++) cnt += __popcll(m[k]);
        if (lane == 0) wave_tot[wave] = cnt;
        __syncthreads();
        int base = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) { const int t = wave_tot[w]; if (w < wave) base += t; total += t; }
#pragma unroll
        for (int k = 0; k < kListTrips; k++) {
            const unsigned long long b = m[k];
            const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0));
            if ((b >> lane) & 1ull) out[base + before] = (uint32_t)(s_wave + k * 64 + lane);
            base += __popcll(b);
        }
    } else {                          // large caches: same scheme, the frame is read twice
        int cnt = 0;
        for (int k = 0; k < trips; k++) {
            const int s = s_wave + k * 64 + lane;
            cnt += __popcll(__builtin_amdgcn_ballot_w64((s < npix) && (z[min(s, npix - 1)].x >= 0.1f)));
        }
        if (lane == 0) wave_tot[wave] = cnt;
        __syncthreads();
        int base = 0;
        for (int w = 0; w < 16; w++) { const int t = wave_tot[w]; if (w < wave) base += t; total += t; }
        for (int k = 0; k < trips; k++) {
            const int s = s_wave + k * 64 + lane;
            const bool v = (s < npix) && (z[min(s, npix - 1)].x >= 0.1f);
            const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
            const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0));
            if (v) out[base + before] = (uint32_t)s;
            base += __popcll(b);
        }
    }
    if (threadIdx.x == 0) counts[f] = total;
}

// ---- the general-K sweep on the compact cache: ONE 16-byte load per source pixel and per tap (5 loads instead of 10), camera-space points re-derived from z with
// the cache builder's exact arithmetic (zn_backproject).  General intrinsics only (skew, or a projective last row): every pinhole case is dense_block_pinhole's.
// The set-up of an item and the stages of a pixel are shared with the objective report (btba_objective.hpp), like the pinhole stages below.
struct ZnItem { DenseCtx C; const float *lut_x, *lut_y; const float4 *zn_t, *zn_s; size_t slot_s; };      // LDS tables (below); the target and the source frame; the source frame's cache slot
// Item set-up, by the kBlock threads of the workgroup: target fi, source fj of instance b; lut = (Wd + Hd) floats of LDS.  Holds a barrier.
__device__ __forceinline__ ZnItem zn_item_setup(const SolveDims &D, const float4 *__restrict__ zn, const float *__restrict__ T, const float *__restrict__ Tinv, int fi, int fj, int b, float *lut)
{
    // lut[0 .. Wd) = (float) full-res column of cache column x, lut[Wd .. Wd+Hd) the same for rows: the per-coordinate
    // arithmetic becomes one LDS read
    for (int e = (int)threadIdx.x; e < D.width + D.height; e += kBlock)
        lut[e] = (float)(e < D.width ? zn_src_coord(e, D.zn_scale_w) : zn_src_coord(e - D.width, D.zn_scale_h));
    __syncthreads();
    ZnItem I;
    I.lut_x = lut; I.lut_y = lut + D.width;
    const size_t fb = (size_t)b * D.n_frames;
    I.C = dense_ctx(D, T, Tinv, (unsigned)b * (unsigned)D.pose_stride, fi, fj, nullptr, nullptr);
    // the relative pose is the same in every lane: keep it in scalar registers (12 VGPRs back)
#pragma unroll
    for (int e = 0; e < 12; e++) I.C.Tij.m[e] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, I.C.Tij.m[e])));
    // wave-uniform by construction; readfirstlane tells the compiler, so the frame bases live in SGPRs and the tap
    // gathers use the scalar-base + 32-bit-offset addressing form
    const size_t slot_t = (size_t)__builtin_amdgcn_readfirstlane((int)frame_slot_of(D, fb + fi));
    I.slot_s = (size_t)__builtin_amdgcn_readfirstlane((int)frame_slot_of(D, fb + fj));
    I.zn_t = zn + slot_t * (size_t)D.npix; I.zn_s = zn + I.slot_s * (size_t)D.npix;
    return I;
}
// stage 1: the source pixel (px, py) with cache entry zs, back-projected, through pixel_geom
__device__ __forceinline__ PixelGeom zn_pixel_geom(const SolveDims &D, const ZnItem &I, int px, int py, const float4 &zs)
{
    const float3 cp = zn_backproject(D.zn_ki, I.lut_x[px], I.lut_y[py], zs.x);
    return pixel_geom(I.C, make_float4(cp.x, cp.y, cp.z, 1.0f), make_float4(zs.y, zs.z, zs.w, 0.0f));
}
// stage 2: the four taps, back-projected, through pixel_blend (the tap indices of a rejected pixel are clamped into the frame all the same)
__device__ __forceinline__ PixelBlend zn_pixel_blend(const SolveDims &D, const ZnItem &I, const PixelGeom &g)
{
    // 32-bit byte offsets from a scalar base: one shift per tap instead of a 64-bit shift-add (a frame is far below 4 GB)
    const char *zt = reinterpret_cast<const char *>(I.zn_t);
    const float4 z00 = *reinterpret_cast<const float4 *>(zt + ((unsigned)g.i00 << 4)), z10 = *reinterpret_cast<const float4 *>(zt + ((unsigned)g.i10 << 4));
    const float4 z01 = *reinterpret_cast<const float4 *>(zt + ((unsigned)g.i01 << 4)), z11 = *reinterpret_cast<const float4 *>(zt + ((unsigned)g.i11 << 4));
    const float xia = I.lut_x[g.xa], xib = I.lut_x[g.xb], yia = I.lut_y[g.ya], yib = I.lut_y[g.yb];
    const float3 c00 = zn_backproject(D.zn_ki, xia, yia, z00.x), c10 = zn_backproject(D.zn_ki, xib, yia, z10.x);
    const float3 c01 = zn_backproject(D.zn_ki, xia, yib, z01.x), c11 = zn_backproject(D.zn_ki, xib, yib, z11.x);
    return pixel_blend(I.C, g, make_float4(c00.x, c00.y, c00.z, 1.f), make_float4(c10.x, c10.y, c10.z, 1.f), make_float4(c01.x, c01.y, c01.z, 1.f), make_float4(c11.x, c11.y, c11.z, 1.f),
                       make_float4(z00.y, z00.z, z00.w, 0.f), make_float4(z10.y, z10.z, z10.w, 0.f), make_float4(z01.y, z01.z, z01.w, 0.f), make_float4(z11.y, z11.z, z11.w, 0.f));
}

template <bool LISTS>
__device__ __forceinline__ void dense_block_zn(const SolveDims &D, const float4 *__restrict__ zn, const int2 ij,
                                               const float *__restrict__ T, const float *__restrict__ Tinv,
                                               float *__restrict__ partials, int tile, int p, int b, float *red,
                                               const uint32_t *__restrict__ valid_lists, const int *__restrict__ valid_counts, float *lut)
{
    const ZnItem I = zn_item_setup(D, zn, T, Tinv, ij.x, ij.y, b, lut);       // ij = (target, source)
    dense_M_store(threadIdx.x, red, dense_M_load(threadIdx.x, T + (unsigned)b * (unsigned)D.pose_stride + 16 * ij.x));
    // LISTS: walk the source frame's ordered list of pixels that carry a depth (masked scenes: ~5 % of the image);
    // otherwise walk all pixels with incrementally advanced coordinates.  Two instantiations rather than one loop
    // with both: the kernel sits at the 96-VGPR / 5-waves-per-SIMD boundary and the merged loop measured 8 % slower.
    const int n_src = LISTS ? valid_counts[I.slot_s] : D.npix;
    const uint32_t *list = LISTS ? valid_lists + I.slot_s * (size_t)D.npix : nullptr;
    const int per = (n_src + D.dense_tiles - 1) / D.dense_tiles;
    const int lo = min(n_src, per * tile), hi = min(n_src, per * (tile + 1));
    const float inv_w = 1.0f / (float)D.width;
    float acc[kDenseVals] = {};

    int t = lo + (int)threadIdx.x;
    int s_n = (t < hi) ? (LISTS ? (int)list[t] : t) : 0;
    int px_i = s_n % D.width, py_i = s_n / D.width;             // incremental coordinates (direct walk only)
    const int step_x = kBlock % D.width, step_y = kBlock / D.width;
    float4 zs_n = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < hi) zs_n = I.zn_s[s_n];
    for (; t < hi; t += kBlock) {
        const float4 zs = zs_n;
        const int s = s_n;
        if (t + kBlock < hi) { s_n = LISTS ? (int)list[t + kBlock] : t + kBlock; zs_n = I.zn_s[s_n]; }      // next pixel's stream loads
        int px, py;
        if (!LISTS) {
            px = px_i; py = py_i;
            px_i += step_x; py_i += step_y;
            if (px_i >= D.width) { px_i -= D.width; py_i++; }
        } else {
            py = (int)((float)s * inv_w);                       // s < 2^24: exact up to one unit, fixed up below
            py -= (py * D.width > s) ? 1 : 0;
            py += ((py + 1) * D.width <= s) ? 1 : 0;
            px = s - py * D.width;
        }
        const PixelGeom g = zn_pixel_geom(D, I, px, py, zs);
        if (__builtin_amdgcn_ballot_w64(g.valid) == 0ull) continue;
        pixel_sums(I.C, g, zn_pixel_blend(D, I, g), acc);
    }
    dense_epilogue(acc, red, dense_record_out(D, partials, p, tile, b), dense_record_mode(D));
}

// ---- the dense sweep for pinhole intrinsics on the GATED compact cache --------------------------------------------
// Same arithmetic per accepted pixel as the general sweep's (dense_block_zn, with the back-projection bracket tabulated: see zn_backproject), re-shaped around what the VALU of gfx950 actually charges
// (scripts/valu_calibrate.hip, profiles/r02/valu_calibration.md): a wave64 fp32 mul / add / fma with VGPR sources issues in
// 2 cycles, but v_cmp*, v_cndmask*, v_cvt*, v_floor, v_min / v_max, v_lshlrev, every VOP3 integer op (v_lshl_add_u32,
// v_mul_lo_u32, ...) and ANY VALU op with an SGPR source take 4, transcendentals 8.  The old loop spent 71 of its 222
// instructions on compares, selects and integer index arithmetic and 35 more on 2-cycle operations slowed down by an SGPR
// operand.  Here:
//   * the cache stores the GATED depth (0 where the reference's camPos is 0: d < 0.1 or NaN, CUDAImageUtil.cu:310-327),
//     so the per-tap `d >= 0.1 ? d : 0` select (5 compares + 5 selects per pixel) is done once, by the cache builder;
//   * a pinhole K^-1 has [15] == 1, so z = d without a multiply;
//   * the projection is CLAMPED to the image, uc = med3(u, 0, W - 1): the in-image test of the rounded coordinates
//     (-0.5 < u < W - 0.5, SolverBundlingDenseUtil.h:91-94) is |u - uc| < 0.5 -- exact, both differences are exact -- and
//     the bilinear taps are floor(uc), ceil(uc): a tap the reference skips because it lies outside the image
//     (ICPUtil.h:96-102) gets weight 0 here, and where the reference renormalises by the surviving weight, alpha / alpha,
//     the clamped coordinate has weight exactly 1.  No tap-validity compares, no weight selects, no reciprocals; when all
//     four taps are in the image the reference divides by (1 - alpha) + alpha = 1 +- 1 ulp, which is dropped (the
//     reference itself is built with -use_fast_math);
//   * tap addresses are computed in fp32 (exact: byte offsets < 2^24) and converted once per tap: 4 v_cvt instead of
//     8 clamps, 2 integer multiplies and 8 shift-adds; LDS look-up addresses likewise;
//   * depth-range tests are one unsigned compare of the bit patterns: for positive floats order is bit order, negative
//     values, zeros and NaN fall outside after the subtraction wraps;
//   * wave-uniform operands of 2-cycle operations (relative pose, intrinsics) live in VGPRs.
struct PinholeCtx {
    float R[9], t[3];                 // relative pose source camera -> target camera (scalar registers)
    float fx, fy, cx, cy, wm1, hm1, wm2, hm2, w16, normal_thresh, dist2_thresh, wdelta, w_dense, ybase4;
    unsigned row16;                   // bytes per cache row
    unsigned zmin_bits, zrange_bits;  // depth_min < z < depth_max  <=>  bits(z) - (bits(depth_min) + 1) < zrange_bits (unsigned)
    // what the phases of dense_block_pinhole share beside the per-pixel constants above
    unsigned tid; int p;              // item_tid(); dense pair of the item
    size_t slot_t, slot_s;            // cache slots of the target and the source frame (scalar registers)
    int bw, bh, r0, nb;               // block walk: blocks per row and column of the cache, first block row and block count of this item's band
    const float2 *rng; float2 zr0, zr1;      // block walk: the band's block ranges (nullptr: no block is skipped); those of blocks tid and tid + kBlock, loaded with the poses
    float *lut; float4 *colA; float *hull; int *hdr; unsigned *blist;      // dynamic LDS (SweepLayout): back-projection terms, rotated rays (colA, rowB behind it), hull entries, the compaction's wave totals, live blocks
    const float4 *zn_s; const char *tap_row0, *tap_row1;      // the source frame; the target frame's first and second row
    float lut_addr_f, ybase4_abs;     // LDS byte addresses of the column and the row table, as floats
};

// 16 bytes at a byte offset, with the constant part of the address as the load's immediate offset (base + zext(byte_off) + IMM in 64 bits: a 32-bit
// `byte_off + IMM` may wrap, so the compiler cannot fold it and spends a vector add per tap)
template <int IMM> __device__ __forceinline__ float4 gather16_imm(const char *base, unsigned byte_off) { return *reinterpret_cast<const float4 *>(base + (size_t)byte_off + IMM); }
// LDS byte address of a pointer into the workgroup's LDS, and two consecutive floats at an absolute LDS byte address: the table base rides in the fp32 address
// arithmetic (exact below 2^24) instead of costing a vector add behind every float -> int conversion
__device__ __forceinline__ unsigned lds_address(const void *p) { return (unsigned)(unsigned long)(const __attribute__((address_space(3))) char *)p; }
__device__ __forceinline__ float2 lds_f32x2_abs(unsigned addr) { const __attribute__((address_space(3))) float *q = (const __attribute__((address_space(3))) float *)(unsigned long)addr; return make_float2(q[0], q[1]); }
// v_min_f32 as the hardware does it: fminf() makes the compiler canonicalise its operands first (v_max_f32 x, x, x -- a half-rate
// instruction per operand, repeated in the loop even for loop invariants); the operands here are never signalling NaNs
__device__ __forceinline__ float min_raw(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// a * b + c as a v_fma_f32 whose destination is none of its sources.  An FMA that overwrites one of its own sources (v_fmac_f32, or v_fma_f32 with
// D = C) issues at HALF rate when its other two sources sit in VGPRs of the same parity or are the same register (profiles/r02/valu_calibration.md,
// rows `x:`); which registers they get is the allocator's business.  With the destination elsewhere the instruction is full rate whatever it does.
__device__ __forceinline__ float fma_nd(float a, float b, float c) { float d; asm("v_fma_f32 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c)); return d; }
// ... with a wave-uniform bound held in a SCALAR register: v_min / v_med3 are half-rate whatever their operands, so the scalar operand costs
// no issue slot and the bound does not occupy a VGPR of a kernel that spills (left alone, the compiler keeps such loop invariants in VGPRs)
__device__ __forceinline__ float min_raw_s(float a, float bound) { float r; asm("v_min_f32 %0, %2, %1" : "=v"(r) : "v"(a), "s"(bound)); return r; }
__device__ __forceinline__ float clamp0_s(float a, float bound) { float r; asm("v_med3_f32 %0, %1, %2, 0" : "=v"(r) : "v"(a), "s"(bound)); return r; }     // med3(a, bound, 0); NaN -> 0
__device__ __forceinline__ float sgpr(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x))); }

// column / row term of the back-projection of cache column / row e (e >= width: row e - width): K^-1[0][0] x_full(e) + K^-1[0][2] resp.
// K^-1[1][1] y_full + K^-1[1][2] -- the cache builder's nearest-neighbour source coordinate, the bracket of zn_backproject's comment
__device__ __forceinline__ float pinhole_lut_entry(const SolveDims &D, int e)
{
    const bool is_x = e < D.width;
    const float c = (float)(is_x ? zn_src_coord(e, D.zn_scale_w) : zn_src_coord(e - D.width, D.zn_scale_h));
    return is_x ? D.zn_ki[0] * c + D.zn_ki[2] : D.zn_ki[5] * c + D.zn_ki[6];
}

// (The dead-block test of the block walk -- is an 8 x 8 block of the source frame PROVABLY without a pixel that lands in the target image? -- is
// btba_hull.hpp: plain C++ that the host compiles too.)

// (target, source, dense pair) of work position q: computed where the work order is the closed form (the default pair policies), read from
// the work table otherwise.  q is wave-uniform: scalar arithmetic / a scalar load.
__device__ __forceinline__ void dense_work_item(const SolveDims &D, int q, int &fi, int &fj, int &p)
{
    if (D.work_formula) {
        int d = 1, rem = q;                        // pairs at frame distance d: (i, i + d), i = 0 .. N-1-d, distances ascending
        while (rem >= D.n_frames - d) { rem -= D.n_frames - d; d++; }
        p = pair_index(rem, rem + d, D.n_frames);  // the canonical list IS the dense pair list of these policies
        fi = D.work_formula == 1 ? rem : rem + d;
        fj = D.work_formula == 1 ? rem + d : rem;
    } else {
        const int4 w = ld_const_i4(D.dense_work + q);
        fi = w.x; fj = w.y; p = w.z;
    }
}

// ---- the dense sweep for pinhole intrinsics on the GATED compact cache --------------------------------------------
// (the arithmetic per accepted pixel is that of dense_block_zn with the back-projection bracket tabulated; the shape is what the VALU of gfx950 charges for, see above)
// The phases of a pinhole item, in the order dense_block_pinhole runs them.  WALK: 0 64-pixel row strips, 1 the source frame's valid-pixel list,
// 2 8 x 8 pixel blocks per wave (cache width and height multiples of 8).

// Phase 1, item and poses.  The prologue is ONE round of memory loads, every address a function of the workgroup's grid position: the item (computed, or one
// scalar load), the two poses (scalar loads: the previous launch wrote them), the target pose for M, the band's block ranges.
// (Round 2: work table -> poses / ranges -> hull test -> list, four dependent round trips, 7.2 of a workgroup's 39 us.)
// Returns this thread's entry of M of the epilogue's congruence (dense_M_load), to be stored behind the table fill.
template <int WALK>
__device__ __forceinline__ float pinhole_item_and_poses(const SolveDims &D, PinholeCtx &C, int q, const float *__restrict__ T, const float *__restrict__ Tinv, int tile, int b)
{
    C.tid = item_tid();
    int fi, fj;                                           // fi = target, fj = source
    dense_work_item(D, q, fi, fj, C.p);
    const size_t fb = (size_t)b * D.n_frames;
    C.slot_t = (size_t)__builtin_amdgcn_readfirstlane((int)frame_slot_of(D, fb + fi));
    C.slot_s = (size_t)__builtin_amdgcn_readfirstlane((int)frame_slot_of(D, fb + fj));
    const unsigned pb = (unsigned)b * (unsigned)D.pose_stride;
    const Mat4 Tinv_i = load_mat4_uniform(Tinv + pb + 16 * fi), T_j = load_mat4_uniform(T + pb + 16 * fj);
    const float m_stage = dense_M_load(C.tid, T + pb + 16 * fi);
    C.bw = D.width >> 3; C.bh = D.height >> 3;
    const int rows_per = (C.bh + D.dense_tiles - 1) / D.dense_tiles;
    const int r1 = min(C.bh, rows_per * (tile + 1));
    C.r0 = min(C.bh, rows_per * tile);
    C.nb = (WALK == 2) ? (r1 - C.r0) * C.bw : 0;          // blocks of this band (the host keeps it <= kMaxBandBlocks)
    C.rng = (WALK == 2 && D.block_ranges) ? D.block_ranges + C.slot_s * (size_t)(C.bw * C.bh) + (size_t)C.r0 * C.bw : nullptr;
    C.zr0 = (C.rng && (int)C.tid < C.nb) ? C.rng[C.tid] : make_float2(0.0f, 0.0f);
    C.zr1 = (C.rng && (int)C.tid + kBlock < C.nb) ? C.rng[C.tid + kBlock] : make_float2(0.0f, 0.0f);      // a one-tile band of a 160 x 120 cache holds 300 blocks: both ranges of a lane in the SAME round of loads
                                                                                                           // (bands of more than 512 blocks fetch the rest in the compaction loop)
    const Mat4 Tij = mat_mul(Tinv_i, T_j);                // source camera -> target camera
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) C.R[3 * r + c] = sgpr(Tij.m[4 * r + c]);
        C.t[r] = sgpr(Tij.m[4 * r + 3]);
    }
    return m_stage;
}

// Phase 2, table fill.  Tables in LDS: lut[0 .. Wd) = K^-1[0][0] x_full(x) + K^-1[0][2] per cache column, lut[Wd .. Wd+Hd) the same for rows (the taps' back-projection),
// and the ROTATED RAYS: the transformed point of source pixel (x, y) with depth d is q = d (R (lx, ly, 1)) + t = d (colA[x] + rowB[y]) + t with
// colA[x] = R[:, 0] lx(x), rowB[y] = R[:, 1] ly(y) + R[:, 2] -- two 16-byte LDS reads, 3 adds and 3 FMAs per pixel instead of 2 reads,
// 2 multiplies and 12 operations with a scalar-register operand (which issue at half rate, profiles/r02/valu_calibration.md).  One pass.
// Behind the tables (SweepLayout): the hull entries of the dead-block test (one per block column and block row, 8 floats apart), the wave totals of the list compaction
// ([0 .. 8): two blocks per lane and pass, [0 .. 4) first halves, [4 .. 8) second), the list of live blocks.
template <int WALK>
__device__ __forceinline__ void pinhole_fill_tables(const SolveDims &D, PinholeCtx &C, float *lut)
{
    const SweepLayout L(D.width, D.height, 0, WALK == 2 ? kSweepLdsBlocks : kSweepLdsStrips);      // (no offset depends on the band's size: it only ends the list)
    char *lds = reinterpret_cast<char *>(lut);
    C.lut = lut; C.colA = reinterpret_cast<float4 *>(lds + L.colA);
    C.hull = reinterpret_cast<float *>(lds + L.hull); C.hdr = reinterpret_cast<int *>(lds + L.hdr); C.blist = reinterpret_cast<unsigned *>(lds + L.blist);
    for (int e = (int)C.tid; e < D.width + D.height; e += kBlock) {
        const float l = pinhole_lut_entry(D, e);
        C.lut[e] = l;
        // rowB follows colA as the row terms follow the column terms in lut: entry e of both tables is colA[e]
        if (e < D.width) C.colA[e] = make_float4(C.R[0] * l, C.R[3] * l, C.R[6] * l, 0.0f);
        else C.colA[e] = make_float4(C.R[1] * l + C.R[2], C.R[4] * l + C.R[5], C.R[7] * l + C.R[8], 0.0f);
    }
}

// Phase 3, the list of live blocks (WALK 2; the other walks only meet the barrier behind the tables).  Returns the number of list entries.
// Blocks that are provably dead (btba_hull.hpp: 90 % of the dead ones at c3) are removed BEFORE the walk; the live ones are compacted
// into an ordered list in LDS (ballot + mbcnt, block order: deterministic) that the four waves share round-robin.
// The test is SEPARABLE: per block column and block row five extremes of the edge forms (35 entries for a 160 x 120 cache, one lane each, filled by the
// last wave -- the first one has the second half of a 300-block band to test); a block's verdict is then two 20-byte LDS reads and ~25 operations,
// where the corner-by-corner evaluation of the forms took ~120 and made wave 0, with two blocks per lane, the slowest of the prologue.
template <int WALK>
__device__ __forceinline__ int pinhole_live_blocks(const SolveDims &D, const PinholeCtx &C)
{
    int n_live = 0;
    if (WALK == 2) {
        const unsigned tid = C.tid;
        const int bw = C.bw, nb = C.nb, r0 = C.r0, n_ent = C.bw + C.bh;
        const int lane_c = (int)tid & 63, wave_c = __builtin_amdgcn_readfirstlane((int)tid >> 6);
        namespace H = btba_hull;
        const H::HullForms F = H::hull_forms(D.fx, D.fy, D.cx, D.cy, D.width, D.height);
        const H::HullBias hb = H::hull_bias(F, C.t);
        if (C.rng) {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
            for (int e = (int)tid - (kBlock - 64); e >= 0 && e < n_ent; e += 64) {      // block column e, or block row e - bw, from its first and last pixel's back-projection terms
                const bool row = e >= bw;
                const int px = row ? D.width + 8 * (e - bw) : 8 * e;
                const H::HullEntry h = H::hull_entry(C.R, F, row, pinhole_lut_entry(D, px), pinhole_lut_entry(D, px + 7));
                *reinterpret_cast<float4 *>(C.hull + 8 * e) = make_float4(h.lmax, h.rmin, h.tmax, h.bmin);
                C.hull[8 * e + 4] = h.zmin;
            }
        }
        __syncthreads();                                      // the entries are read by the test
        const float inv_bw = fast_rcp((float)bw);             // block row of a block index: idx < kMaxBandBlocks, so the product's error, at most (1024 / bw) 3 2^-23, is far below the margin 0.5 / bw
        // Two blocks per lane and pass (idx, idx + 256): every band of a 160 x 120 cache -- 300 blocks at one tile -- is tested and compacted in ONE pass,
        // one exchange of wave totals and two barriers behind the one in front of the test: three in all (before round 5: two passes of 256, the second with a
        // fresh round of range loads in front of it and two more barriers).  The list keeps its order -- blocks 0 .. 255 of the pass, then 256 .. 511 -- so the walk
        // and every sum are what they were.
        auto is_live = [&](const float2 &zr, int bxl, int byg) {
            const float *ce = C.hull + 8 * bxl, *re = C.hull + 8 * (bw + byg);
            const float4 c4 = *reinterpret_cast<const float4 *>(ce), r4 = *reinterpret_cast<const float4 *>(re);
            const H::HullEntry hc = { c4.x, c4.y, c4.z, c4.w, ce[4] }, hr = { r4.x, r4.y, r4.z, r4.w, re[4] };
            return H::hull_block_live(hc, hr, hb, zr.x, zr.y, D.depth_min, D.depth_max);
        };
        for (int c0 = 0; c0 < nb; c0 += 2 * kBlock) {
            const int idx0 = c0 + (int)tid, idx1 = idx0 + kBlock;
            bool live0 = false, live1 = false;
            unsigned code0 = 0, code1 = 0;
            auto test = [&](int idx, const float2 &zr, unsigned &code, bool &live) {
                if (idx >= nb) return;
                const int byl = (int)(((float)idx + 0.5f) * inv_bw), bxl = idx - byl * bw, byg = r0 + byl;
                code = ((unsigned)byg << 16) | (unsigned)bxl;
                live = C.rng ? is_live(c0 ? C.rng[idx] : zr, bxl, byg) : true;
            };
            test(idx0, C.zr0, code0, live0);
            test(idx1, C.zr1, code1, live1);
            const unsigned long long bal0 = __builtin_amdgcn_ballot_w64(live0), bal1 = __builtin_amdgcn_ballot_w64(live1);
            if (lane_c == 0) { C.hdr[wave_c] = __popcll(bal0); C.hdr[4 + wave_c] = __popcll(bal1); }
            __syncthreads();
            int base0 = n_live, total0 = 0, base1 = 0, total1 = 0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; w++) {
                const int t0 = C.hdr[w], t1 = C.hdr[4 + w];
                if (w < wave_c) { base0 += t0; base1 += t1; }
                total0 += t0; total1 += t1;
            }
            base1 += n_live + total0;
            const int before0 = __builtin_amdgcn_mbcnt_hi((unsigned)(bal0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal0, 0));
            const int before1 = __builtin_amdgcn_mbcnt_hi((unsigned)(bal1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal1, 0));
            if (live0) C.blist[base0 + before0] = code0;
            if (live1) C.blist[base1 + before1] = code1;
            n_live += total0 + total1;
            __syncthreads();
        }
    } else __syncthreads();
    return n_live;
}

// Phase 4, the per-pixel constants of the walk.
__device__ __forceinline__ void pinhole_walk_constants(const SolveDims &D, PinholeCtx &C, const float4 *__restrict__ zn)
{
    C.fx = D.fx; C.fy = D.fy; C.cx = D.cx; C.cy = D.cy;
    // the clamp bounds come from the host: a float the kernel makes itself (v_cvt_f32_i32) lives in a VGPR for the whole loop; as kernel arguments
    // they are scalar operands of clamp0_s / min_raw_s
    C.wm1 = D.wm1; C.hm1 = D.hm1; C.wm2 = D.wm2; C.hm2 = D.hm2;
    C.w16 = 16.0f * (float)D.width; C.row16 = 16u * (unsigned)D.width;
    C.ybase4 = 4.0f * (float)D.width;                     // LDS byte offset of the row table
    C.normal_thresh = D.normal_thresh; C.dist2_thresh = D.dist2_thresh;
    C.wdelta = D.w_dense * D.robust_delta; C.w_dense = D.w_dense;
    C.zmin_bits = __float_as_uint(D.depth_min) + 1u; C.zrange_bits = __float_as_uint(D.depth_max) - __float_as_uint(D.depth_min) - 1u;
    C.zn_s = zn + C.slot_s * (size_t)D.npix;
    C.tap_row0 = reinterpret_cast<const char *>(zn + C.slot_t * (size_t)D.npix); C.tap_row1 = C.tap_row0 + C.row16;
    C.lut_addr_f = (float)lds_address(C.lut); C.ybase4_abs = C.ybase4 + C.lut_addr_f;
}

// ---- the stages of one source pixel, in the order they run.  pinhole_pixel accumulates the Jacobian sums behind them, the objective report
// (btba_objective.hpp) its fp64 cost: both form the residual and the accept tests from these statements and no others.
// Stage 1, project.  zs = the pixel's (gated depth, normal), ox / oy = LDS byte offsets of its column / row entries in the ray tables (from colA).
// The three tests stay SINGLE comparisons: the sweep ballots each on its own (see pinhole_pixel), the report ANDs them.
struct PinholeProj { float qx, qy, qz, uc, vc; bool src_ok, in_u, in_v; };
__device__ __forceinline__ PinholeProj pinhole_project(const PinholeCtx &C, const float4 &zs, unsigned ox, unsigned oy)
{
    PinholeProj P;
    // source pixel -> camera space (gated depth: 0 where invalid), depth-range test on the bit pattern
    const float d = zs.x;
    P.src_ok = (__float_as_uint(d) - C.zmin_bits) < C.zrange_bits;
    // transform the point, project
    const float4 ra = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(C.colA) + ox), rb = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(C.colA) + oy);
    P.qx = (ra.x + rb.x) * d + C.t[0]; P.qy = (ra.y + rb.y) * d + C.t[1]; P.qz = (ra.z + rb.z) * d + C.t[2];
    const float rqz = fast_rcp(P.qz);
    // (u, v through the compiler's own FMAs, not fma_nd: an inline-asm consumer directly behind v_rcp_f32 is invisible to the hazard recognizer, which then
    // does not insert the wait state gfx950 needs between a transcendental and a VALU use of its result -- a round-6 build that did so read a stale
    // reciprocal now and then: non-deterministic poses, 2e-4 off, caught by tests/test_cpp_bundler.py and scripts/r06/determinism.py)
    const float u = P.qx * C.fx * rqz + C.cx, v = P.qy * C.fy * rqz + C.cy;
    P.uc = clamp0_s(u, C.wm1); P.vc = clamp0_s(v, C.hm1);      // NaN -> 0: addresses stay in the frame
    P.in_u = fabsf(u - P.uc) < 0.5f; P.in_v = fabsf(v - P.vc) < 0.5f;
    return P;
}
// the source normal in the target camera
__device__ __forceinline__ float3 pinhole_rotate_normal(const PinholeCtx &C, const float4 &zs) { return make_float3(C.R[0] * zs.y + C.R[1] * zs.z + C.R[2] * zs.w, C.R[3] * zs.y + C.R[4] * zs.z + C.R[5] * zs.w, C.R[6] * zs.y + C.R[7] * zs.z + C.R[8] * zs.w); }
// Stage 2, taps: (x0, x0 + 1) x (y0, y0 + 1) with x0 = min(floor(uc), W - 2): at the right / bottom edge (uc = W - 1) the weights are (0, 1)
// instead of (1, -) -- the same blend, and the four taps are always the 2 x 2 block at ONE computed address
struct PinholeTaps { float fx0, fy0, alpha, beta; unsigned o00; };
__device__ __forceinline__ PinholeTaps pinhole_taps(const PinholeCtx &C, const PinholeProj &P)
{
    PinholeTaps K;
    K.fx0 = min_raw_s(floorf(P.uc), C.wm2); K.fy0 = min_raw_s(floorf(P.vc), C.hm2);
    K.alpha = P.uc - K.fx0; K.beta = P.vc - K.fy0;
    // one computed byte offset for the 2 x 2 block: the second row's base is a scalar add (wave-uniform), the + 16 the load's immediate offset field
    K.o00 = (unsigned)(K.fy0 * C.w16 + 16.0f * K.fx0);                                       // byte offset, fp32-exact below 2^24; 0 <= fx0 <= W - 2, 0 <= fy0 <= H - 2: inside the frame
    return K;
}
__device__ __forceinline__ void pinhole_gather(const PinholeCtx &C, const PinholeTaps &K, float4 &z00, float4 &z10, float4 &z01, float4 &z11)
{ z00 = gather16_imm<0>(C.tap_row0, K.o00); z10 = gather16_imm<16>(C.tap_row0, K.o00); z01 = gather16_imm<0>(C.tap_row1, K.o00); z11 = gather16_imm<16>(C.tap_row1, K.o00); }
// Stage 3, blend: the target's normal n_i and q - c_i at the projection, and the three target tests (single comparisons, as in stage 1).  nq: the rotated source normal.
struct PinholeBlend { float nix, niy, niz, dx, dy, dz; bool ciz_ok, dn_ok, dist_ok; };
__device__ __forceinline__ PinholeBlend pinhole_blend(const PinholeCtx &C, const PinholeProj &P, const PinholeTaps &K, const float4 &z00, const float4 &z10, const float4 &z01, const float4 &z11, const float3 &nq)
{
    PinholeBlend B;
    const float2 xi2 = lds_f32x2_abs((unsigned)(4.0f * K.fx0 + C.lut_addr_f)), yi2 = lds_f32x2_abs((unsigned)(4.0f * K.fy0 + C.ybase4_abs));
    const float a0 = 1.0f - K.alpha, b0 = 1.0f - K.beta;
    // blend of the taps' camera-space points (x = column term * z, y = row term * z, z = gated depth) and normals; the
    // column / row terms are shared by the taps of a column / row, so they multiply the partial sums:
    //     cix = xi2.x (t00 + t01) + xi2.y (t10 + t11),  ciy = yi2.x (t00 + t10) + yi2.y (t01 + t11),  ciz = (t00 + t01) + (t10 + t11),  t = c z
    //     ni  = c00 z00.n + c10 z10.n + c01 z01.n + c11 z11.n
    // written out as the fused multiply-adds the compiler contracts these expressions to (x y + z w -> fma(x, y, z w), left to right --
    // the bits of every build since round 1), each as fma_nd: 13 of the 20 were v_fmac whose two multiplicands happened to sit in VGPRs
    // of the same parity, which issue at half rate (26 of a trip's ~400 issue cycles).
    const float c00 = b0 * a0, c10 = b0 * K.alpha, c01 = K.beta * a0, c11 = K.beta * K.alpha;
    const float t10 = c10 * z10.x, t01 = c01 * z01.x, t11 = c11 * z11.x;
    const float s0x = fma_nd(c00, z00.x, t01), s0y = fma_nd(c00, z00.x, t10);       // t00 + t01, t00 + t10
    const float s1x = fma_nd(c10, z10.x, t11), s1y = fma_nd(c01, z01.x, t11);       // t10 + t11, t01 + t11
    const float cix = fma_nd(xi2.x, s0x, xi2.y * s1x);
    const float ciy = fma_nd(yi2.x, s0y, yi2.y * s1y);
    const float ciz = s0x + s1x;
    B.nix = fma_nd(c11, z11.y, fma_nd(c01, z01.y, fma_nd(c00, z00.y, c10 * z10.y)));
    B.niy = fma_nd(c11, z11.z, fma_nd(c01, z01.z, fma_nd(c00, z00.z, c10 * z10.z)));
    B.niz = fma_nd(c11, z11.w, fma_nd(c01, z01.w, fma_nd(c00, z00.w, c10 * z10.w)));
    B.dx = P.qx - cix; B.dy = P.qy - ciy; B.dz = P.qz - ciz;
    const float dist2 = fma_nd(B.dz, B.dz, fma_nd(B.dx, B.dx, B.dy * B.dy));
    const float dn = fma_nd(nq.z, B.niz, fma_nd(nq.x, B.nix, nq.y * B.niy));
    B.ciz_ok = (__float_as_uint(ciz) - C.zmin_bits) < C.zrange_bits; B.dn_ok = dn >= C.normal_thresh; B.dist_ok = dist2 <= C.dist2_thresh;
    return B;
}
// Stage 4, residual, with the sweep's sign: res+ = (q - c_i) . n_i = -res (SIGNS in pinhole_pixel)
__device__ __forceinline__ float pinhole_residual(const PinholeBlend &B) { return fma_nd(B.dz, B.niz, fma_nd(B.dx, B.nix, B.dy * B.niy)); }

// One source pixel of the sweep.  acc: the lane's 27 sums; n_ok: accepted pixels of this WAVE (scalar register), which joins the record as acc[27] behind the walk.
__device__ __forceinline__ void pinhole_pixel(const PinholeCtx &C, const float4 &zs, unsigned ox, unsigned oy, float (&acc)[kDenseVals], int &n_ok)
{
    const PinholeProj P = pinhole_project(C, zs, ox, oy);
    const bool valid = P.src_ok & P.in_u & P.in_v;
    // (the wave's mask of `valid`, AND-ed from the ballots of the single tests: see ok_mask below)
    const unsigned long long valid_mask = __builtin_amdgcn_ballot_w64(P.src_ok) & __builtin_amdgcn_ballot_w64(P.in_u) & __builtin_amdgcn_ballot_w64(P.in_v);
    if (valid_mask == 0ull) return;
    // rotate the normal (only the waves that go on need it: half of the block trips end above)
    const float3 nq = pinhole_rotate_normal(C, zs);
    const PinholeTaps K = pinhole_taps(C, P);
    // Lanes that already failed the in-image / source-depth tests (8.8 % in the trips that go on, clustered along block edges: profiles/r06/sweep_census.json) issue no
    // taps.  The texture addresser's service time per gather is exposed almost in full (profiles/r06/bound_probes.json: one more 16-byte gather per trip = +13.4 us
    // per launch, linear) and it skips idle quads (profiles/r06/taps_exec.json: same bits, -1.5 % on the launch).  The registers of those lanes stay undefined
    // and are never used: `ok` contains `valid`, and nothing behind `ok` runs for a rejected lane.
    float4 z00, z10, z01, z11;
    if (valid) pinhole_gather(C, K, z00, z10, z01, z11);
    const PinholeBlend B = pinhole_blend(C, P, K, z00, z10, z01, z11, nq);
    // the accept mask of the wave, AND-ed from the ballots of the single tests (a ballot of one comparison is the comparison's own scalar result; the
    // ballot of a combined flag is lowered through a select and a second compare)
    const unsigned long long ok_mask = valid_mask & __builtin_amdgcn_ballot_w64(B.ciz_ok) & __builtin_amdgcn_ballot_w64(B.dn_ok) & __builtin_amdgcn_ballot_w64(B.dist_ok);
    // Rejected pixels contribute NOTHING: the count is a popcount of the wave's accept mask in a scalar register, and the residual, the weight, the row
    // and the 27 accumulates run under the exec mask of `ok` like the taps above.  A sum that is not added to equals the sum that got + 0.0f (the
    // accumulators start at + 0.0f and so never hold - 0.0f), so every sum keeps its bits; a rejected lane's blend -- undefined taps, a NaN or inf target
    // normal -- is never read past `ok`.
    n_ok += __popcll(ok_mask);
    if (__builtin_amdgcn_inverse_ballot_w64(ok_mask)) {
        // SIGNS: the row is accumulated as a+ = [n_i ; n_i x q] and the residual as res+ = (q - c_i) . n_i, i.e. a = D a+ with
        // D = diag(-1, -1, -1, 1, 1, 1) and res = -res+ (SolverBundlingDenseUtil.h:78-110, LieDerivUtil.h:228-273).  Then S = D S+ D and
        // g = -D g+ : exact sign changes of whole sums, applied once per workgroup in the epilogue instead of four negations per pixel.
        const float res = pinhole_residual(B);
        // Huber (SolverBundlingUtil.h:24-40) times the dense weight: rho' = 1 for e <= delta^2, delta / sqrt(e) above  <=>  min(1, delta rsq(e))
        // (res = 0: rsq(0) = inf, min(inf, w) = w).
        const float wgt = min_raw_s(C.wdelta * fast_rsq(res * res), C.w_dense);
        const float a[6] = { B.nix, B.niy, B.niz, B.niy * P.qz - B.niz * P.qy, B.niz * P.qx - B.nix * P.qz, B.nix * P.qy - B.niy * P.qx };
        int k = 0;
        // acc += wa_r * a_c is a read-modify-write FMA: it issues at full rate only when its two multiplicands sit in VGPRs of
        // different parity (profiles/r02/valu_calibration.md).  (wa_r, a_r) held as an aligned register PAIR puts every wa in an
        // even and every a in an odd register, whatever the allocator does with the rest.
        typedef float f2v __attribute__((ext_vector_type(2)));
        f2v pr[6];
#pragma unroll
        for (int r = 0; r < 6; r++) { pr[r] = (f2v){ wgt * a[r], a[r] }; asm volatile("" : "+v"(pr[r])); }
        f2v rr = (f2v){ wgt, res };
        asm volatile("" : "+v"(rr));
#pragma unroll
        for (int r = 0; r < 6; r++) {
#pragma unroll
            for (int c = r; c < 6; c++) acc[k++] += pr[r].x * pr[c].y;
            acc[21 + r] += pr[r].x * rr.y;
        }
    }
}

// Phase 5 (WALK 2).  Waves walk 8 x 8 pixel blocks of this band of block rows; lane = (row, column) inside the block.  The region of a source
// frame that projects into the target is a compact blob, so whole blocks fall outside it (51 % of them at c3; 64 x 1 strips:
// 31 %), and a block's taps land in a compact patch of the target.  The list holds the blocks that are not provably dead.
__device__ __forceinline__ void walk_blocks(const SolveDims &D, const PinholeCtx &C, int n_live, float (&acc)[kDenseVals], int &n_ok)
{
    const int lane = (int)C.tid & 63, wave = __builtin_amdgcn_readfirstlane((int)C.tid >> 6);
    n_live = __builtin_amdgcn_readfirstlane(n_live);
    if (D.live_blocks && C.tid == 0) atomicAdd(D.live_blocks, (unsigned long long)n_live);
    const unsigned lx = (unsigned)lane & 7u, ly = (unsigned)lane >> 3;
    const unsigned lane_px = ly * (unsigned)D.width + lx;          // pixel offset of the lane inside its block
    const unsigned ox_l = 16u * lx, oy_l = 16u * ly + 16u * (unsigned)D.width;
    unsigned lane_off16 = 16u * lane_px;
    constexpr unsigned kBlockStep = 128u;            // 8 entries of 16 bytes
    // This wave's blocks: list entries wave, wave + 4, ... -- nt of them.  While block i is worked on, block i + 1's pixels are in flight.
    // The prefetch is UNCONDITIONAL (the last trip re-reads its own block): with a conditional one the number of loads in flight behind it
    // depended on the path taken and the compiler had to wait for ALL of them (`s_waitcnt vmcnt(0)` right behind the prefetch it had just
    // issued: the stream latency was paid in full on every trip, 2 % of the launch); now the wait for the current block's pixels is `vmcnt(1)`.
    // (Reading the list entry one more trip ahead, so that the prefetch is issued from a scalar register without an LDS round trip in
    // front of it: no change, r03 call 40.)
    // Two trips per loop iteration with the two register sets swapping roles: a single-trip loop rotates (next -> current) through
    // eight v_mov per trip, 5 % of its instructions.
    const int nt = (n_live > wave) ? (n_live - wave + kBlock / 64 - 1) / (kBlock / 64) : 0;
    // this wave's list entries ride in a register, 64 at a time (lane l: entry 64 c + l of the wave), and a trip takes its entry with v_readlane_b32:
    // no LDS round trip (address move, ds_read, wait, readfirstlane) at the top of every trip
    int list_chunk = 0;
    unsigned list_reg = nt > 0 ? C.blist[wave + (kBlock / 64) * min(lane, nt - 1)] : 0u;
    auto fetch = [&](int i, unsigned &code, float4 &zs) {
        const int idx = min(i, nt - 1);
        if ((idx >> 6) != list_chunk) { list_chunk = idx >> 6; list_reg = C.blist[wave + (kBlock / 64) * min(64 * list_chunk + lane, nt - 1)]; }
        code = (unsigned)__builtin_amdgcn_readlane((int)list_reg, idx & 63);
        // block base in the scalar address (wave-uniform), the lane's pixel inside the block as the constant vector offset: no vector add per trip
        // (the lane offset goes through an opaque copy: seen as loop-invariant, `frame base + lane offset` is hoisted as a 64-bit VECTOR address and the block
        // offset becomes a 64-bit vector add per trip)
        asm volatile("" : "+v"(lane_off16));          // (in place: no copy)
        zs = gather16_imm<0>(reinterpret_cast<const char *>(C.zn_s) + (size_t)(16u * ((code >> 16) * 8u * (unsigned)D.width + (code & 0xFFFFu) * 8u)), lane_off16);
    };
    auto work = [&](const float4 &zs, unsigned code) { pinhole_pixel(C, zs, ox_l + kBlockStep * (code & 0xFFFFu), oy_l + kBlockStep * (code >> 16), acc, n_ok); };
    if (nt > 0) {
        unsigned code_a, code_b = 0u;
        float4 zs_a, zs_b = make_float4(0.f, 0.f, 0.f, 0.f);
        fetch(0, code_a, zs_a);
        for (int i = 0;;) {
            fetch(i + 1, code_b, zs_b);
            work(zs_a, code_a);
            if (++i >= nt) break;
            fetch(i + 1, code_a, zs_a);
            work(zs_b, code_b);
            if (++i >= nt) break;
        }
    }
}

// Phase 5 (WALK 0 and 1): this tile's share of the source frame's pixels (LISTS: of its valid-pixel list), one pixel per lane and trip.
template <bool LISTS>
__device__ __forceinline__ void walk_strips(const SolveDims &D, const PinholeCtx &C, int tile, const uint32_t *__restrict__ valid_lists, const int *__restrict__ valid_counts, float (&acc)[kDenseVals], int &n_ok)
{
    const int n_src = LISTS ? valid_counts[C.slot_s] : D.npix;
    const uint32_t *list = LISTS ? valid_lists + C.slot_s * (size_t)D.npix : nullptr;
    const int per = (n_src + D.dense_tiles - 1) / D.dense_tiles;
    const int lo = min(n_src, per * tile), hi = min(n_src, per * (tile + 1));
    const float inv_w = 1.0f / (float)D.width;
    int t = lo + (int)C.tid;
    int s_n = (t < hi) ? (LISTS ? (int)list[t] : t) : 0;
    // direct walk: LDS byte offsets of the pixel's column / row entries (row table behind the column table), advanced by
    // one workgroup stride per trip
    const unsigned w4 = 4u * (unsigned)D.width;
    unsigned px4 = 4u * (unsigned)(s_n % D.width), py4 = 4u * (unsigned)(s_n / D.width) + w4;
    const unsigned step_x4 = 4u * (unsigned)(kBlock % D.width), step_y4 = 4u * (unsigned)(kBlock / D.width);
    float4 zs_n = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < hi) zs_n = C.zn_s[s_n];
    for (; t < hi; t += kBlock) {
        const float4 zs = zs_n;
        const int s = s_n;
        // next pixel's stream loads, UNCONDITIONAL like the block walk's (the last trip re-reads the lane's last pixel): the wait for
        // this trip's taps then does not have to cover a load that only some paths issue
        const int tn = min(t + (int)kBlock, hi - 1);
        s_n = LISTS ? (int)list[tn] : tn; zs_n = C.zn_s[s_n];
        unsigned ox, oy;
        if (!LISTS) {
            ox = px4; oy = py4;
            px4 += step_x4; py4 += step_y4;
            if (px4 >= w4) { px4 -= w4; py4 += 4u; }
        } else {
            const float sf = (float)s;
            const float pyf = floorf((sf + 0.5f) * inv_w);              // exact: the margin 0.5 / W is far above the rounding of the product
            ox = (unsigned)(4.0f * (sf - pyf * (float)D.width)); oy = (unsigned)(4.0f * pyf + C.ybase4);
        }
        pinhole_pixel(C, zs, 4u * ox, 4u * oy, acc, n_ok);      // 4-byte table offsets -> 16-byte entries (rowB follows colA as the row table follows the column table)
    }
}

// Phase 6, epilogue: the wave's count joins the sums, then the workgroup's record (dense_epilogue, with the signs of pinhole_pixel's row put right).
__device__ __forceinline__ void pinhole_epilogue(const SolveDims &D, const PinholeCtx &C, float (&acc)[kDenseVals], int n_ok, float *red, float *__restrict__ partials, int tile, int b)
{
    // the wave's count, converted once: an integer far below 2^24 in one lane and zeros in the others fold to the float the per-lane counts summed to
    acc[27] = (C.tid & 63u) == 0u ? (float)n_ok : 0.0f;
    dense_epilogue<true>(acc, red, dense_record_out(D, partials, C.p, tile, b), dense_record_mode(D));
}

template <int WALK>
__device__ __forceinline__ void dense_block_pinhole(const SolveDims &D, const float4 *__restrict__ zn, int q, const float *__restrict__ T, const float *__restrict__ Tinv, float *__restrict__ partials,
                                                    int tile, int b, float *red, const uint32_t *__restrict__ valid_lists, const int *__restrict__ valid_counts, float *lut)
{
    PinholeCtx C;
    const float m_stage = pinhole_item_and_poses<WALK>(D, C, q, T, Tinv, tile, b);
    pinhole_fill_tables<WALK>(D, C, lut);
    dense_M_store(C.tid, red, m_stage);
    const int n_live = pinhole_live_blocks<WALK>(D, C);
    pinhole_walk_constants(D, C, zn);
    float acc[kDenseVals] = {};
    int n_ok = 0;
    if (WALK == 2) walk_blocks(D, C, n_live, acc, n_ok);
    else walk_strips<WALK == 1>(D, C, tile, valid_lists, valid_counts, acc, n_ok);
    pinhole_epilogue(D, C, acc, n_ok, red, partials, tile, b);
}

template <bool SIMPLE, bool LISTS>
__global__ void __launch_bounds__(kBlock, 5) k_dense_sweep_zn(SolveDims D, const float4 *__restrict__ zn, const int2 *__restrict__ dense_pairs,
                                                             const float *__restrict__ T, const float *__restrict__ Tinv, float *__restrict__ partials,
                                                             const uint32_t *__restrict__ valid_lists, const int *__restrict__ valid_counts)
{
    __shared__ float red[kRedFloats];
    extern __shared__ __attribute__((aligned(16))) float zn_lut[];        // (Wd + Hd) floats
    int tile, p, b;
    dense_grid_decode(D, xcd_remap(blockIdx.x, gridDim.x), tile, p, b);
    // pinhole intrinsics: the same block as in the fused launch (same partial sums, bit for bit); `p` is then a WORK POSITION (dense_work_item)
    if (SIMPLE && LISTS) dense_block_pinhole<1>(D, zn, p, T, Tinv, partials, tile, b, red, valid_lists, valid_counts, zn_lut);
    else if (SIMPLE && D.walk_blocks) dense_block_pinhole<2>(D, zn, p, T, Tinv, partials, tile, b, red, valid_lists, valid_counts, zn_lut);
    else if (SIMPLE) dense_block_pinhole<0>(D, zn, p, T, Tinv, partials, tile, b, red, valid_lists, valid_counts, zn_lut);
    else dense_block_zn<LISTS>(D, zn, dense_pairs[p], T, Tinv, partials, tile, p, b, red, valid_lists, valid_counts, zn_lut);
}

// 1-D grid of dense_tiles * Pd * B workgroups (XCD-remapped).
__global__ void __launch_bounds__(kBlock, 3) k_dense_sweep(SolveDims D, const float4 *__restrict__ campos, const float4 *__restrict__ normals,
                                                              const int2 *__restrict__ dense_pairs, const float *__restrict__ T, const float *__restrict__ Tinv,
                                                              float *__restrict__ partials)
{
    __shared__ float red[kRedFloats];
    int tile, p, b;
    dense_grid_decode(D, xcd_remap(blockIdx.x, gridDim.x), tile, p, b);
    dense_block(D, campos, normals, dense_pairs[p], T, Tinv, partials, tile, p, b, red);
}

// Both sweeps of one Gauss-Newton iteration in ONE launch: n_d dense workgroups (VALU-bound) interleaved with
// n_s sparse workgroups (HBM-streaming) so the two overlap on every CU instead of running back to back.
// Per XCD x (blocks g = 8 s + x, s = slot): a contiguous range of dense items (L2 locality, as in xcd_remap)
// and every R_x-th slot a sparse item.
template <int LAYOUT>   // 0: float4 camPos + float4 normals; compact cache: 1 zero-skew K, 2 general K, 3 / 4 the same walking valid-pixel lists
__device__ __forceinline__ void fused_item(const SolveDims &D, unsigned n_d, unsigned n_s, unsigned g,
                                           const float4 *__restrict__ campos, const float4 *__restrict__ normals,
                                           const int2 *__restrict__ dense_pairs, const float *__restrict__ T, const float *__restrict__ Tinv,
                                           float *__restrict__ dense_partials,
                                           const float4 *__restrict__ corr, const uint32_t *__restrict__ pair_offsets, float *__restrict__ sparse_partials,
                                           const uint32_t *__restrict__ valid_lists, const int *__restrict__ valid_counts, float *red, float *zn_lut)
{
    const unsigned G = n_d + n_s, xcd = g & 7u, slot = g >> 3;
    const unsigned qd = n_d >> 3, rd = n_d & 7u;
    const unsigned Gx = (G - xcd + 7u) >> 3, ndx = qd + (xcd < rd ? 1u : 0u), nsx = Gx - ndx;
    unsigned sparse_base = 0;                                   // sparse items owned by lower XCDs
    for (unsigned y = 0; y < xcd; y++) sparse_base += ((G - y + 7u) >> 3) - (qd + (y < rd ? 1u : 0u));
    // Sparse items: a share of them (D.sparse_tail_256 / 256) is HELD BACK to the end of the XCD's sequence, the rest is interleaved evenly
    // among the dense items.  A launch ends with its occupancy falling for ~30 us while the last long dense items finish (12-15 % of its
    // span); short, HBM-streaming sparse items fill those emptying slots, and the dense items start that much earlier.
    const unsigned nst = (nsx * (unsigned)D.sparse_tail_256) >> 8, nsi = nsx - nst, Gi = ndx + nsi;
    // (an even interleave period from 4 on is lowered to the odd one below it: with periods 4 and 6 the sparse items of an XCD kept landing on
    // the same compute units of the dispatcher's round robin -- 196 and 182 us per launch against 171 us at period 5, gpurun_out/r03_24;
    // period 2, the masked launch's plain alternation, measured fine)
    const unsigned Rx0 = nsi ? Gi / nsi : 0xFFFFFFFFu;
    const unsigned Rx = (nsi && Rx0 >= 4u && !(Rx0 & 1u)) ? Rx0 - 1u : Rx0;
    const bool in_tail = slot >= Gi;
    const bool is_sparse = in_tail || (nsi && (slot % Rx == 0u) && (slot / Rx < nsi));
    const unsigned sparse_local = in_tail ? nsi + (slot - Gi) : slot / Rx;
    if (is_sparse) {
        const unsigned i = sparse_base + sparse_local;           // (chunk fastest, then pair, then instance)
        const int chunk = (int)(i % (unsigned)D.sparse_chunks);
        const int p = (int)((i / (unsigned)D.sparse_chunks) % (unsigned)D.n_pairs);
        const int b = (int)(i / ((unsigned)D.sparse_chunks * (unsigned)D.n_pairs));
        sparse_block(D, corr, pair_offsets, T, sparse_partials, chunk, p, b, red);
    } else {
        const unsigned before = nsi ? min(nsi, (slot + Rx - 1u) / Rx) : 0u;     // sparse slots of this XCD before `slot`
        const unsigned dl = slot - before;                                      // dense item local to the XCD
        const unsigned L = (xcd < rd ? xcd * (qd + 1u) : rd * (qd + 1u) + (xcd - rd) * qd) + dl;
        const int b = (int)(L / ((unsigned)D.dense_tiles * (unsigned)D.n_dense_pairs));
        const unsigned Lb = L - (unsigned)b * (unsigned)D.dense_tiles * (unsigned)D.n_dense_pairs;
        const int tile = D.tile_major ? (int)(Lb / (unsigned)D.n_dense_pairs) : (int)(Lb % (unsigned)D.dense_tiles);
        int p = D.tile_major ? (int)(Lb % (unsigned)D.n_dense_pairs) : (int)(Lb / (unsigned)D.dense_tiles);
        // work order: the pairs of a band heaviest first, so that the workgroups still running when the launch drains are short ones.
        // p is a WORK POSITION: the pinhole blocks compute their item from it (dense_work_item), the other layouts read the work table entry
        if (LAYOUT == 1 && D.walk_blocks) dense_block_pinhole<2>(D, campos, p, T, Tinv, dense_partials, tile, b, red, valid_lists, valid_counts, zn_lut);
        else if (LAYOUT == 1) dense_block_pinhole<0>(D, campos, p, T, Tinv, dense_partials, tile, b, red, valid_lists, valid_counts, zn_lut);     // `campos` carries the compact cache
        else if (LAYOUT == 3) dense_block_pinhole<1>(D, campos, p, T, Tinv, dense_partials, tile, b, red, valid_lists, valid_counts, zn_lut);
        else {
            const int4 w = D.dense_work[p];
            const int2 ij = make_int2(w.x, w.y);
            p = w.z;
            if (LAYOUT == 0) dense_block(D, campos, normals, ij, T, Tinv, dense_partials, tile, p, b, red);
            else if (LAYOUT == 2) dense_block_zn<false>(D, campos, ij, T, Tinv, dense_partials, tile, p, b, red, valid_lists, valid_counts, zn_lut);
            else dense_block_zn<true>(D, campos, ij, T, Tinv, dense_partials, tile, p, b, red, valid_lists, valid_counts, zn_lut);
        }
    }
}

#define BTBA_FUSED_ITEM_ARGS D, n_d, n_s, g, campos, normals, dense_pairs, T, Tinv, dense_partials, corr, pair_offsets, sparse_partials, valid_lists, valid_counts, red, zn_lut
template <int LAYOUT>
__global__ void __launch_bounds__(kBlock, BTBA_FUSED_WAVES) k_fused_sweeps(SolveDims D, unsigned n_d, unsigned n_s,
                                                           const float4 *__restrict__ campos, const float4 *__restrict__ normals,
                                                           const int2 *__restrict__ dense_pairs, const float *__restrict__ T, const float *__restrict__ Tinv,
                                                           float *__restrict__ dense_partials,
                                                           const float4 *__restrict__ corr, const uint32_t *__restrict__ pair_offsets, float *__restrict__ sparse_partials,
                                                           const uint32_t *__restrict__ valid_lists, const int *__restrict__ valid_counts)
{
    __shared__ float red[kRedFloats];
    extern __shared__ __attribute__((aligned(16))) float zn_lut[];        // (Wd + Hd) floats (+ the block walk's list), compact layouts only
    const unsigned g = blockIdx.x;
    fused_item<LAYOUT>(BTBA_FUSED_ITEM_ARGS);
}

#undef BTBA_FUSED_ITEM_ARGS

}  // namespace btba
