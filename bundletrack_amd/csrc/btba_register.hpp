// btba_register.hpp -- frame-to-model registration (btba_register_index / btba_register_frames / btba_register_associate, include/btba.h):
// batched point-to-plane Gauss-Newton ICP of frames and point lists against the voxel cloud of btba_fuse_frames.
//
// Items travel in chunks of BTBA_FUSE_CHUNK as kernel arguments; the current poses, the stop flags and the partial records live in the
// workspace's scratch (btba_register_layout.hpp).  Launches of one btba_register_frames call:
//   k_register_init        per chunk: the segments' poses -> scratch, flags cleared
//   k_register_accumulate  per chunk and iteration, grid (point blocks, item): workgroup k of an item takes its points 2048 k .. 2048 k + 2047,
//                          eight per thread.  An invalid pixel costs its depth load and nothing else (masked frames are ~5 % valid); a
//                          survivor does the dependent gathers -- cell index, then two float4 of the model, L2-resident (a 5 mm object
//                          model is ~3 000 records in a box of ~17 000 cells).  Every thread keeps 28 fp64 sums (H's lower triangle, g,
//                          cost) and three counts; a wave folds them by butterfly (skipped, exact zeros, by a wave without a match), the
//                          four waves are added in order through LDS, one 256-byte partial record per workgroup.
//   k_register_solve       per chunk and iteration, one wave per item: 32 lanes sum the item's partial records in index order, lane 0
//                          runs the 6 x 6 Cholesky, the exponential and the update in fp64 and writes the trace entry and the flag.
// and once more accumulate + solve in `final` mode (no solve: the result at pose_out).  k_register_associate is one pass over the same
// register_match.  Staging the model in LDS was not built: nothing here has been measured yet against the plain gathers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/btba.h"
#include "btba_fusion_point.hpp"
#include "btba_register_layout.hpp"

namespace btba {

struct RegItems {                                      // one chunk, structure-of-arrays; 56 bytes per item
    const void *geom[kFuseChunk];                      // frame: float depth [H*W]; list: float4 xyz [n]
    const float4 *normal[kFuseChunk];                  // or nullptr
    int32_t n[kFuseChunk];                             // pixels or points
    int32_t kind_instance[kFuseChunk];                 // instance * 2 + kind
    int32_t min_b[kFuseChunk][3], dims[kFuseChunk][3]; // the instance's box
    uint32_t vox_off[kFuseChunk];                      // the instance's first cell of the index
    uint32_t part_off[kFuseChunk];                     // the item's first partial record
    int32_t first;                                     // index of the chunk's first item in the call
};
static_assert(sizeof(RegItems) <= 2048, "a chunk of items travels as a kernel argument");

struct RegPoses { float pose[kFuseChunk][12]; };       // the initial poses of a chunk (k_register_init, k_register_associate)

struct RegModel {
    const float4 *xyz, *normal;                        // [n_instances][capacity]
    const int32_t *cell;                               // [V]
    int capacity;
};

struct RegParams {
    float inv_leaf, max_dist2, min_cos, delta;
    int radius, require_normals, min_matches, n_iters;
    double eps_rot, eps_trans;
};

struct RegScratch {
    double *partials;
    float *poses;
    int32_t *state;
};

struct RegMatch { float3 d, n; };                      // q - m and the model normal of the matched record

// Rules 2 and 3 of the header for the model-frame point q with rotated source normal nrm: the matched record, or -1 .. -3.
__device__ __forceinline__ int register_match(const RegItems &S, int z, const RegModel &M, const RegParams &P, const float3 &q, const float3 &nrm,
                                              bool normal_gate, RegMatch &out)
{
#pragma clang fp contract(off)
    int cx, cy, cz;
    if (!fuse_cell(q, P.inv_leaf, cx, cy, cz)) return -1;
    const long long ix = (long long)cx - S.min_b[z][0], iy = (long long)cy - S.min_b[z][1], iz = (long long)cz - S.min_b[z][2];
    const int dx = S.dims[z][0], dy = S.dims[z][1], dz = S.dims[z][2];
    const int32_t *cell = M.cell + S.vox_off[z];
    const float4 *mx = M.xyz + (size_t)(S.kind_instance[z] >> 1) * (size_t)M.capacity;
    int best = -1;
    float best_d2 = 0.0f;
    float3 bd = make_float3(0.f, 0.f, 0.f);
    const int r = P.radius;
    for (int oz = -r; oz <= r; oz++) {
        const long long jz = iz + oz;
        if (jz < 0 || jz >= dz) continue;
        for (int oy = -r; oy <= r; oy++) {
            const long long jy = iy + oy;
            if (jy < 0 || jy >= dy) continue;
            for (int ox = -r; ox <= r; ox++) {
                const long long jx = ix + ox;
                if (jx < 0 || jx >= dx) continue;
                const int k = cell[(size_t)(jx + dx * (jy + dy * jz))];
                if (k < 0 || k >= M.capacity) continue;
                const float4 m = mx[k];
                const float ex = q.x - m.x, ey = q.y - m.y, ez = q.z - m.z;
                const float d2 = (ex * ex + ey * ey) + ez * ez;
                if (best < 0 || d2 < best_d2) { best = k; best_d2 = d2; bd = make_float3(ex, ey, ez); }
            }
        }
    }
    if (best < 0) return -1;
    if (!(best_d2 <= P.max_dist2)) return -2;
    const float4 mn = (M.normal + (size_t)(S.kind_instance[z] >> 1) * (size_t)M.capacity)[best];
    if (mn.x == 0.0f && mn.y == 0.0f && mn.z == 0.0f) return -3;
    if (normal_gate && !((nrm.x * mn.x + nrm.y * mn.y) + nrm.z * mn.z >= P.min_cos)) return -3;
    out.d = bd;
    out.n = make_float3(mn.x, mn.y, mn.z);
    return best;
}

// Rules 1 - 3 for element e of item z at the pose T: the matched record, -1 .. -3, or -4 for a dropped element.
__device__ __forceinline__ int register_point(const RegItems &S, int z, int e, int W, const Mat4 &Kinv, const float *T, const RegModel &M, const RegParams &P,
                                              float3 &q, RegMatch &out)
{
    const float4 *nmap = S.normal[z];
    const bool gate = nmap != nullptr && P.min_cos > -1.0f;
    float3 nrm;
    if (!fuse_point_at((S.kind_instance[z] & 1) == BTBA_FUSE_FRAME, S.geom[z], nmap, T, e, W, Kinv, P.require_normals != 0, gate, q, nrm)) return -4;
    return register_match(S, z, M, P, q, nrm, gate, out);
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid (blocks over the capacity, instances of the chunk); the cells were set to -1 by the host's memset
struct RegIndexInstances { uint32_t vox_off[kFuseChunk]; int32_t n_vox[kFuseChunk]; };
__global__ void __launch_bounds__(256) k_register_index(const RegIndexInstances I, int first_instance, int capacity, const int32_t *lin, const int32_t *n_out,
                                                        int32_t *cell)
{
    const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const int n = min(n_out[first_instance + b], capacity);
    if (k >= n) return;
    const int l = lin[(size_t)(first_instance + b) * (size_t)capacity + k];
    if (l < 0 || l >= I.n_vox[b]) return;
    cell[(size_t)I.vox_off[b] + l] = k;
}

__global__ void __launch_bounds__(256) k_register_init(const RegPoses Q, int first, int n, RegScratch X)
{
    const int t = threadIdx.x + blockIdx.x * 256;
    if (t < n * 12) X.poses[(size_t)first * 12 + t] = Q.pose[t / 12][t % 12];
    if (t < n * 2) X.state[(size_t)first * 2 + t] = 0;
}

__global__ void __launch_bounds__(kRegThreads) k_register_accumulate(int W, Mat4 Kinv, RegParams P, const RegItems S, RegModel M, RegScratch X, int final)
{
    __shared__ double red[4][28];
    __shared__ int cnt[4][3];
    const int z = blockIdx.y, n = S.n[z], item = S.first + z;
    if ((int64_t)blockIdx.x * kRegBlockPoints >= n) return;                  // (uniform)
    if (!final && X.state[2 * (size_t)item] != 0) return;                    // stopped (uniform)
    float T[12];
    for (int k = 0; k < 12; k++) T[k] = X.poses[12 * (size_t)item + k];
    double acc[28];
    for (int k = 0; k < 28; k++) acc[k] = 0.0;
    int n_valid = 0, n_matched = 0, n_beyond = 0;
    const double delta = (double)P.delta;
    for (int j = 0; j < kRegPointsPerThread; j++) {
        const int e = blockIdx.x * kRegBlockPoints + j * kRegThreads + (int)threadIdx.x;
        if (e >= n) break;
        float3 q;
        RegMatch m;
        const int k = register_point(S, z, e, W, Kinv, T, M, P, q, m);
        if (k == -4) continue;
        n_valid++;
        if (k < 0) continue;
        n_matched++;
        float a[6], r;
        {
#pragma clang fp contract(off)
            r = (m.n.x * m.d.x + m.n.y * m.d.y) + m.n.z * m.d.z;
            a[0] = q.y * m.n.z - q.z * m.n.y;
            a[1] = q.z * m.n.x - q.x * m.n.z;
            a[2] = q.x * m.n.y - q.y * m.n.x;
            a[3] = m.n.x; a[4] = m.n.y; a[5] = m.n.z;
        }
        const double rd = (double)r, ar = fabs(rd);
        const bool inside = fabsf(r) <= P.delta;
        if (!inside) n_beyond++;
        {
#pragma clang fp contract(off)                                               // every term is rounded as the restatement rounds it: (w a_i) a_j, no fma
            const double w = inside ? 1.0 : delta / ar;
            int s = 0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const double wa = w * (double)a[i];
#pragma unroll
                for (int c = 0; c <= i; c++) { const double t = wa * (double)a[c]; acc[s++] += t; }
                const double tg = wa * rd;
                acc[kRegSlotG + i] += tg;
            }
            const double rho = inside ? rd * rd : (2.0 * delta) * ar - delta * delta;
            acc[kRegSlotCost] += rho;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    n_valid = wave_sum_i(n_valid);
    n_matched = wave_sum_i(n_matched);
    n_beyond = wave_sum_i(n_beyond);
    if (n_matched > 0) {                                                     // (wave-uniform) a wave without a match adds exact zeros
#pragma unroll
        for (int k = 0; k < 28; k++) acc[k] = wave_sum_f64(acc[k]);
    }
    if (lane == 0) {
        for (int k = 0; k < 28; k++) red[wave][k] = acc[k];
        cnt[wave][0] = n_valid; cnt[wave][1] = n_matched; cnt[wave][2] = n_beyond;
    }
    __syncthreads();
    double *rec = X.partials + ((size_t)S.part_off[z] + blockIdx.x) * kRegRecord;
    const int t = threadIdx.x;
    if (t < 28) rec[t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    else if (t < 31) rec[t] = (double)(((cnt[0][t - 28] + cnt[1][t - 28]) + cnt[2][t - 28]) + cnt[3][t - 28]);
    else if (t == 31) rec[t] = 0.0;
}

// H (lower triangle, row-major) = L L^T in place of L; false at the first pivot that is not positive and finite.  ratio: min_j d_j / H_jj.
__device__ __forceinline__ bool register_cholesky(const double *H, double *L, double &ratio)
{
    ratio = 0.0;
    double rmin = 0.0;
    for (int j = 0; j < 6; j++) {
        const double hjj = H[j * (j + 1) / 2 + j];
        double d = hjj;
        for (int k = 0; k < j; k++) d -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        if (!(d > 0.0) || !(d < INFINITY)) return false;
        const double pr = hjj > 0.0 ? d / hjj : 0.0;
        rmin = j == 0 ? pr : fmin(rmin, pr);
        const double ljj = sqrt(d);
        L[j * (j + 1) / 2 + j] = ljj;
        for (int i = j + 1; i < 6; i++) {
            double s = H[i * (i + 1) / 2 + j];
            for (int k = 0; k < j; k++) s -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = s / ljj;
        }
    }
    ratio = rmin;
    return true;
}

// T <- Exp(xi) T in fp64, rounded to fp32 once (rule 7 of the header)
__device__ __forceinline__ void register_update(const double *xi, float *T)
{
    const double wx = xi[0], wy = xi[1], wz = xi[2];
    const double th = sqrt((wx * wx + wy * wy) + wz * wz);
    double A, B, C;
    if (th < 1e-12) { A = 1.0; B = 0.5; C = 0.0; }
    else { A = sin(th) / th; B = (1.0 - cos(th)) / (th * th); C = (th - sin(th)) / (th * th * th); }
    const double K[9] = { 0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0 };
    double K2[9], R[9], V[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) K2[3 * i + j] = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
    const bool small = th < 1e-12;
    for (int k = 0; k < 9; k++) {
        const double eye = (k % 4 == 0) ? 1.0 : 0.0;
        R[k] = small ? eye + K[k] : (eye + A * K[k]) + B * K2[k];
        V[k] = small ? eye + 0.5 * K[k] : (eye + B * K[k]) + C * K2[k];
    }
    double t[3], out[12];
    for (int i = 0; i < 3; i++) t[i] = (V[3 * i] * xi[3] + V[3 * i + 1] * xi[4]) + V[3 * i + 2] * xi[5];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 4; j++)
            out[4 * i + j] = (R[3 * i] * (double)T[j] + R[3 * i + 1] * (double)T[4 + j]) + R[3 * i + 2] * (double)T[8 + j];
        out[4 * i + 3] += t[i];
    }
    for (int k = 0; k < 12; k++) T[k] = (float)out[k];
}

// grid (items of the chunk), one wave each.  iter: the iteration's index; final: write the result and pose_out instead of solving.
__global__ void __launch_bounds__(64) k_register_solve(RegParams P, const RegItems S, RegScratch X, int iter, int final, float *pose_out,
                                                       btba_register_result *result, btba_register_iter *trace)
{
    __shared__ double rec[kRegRecord];
    const int z = blockIdx.x, item = S.first + z, lane = threadIdx.x;
    int32_t *state = X.state + 2 * (size_t)item;
    const int st = state[0];
    const bool skipped = !final && st != 0;
    if (lane < kRegRecord) {
        double s = 0.0;
        if (!skipped) {
            const int nb = (int)register_blocks(S.n[z]);
            const double *p = X.partials + (size_t)S.part_off[z] * kRegRecord + lane;
#pragma unroll 8                                                             // the loads are independent: several in flight, the additions still in index order
            for (int b = 0; b < nb; b++) s += p[(size_t)b * kRegRecord];
        }
        rec[lane] = s;
    }
    __syncthreads();
    if (lane != 0) return;
    float *T = X.poses + 12 * (size_t)item;
    const int n_valid = (int)rec[kRegSlotValid], n_matched = (int)rec[kRegSlotMatched], n_beyond = (int)rec[kRegSlotBeyond];
    if (final) {
        btba_register_result r;
        r.status = st != 0 ? st - 1 : (state[1] == 0 && n_matched < P.min_matches ? BTBA_REG_TOO_FEW : BTBA_REG_MAX_ITERS);
        r.iters_done = state[1];
        r.n_valid = n_valid; r.n_matched = n_matched; r.n_beyond = n_beyond; r.reserved = 0;
        r.cost = rec[kRegSlotCost];
        result[item] = r;
        for (int k = 0; k < 12; k++) pose_out[12 * (size_t)item + k] = T[k];
        return;
    }
    btba_register_iter *tr = trace ? trace + (size_t)item * P.n_iters + iter : nullptr;
    if (skipped) {
        if (tr) {
            btba_register_iter e{};
            e.status = BTBA_REG_SKIPPED;
            *tr = e;
        }
        return;
    }
    btba_register_iter e{};
    e.n_valid = n_valid; e.n_matched = n_matched; e.n_beyond = n_beyond;
    e.cost = rec[kRegSlotCost];
    for (int k = 0; k < 21; k++) e.H[k] = rec[k];
    for (int k = 0; k < 6; k++) e.g[k] = rec[kRegSlotG + k];
    int status = BTBA_REG_MAX_ITERS;
    double L[21];
    if (n_matched < P.min_matches) {
        status = BTBA_REG_TOO_FEW;
    } else if (!register_cholesky(e.H, L, e.pivot_ratio)) {
        status = BTBA_REG_DEGENERATE;
    } else {
        double y[6];
        for (int i = 0; i < 6; i++) {                                        // L y = -g
            double s = -e.g[i];
            for (int k = 0; k < i; k++) s -= L[i * (i + 1) / 2 + k] * y[k];
            y[i] = s / L[i * (i + 1) / 2 + i];
        }
        for (int i = 5; i >= 0; i--) {                                       // L^T xi = y
            double s = y[i];
            for (int k = i + 1; k < 6; k++) s -= L[k * (k + 1) / 2 + i] * e.xi[k];
            e.xi[i] = s / L[i * (i + 1) / 2 + i];
        }
        float Tn[12];
        for (int k = 0; k < 12; k++) Tn[k] = T[k];
        register_update(e.xi, Tn);
        for (int k = 0; k < 12; k++) T[k] = Tn[k];
        const double nw = sqrt((e.xi[0] * e.xi[0] + e.xi[1] * e.xi[1]) + e.xi[2] * e.xi[2]);
        const double nu = sqrt((e.xi[3] * e.xi[3] + e.xi[4] * e.xi[4]) + e.xi[5] * e.xi[5]);
        if (nw < P.eps_rot && nu < P.eps_trans) status = BTBA_REG_CONVERGED;
    }
    e.status = status;
    for (int k = 0; k < 12; k++) e.pose[k] = T[k];
    if (tr) *tr = e;
    state[1] += 1;
    if (status != BTBA_REG_MAX_ITERS) state[0] = 1 + status;
}

struct RegMatchOut { int32_t *out[kFuseChunk]; };
__global__ void __launch_bounds__(256) k_register_associate(int W, Mat4 Kinv, RegParams P, const RegItems S, const RegPoses Q, RegModel M, const RegMatchOut O)
{
    const int z = blockIdx.y, n = S.n[z];
    float T[12];
    for (int k = 0; k < 12; k++) T[k] = Q.pose[z][k];
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        float3 q;
        RegMatch m;
        O.out[z][e] = register_point(S, z, e, W, Kinv, T, M, P, q, m);
    }
}

}  // namespace btba
